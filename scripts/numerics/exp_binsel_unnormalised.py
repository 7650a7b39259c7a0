#!/usr/bin/env python3
"""CPU experiment (NumPy): the sampling direction's bin selection of the shift-free conditioned spline
(cnf_device.h, cond_spline_rows), emulated in float32 operation by operation in two forms and compared with float64:

  knots : today's general form -- every bin normalised (w_k = e_k a + min_bin), two running knots, masks on
          v - knot, the selected x0 / y0 / bw / bh picked with 0/1 masks, the last bin closed with hi - knot;
  sums  : the masks on the unnormalised prefix sums, m_k = [(v - lo - k min_bin) sh / span > ch_k], the selected
          RAW exponentials summed with the masks and the four results scaled once.

Logits are in log2 units with the group maximum within +-4 of zero (what the table builder guarantees for
shift-free cells) and a spread of 1, 4 or 12 below it; v is uniform over the spline's range.  Reported per
spread: the largest error of x0, bw, y0, bh against float64, the samples whose bin differs from float64's, and how
far the last bin's top x0 + bw, y0 + bh is from hi.  A fused multiply-add is emulated as a float64 product and sum
rounded to float32.
Usage: python scripts/numerics/exp_binsel_unnormalised.py [samples per spread] [seed]"""
import sys
import numpy as np

K = 5
LO, HI, MINB = np.float32(-10.0), np.float32(10.0), np.float32(1e-4)
SPAN = np.float32(np.float32(HI - LO) - np.float32(K) * MINB)
f32 = np.float32


def fma(a, b, c):
  return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(f32)


def rcp(x):
  return (1.0 / x.astype(np.float64)).astype(f32)


def step(d):
  return (d > 0).astype(f32)              # clamp(d 2^60): 0 or 1 (differences below 2^-60 do not occur here)


def sums32(tw, th):
  ew, eh = np.exp2(tw).astype(f32), np.exp2(th).astype(f32)
  cw, chh = [ew[:, 0]], [eh[:, 0]]
  for k in range(1, K):
    cw.append(cw[-1] + ew[:, k]); chh.append(chh[-1] + eh[:, k])
  sw, sh = cw[-1], chh[-1]
  r = rcp(sw * sh) * SPAN
  return ew, eh, chh, sw, sh, r * sh, r * sw


def form_knots(tw, th, v):
  ew, eh, _, _, _, aw, ah = sums32(tw, th)
  px = np.full_like(v, LO); py = px.copy()
  wp, hp = fma(ew[:, 0], aw, MINB), fma(eh[:, 0], ah, MINB)
  x0, y0 = px.copy(), py.copy()
  mprev = np.ones_like(v); bw = np.zeros_like(v); bh = np.zeros_like(v); kf = np.zeros_like(v)
  for k in range(1, K):
    px = px + wp; py = py + hp
    m = step(v - py)
    o = mprev - m
    bw, bh = fma(o, wp, bw), fma(o, hp, bh)
    kf = kf + m
    x0, y0 = fma(m, wp, x0), fma(m, hp, y0)
    if k == K - 1:
      wp, hp = HI - px, HI - py
    else:
      wp, hp = fma(ew[:, k], aw, MINB), fma(eh[:, k], ah, MINB)
    mprev = m
  return x0, fma(mprev, wp, bw), y0, fma(mprev, hp, bh), kf


def form_sums(tw, th, v):
  ew, eh, ch, _, sh, aw, ah = sums32(tw, th)
  t = sh * f32(f32(1.0) / SPAN)
  m = [None] + [step(fma(v - f32(LO + f32(k) * MINB), t, -ch[k - 1])) for k in range(1, K)]
  xs, ys = m[1] * ew[:, 0], m[1] * eh[:, 0]
  ws, hs = ew[:, 0] - xs, eh[:, 0] - ys
  kf = m[1].copy()
  for k in range(1, K):
    o = m[k] if k == K - 1 else m[k] - m[k + 1]
    ws, hs = fma(o, ew[:, k], ws), fma(o, eh[:, k], hs)
    if k > 1:
      xs, ys = fma(m[k], ew[:, k - 1], xs), fma(m[k], eh[:, k - 1], ys)
      kf = kf + m[k]
  base = fma(kf, MINB, LO)
  return fma(xs, aw, base), fma(ws, aw, MINB), fma(ys, ah, base), fma(hs, ah, MINB), kf


def exact(tw, th, v):
  tw, th, v = tw.astype(np.float64), th.astype(np.float64), v.astype(np.float64)
  span = (float(HI) - float(LO)) - K * float(MINB)
  out = []
  for t in (tw, th):
    e = np.exp2(t)
    w = e / e.sum(1, keepdims=True) * span + float(MINB)
    out.append((np.concatenate([np.full((len(t), 1), float(LO)), float(LO) + np.cumsum(w[:, :-1], 1)], 1), w))
  (xk, w), (yk, h) = out
  k = (v[:, None] > yk[:, 1:]).sum(1)
  r = np.arange(len(v))
  return xk[r, k], w[r, k], yk[r, k], h[r, k], k


def main():
  n = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
  rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
  for spread in (1.0, 4.0, 12.0):
    t = -spread * rng.random((n, 2 * K))
    t[np.arange(n), rng.integers(0, K, n)] = 0.0                    # each group's maximum ...
    t[np.arange(n), K + rng.integers(0, K, n)] = 0.0
    t[:, :K] += rng.uniform(-4, 4, (n, 1)); t[:, K:] += rng.uniform(-4, 4, (n, 1))     # ... within +-4 of zero
    t = t.astype(f32)
    v = rng.uniform(float(LO), float(HI), n).astype(f32)
    ref = exact(t[:, :K], t[:, K:], v)
    print(f"spread {spread:4.1f}, {n} logit sets")
    for name, form in (("knots", form_knots), ("sums ", form_sums)):
      got = form(t[:, :K], t[:, K:], v)
      same = got[4].astype(int) == ref[4]
      err = [np.abs(g.astype(np.float64) - e)[same].max() for g, e in zip(got[:4], ref[:4])]
      last = got[4].astype(int) == K - 1
      top = max(np.abs(got[0][last].astype(np.float64) + got[1][last] - float(HI)).max(),
                np.abs(got[2][last].astype(np.float64) + got[3][last] - float(HI)).max())
      # a sample whose bin differs sits on a knot: the two bins' values of the spline agree there
      off = np.abs(v[~same].astype(np.float64) - np.where(got[4][~same] > ref[4][~same], got[2][~same], ref[2][~same]))
      print(f"  {name}: max err x0 {err[0]:.2e} bw {err[1]:.2e} y0 {err[2]:.2e} bh {err[3]:.2e}; other bin than "
            f"float64: {(~same).sum()} (|v - knot| <= {off.max() if off.size else 0.0:.1e}); "
            f"last bin's top misses hi by {top:.2e}")


if __name__ == "__main__":
  main()
