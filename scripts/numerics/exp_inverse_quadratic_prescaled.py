#!/usr/bin/env python3
"""CPU experiment (NumPy): the root of the sampling direction's quadratic (cnf_device.h, rqs_bin_eval, INV,
NEWTON=false), emulated in float32 operation by operation in two forms and compared with float64:

  parent    : c = -s dy, b = d0 bh - st dy, a = s bh - b, disc = b^2 + (a c)(-4), z = (c (-2)) rcp(b + sqrt(disc));
  prescaled : c2 = 2s dy, b = d0bh - st dy, a = s bh - b, disc = b^2 + a (c2 + c2), z = c2 rcp(b + sqrt(disc)) with 2s
              shared with the derivative's numerator and d0bh = d0 bh formed per sample (conditioned spline), or both
              read from the table, d0bh rounded once from float64 (`first`);
  four-field: the `first` form with two more table fields, a = sbh - b and disc = b^2 + a (4s dy) -- the same
              number of operations as `prescaled`, two more table reads per sample; measured here, not built.

Two populations.  `cond`: what the table builder admits to the shift-free form -- bins from min_bin = 1e-4 to the
range of 20, slopes softplus(t) + 1e-4 with t in [-3, 40]; s = bh rcp(bw) and st = d0 + d1 - 2s are formed in
float32 as the kernel forms them.  `first`: the shared spline, whose bins and slopes are normalised in float64 and
rounded to the table -- bins from 1e-4 to 20, slopes from the floor 1e-4 to 40; `first, moderate`: the same with
bins in [0.25, 8] and slopes in [0.05, 20], where float32 itself is accurate.  Log-uniform draws over five decades
put many samples where the float32 quadratic is ill-conditioned in EITHER form (knot slopes far from the bin's own
slope: errors of order 0.1 in z, discriminants lost to cancellation); those dominate both forms' largest errors
alike, so the comparison is repeated on the samples whose discriminants stay positive and on the well-conditioned
ones; there too both forms' largest errors are the same ill-conditioned samples, and only `first, moderate`
discriminates between the forms.  dy is uniform over the bin, with
both ends included.  A fused multiply-add is emulated as a float64 product and sum rounded to float32; v_rcp_f32 and
v_sqrt_f32 as correctly rounded (their 1 ulp is common to both forms).

Reported per population: the largest error of z and of out = x0 + bw z against float64 for both forms, and the
largest difference between the forms.  The bar (the parent form is the yardstick): the prescaled form's largest
error of out may exceed the parent form's by at most one float32 spacing at 10, 9.5e-7; of z by at most 2^-23.
Usage: python scripts/numerics/exp_inverse_quadratic_prescaled.py [samples per population] [seed]"""
import sys
import numpy as np

f32, f64 = np.float32, np.float64
LO, HI, MINB, MINS = -10.0, 10.0, 1e-4, 1e-4
SPACING_AT_10 = 9.5367431640625e-07


def fma(a, b, c):
  return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def rcp(x):
  return (1.0 / x.astype(f64)).astype(f32)


NEG, POS = {}, {}                     # form -> how many discriminants came out negative in the last call; which did not


def sqrt(x):
  with np.errstate(invalid="ignore"):
    return np.sqrt(x.astype(f64)).astype(f32)


def clip01(z):                        # the clamp modifier: NaN (the root of a negative discriminant) becomes 0
  return np.where(np.isnan(z), f32(0), np.minimum(np.maximum(z, f32(0)), f32(1))).astype(f32)


def parent_form(dy, bh, s, st, d0):
  c = -s * dy
  b = fma(-st, dy, d0 * bh)
  a = fma(s, bh, -b)
  disc = fma(b, b, a * c * f32(-4))
  NEG["parent   "], POS["parent   "] = int((disc < 0).sum()), disc >= 0
  return clip01(c * f32(-2) * rcp(b + sqrt(disc)))


def prescaled_form(dy, bh, s, st, d0, tab=None):
  if tab is None:                     # conditioned spline: 2s from the derivative's numerator
    s2 = s * f32(2)
    c2 = s2 * dy
    b = fma(-st, dy, d0 * bh)
    a = fma(s, bh, -b)
    c4 = c2 + c2
  else:                               # `first`: d0 bh and 2s from the table
    d0bh, _, s2, _ = tab
    c2 = s2 * dy
    b = fma(-st, dy, d0bh)
    a = fma(s, bh, -b)
    c4 = c2 + c2
  disc = fma(b, b, a * c4)
  NEG["prescaled"], POS["prescaled"] = int((disc < 0).sum()), disc >= 0
  return clip01(c2 * rcp(b + sqrt(disc)))


def four_field_form(dy, st, tab):
  d0bh, sbh, s2, s4 = tab
  b = fma(-st, dy, d0bh)
  disc = fma(b, b, (sbh - b) * (s4 * dy))
  return clip01(s2 * dy * rcp(b + sqrt(disc)))


def exact_root(dy, bh, s, st, d0):
  c = -s * dy
  b = d0 * bh - st * dy
  a = s * bh - b
  return np.clip(-2.0 * c / (b + np.sqrt(np.maximum(b * b - 4.0 * a * c, 0.0))), 0.0, 1.0)


def log_uniform(rng, lo, hi, n):
  return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def population(rng, n, which):
  if which == "first, moderate":
    bw, bh = log_uniform(rng, 0.25, 8.0, n), log_uniform(rng, 0.25, 8.0, n)
  else:
    bw = np.minimum(log_uniform(rng, MINB, HI - LO, n), HI - LO)
    bh = np.minimum(log_uniform(rng, MINB, HI - LO, n), HI - LO)
  x0 = LO + rng.random(n) * ((HI - LO) - bw)
  if which == "cond":
    t0, t1 = rng.uniform(-3, 40, n), rng.uniform(-3, 40, n)
    d0, d1 = np.logaddexp(0, t0) + MINS, np.logaddexp(0, t1) + MINS
  elif which == "first, moderate":
    d0, d1 = log_uniform(rng, 0.05, 20.0, n), log_uniform(rng, 0.05, 20.0, n)
  else:
    d0, d1 = log_uniform(rng, MINS, 40.0, n), log_uniform(rng, MINS, 40.0, n)
  w = rng.random(n)
  w[: n // 64] = 0.0; w[n // 64: n // 32] = 1.0           # both ends of the bin
  return x0, bw, bh, d0, d1, w


def main():
  n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
  rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
  ok = True
  for which in ("cond", "first", "first, moderate"):
    x0, bw, bh, d0, d1, w = population(rng, n, which)
    if which == "cond":               # the kernel's own float32 values are the inputs of both forms and of float64
      x0, bw, bh, d0, d1 = (a.astype(f32) for a in (x0, bw, bh, d0, d1))
      s = bh * rcp(bw)
      st = d1 + d0 - s * f32(2)
      dy = (w * bh.astype(f64)).astype(f32)
      tab = None
      e = [a.astype(f64) for a in (dy, bh, s, st, d0)]
      e[2] = e[1] / bw.astype(f64); e[3] = d1.astype(f64) + e[4] - 2.0 * e[2]
      x0e, bwe = x0.astype(f64), bw.astype(f64)
    else:                             # float64 parameters, rounded once per table field
      s64 = bh / bw
      st64 = d1 + d0 - 2.0 * s64
      tab = tuple(a.astype(f32) for a in (d0 * bh, s64 * bh))
      s = s64.astype(f32)
      tab = tab + (f32(2) * s, f32(4) * s)
      st = st64.astype(f32)
      dy = np.minimum((w * bh).astype(f32), bh.astype(f32))
      e = [dy.astype(f64), bh, s64, st64, d0]
      x0e, bwe = x0, bw
      x0, bw, bh, d0 = (a.astype(f32) for a in (x0, bw, bh, d0))
    ze = exact_root(*e)
    oute = x0e + bwe * ze
    res = {}
    for name, z in (("parent   ", parent_form(dy, bh, s, st, d0)), ("prescaled", prescaled_form(dy, bh, s, st, d0, tab))):
      out = fma(bw, z, x0)
      res[name] = (z, out, np.abs(z.astype(f64) - ze).max(), np.abs(out.astype(f64) - oute).max())
    (zp, op, ezp, eop), (zn, on, ezn, eon) = res["parent   "], res["prescaled"]
    print(f"{which}: {n} samples")
    for name in res:
      print(f"  {name}: max |z - float64| {res[name][2]:.3e}   max |out - float64| {res[name][3]:.3e}   "
            f"negative discriminants {NEG[name]}")
    print(f"  forms differ: z by at most {np.abs(zp.astype(f64) - zn).max():.3e}, out by at most "
          f"{np.abs(op.astype(f64) - on).max():.3e}; bitwise equal in {np.mean(op == on) * 100:.2f} % of the samples")
    good = eon <= eop + SPACING_AT_10 and ezn <= ezp + 2.0 ** -23
    print(f"  bar: out {eon:.3e} <= {eop:.3e} + 9.5e-7 and z {ezn:.3e} <= {ezp:.3e} + 1.2e-7: {'met' if good else 'MISSED'}")
    ok &= good
    # the same where neither form lost its discriminant to cancellation (a knot slope far below the bin's own slope,
    # disc << b^2): there the largest error is the lost root's, the same in both forms, and hides everything else
    both = POS["parent   "] & POS["prescaled"]
    only_p, only_n = int((~POS["parent   "] & POS["prescaled"]).sum()), int((POS["parent   "] & ~POS["prescaled"]).sum())
    print(f"  discriminant negative in the parent form only: {only_p}, in the prescaled form only: {only_n}, in both: "
          f"{int((~POS['parent   '] & ~POS['prescaled']).sum())}")
    sub = [np.abs(r[1].astype(f64) - oute)[both].max() for r in (res["parent   "], res["prescaled"])]
    subz = [np.abs(r[0].astype(f64) - ze)[both].max() for r in (res["parent   "], res["prescaled"])]
    good = sub[1] <= sub[0] + SPACING_AT_10 and subz[1] <= subz[0] + 2.0 ** -23
    print(f"  discriminant positive in both forms ({both.sum()} samples): out {sub[1]:.3e} <= {sub[0]:.3e} + 9.5e-7 "
          f"and z {subz[1]:.3e} <= {subz[0]:.3e} + 1.2e-7: {'met' if good else 'MISSED'}")
    ok &= good
    # and where the quadratic is well conditioned in float64 itself, disc >= 2^-10 b^2: the rounding of the forms alone
    c64, b64 = -e[2] * e[0], e[4] * e[1] - e[3] * e[0]
    well = b64 * b64 - 4.0 * (e[2] * e[1] - b64) * c64 >= 2.0 ** -10 * b64 * b64
    sub = [np.abs(r[1].astype(f64) - oute)[well].max() for r in (res["parent   "], res["prescaled"])]
    subz = [np.abs(r[0].astype(f64) - ze)[well].max() for r in (res["parent   "], res["prescaled"])]
    good = sub[1] <= sub[0] + SPACING_AT_10 and subz[1] <= subz[0] + 2.0 ** -23
    print(f"  disc >= 2^-10 b^2 in float64 ({well.sum()} samples): out {sub[1]:.3e} <= {sub[0]:.3e} + 9.5e-7 "
          f"and z {subz[1]:.3e} <= {subz[0]:.3e} + 1.2e-7: {'met' if good else 'MISSED'}")
    ok &= good
    if tab is not None:
      z4 = four_field_form(dy, st, tab)
      print(f"  four-field: max |z - float64| {np.abs(z4.astype(f64) - ze).max():.3e}   max |out - float64| "
            f"{np.abs(fma(bw, z4, x0).astype(f64) - oute).max():.3e}")
  return 0 if ok else 1


if __name__ == "__main__":
  sys.exit(main())
