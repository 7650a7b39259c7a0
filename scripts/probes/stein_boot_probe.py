"""cnf_stein_boot (the wild-bootstrap test of the kernel Stein discrepancy) at P = 256 sign vectors and two
terms, beside
  (a) the torch composition: the Stein kernel matrix H materialised in float32 in row chunks (cdist^2 and three matmuls
      for the inner products, then the powers or the exponentials), H @ E by torch.matmul and the signed sums; timed on
      ONE set and scaled by S (`composed_scaled_from_one_set`), and
  (b) cnf_mmd_perm at the same pooled size n = N, the same P and D, with two Gaussian bandwidths: the same matrix work
      with the cheaper pair value.
Shapes: 9 sets of 8 192 points and 1 set of 32 768 points, at D = 2 and D = 10, IMQ and Gaussian.

Timing: HIP events around one call after --warmup rounds; the routes are timed INTERLEAVED (one run of each in turn,
--runs of them) and the medians are reported with min and max.  Pairs: S N^2.  `mfma_fraction`: 2 N^2 P S flop over the
time, as a fraction of the f32-MFMA ceiling of 157.3 TFLOP/s.  `fused_slowest_beats_composed_fastest` is the one
condition on the unit.  One JSON line per case; --out FILE writes all.

  python scripts/probes/stein_boot_probe.py --out profiles/stein_boot/stein_boot_probe.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interaction_probe import interleaved_ms
from cnf_ot_amd import _capi, utils
from cnf_ot_amd.flows import _stream_ptr

P = 256
CEILING = 157.3e12
CASES = [(9, 8192, 2), (9, 8192, 10), (1, 32768, 2), (1, 32768, 10)]      # (S, N, D)
KINDS = ["imq", "gaussian"]
BETA = -0.5


def boot_call(dev, spec, x, s, words):
  S, N, D = x.shape
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_stein_boot_workspace(S, N, D, P, ctypes.byref(nbytes)), "cnf_stein_boot_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  stats = torch.empty(S, P, dtype=torch.float64, device=dev)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_stein_boot(ctypes.byref(spec), S, x.data_ptr(), s.data_ptr(), N, D, words.data_ptr(), P,
                                   stats.data_ptr(), None, ws.data_ptr(), nbytes.value, stream), "cnf_stein_boot")
  return run, stats, nbytes.value


def perm_call(dev, spec, x, y, words):
  (S, N, D), M = x.shape, y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_perm_workspace(S, N, M, D, P, ctypes.byref(nbytes)), "cnf_mmd_perm_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  stats = torch.empty(S, P, dtype=torch.float64, device=dev)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_mmd_perm(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, words.data_ptr(), P,
                                 stats.data_ptr(), None, ws.data_ptr(), nbytes.value, stream), "cnf_mmd_perm")
  return run


def composed_set(x, s, signs, bws, kind, rows):
  """q [P] = e' H e of ONE set in float32: H in chunks of `rows` rows, H @ signs by matmul"""
  N, D = x.shape
  q = torch.zeros(signs.shape[1], dtype=torch.float64, device=x.device)
  xs = (x * s).sum(1)
  for i0 in range(0, N, rows):
    xi, si = x[i0:i0 + rows], s[i0:i0 + rows]
    d2 = torch.cdist(xi, x) ** 2
    ss = si @ s.T
    # d . (s_j - s_i) with d = x_i - x_j, from inner products
    dds = xi @ s.T - xs[i0:i0 + rows, None] - xs[None, :] + si @ x.T
    p0, p1, p2 = torch.zeros_like(d2), torch.zeros_like(d2), torch.zeros_like(d2)
    for bw in bws:
      if kind == "imq":
        u = d2 + bw * bw
        t = u ** BETA
        p0 += t
        t = t / u
        p1 += BETA * t
        p2 += BETA * (BETA - 1.0) * (t / u)
      else:
        ib = 0.5 / (bw * bw)
        e = torch.exp(d2 * (-ib))
        p0 += e
        p1 -= ib * e
        p2 += ib * ib * e
    h = p0 * ss + 2.0 * p1 * dds - 4.0 * p2 * d2 - 2.0 * D * p1
    idx = torch.arange(h.shape[0], device=x.device)
    h[idx, i0 + idx] = 0.0
    q += (signs[i0:i0 + rows] * (h @ signs)).sum(0).double()
  return q


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=1)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "stein_boot_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out = []
  for S, N, D in CASES:
    gen = torch.Generator(device=dev).manual_seed(100 * D + S)
    x = 0.1 + 1.05 * torch.randn(S, N, D, device=dev, generator=gen)
    s = -x                                             # the score of N(0, I)
    sw = utils.rademacher_signs(N, P - 1, seed=D)
    words = sw.to(dev)
    plus = ((sw.numpy().view(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(N, P).astype(bool)
    signs = torch.from_numpy(np.where(plus, 1.0, -1.0).astype(np.float32)).to(dev)
    bws = utils.median_bandwidths(x[0].cpu())[2:4]     # two terms: the median distance and twice it
    rows = max(1, min(N, args.chunk_mb * (1 << 20) // (4 * N * 8)))
    # cnf_mmd_perm on the same points as a pooled sample of n = N: the two halves, 255 relabellings
    labels = utils.permutation_labels(N // 2, N - N // 2, P - 1, seed=D).to(dev)
    xa, xb = x[:, :N // 2].contiguous(), x[:, N // 2:].contiguous()
    perm = perm_call(dev, utils.mmd_spec(bws, "gaussian")[0], xa, xb, labels)
    for kind in KINDS:
      spec = utils.stein_spec(kind, bws, BETA)
      bw32 = [float(spec.bw[i]) for i in range(spec.n_terms)]
      boot, stats, ws_bytes = boot_call(dev, spec, x, s, words)
      comp = lambda: composed_set(x[0], s[0], signs, bw32, kind, rows)
      (b_med, b_min, b_max), (c_med, c_min, c_max), (m_med, m_min, m_max) = interleaved_ms([boot, comp, perm], args.runs,
                                                                                             args.warmup)
      boot()
      q0 = comp()
      torch.cuda.synchronize()
      pairs = float(S) * N * N
      row = {"S": S, "N": N, "D": D, "kind": kind, "n_terms": len(bw32), "P": P, "runs": args.runs,
             "boot_ms": b_med, "boot_ms_min": b_min, "boot_ms_max": b_max,
             "composed_ms": c_med * S, "composed_ms_min": c_min * S, "composed_ms_max": c_max * S,
             "composed_scaled_from_one_set": S > 1, "composed_chunk_rows": rows,
             "mmd_perm_ms": m_med, "mmd_perm_ms_min": m_min, "mmd_perm_ms_max": m_max,
             "speedup_over_composed": c_med * S / b_med, "time_over_mmd_perm": b_med / m_med,
             "fused_slowest_beats_composed_fastest": b_max < c_min * S,
             "pairs": pairs, "boot_pairs_per_s": pairs / (b_med * 1e-3), "boot_pair_uses_per_s": pairs * P / (b_med * 1e-3),
             "mfma_fraction": 2.0 * pairs * P / (b_med * 1e-3) / CEILING,
             "mmd_perm_mfma_fraction": 2.0 * pairs * P / (m_med * 1e-3) / CEILING,
             "splits": _capi.lib().cnf_stein_boot_splits(S, N, D), "workspace_bytes": ws_bytes,
             "stat_abs_diff_to_composed_set0": float((stats[0] - q0 / (float(N) * (N - 1.0))).abs().max()),
             "stat_abs_max_set0": float(stats[0].abs().max())}
      print(json.dumps(row), flush=True)
      rows_out.append(row)
      del boot, stats
    del x, s, signs, words, perm, xa, xb, labels
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
