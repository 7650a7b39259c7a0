"""cnf_mmd_perm (the permutation test of the kernel two-sample statistics) at P = 256 label vectors, beside
  (a) cnf_mmd2, value only, on 32 relabelled copies of one set in one call -- what a user could do before: every pair
      kernel value once per label vector -- SCALED to P vectors and S sets (`mmd2_scaled_from_32_copies_of_one_set`), and
  (b) the torch composition: the pooled kernel matrix K materialised in float32 in row chunks (cdist^2, exp or sqrt), then
      K @ S' by torch.matmul and the signed sums; timed on ONE set and scaled by S (`composed_scaled_from_one_set`).
Shapes: 9 sets of 4 096 + 4 096 points and 1 set of 32 768 + 32 768 points, at D = 2 and D = 10, with the five default
bandwidths and with the energy kernel.

Timing: HIP events around one call after --warmup rounds; the routes are timed INTERLEAVED (one run of each in turn,
--runs of them) and the medians are reported with min and max.  Pairs: S n^2 (the pooled matrix; cnf_mmd2's own count
per copy is N^2 + M^2 + N M).  `mfma_fraction`: 2 n^2 P S flop over the time, as a fraction of the f32-MFMA ceiling of
157.3 TFLOP/s.  One JSON line per case; --out FILE writes all.

  python scripts/probes/mmd_perm_probe.py --out profiles/mmd_perm/mmd_perm_probe.json
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
COPIES = 32
CEILING = 157.3e12
CASES = [(9, 4096, 2), (9, 4096, 10), (1, 32768, 2), (1, 32768, 10)]      # (S, N = M, D)
KINDS = ["gaussian", "energy"]


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
  return run, stats, nbytes.value


def mmd2_call(dev, spec, x, y):
  (S, N, D), M = x.shape, y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_workspace(S, N, M, D, 0, ctypes.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_mmd2(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, sums.data_ptr(), None, ws.data_ptr(),
                             nbytes.value, stream), "cnf_mmd2")
  return run, sums


def composed_set(z, signs, bws, kind, rows):
  """(q [P], r [P], t) of ONE set in float32: K in chunks of `rows` rows, K @ signs by matmul"""
  n = z.shape[0]
  q = torch.zeros(signs.shape[1], dtype=torch.float64, device=z.device)
  r = torch.zeros_like(q)
  t = torch.zeros((), dtype=torch.float64, device=z.device)
  for i0 in range(0, n, rows):
    d2 = torch.cdist(z[i0:i0 + rows], z) ** 2
    if kind == "energy":
      k = -torch.sqrt(d2)
    else:
      k = torch.zeros_like(d2)
      for bw in bws:
        k += torch.exp(d2 * (-0.5 / (bw * bw)))
    idx = torch.arange(k.shape[0], device=z.device)
    k[idx, i0 + idx] = 0.0
    c = k @ signs
    q += (signs[i0:i0 + rows] * c).sum(0).double()
    r += c.sum(0).double()
    t += k.sum().double()
  return q, r, t


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=1)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "mmd_perm_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out = []
  for S, N, D in CASES:
    M, n = N, 2 * N
    gen = torch.Generator(device=dev).manual_seed(100 * D + S)
    x = torch.randn(S, N, D, device=dev, generator=gen)
    y = 0.1 + 1.05 * torch.randn(S, M, D, device=dev, generator=gen)
    labels = utils.permutation_labels(N, M, P - 1, seed=D)
    words = labels.to(dev)
    member = ((labels.numpy().view(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, P).astype(bool)
    signs = torch.from_numpy(np.where(member, 1.0, -1.0).astype(np.float32)).to(dev)
    # 32 relabelled copies of set 0: label vectors 0..31 as gathers of the pooled sample
    z0 = torch.cat([x[0], y[0]])
    order = torch.from_numpy(np.stack([np.concatenate([np.flatnonzero(member[:, p]), np.flatnonzero(~member[:, p])])
                                       for p in range(COPIES)])).to(dev)
    xc, yc = z0[order[:, :N]].contiguous(), z0[order[:, N:]].contiguous()
    bws_default = utils.median_bandwidths(y.cpu())
    rows = max(1, min(n, args.chunk_mb * (1 << 20) // (4 * n * 3)))
    for kind in KINDS:
      spec, bws = utils.mmd_spec(bws_default, kind)
      perm, stats, ws_bytes = perm_call(dev, spec, x, y, words)
      copies, sums = mmd2_call(dev, spec, xc, yc)
      comp = lambda: composed_set(z0, signs, bws, kind, rows)
      (p_med, p_min, p_max), (m_med, m_min, m_max), (c_med, c_min, c_max) = interleaved_ms([perm, copies, comp], args.runs,
                                                                                             args.warmup)
      perm()
      copies()
      torch.cuda.synchronize()
      by_copies = utils.mmd2_from_sums(sums, N, M)
      m_scale, pairs = S * P / float(COPIES), float(S) * n * n
      copy_pairs = float(COPIES) * (N * N + M * M + N * M)
      row = {"S": S, "N": N, "M": M, "D": D, "kind": kind, "n_bw": len(bws), "P": P, "runs": args.runs,
             "perm_ms": p_med, "perm_ms_min": p_min, "perm_ms_max": p_max,
             "mmd2_ms": m_med * m_scale, "mmd2_ms_min": m_min * m_scale, "mmd2_ms_max": m_max * m_scale,
             "mmd2_32_copies_ms": m_med, "mmd2_scaled_from_32_copies_of_one_set": True,
             "composed_ms": c_med * S, "composed_ms_min": c_min * S, "composed_ms_max": c_max * S,
             "composed_scaled_from_one_set": S > 1, "composed_chunk_rows": rows,
             "speedup_over_mmd2_copies": m_med * m_scale / p_med, "speedup_over_composed": c_med * S / p_med,
             "pairs": pairs, "perm_pairs_per_s": pairs / (p_med * 1e-3), "perm_pair_uses_per_s": pairs * P / (p_med * 1e-3),
             "mmd2_pairs_per_s": copy_pairs / (m_med * 1e-3),
             "rate_over_mmd2": pairs * P / (p_med * 1e-3) / (copy_pairs / (m_med * 1e-3)),
             "mfma_fraction": 2.0 * pairs * P / (p_med * 1e-3) / CEILING,
             "splits": _capi.lib().cnf_mmd_perm_splits(S, N, M, D), "workspace_bytes": ws_bytes,
             "stat_abs_diff_to_mmd2_copies_set0": float((stats[0, :COPIES] - by_copies).abs().max()),
             "stat_abs_max_set0": float(stats[0].abs().max())}
      print(json.dumps(row), flush=True)
      rows_out.append(row)
      del perm, copies, stats, sums
    del x, y, xc, yc, z0, signs, words
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
