"""cnf_mmd2 (MMD^2 / energy distance between sample sets, one fused launch plus a finish launch) against its torch
composition: float32, direct coordinate differences, the three pair blocks of every set, the pair matrices reduced in
float64 -- what utils.mmd2 replaces.  Shapes: the training shape S = 8, N = M = 2 048 and the evaluation shape S = 9,
N = M = 32 768; D = 2 and D = 10; the Gaussian sum with 5 bandwidths and the energy kernel; with and without the
gradient in x.

Timing: HIP events around one call, after a warm-up, the median of --runs (default 21) runs with min and max; inputs
are random, the workspace and outputs are allocated once.  The composition is chunked over rows so that a chunk's
[rows, M, D] difference tensor stays under --chunk-mb (default 2 048 MB); at the evaluation shape it is timed on ONE of
the nine sets (the sets are independent: the loop over them repeats the same work) and `composed_ms` is that time
times S, marked `composed_scaled_from_one_set`.  One JSON line per case; --out FILE writes them all to FILE.

  python scripts/probes/mmd_probe.py --dims 2 10 --out profiles/mmd/mmd_probe.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cnf_ot_amd import _capi, utils
from cnf_ot_amd.flows import _stream_ptr

SHAPES = {"train": (8, 2048, 2048), "eval": (9, 32768, 32768)}


def event_ms(fn, runs, warmup):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  out = []
  for _ in range(runs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b))
  return statistics.median(out), min(out), max(out)


def fused_call(dev, x, y, bws, kind, want_grad):
  spec, _ = utils.mmd_spec(bws, kind)
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_workspace(S, N, M, D, int(want_grad), ctypes.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_mmd2(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, sums.data_ptr(),
                             None if grad is None else grad.data_ptr(), ws.data_ptr(), nbytes.value, stream), "cnf_mmd2")
  return run, sums, grad, nbytes.value


def composed_set(x, y, bws, kind, want_grad, rows):
  """(sxx, syy, sxy) and N-scaled-free gradient sums of ONE set, chunked over `rows` rows"""
  def block(a, b, skip, grad):
    total = torch.zeros((), dtype=torch.float64, device=a.device)
    g = torch.empty_like(a, dtype=torch.float64) if grad else None
    for i0 in range(0, len(a), rows):
      diff = a[i0:i0 + rows, None, :] - b[None, :, :]
      d2 = (diff * diff).sum(-1)
      if kind == "energy":
        d = torch.sqrt(d2)
        k = -d
        w = torch.where(d > 0, 1.0 / d, torch.zeros_like(d)) if grad else None
      else:
        k = torch.zeros_like(d2)
        w = torch.zeros_like(d2) if grad else None
        for bw in bws:
          e = torch.exp(d2 * (-0.5 / (bw * bw)))
          k += e
          if grad:
            w += e * (1.0 / (bw * bw))
      if skip:
        n = min(rows, len(a) - i0)
        idx = torch.arange(n, device=a.device)
        k[idx, i0 + idx] = 0.0
      total += k.double().sum()
      if grad:
        g[i0:i0 + rows] = -(diff * w[:, :, None]).double().sum(1)      # (the diagonal's diff is 0)
    return total, g
  sxx, gxx = block(x, x, True, want_grad)
  syy, _ = block(y, y, True, False)
  sxy, gxy = block(x, y, False, want_grad)
  N, M = len(x), len(y)
  g = (2.0 / (N * (N - 1.0)) * gxx - 2.0 / (float(N) * M) * gxy).float() if want_grad else None
  return torch.stack([sxx, syy, sxy]), g


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--shapes", nargs="+", default=["train", "eval"], choices=list(SHAPES))
  ap.add_argument("--runs", type=int, default=21)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--chunk-mb", type=int, default=2048)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "mmd_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out = []
  for name in args.shapes:
    S, N, M = SHAPES[name]
    for D in args.dims:
      g = torch.Generator(device=dev).manual_seed(10 * D + len(name))
      x = torch.randn(S, N, D, device=dev, generator=g)
      y = 0.3 + 1.2 * torch.randn(S, M, D, device=dev, generator=g)
      bws = [float(b) for b in utils.median_bandwidths(y)]
      rows = max(1, min(N, args.chunk_mb * (1 << 20) // (4 * M * D)))
      n_sets = 1 if name == "eval" else S
      for kind in ("gaussian", "energy"):
        for want_grad in (False, True):
          run, sums, grad, ws_bytes = fused_call(dev, x, y, bws, kind, want_grad)
          f_med, f_min, f_max = event_ms(run, args.runs, args.warmup)
          comp = lambda: [composed_set(x[s], y[s], bws, kind, want_grad, rows) for s in range(n_sets)]
          c_med, c_min, c_max = event_ms(comp, args.runs, 2)
          c_scale = S / n_sets
          # the two routes agree (set 0): relative to the sums' own size
          ref_s, ref_g = composed_set(x[0], y[0], bws, kind, want_grad, rows)
          run()
          torch.cuda.synchronize()
          rel = float(((sums[0] - ref_s).abs() / ref_s.abs().clamp_min(1e-30)).max())
          gerr = float((grad[0] - ref_g).abs().max() * N) if want_grad else None
          pairs = S * (N * (N - 1.0) + M * (M - 1.0) + float(N) * M)
          row = {"shape": name, "S": S, "N": N, "M": M, "D": D, "kind": kind, "n_bw": len(bws) if kind == "gaussian" else 0,
                 "grad": want_grad, "runs": args.runs, "fused_ms": f_med, "fused_ms_min": f_min, "fused_ms_max": f_max,
                 "composed_ms": c_med * c_scale, "composed_ms_min": c_min * c_scale, "composed_ms_max": c_max * c_scale,
                 "composed_scaled_from_one_set": n_sets != S, "composed_chunk_rows": rows,
                 "speedup": c_med * c_scale / f_med, "pairs": pairs, "fused_pairs_per_s": pairs / (f_med * 1e-3),
                 "splits": _capi.lib().cnf_mmd_splits(S, N, M, D), "workspace_bytes": ws_bytes,
                 "sums_rel_diff_set0": rel, "N_xgrad_abs_diff_set0": gerr}
          print(json.dumps(row), flush=True)
          rows_out.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
