"""cnf_knn (the k nearest neighbours of x in x and in y over all sets: one scan launch, a merge and a sum launch)
against its torch composition, torch.cdist + torch.topk(largest=False) per set and block -- what utils.knn replaces --
and beside cnf_mmd2's energy kernel on the same clouds, whose pair loop the scan is built from.  Shapes: the siblings'
training shape S = 8, N = M = 2 048 and evaluation shape S = 9, N = M = 32 768; D = 2 and D = 10; k = 4 and k = 16.

Timing: HIP events around one call after a warm-up; the fused call and the composition are timed INTERLEAVED (one run
of each in turn, --runs of them, default 11) and the medians are reported with min and max; inputs are random, the
workspace and outputs are allocated once.  The composition is chunked over rows so that a chunk's [rows, M] distance
matrix stays under --chunk-mb (default 1 024 MB); at the evaluation shape it is timed on ONE of the nine sets (the sets
are independent: the loop over them repeats the same work) and `composed_ms` is that time times S, marked
`composed_scaled_from_one_set`.  One JSON line per case; --out FILE writes them all to FILE.

  python scripts/probes/knn_probe.py --dims 2 10 --out profiles/knn/knn_probe.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cnf_ot_amd import _capi, utils
from cnf_ot_amd.flows import _stream_ptr

SHAPES = {"train": (8, 2048, 2048), "eval": (9, 32768, 32768)}


def interleaved_ms(fns, runs, warmup):
  """[(median, min, max)] per function, one run of each in turn"""
  for _ in range(warmup):
    for fn in fns:
      fn()
  torch.cuda.synchronize()
  out = [[] for _ in fns]
  for _ in range(runs):
    for fn, times in zip(fns, out):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      b.synchronize()
      times.append(a.elapsed_time(b))
  return [(statistics.median(t), min(t), max(t)) for t in out]


def fused_call(dev, x, y, k):
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_knn_workspace(S, N, M, D, k, ctypes.byref(nbytes)), "cnf_knn_workspace")
  ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 2, k, 2, dtype=torch.float64, device=dev)
  dxx, dxy = (torch.empty(S, N, k, dtype=torch.float32, device=dev) for _ in range(2))
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_knn(S, x.data_ptr(), N, y.data_ptr(), M, D, k, dxx.data_ptr(), None, dxy.data_ptr(), None,
                            sums.data_ptr(), ws.data_ptr(), nbytes.value, stream), "cnf_knn")
  return run, (dxx, dxy, sums), nbytes.value


def energy_call(dev, x, y):
  spec, _ = utils.mmd_spec(None, "energy")
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_workspace(S, N, M, D, 0, ctypes.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_mmd2(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, sums.data_ptr(), None, ws.data_ptr(),
                             nbytes.value, stream), "cnf_mmd2")
  return run


def composed_set(x, y, k, rows):
  """(dist_xx [N, k], dist_xy [N, k]) of ONE set: cdist + topk, chunked over `rows` rows"""
  N = len(x)
  dxx, dxy = (torch.empty(N, k, dtype=torch.float32, device=x.device) for _ in range(2))
  for i0 in range(0, N, rows):
    d = torch.cdist(x[i0:i0 + rows], x)
    idx = torch.arange(len(d), device=x.device)
    d[idx, i0 + idx] = float("inf")
    dxx[i0:i0 + rows] = torch.topk(d, k, dim=1, largest=False).values
    dxy[i0:i0 + rows] = torch.topk(torch.cdist(x[i0:i0 + rows], y), k, dim=1, largest=False).values
  return dxx, dxy


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--ks", type=int, nargs="+", default=[4, 16])
  ap.add_argument("--shapes", nargs="+", default=["train", "eval"], choices=list(SHAPES))
  ap.add_argument("--runs", type=int, default=11)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "knn_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out = []
  for name in args.shapes:
    S, N, M = SHAPES[name]
    for D in args.dims:
      g = torch.Generator(device=dev).manual_seed(10 * D + len(name))
      x = torch.randn(S, N, D, device=dev, generator=g)
      y = 0.3 + 1.2 * torch.randn(S, M, D, device=dev, generator=g)
      rows = max(1, min(N, args.chunk_mb * (1 << 20) // (4 * max(N, M))))
      n_sets = 1 if name == "eval" else S
      energy = energy_call(dev, x, y)
      for k in args.ks:
        run, (dxx, dxy, sums), ws_bytes = fused_call(dev, x, y, k)
        comp = lambda: [composed_set(x[s], y[s], k, rows) for s in range(n_sets)]
        (f_med, f_min, f_max), (c_med, c_min, c_max), (e_med, e_min, e_max) = interleaved_ms([run, comp, energy], args.runs,
                                                                                               args.warmup)
        c_scale = S / n_sets
        # the two routes agree (set 0): cdist goes through a matrix product at these sizes, so to its accuracy only
        ref_xx, ref_xy = composed_set(x[0], y[0], k, rows)
        run()
        torch.cuda.synchronize()
        diff = max(float((dxx[0] - ref_xx).abs().max()), float((dxy[0] - ref_xy).abs().max()))
        pairs = S * (N * (N - 1.0) + float(N) * M)
        e_pairs = S * (N * (N - 1.0) + M * (M - 1.0) + float(N) * M)
        row = {"shape": name, "S": S, "N": N, "M": M, "D": D, "k": k, "runs": args.runs, "fused_ms": f_med, "fused_ms_min": f_min,
               "fused_ms_max": f_max, "composed_ms": c_med * c_scale, "composed_ms_min": c_min * c_scale,
               "composed_ms_max": c_max * c_scale, "composed_scaled_from_one_set": n_sets != S, "composed_chunk_rows": rows,
               "speedup": c_med * c_scale / f_med, "pairs": pairs, "fused_pairs_per_s": pairs / (f_med * 1e-3),
               "mmd_energy_ms": e_med, "mmd_energy_ms_min": e_min, "mmd_energy_ms_max": e_max,
               "mmd_energy_pairs_per_s": e_pairs / (e_med * 1e-3), "splits": _capi.lib().cnf_knn_splits(S, N, M, D),
               "workspace_bytes": ws_bytes, "dist_abs_diff_set0": diff, "zeros": float(sums[..., 1].sum())}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
