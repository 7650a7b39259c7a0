"""cnf_sliced_w2 (the sliced Wasserstein distance between sample sets: per group of projections one sort launch, the
merge passes, one rank launch and the finishes) against its torch composition on the device -- float32: a matrix
product for the keys, torch.sort, then for N = M the sorted pairing (with the gradient: a scatter through the sort's
indices and a product with the directions) and otherwise the merged-quantile sum -- which is what
utils.sliced_wasserstein replaces.  Shapes, all with P = 64 directions: the training shape S = 8, N = M = 2 048, D = 2
with the gradient; the large-batch shape S = 8, N = M = 131 072, D = 2 with the gradient; the evaluation shape S = 9,
N = M = 524 288, D = 2 and D = 10, values only.  The fused call uses utils.sliced_group's G (the largest group within
1 GiB of workspace).

Timing: HIP events around one call after a warm-up; fused and composed are timed INTERLEAVED (A B A B ...), the median
of --runs runs each with min and max; inputs are random, workspaces and outputs are allocated once.  One JSON line per
case; --out FILE writes them all to FILE.  --pairs: also cnf_mmd2 (Gaussian x 1, value only, one run) and cnf_sinkhorn
(--sinkhorn-iters iterations, one run, reported per pass and scaled to utils.sinkhorn_schedule's default count) at the
evaluation shape, D = 2, the largest of these shapes that all three calls accept.  --lib PATH: measure another build of
the library (an experiment with another SL_TILE).

  python scripts/probes/sliced_probe.py --pairs --out profiles/sliced/sliced_probe.json
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

P = 64
# name -> (S, N, M, dims, with the gradient)
SHAPES = {"train": (8, 2048, 2048, (2,), True), "large": (8, 131072, 131072, (2,), True),
          "eval": (9, 524288, 524288, (2, 10), False)}


def ab_ms(fa, fb, runs, warmup):
  """(median, min, max) of fa and of fb, timed alternately with device events"""
  for _ in range(warmup):
    fa()
    fb()
  torch.cuda.synchronize()
  out = ([], [])
  for _ in range(runs):
    for k, fn in enumerate((fa, fb)):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      b.synchronize()
      out[k].append(a.elapsed_time(b))
  return tuple((statistics.median(v), min(v), max(v)) for v in out)


def fused_call(dev, x, y, theta, want_grad):
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  G, nbytes = utils.sliced_group(S, N, M, D, P, want_grad)
  ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
  sums = torch.empty(S, P + 2, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_sliced_w2(S, x.data_ptr(), N, y.data_ptr(), M, D, theta.data_ptr(), P, G, sums.data_ptr(),
                                  None if grad is None else grad.data_ptr(), ws.data_ptr(), nbytes, stream), "cnf_sliced_w2")
  return run, sums, grad, G, nbytes


def composed(x, y, theta, want_grad):
  """All sets in torch float32: (w [S, P] float64, grad [S, N, D] or None)"""
  S, N, _ = x.shape
  M = y.shape[1]
  kx, ky = (x @ theta.T).transpose(1, 2).contiguous(), (y @ theta.T).transpose(1, 2).contiguous()      # [S, P, n]
  sx, px = torch.sort(kx, dim=2)
  sy, _ = torch.sort(ky, dim=2)
  if N == M:
    diff = sx - sy
    w = 0.5 * (diff * diff).mean(2)
    a_rank = diff / N
  else:
    cuts = torch.unique(torch.cat([torch.arange(N, device=x.device) * M, torch.arange(M, device=x.device) * N]))
    length = torch.diff(torch.cat([cuts, torch.tensor([N * M], device=x.device)]))
    ix, iy, o = cuts // M, cuts // N, (length.double() / float(N * M)).float()
    diff = sx[:, :, ix] - sy[:, :, iy]
    w = 0.5 * (o * diff * diff).sum(2)
    a_rank = torch.zeros_like(sx).index_add_(2, ix, o * diff) if want_grad else None
  if not want_grad:
    return w.double(), None
  a = torch.empty_like(a_rank).scatter_(2, px, a_rank)
  return w.double(), torch.einsum("spn,pd->snd", a, theta) / theta.shape[0]


def pair_statistics(dev, x, y, iters):
  """cnf_mmd2 and cnf_sinkhorn on the same clouds, one run each: a dict of times"""
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  stream = _stream_ptr(dev)
  nbytes = ctypes.c_int64(0)

  def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)
  spec, _ = utils.mmd_spec([float(np.sqrt(D))], "gaussian")
  _capi.check(lib.cnf_mmd_workspace(S, N, M, D, 0, ctypes.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  mmd_ms = once(lambda: _capi.check(lib.cnf_mmd2(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, sums.data_ptr(),
                                                 None, ws.data_ptr(), nbytes.value, stream), "cnf_mmd2"))
  del ws
  full = utils.sinkhorn_schedule(x, y, 0.05)
  sched = full[:iters]
  _capi.check(lib.cnf_sinkhorn_workspace(S, N, M, D, ctypes.byref(nbytes)), "cnf_sinkhorn_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 6, dtype=torch.float64, device=dev)
  eps = (ctypes.c_double * len(sched))(*sched)
  sk_ms = once(lambda: _capi.check(lib.cnf_sinkhorn(S, x.data_ptr(), N, y.data_ptr(), M, D, eps, len(sched), sums.data_ptr(),
                                                    None, None, None, ws.data_ptr(), nbytes.value, stream), "cnf_sinkhorn"))
  per_pass = sk_ms / (len(sched) + 1)
  return {"mmd_gaussian_ms": mmd_ms, "sinkhorn_ms_per_pass": per_pass, "sinkhorn_measured_iterations": len(sched),
          "sinkhorn_default_iterations": len(full), "sinkhorn_ms_scaled_to_default": per_pass * (len(full) + 1)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
  ap.add_argument("--runs", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--pairs", action="store_true")
  ap.add_argument("--sinkhorn-iters", type=int, default=5)
  ap.add_argument("--lib", default=None)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "sliced_probe measures on the GPU; there is no fall-back"
  if args.lib:
    _capi.LIB_PATH = os.path.abspath(args.lib)
  dev = torch.device("cuda", 0)
  rows_out = []
  for name in args.shapes:
    S, N, M, dims, want_grad = SHAPES[name]
    for D in dims:
      g = torch.Generator(device=dev).manual_seed(10 * D + len(name))
      x = torch.randn(S, N, D, device=dev, generator=g)
      y = 0.3 + 1.2 * torch.randn(S, M, D, device=dev, generator=g)
      theta = utils.sliced_directions(D, P, 0).to(dev)
      run, sums, grad, G, ws_bytes = fused_call(dev, x, y, theta, want_grad)
      (f_med, f_min, f_max), (c_med, c_min, c_max) = ab_ms(run, lambda: composed(x, y, theta, want_grad), args.runs, args.warmup)
      # the two routes agree
      ref_w, ref_g = composed(x, y, theta, want_grad)
      run()
      torch.cuda.synchronize()
      row = {"shape": name, "S": S, "N": N, "M": M, "D": D, "P": P, "G": G, "with_gradient": want_grad, "runs": args.runs,
             "tile": _capi.lib().cnf_sliced_tile(), "fused_ms": f_med, "fused_ms_min": f_min, "fused_ms_max": f_max,
             "composed_ms": c_med, "composed_ms_min": c_min, "composed_ms_max": c_max, "speedup": c_med / f_med,
             "keys_per_s": S * P * float(N + M) / (f_med * 1e-3), "workspace_bytes": ws_bytes,
             "sw_set0": float(sums[0, P]), "values_max_abs_diff": float((sums[:, :P] - ref_w).abs().max())}
      if want_grad:
        row["N_grad_max_abs_diff"] = float((grad - ref_g).abs().max() * N)
      del ref_w, ref_g
      if args.pairs and name == "eval" and D == 2:
        row.update(pair_statistics(dev, x, y, args.sinkhorn_iters))
      print(json.dumps(row), flush=True)
      rows_out.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
