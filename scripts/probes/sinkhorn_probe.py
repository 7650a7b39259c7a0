"""cnf_sinkhorn (the Sinkhorn divergence between sample sets: per iteration one pair launch over the four blocks of all
sets and one merge launch) against its torch composition -- float32, direct coordinate differences, logsumexp over the
materialised pair matrices, what utils.sinkhorn replaces -- and beside cnf_mmd2 on the same clouds, whose pair loop is
the same sweep with a sum in place of the log-sum-exp.  Shapes: the training shape S = 8, N = M = 2 048 with 40
iterations (and the gradient), and the evaluation shape S = 5, N = M = 8 192 on utils.sinkhorn_schedule's default at
eps = 0.05 (gradient and map); D = 2 and D = 10.

Timing: HIP events around one call, after a warm-up, the median of --runs (default 11) runs with min and max; inputs
are random, the workspace and outputs are allocated once.  The composition is timed on ONE set for --composed-iters
iterations (the sets are independent and the iterations repeat the same work), chunked over rows so that a chunk's
[rows, M, D] difference tensor stays under --chunk-mb, and `composed_ms` is that time scaled to S sets and
n_iters + 1 passes (`composed_scaled_from`).  pairs_per_s: S (2 N M + N^2 + M^2) (n_iters + 1) pair terms over the fused
time; mmd_pairs_per_s: cnf_mmd2's S (N (N - 1) + M (M - 1) + N M) over its own time, Gaussian x 1 and energy, value
only.  One JSON line per case; --out FILE writes them all to FILE.

  python scripts/probes/sinkhorn_probe.py --out profiles/sinkhorn/sinkhorn_probe.json
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

SHAPES = {"train": (8, 2048, 2048), "eval": (5, 8192, 8192)}


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


def fused_call(dev, x, y, sched, want_map):
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_sinkhorn_workspace(S, N, M, D, ctypes.byref(nbytes)), "cnf_sinkhorn_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 6, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev)
  tmap = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_map else None
  eps = (ctypes.c_double * len(sched))(*sched)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_sinkhorn(S, x.data_ptr(), N, y.data_ptr(), M, D, eps, len(sched), sums.data_ptr(), None,
                                 grad.data_ptr(), None if tmap is None else tmap.data_ptr(), ws.data_ptr(), nbytes.value,
                                 stream), "cnf_sinkhorn")
  return run, sums, grad, nbytes.value


def mmd_call(dev, x, y, bws, kind):
  spec, _ = utils.mmd_spec(bws, kind)
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_workspace(S, N, M, D, 0, ctypes.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  stream = _stream_ptr(dev)
  return lambda: _capi.check(lib.cnf_mmd2(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, sums.data_ptr(), None,
                                          ws.data_ptr(), nbytes.value, stream), "cnf_mmd2")


def composed_set(x, y, sched, rows, final=True):
  """The recursion on ONE set in torch float32: (the four final potentials, the divergence, N xgrad or None)"""
  N, M = len(x), len(y)

  def T(h, a, b, eps, want_map=False):
    out = torch.empty(len(a), dtype=torch.float32, device=a.device)
    bary = torch.empty_like(a) if want_map else None
    for i0 in range(0, len(a), rows):
      diff = a[i0:i0 + rows, None, :] - b[None, :, :]
      arg = (h[None, :] - 0.5 * (diff * diff).sum(-1)) / np.float32(eps)
      out[i0:i0 + rows] = -np.float32(eps) * (torch.logsumexp(arg, 1) - np.float32(np.log(len(b))))
      if want_map:
        bary[i0:i0 + rows] = torch.softmax(arg, 1) @ b
    return (out, bary) if want_map else out

  f, g, p, q = (torch.zeros(n, dtype=torch.float32, device=x.device) for n in (N, M, N, M))
  for e in sched:
    f, g, p, q = 0.5 * (f + T(g, x, y, e)), 0.5 * (g + T(f, y, x, e)), 0.5 * (p + T(p, x, x, e)), 0.5 * (q + T(q, y, y, e))
  if not final:
    return (f, g, p, q), None, None
  e = sched[-1]
  (fs, txy), (ps, txx) = T(g, x, y, e, True), T(p, x, x, e, True)
  gs, qs = T(f, y, x, e), T(q, y, y, e)
  div = (fs.double().sum() - ps.double().sum()) / N + (gs.double().sum() - qs.double().sum()) / M
  return (fs, gs, ps, qs), div, txx - txy


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--shapes", nargs="+", default=["train", "eval"], choices=list(SHAPES))
  ap.add_argument("--runs", type=int, default=11)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--composed-iters", type=int, default=3)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "sinkhorn_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out = []
  for name in args.shapes:
    S, N, M = SHAPES[name]
    for D in args.dims:
      g = torch.Generator(device=dev).manual_seed(10 * D + len(name))
      x = torch.randn(S, N, D, device=dev, generator=g)
      y = 0.3 + 1.2 * torch.randn(S, M, D, device=dev, generator=g)
      full = utils.sinkhorn_schedule(x, y, 0.05)
      sched = full if name == "eval" else [full[0] * (0.05 / full[0]) ** (k / 29.0) for k in range(30)] + [0.05] * 10
      n_pass = len(sched) + 1
      run, sums, grad, ws_bytes = fused_call(dev, x, y, sched, want_map=name == "eval")
      f_med, f_min, f_max = event_ms(run, args.runs, args.warmup)
      rows = max(1, min(N, args.chunk_mb * (1 << 20) // (4 * M * D)))
      k = min(args.composed_iters, len(sched))
      comp = lambda: composed_set(x[0], y[0], sched[:k], rows, final=False)
      c_med, c_min, c_max = event_ms(comp, 3, 1)
      c_scale = S * n_pass / float(k)
      # the two routes agree (set 0) on the whole schedule
      _, ref_div, ref_g = composed_set(x[0], y[0], sched, rows)
      run()
      torch.cuda.synchronize()
      div = (sums[0, 0] - sums[0, 2]) / N + (sums[0, 1] - sums[0, 3]) / M
      pairs = S * (2.0 * N * M + float(N) * N + float(M) * M)
      row = {"shape": name, "S": S, "N": N, "M": M, "D": D, "iterations": len(sched), "runs": args.runs,
             "fused_ms": f_med, "fused_ms_min": f_min, "fused_ms_max": f_max, "fused_us_per_pass": 1e3 * f_med / n_pass,
             "composed_ms": c_med * c_scale, "composed_ms_min": c_min * c_scale, "composed_ms_max": c_max * c_scale,
             "composed_scaled_from": f"1 set, {k} iterations", "composed_chunk_rows": rows,
             "speedup": c_med * c_scale / f_med, "pairs_per_pass": pairs, "pairs_per_s": pairs * n_pass / (f_med * 1e-3),
             "splits": _capi.lib().cnf_sinkhorn_splits(S, N, M, D), "workspace_bytes": ws_bytes,
             "divergence_set0": float(div), "divergence_abs_diff_set0": abs(float(div) - float(ref_div)),
             "N_xgrad_abs_diff_set0": float((grad[0] - ref_g / N).abs().max() * N),
             "change_set0": [float(v) for v in sums[0, 4:]]}
      mmd_pairs = S * (N * (N - 1.0) + M * (M - 1.0) + float(N) * M)
      for kind, bws in (("gaussian", [float(np.sqrt(D))]), ("energy", None)):
        m_med, _, _ = event_ms(mmd_call(dev, x, y, bws, kind), args.runs, args.warmup)
        row[f"mmd_{kind}_ms"] = m_med
        row[f"mmd_{kind}_pairs_per_s"] = mmd_pairs / (m_med * 1e-3)
      print(json.dumps(row), flush=True)
      rows_out.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
