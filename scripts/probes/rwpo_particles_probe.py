"""cnf_rwpo_particles (the particle reference of the rwpo problems: one wave per outer particle over its inner draws, then
the Brownian bridges) against what it replaces and against the random numbers it is made of, in one run:
  composed      a chunked torch float64 composition of the same sums: per chunk of outer particles the inner draws
                (torch.randn), the log-weights, log h, ess, E[X_T | y], the selection by cumulative sum and the bridge's
                moments -- every [chunk, K, D] intermediate through memory
  fill_normal   two cnf_fill_normal calls of N K 4 ceil((D + 1) / 4) elements: the Philox / Box-Muller work of the call's
                two passes with the stores added -- a yardstick, not a bar
  value only    the same call without u: log_h, ess and mean_T alone, one pass over the draws
Shape: N = 16 384 outer particles, K = 4 096 inner draws, D = 2, 6 and 10, the double well (a = 1, T = 1, beta = 4) with
applications.rwpo_proposal, S = 4 times, sums and histogram-free.

Timing: HIP events around the whole of each route, after --warmup rounds (default 1); the routes are timed INTERLEAVED
(one run of each in turn, --runs of them, default 5); medians with min and max; buffers are allocated once where the
route allows it.  One JSON line per D; --out FILE writes them all to FILE.

  python scripts/probes/rwpo_particles_probe.py --out profiles/rwpo_particles/rwpo_particles_probe.json
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from interaction_probe import interleaved_ms
from cnf_ot_amd import _capi, applications as app
from cnf_ot_amd.flows import _stream_ptr

SUB, A, T, BETA, SEED = "double_well", 1.0, 1.0, 4.0, 7
TIMES = (0.0, 0.3, 0.7, 1.0)


def fused_call(dev, N, K, D, with_u):
  lib, C = _capi.lib(), ctypes
  S = len(TIMES)
  prop = app.rwpo_proposal(D, T, BETA, A, SUB)
  centre = np.ascontiguousarray(prop["centre"], dtype=np.float64)
  ts = np.asarray(TIMES, dtype=np.float64)
  nb = C.c_int64(0)
  _capi.check(lib.cnf_rwpo_particles_workspace(N, D, S, C.byref(nb)), "cnf_rwpo_particles_workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  ws = torch.empty(nb.value // 8, **f64)
  log_h, ess, mean_T = torch.empty(N, **f64), torch.empty(N, **f64), torch.empty(N, D, **f64)
  sel, sums = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(S, 2 + D + D * D, **f64)
  u = torch.as_tensor(app.rwpo_selection_uniforms(N, SEED), device=dev)
  dptr = C.POINTER(C.c_double)
  stream = _stream_ptr(dev)
  var0 = app.rwpo_initial_variance(T, BETA)

  def run():
    _capi.check(lib.cnf_rwpo_particles(_capi.POTENTIALS[SUB], D, A, T, BETA, var0, prop["shrink"], prop["prop_var"],
                                       centre.ctypes.data_as(dptr), K, SEED, 0, N, u.data_ptr() if with_u else None,
                                       ts.ctypes.data_as(dptr), S, None, log_h.data_ptr(), ess.data_ptr(), mean_T.data_ptr(),
                                       sel.data_ptr() if with_u else None, None, sums.data_ptr() if with_u else None, None,
                                       ws.data_ptr(), nb.value, stream), "cnf_rwpo_particles")
  return run, log_h, ess


def composed_call(dev, N, K, D, chunk):
  prop = app.rwpo_proposal(D, T, BETA, A, SUB)
  m = torch.as_tensor(prop["centre"], device=dev)
  shrink, pv, s2 = prop["shrink"], prop["prop_var"], 2.0 * T / BETA
  var0 = app.rwpo_initial_variance(T, BETA)
  f64 = dict(dtype=torch.float64, device=dev)
  u_all = torch.as_tensor(app.rwpo_selection_uniforms(N, SEED), device=dev)

  def run():
    sums = torch.zeros(len(TIMES), 2 + D + D * D, **f64)
    log_hs = []
    for i0 in range(0, N, chunk):
      n = min(chunk, N - i0)
      y = math.sqrt(var0) * torch.randn(n, D, **f64)
      mu = shrink * y
      sg = torch.where(torch.randn(n, K, 1, **f64) >= 0, 1.0, -1.0)
      z = mu[:, None, :] + sg * m + math.sqrt(pv) * torch.randn(n, K, D, **f64)
      g = ((z - A) ** 2).sum(-1) * ((z + A) ** 2).sum(-1) * 0.25
      r = z - mu[:, None, :]
      lae = torch.logaddexp(-((r - m) ** 2).sum(-1) / (2 * pv), -((r + m) ** 2).sum(-1) / (2 * pv))
      l = -BETA * g / 2 - ((z - y[:, None, :]) ** 2).sum(-1) / (2 * s2) + 0.5 * D * math.log(pv / s2) - lae + math.log(2.0)
      mx = l.max(1, keepdim=True).values
      e = torch.exp(l - mx)
      tot = e.sum(1)
      w = e / tot[:, None]
      log_hs.append(mx[:, 0] + torch.log(tot) - math.log(K))
      ess = 1.0 / (w * w).sum(1)                             # noqa: F841  (part of the work that is timed)
      mean_T = (w[:, :, None] * z).sum(1)                    # noqa: F841
      sel = torch.searchsorted(torch.cumsum(e, 1), (u_all[i0:i0 + n] * tot)[:, None], right=True).clamp_(max=K - 1)
      zs = torch.gather(z, 1, sel[:, :, None].expand(n, 1, D))[:, 0]
      x, prev = y, 0.0
      for s, t in enumerate(TIMES):
        if t == T:
          x = zs
        else:
          x = x + (t - prev) / (T - prev) * (zs - x) \
            + math.sqrt(2.0 / BETA * (t - prev) * (T - t) / (T - prev)) * torch.randn(n, D, **f64)
        prev = t
        sums[s, 0] += n
        sums[s, 2:2 + D] += x.sum(0)
        sums[s, 2 + D:] += (x[:, :, None] * x[:, None, :]).sum(0).reshape(-1)
    return torch.cat(log_hs), sums
  return run


def fill_calls(dev, N, K, D):
  n = N * K * 4 * (-(-(D + 1) // 4))
  out = torch.empty(n, dtype=torch.float32, device=dev)
  lib, stream = _capi.lib(), _stream_ptr(dev)

  def run():
    for _ in range(2):
      _capi.check(lib.cnf_fill_normal(SEED, 0, n, out.data_ptr(), stream), "cnf_fill_normal")
  return run, n


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 6, 10])
  ap.add_argument("--particles", type=int, default=16384)
  ap.add_argument("--inner", type=int, default=4096)
  ap.add_argument("--chunk", type=int, default=256, help="outer particles per chunk of the torch composition")
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=1)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "rwpo_particles_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  N, K = args.particles, args.inner
  rows = []
  for D in args.dims:
    fused, log_h, ess = fused_call(dev, N, K, D, True)
    value_only, _, _ = fused_call(dev, N, K, D, False)
    fill, n_fill = fill_calls(dev, N, K, D)
    (f, f_min, f_max), (v, v_min, v_max), (c, c_min, c_max), (r, r_min, r_max) = interleaved_ms(
      [fused, value_only, composed_call(dev, N, K, D, args.chunk), fill], args.runs, args.warmup)
    draws = float(N) * K
    row = {"N": N, "K": K, "D": D, "S": len(TIMES), "potential": SUB, "runs": args.runs,
           "fused_ms": f, "fused_ms_min": f_min, "fused_ms_max": f_max,
           "value_only_ms": v, "value_only_ms_min": v_min, "value_only_ms_max": v_max,
           "composed_ms": c, "composed_ms_min": c_min, "composed_ms_max": c_max, "composed_over_fused": c / f,
           "fill_normal_2x_ms": r, "fill_normal_2x_ms_min": r_min, "fill_normal_2x_ms_max": r_max,
           "fill_elements_per_call": n_fill, "fused_over_fill": f / r,
           "fused_draw_evaluations_per_s": 2.0 * draws / (f * 1e-3), "value_only_draws_per_s": draws / (v * 1e-3),
           "true_val": float(-(2.0 / BETA) * log_h.mean()), "ess_median": float(ess.median()), "ess_min": float(ess.min())}
    print(json.dumps(row), flush=True)
    rows.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      json.dump(rows, fh, indent=1)


if __name__ == "__main__":
  main()
