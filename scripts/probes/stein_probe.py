"""cnf_stein (the kernel Stein discrepancy), with and without its gradients, beside its torch
composition -- float32 N x N pair matrices reduced in float64, the gradients in x and in the score by autograd -- and
beside cnf_interaction_vjp with two Gaussian terms on the same clouds, the pair pass it is built like.  Shapes, at D = 2
and 10, both kinds with two terms:
  config3   S = 32 sets of N = 4 096
  eval      S = 9, N = 32 768
Then (--steps) value_and_grad of applications.ksd_loss_fn against a Gaussian target at
  default   dim 2, 2 048 samples, one time
  config4   dim 10, 4 096 samples per time, 32 times

Timing: HIP events around one call after --warmup rounds; the routes are timed INTERLEAVED (one run of each in turn,
--runs of them) and the medians are reported with min and max.  The composition is chunked over rows so that a chunk's
[rows, N, D] differences stay under --chunk-mb; at the eval shape it is timed on ONE of the nine sets and scaled by S
(`composed_scaled_from_one_set`).  Pairs: S N (N - 1).  One JSON line per case; --out FILE writes all.

  python scripts/probes/stein_probe.py --steps --out profiles/stein/stein_probe.json
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
from interaction_probe import KINDS as IA_KINDS, interleaved_ms
from interaction_vjp_probe import vjp_call
from cnf_ot_amd import _capi, applications as app, utils
from cnf_ot_amd.flows import _stream_ptr

SHAPES = {"config3": (32, 4096), "eval": (9, 32768)}
KINDS = {"imq": dict(kind="imq", bandwidths=[1.0, 2.0], weights=[1.0, 0.5], beta=-0.5),
         "gaussian": dict(kind="gaussian", bandwidths=[1.0, 2.0], weights=[1.0, 0.5])}


def stein_call(dev, x, s, kw, want_grad):
  spec = utils.stein_spec(**kw)
  S, N, D = x.shape
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_stein_workspace(S, N, D, int(want_grad), ctypes.byref(nbytes)), "cnf_stein_workspace")
  ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 2, dtype=torch.float64, device=dev)
  gx = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  gs = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  ptr = lambda t: None if t is None else t.data_ptr()
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_stein(ctypes.byref(spec), S, x.data_ptr(), s.data_ptr(), N, D, sums.data_ptr(), None, ptr(gx), ptr(gs),
                              ws.data_ptr(), nbytes.value, stream), "cnf_stein")
  return run, sums, gx, gs, nbytes.value


def _phis(q, kw):
  p = [torch.zeros_like(q) for _ in range(3)]
  for w, b in zip(kw["weights"], kw["bandwidths"]):
    if kw["kind"] == "imq":
      be, u = kw["beta"], q + b * b
      t = w * u ** be
      cs = (1.0, be, be * (be - 1.0))
    else:
      ib, u = 0.5 / (b * b), None
      t = w * torch.exp(-q * ib)
      cs = (1.0, -ib, ib * ib)
    for m in range(3):
      p[m] = p[m] + cs[m] * (t if u is None else t / u ** m)
  return p


def composed_set(x, s, kw, want_grad, rows):
  """(sum over i != j of k_p, (grad_x, grad_s) [N, D] or None) of ONE set: float32 pair matrices reduced in float64, `rows`
  rows at a time; the gradients by autograd (a chunk's rows carry the row side of every pair, the full set the column
  side), times 1 / (N (N - 1))"""
  N, D = x.shape
  total = torch.zeros((), dtype=torch.float64, device=x.device)
  b, sb = x.detach().requires_grad_(want_grad), s.detach().requires_grad_(want_grad)
  for i0 in range(0, N, rows):
    a, sa = b[i0:i0 + rows], sb[i0:i0 + rows]
    d = a[:, None, :] - b[None, :, :]
    ds = sb[None, :, :] - sa[:, None, :]
    q = (d * d).sum(-1)
    p0, p1, p2 = _phis(q, kw)
    kp = p0 * (sa @ sb.T) + 2.0 * p1 * (d * ds).sum(-1) - 4.0 * p2 * q - (2.0 * D) * p1
    idx = torch.arange(len(a), device=x.device)
    mask = torch.ones_like(kp, dtype=torch.bool)
    mask[idx, i0 + idx] = False
    part = torch.where(mask, kp, torch.zeros_like(kp)).double().sum()
    if want_grad:
      (part / (N * (N - 1.0))).backward()
    total = total + part.detach()
  return total, ((b.grad, sb.grad) if want_grad else None)


def kernel_cases(dev, args, rows_out):
  for name in args.shapes:
    S, N = SHAPES[name]
    for D in args.dims:
      gen = torch.Generator(device=dev).manual_seed(10 * D + len(name))
      x = 1.2 * torch.randn(S, N, D, device=dev, generator=gen)
      s = -x + 0.3 * torch.randn(S, N, D, device=dev, generator=gen)
      rows = max(1, min(N, args.chunk_mb * (1 << 20) // (4 * N * D * 10)))      # (autograd keeps ~10 pair tensors)
      n_sets = 1 if name == "eval" else S
      amps, bws = IA_KINDS["gaussian"]
      vjp, _, _ = vjp_call(dev, x, s, "gaussian", amps, bws)
      for kind in args.kinds:
        kw = KINDS[kind]
        plain, sums0, _, _, _ = stein_call(dev, x, s, kw, False)
        grad, sums, gx, gs, ws_bytes = stein_call(dev, x, s, kw, True)
        comp = lambda: [composed_set(x[k], s[k], kw, True, rows) for k in range(n_sets)]
        timed = interleaved_ms([plain, grad, vjp, comp], args.runs, args.warmup)
        (p_med, p_min, p_max), (g_med, g_min, g_max), (v_med, v_min, v_max), (c_med, c_min, c_max) = timed
        c_scale = S / n_sets
        grad()
        torch.cuda.synchronize()
        total, (cx, cs) = composed_set(x[0], s[0], kw, True, rows)
        pairs = S * N * (N - 1.0)
        row = {"case": "kernel", "shape": name, "S": S, "N": N, "D": D, "kind": kind, "n_terms": len(kw["bandwidths"]),
               "runs": args.runs, "stein_ms": p_med, "stein_ms_min": p_min, "stein_ms_max": p_max, "stein_grad_ms": g_med,
               "stein_grad_ms_min": g_min, "stein_grad_ms_max": g_max, "interaction_vjp_ms": v_med,
               "interaction_vjp_ms_min": v_min, "interaction_vjp_ms_max": v_max, "composed_ms": c_med * c_scale,
               "composed_ms_min": c_min * c_scale, "composed_ms_max": c_max * c_scale,
               "composed_scaled_from_one_set": n_sets != S, "composed_chunk_rows": rows,
               "speedup_over_composed": c_med * c_scale / g_med, "pairs": pairs,
               "stein_pairs_per_s": pairs / (p_med * 1e-3), "stein_grad_pairs_per_s": pairs / (g_med * 1e-3),
               "interaction_vjp_pairs_per_s": pairs / (v_med * 1e-3), "grad_rate_over_interaction_vjp": v_med / g_med,
               "plain_rate_over_interaction_vjp": v_med / p_med, "splits": _capi.lib().cnf_stein_splits(S, N, D),
               "workspace_bytes": ws_bytes, "sum_rel_diff_set0": abs(float(sums[0, 0]) - float(total)) / abs(float(total)),
               "grad_x_abs_diff_set0": float((gx[0] - cx).abs().max()), "grad_x_abs_max_set0": float(gx[0].abs().max()),
               "grad_s_abs_diff_set0": float((gs[0] - cs).abs().max()), "grad_s_abs_max_set0": float(gs[0].abs().max())}
        print(json.dumps(row), flush=True)
        rows_out.append(row)


def step_cases(dev, args, rows_out):
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  for name, (D, B, tbs, scale) in {"default": (2, 2048, 1, 0.2), "config4": (10, 4096, 32, 0.12)}.items():
    cfg = FlowConfig(dim=D)
    model, params = FlowModel(cfg), Params.random(cfg, scale, seed=42, device=dev)
    tgt = app.GaussianMixtureTarget(np.full((1, D), 0.5), 1.5)
    conds = np.linspace(0.1, 0.9, tbs).astype(np.float32)
    for kind in args.kinds:
      kw = {k: v for k, v in KINDS[kind].items()}
      vg = app.value_and_grad(lambda p, rng, **k: app.ksd_loss_fn(model, D, p, tgt, conds, rng, B, **kw, **k))
      value = lambda: app.ksd_loss_fn(model, D, params, tgt, conds, 42, B, **kw)
      (a_med, a_min, a_max), (b_med, b_min, b_max) = interleaved_ms([lambda: vg(params, 42), value], args.runs, args.warmup)
      row = {"case": "step", "shape": name, "dim": D, "samples_per_time": B, "times": tbs, "kind": kind, "runs": args.runs,
             "value_and_grad_ms": a_med, "value_and_grad_ms_min": a_min, "value_and_grad_ms_max": a_max, "value_ms": b_med,
             "value_ms_min": b_min, "value_ms_max": b_max}
      print(json.dumps(row), flush=True)
      rows_out.append(row)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=list(KINDS))
  ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
  ap.add_argument("--steps", action="store_true", help="also time value_and_grad of ksd_loss_fn")
  ap.add_argument("--runs", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "stein_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out = []
  kernel_cases(dev, args, rows_out)
  if args.steps:
    step_cases(dev, args, rows_out)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
