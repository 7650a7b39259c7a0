"""cnf_interaction_vjp (the pair-Hessian pass behind the interacting Fokker-Planck residual) beside cnf_interaction with
the force on the same clouds, whose pair loop it is built from, and against its torch composition: per set the force as
the autograd gradient of the float32 pair energy (create_graph) and a second backward of sum g . f through it -- a double
backward through the N x N x D pair tensor, which is what utils.interaction_force_vjp replaces.  Shapes, at D = 2 and 10
and for interaction_probe's kinds (Gaussian and exponential with two signed terms, quadratic, the power kind):
  config3   S = 32 sets of N = 4 096 (batch 131 072 // 32 at 32 time slices)
  eval      S = 9, N = 32 768
Then (--steps) value_and_grad of the interacting fp step, beside the same configuration without the interaction and
beside the step whose force and force backward are the torch composition, at
  default   dim 2, batch 2 048, one time, drift "gradient" (64 samples per time)
  config4   dim 10, one GPU's 32 768-sample shard, 32 times, drift "ou" (1 024 samples per time)

Timing: HIP events around one call after --warmup rounds; the routes are timed INTERLEAVED (one run of each in turn,
--runs of them) and the medians are reported with min and max.  The composition is chunked over rows so that a chunk's
[rows, N, D] differences stay under --chunk-mb; at the eval shape it is timed on ONE of the nine sets and scaled by S
(`composed_scaled_from_one_set`).  Pairs: S N (N - 1) for both kernels.  One JSON line per case; --out FILE writes all.

  python scripts/probes/interaction_vjp_probe.py --steps --out profiles/interaction_vjp/interaction_vjp_probe.json
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interaction_probe import KINDS, POWER_EXPONENTS, fused_call, interleaved_ms, power_terms, spec_kwargs
from cnf_ot_amd import _capi, applications as app, interaction as ia, utils
from cnf_ot_amd.flows import _stream_ptr

SHAPES = {"config3": (32, 4096), "eval": (9, 32768)}


def vjp_call(dev, x, g, kind, amps, bws):
  spec = ia.interaction_vjp_check_spec(utils.interaction_spec(**spec_kwargs(kind, amps, bws)))
  S, N, D = x.shape
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_interaction_vjp_workspace(S, N, D, ctypes.byref(nbytes)), "cnf_interaction_vjp_workspace")
  ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  xbar = torch.empty(S, N, D, dtype=torch.float32, device=dev)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_interaction_vjp(ctypes.byref(spec), S, x.data_ptr(), g.data_ptr(), N, D, xbar.data_ptr(),
                                        ws.data_ptr(), nbytes.value, stream), "cnf_interaction_vjp")
  return run, xbar, nbytes.value


def _pair_energy(a, b, kind, amps, bws, skip0):
  """sum_i sum_j W(a_i - b_j) in float32 (the pair i0 + i == j set to 0), as autograd sees it"""
  diff = a[:, None, :] - b[None, :, :]
  d2 = (diff * diff).sum(-1)
  if kind == "quadratic":
    W = (0.5 * amps[0]) * d2
  elif kind in POWER_EXPONENTS:            # (eps > 0: the pair i == i is smooth, and masked like the others)
    idx = torch.arange(len(a), device=a.device)
    mask = torch.ones_like(d2, dtype=torch.bool)
    mask[idx, skip0 + idx] = False
    W = torch.where(mask, power_terms(d2, kind, amps, bws)[0], torch.zeros_like(d2))
  else:
    idx = torch.arange(len(a), device=a.device)
    mask = torch.ones_like(d2, dtype=torch.bool)
    mask[idx, skip0 + idx] = False
    arg = d2 if kind == "gaussian" else torch.sqrt(torch.where(mask, d2, torch.ones_like(d2)))
    W = torch.zeros_like(d2)
    for amp, bw in zip(amps, bws):
      W = W + amp * torch.exp(arg * (-0.5 / (bw * bw) if kind == "gaussian" else -1.0 / bw))
    W = torch.where(mask, W, torch.zeros_like(W))
  return W.sum()


def composed_force(x, kind, amps, bws, rows):
  """f [N, D] of ONE set: the autograd gradient of the pair energy over the rows' own leaf, `rows` rows at a time"""
  N = len(x)
  out = torch.empty_like(x)
  for i0 in range(0, N, rows):
    a = x[i0:i0 + rows].detach().requires_grad_(True)
    out[i0:i0 + rows] = torch.autograd.grad(_pair_energy(a, x.detach(), kind, amps, bws, i0), a)[0] / (N - 1.0)
  return out


def composed_vjp(x, g, kind, amps, bws, rows):
  """xbar [N, D] of ONE set: the double backward, `rows` rows at a time (the rows' leaf carries the row side of every
  pair, the full set's leaf the column side)"""
  N = len(x)
  xbar = torch.zeros_like(x)
  for i0 in range(0, N, rows):
    a = x[i0:i0 + rows].detach().requires_grad_(True)
    b = x.detach().requires_grad_(True)
    f = torch.autograd.grad(_pair_energy(a, b, kind, amps, bws, i0), a, create_graph=True)[0] / (N - 1.0)
    ga, gb = torch.autograd.grad((f * g[i0:i0 + rows]).sum(), (a, b))
    xbar[i0:i0 + rows] += ga
    xbar += gb
  return xbar


def kernel_cases(dev, args, rows_out):
  for name in args.shapes:
    S, N = SHAPES[name]
    for D in args.dims:
      gen = torch.Generator(device=dev).manual_seed(10 * D + len(name))
      x = 1.2 * torch.randn(S, N, D, device=dev, generator=gen)
      g = torch.randn(S, N, D, device=dev, generator=gen)
      rows = max(1, min(N, args.chunk_mb * (1 << 20) // (4 * N * D * 8)))      # (the double backward keeps ~8 pair tensors)
      n_sets = 1 if name == "eval" else S
      for kind in args.kinds:
        amps, bws = KINDS[kind]
        vjp, xbar, ws_bytes = vjp_call(dev, x, g, kind, amps, bws)
        force, _, _ = fused_call(dev, x, kind, amps, bws, True)
        comp = lambda: [composed_vjp(x[s], g[s], kind, amps, bws, rows) for s in range(n_sets)]
        (v_med, v_min, v_max), (f_med, f_min, f_max), (c_med, c_min, c_max) = interleaved_ms([vjp, force, comp], args.runs,
                                                                                               args.warmup)
        c_scale = S / n_sets
        vjp()
        torch.cuda.synchronize()
        diff = float((xbar[0] - composed_vjp(x[0], g[0], kind, amps, bws, rows)).abs().max())
        pairs = S * N * (N - 1.0)
        row = {"case": "kernel", "shape": name, "S": S, "N": N, "D": D, "kind": kind, "n_terms": len(amps), "runs": args.runs,
               "vjp_ms": v_med, "vjp_ms_min": v_min, "vjp_ms_max": v_max, "force_ms": f_med, "force_ms_min": f_min,
               "force_ms_max": f_max, "composed_ms": c_med * c_scale, "composed_ms_min": c_min * c_scale,
               "composed_ms_max": c_max * c_scale, "composed_scaled_from_one_set": n_sets != S, "composed_chunk_rows": rows,
               "speedup_over_composed": c_med * c_scale / v_med, "pairs": pairs, "vjp_pairs_per_s": pairs / (v_med * 1e-3),
               "force_pairs_per_s": pairs / (f_med * 1e-3), "vjp_rate_over_force": f_med / v_med,
               "splits": _capi.lib().cnf_interaction_splits(S, N, 0, D), "workspace_bytes": ws_bytes,
               "xbar_abs_diff_set0": diff, "xbar_abs_max_set0": float(xbar[0].abs().max())}
        print(json.dumps(row), flush=True)
        rows_out.append(row)


def step_cases(dev, args, rows_out):
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  for name, (D, B, tbs, sub, scale) in {"default": (2, 2048, 1, "gradient", 0.2), "config4": (10, 32768, 32, "ou", 0.12)}.items():
    cfg = FlowConfig(dim=D)
    model, params = FlowModel(cfg), Params.random(cfg, scale, seed=42, device=dev)
    for kind in args.kinds:
      amps, bws = KINDS[kind]
      kw = spec_kwargs(kind, amps, bws)
      rows = max(1, min(B // 32, args.chunk_mb * (1 << 20) // (4 * (B // 32) * D * 8)))
      loss = lambda p, rng, **k: app.fp_loss_fn(model, D, 1.0, 1.0, 0.5, 0.01, 0.01, tbs, sub, p, rng, 5000.0, B, **k)
      vg = app.value_and_grad(loss)
      with_ia = lambda: vg(params, 42, interaction=(kw, 0.8))
      without = lambda: vg(params, 42)
      fused = (ia.force_of_sets, ia.force_vjp_of_sets)
      torch_force = lambda spec, x3: torch.stack([composed_force(x, kind, amps, bws, rows) for x in x3])
      torch_vjp = lambda spec, x3, g3: torch.stack([composed_vjp(x, g, kind, amps, bws, rows) for x, g in zip(x3, g3)])

      def composed():
        ia.force_of_sets, ia.force_vjp_of_sets = torch_force, torch_vjp
        try:
          return vg(params, 42, interaction=(kw, 0.8))
        finally:
          ia.force_of_sets, ia.force_vjp_of_sets = fused
      (a_med, a_min, a_max), (b_med, b_min, b_max), (c_med, c_min, c_max) = interleaved_ms([with_ia, without, composed],
                                                                                             args.runs, args.warmup)
      (l1, g1), (l2, g2) = with_ia(), composed()
      row = {"case": "step", "shape": name, "dim": D, "batch": B, "t_batch_size": tbs, "samples_per_time": B // 32, "drift": sub,
             "kind": kind, "runs": args.runs, "interacting_ms": a_med, "interacting_ms_min": a_min, "interacting_ms_max": a_max,
             "plain_ms": b_med, "plain_ms_min": b_min, "plain_ms_max": b_max, "composed_ms": c_med, "composed_ms_min": c_min,
             "composed_ms_max": c_max, "over_plain": a_med / b_med, "speedup_over_composed": c_med / a_med,
             "loss_rel_diff_composed": abs(float(l1) - float(l2)) / abs(float(l1)),
             "grad_abs_diff_composed": float((g1.flat - g2.flat).abs().max()), "grad_abs_max": float(g1.flat.abs().max())}
      print(json.dumps(row), flush=True)
      rows_out.append(row)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=list(KINDS))
  ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
  ap.add_argument("--steps", action="store_true", help="also time the interacting fp step")
  ap.add_argument("--runs", type=int, default=11)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "interaction_vjp_probe measures on the GPU; there is no fall-back"
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
