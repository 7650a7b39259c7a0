#!/usr/bin/env python3
"""Time the fp particle reference (cnf_fp_particles) against the same ensemble written in torch, and evaluate_fp_path:
  python scripts/exp_fp_particles.py [--particles 1048576] [--steps 1000] [--runs 7] [--out FILE.json]
Workload: N particles x `steps` Euler-Maruyama steps of h = 1 / steps with a 100 x 100 histogram at 5 times, for lorenz
(dim 3) and gradient (dim 2).  Baseline: torch.randn + elementwise float64 steps + torch.histogramdd, as a user would
have written it.  The two are interleaved in one process; the figure is the median of `runs` after one warm-up each,
host clock around a device synchronise.  Then evaluate_fp_path for the default fp figure (random parameters)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnf_ot_amd import FlowConfig, Params, applications as app, solvers      # noqa: E402

DOMAIN = [-2.0, 2.0, -2.0, 2.0]


def torch_drift(x, subtype, a):
  if subtype == "gradient":
    q = (x[:, 0] ** 2 + x[:, 1] ** 2 - 4.0)
    return torch.stack([-q * x[:, 0], -q * x[:, 1] - 2.0 * (x[:, 1] - 1.0)], 1) * a
  X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
  return torch.stack([10.0 * (Y - X), 9.0 * X * (28.0 / 9.0 - Z) - Y, 9.0 * X * Y - Z * 8.0 / 3.0], 1)


def torch_ensemble(dev, subtype, dim, n, steps, snaps, a=1.0, sigma=0.5, var0=1.0):
  h = 1.0 / steps
  x = torch.randn(n, dim, dtype=torch.float64, device=dev) * var0 ** 0.5
  sdn = (2.0 * sigma * h) ** 0.5
  step = 4.0 / 99
  edges = [torch.linspace(-2.0 - step / 2, 2.0 + step / 2, 101, dtype=torch.float64, device=dev)] * 2
  hists = []
  for k in range(steps + 1):
    if k in snaps:
      # torch.histogramdd has no device kernel: the user's version bins by index arithmetic and bincount
      j = torch.floor((x[:, :2] - edges[0][0]) / step).long()
      ok = ((j >= 0) & (j < 100)).all(1)
      hists.append(torch.bincount(j[ok, 1] * 100 + j[ok, 0], minlength=10000))
    if k < steps:
      x = x + h * torch_drift(x, subtype, a) + sdn * torch.randn(n, dim, dtype=torch.float64, device=dev)
  return torch.stack(hists)


def timed(fn, dev):
  torch.cuda.synchronize(dev)
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize(dev)
  return time.perf_counter() - t0


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--particles", type=int, default=1 << 20)
  p.add_argument("--steps", type=int, default=1000)
  p.add_argument("--runs", type=int, default=7)
  p.add_argument("--out", default=None)
  args = p.parse_args()
  dev = torch.device("cuda", 0)
  n, steps = args.particles, args.steps
  h = 1.0 / steps
  snaps = [0, steps // 20, steps // 10, 3 * steps // 10, steps]
  times = [k * h for k in snaps]
  res = {"particles": n, "steps": steps, "runs": args.runs, "cases": {}}
  for subtype, dim in (("lorenz", 3), ("gradient", 2)):
    ours = lambda: app.fp_reference_particles(dim, 1.0, 1.0, 0.5, subtype, times, n, h, seed=3, grid=(DOMAIN, 100))
    theirs = lambda: torch_ensemble(dev, subtype, dim, n, steps, snaps)
    timed(ours, dev), timed(theirs, dev)
    a, b = [], []
    for _ in range(args.runs):
      a.append(timed(ours, dev))
      b.append(timed(theirs, dev))
    r = ours()
    res["cases"][f"{subtype}_d{dim}"] = {
      "hip_ms": [1e3 * t for t in a], "torch_ms": [1e3 * t for t in b], "hip_median_ms": 1e3 * statistics.median(a),
      "torch_median_ms": 1e3 * statistics.median(b), "ratio": statistics.median(b) / statistics.median(a),
      "particle_steps_per_s": n * steps / statistics.median(a), "bad": r["bad"].tolist(),
      "inside_grid": (r["hist"].sum((1, 2)).double() / n).tolist()}
    print(subtype, json.dumps(res["cases"][f"{subtype}_d{dim}"]), flush=True)
  config = solvers.load_config(overrides={"general": {"type": "fp"}})
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  run = lambda: solvers.evaluate_fp_path(config, model, params, n_particles=n, h=h)
  timed(run, dev)
  t = [timed(run, dev) for _ in range(3)]
  res["evaluate_fp_path_default_ms"] = [1e3 * v for v in t]
  print("evaluate_fp_path", res["evaluate_fp_path_default_ms"], flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(res, f, indent=1)


if __name__ == "__main__":
  main()
