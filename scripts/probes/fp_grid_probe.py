"""cnf_fp_grid_steps (the finite-volume reference of the 2-D fp problems) at K = 1, 2, 4 and 8 steps per launch, against
what else gives a reference density and against a composition of the same step, in one run:
  steps K       the n explicit steps from t = 0 to T (n = ceil(T rate / 0.9)) on the grid, K per launch
  particles     applications.fp_reference_particles at --particles (default 2^20) particles, h = 1e-3, over the same time,
                with its histogram on the same grid: the Monte-Carlo reference this one stands beside
  composed      the same step as torch float64 tensor operations (pad, slice, multiply, subtract); --composed-steps of them
                (default 200) are timed and scaled to n
Shapes: ou at 257^2 and 513^2 over [-6, 6]^2, smile at 257^2 over [-4, 4]^2; a = 1, sigma = 0.5, T = 1, var0 = 1.

Timing: HIP events around the whole of each route, after --warmup rounds (default 1); the routes are timed INTERLEAVED
(one run of each in turn, --runs of them, default 5); medians with min and max.  One JSON line per shape; --out FILE
writes them all to FILE.

  python scripts/probes/fp_grid_probe.py --out profiles/fp_grid/fp_grid_probe.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from interaction_probe import interleaved_ms
from cnf_ot_amd import _capi, applications as app
from cnf_ot_amd.flows import _stream_ptr

A, SIGMA, T, VAR0 = 1.0, 0.5, 1.0, 1.0
SHAPES = (("ou", (-6.0, 6.0, -6.0, 6.0), 257), ("ou", (-6.0, 6.0, -6.0, 6.0), 513), ("smile", (-4.0, 4.0, -4.0, 4.0), 257))


def steps_call(dev, coef, n, dt, n_steps, K, start):
  lib, stream = _capi.lib(), _stream_ptr(dev)
  rho, ws = start.clone(), torch.empty(n * n, dtype=torch.float64, device=dev)

  def run():
    rho.copy_(start)
    _capi.check(lib.cnf_fp_grid_steps(coef.data_ptr(), n, n, dt, n_steps, K, rho.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                      stream), "cnf_fp_grid_steps")
  return run, rho


def composed_call(coef, dt, n_steps, start):
  cxL, cxR, cyL, cyR = coef[:4]
  pad = torch.nn.functional.pad

  def run():
    rho = start
    for _ in range(n_steps):
      p = pad(rho, (1, 1, 1, 1))
      F = cxL * p[1:-1, :-1] - cxR * p[1:-1, 1:]
      G = cyL * p[:-1, 1:-1] - cyR * p[1:, 1:-1]
      rho = rho + dt * ((F[:, :-1] - F[:, 1:]) + (G[:-1, :] - G[1:, :]))
    return rho
  return run


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--particles", type=int, default=1 << 20)
  ap.add_argument("--composed-steps", type=int, default=200)
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=1)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "fp_grid_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows = []
  for sub, box, n in SHAPES:
    grid = (box, n)
    coef = app.fp_grid_coefficients(A, SIGMA, sub, grid)
    rate = float(coef[4])
    n_steps = app.fp_grid_step_count(T, rate)
    dt = T / n_steps
    start = torch.as_tensor(app.fp_grid_initial(app.stats_grid(grid, (0, 1), 2), VAR0), device=dev)
    calls = [steps_call(dev, coef[0], n, dt, n_steps, K, start) for K in app.FP_GRID_K]
    c_steps = min(args.composed_steps, n_steps)
    composed = composed_call(coef, dt, c_steps, start)

    def particles():
      app.fp_reference_particles(2, T, A, SIGMA, sub, [T], args.particles, 1e-3, 0, var0=VAR0, grid=grid)

    res = interleaved_ms([c[0] for c in calls] + [composed, particles], args.runs, args.warmup)
    same = all(c[1].equal(calls[0][1]) for c in calls[1:])
    close = float((composed() - start).abs().max()) > 0.0 if c_steps else True
    row = {"drift": sub, "n": n, "box": box, "n_steps": n_steps, "rate": rate, "runs": args.runs, "bit_identical": same,
           "composed_moves": close}
    for K, (med, lo, hi) in zip(app.FP_GRID_K, res[:4]):
      row[f"k{K}_ms"], row[f"k{K}_ms_min"], row[f"k{K}_ms_max"] = med, lo, hi
      row[f"k{K}_steps_per_s"] = n_steps / (med * 1e-3)
      row[f"k{K}_cells_per_s"] = n_steps * float(n * n) / (med * 1e-3)
    (cm, cl, ch), (pm, pl, ph) = res[4], res[5]
    scale = n_steps / max(c_steps, 1)
    row.update({"composed_steps_timed": c_steps, "composed_ms_scaled": cm * scale, "composed_ms_scaled_min": cl * scale,
                "composed_ms_scaled_max": ch * scale, "particles": args.particles, "particles_ms": pm,
                "particles_ms_min": pl, "particles_ms_max": ph})
    print(json.dumps(row), flush=True)
    rows.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      json.dump(rows, fh, indent=1)


if __name__ == "__main__":
  main()
