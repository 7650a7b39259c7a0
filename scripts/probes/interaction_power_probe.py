"""The power kind of the pair units (softened power laws and the log kernel) beside the Gaussian kind, in one process:
cnf_interaction with the force, cnf_interaction_vjp and cnf_mv_particles (profiles/interaction_power/README.md).

Pair rates: the shapes of profiles/interaction's table, S x N = 32 x 4 096 and 9 x 32 768 at D = 2 and 10; the kinds
`power/2` (exponents 4 and 1, amplitudes 1 and -1, eps 0.05), `power/log` (one exponent 0, eps 0.1) and `gaussian/2`
(amplitudes 1 and -0.5, bandwidths 1 and 2), with `gaussian/1` for the one-term comparison: interaction_probe.py's kinds,
launched by its and interaction_vjp_probe.py's calls.  HIP events around one call; after --warmup rounds the kinds are
timed INTERLEAVED (one call of each in turn), --runs calls per round, --rounds rounds (default 5); a round's figure is
the median of its calls, the reported one the median of the rounds, with the rounds' min and max -- the Gaussian
kind's own round-to-round spread is what a ratio is read against.  Pairs: S N (N - 1).

Particles (--particles): cnf_mv_particles at R = 2, N = 16 384, D = 2, 1 000 steps of h = 1e-3 with no drift, the log
kernel beside the Gaussian kernel, wall time around a synchronised call, --rounds times each in turn.

One JSON line per case; --out FILE writes them all to FILE.

  python scripts/probes/interaction_power_probe.py --particles --out profiles/interaction_power/interaction_power_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from interaction_probe import KINDS as PROBE_KINDS, fused_call, spec_kwargs
from interaction_vjp_probe import vjp_call

SHAPES = {"config3": (32, 4096), "eval": (9, 32768)}
# name -> interaction_probe's (kind, amplitudes, bandwidths)
KINDS = {"gaussian/2": ("gaussian",) + PROBE_KINDS["gaussian"], "power/2": ("power",) + PROBE_KINDS["power"],
         "gaussian/1": ("gaussian", [1.0], [1.0]), "power/log": ("power_log",) + PROBE_KINDS["power_log"]}


def rounds_ms(fns, rounds, runs, warmup):
  """Per function the list of its rounds' medians: one call of each in turn, `runs` turns per round"""
  for _ in range(warmup):
    for fn in fns:
      fn()
  torch.cuda.synchronize()
  out = [[] for _ in fns]
  for _ in range(rounds):
    times = [[] for _ in fns]
    for _ in range(runs):
      for fn, t in zip(fns, times):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    for o, t in zip(out, times):
      o.append(statistics.median(t))
  return out


def particles_seconds(kw, strength, R, N, D, steps, h):
  from cnf_ot_amd import applications as app
  T = steps * h
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  res = app.mv_reference_particles(D, T, 0.0, 0.25, "ou", kw, strength, [0.0, T], n_particles=N, replicas=R, h=h, seed=3, var0=1.0)
  torch.cuda.synchronize()
  assert not bool(res["bad"].any())
  return time.perf_counter() - t0


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--runs", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--particles", action="store_true")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  dev = torch.device("cuda", 0)
  rows = []
  names = list(KINDS)
  for shape in args.shapes:
    S, N = SHAPES[shape]
    for D in args.dims:
      gen = torch.Generator(device=dev).manual_seed(100 + D)
      x = torch.randn(S, N, D, device=dev, generator=gen)
      g = torch.randn(S, N, D, device=dev, generator=gen) * 0.75
      pairs = S * N * (N - 1.0)
      for unit, make in (("cnf_interaction+force", lambda k: fused_call(dev, x, *k, True)[0]),
                         ("cnf_interaction_vjp", lambda k: vjp_call(dev, x, g, *k)[0])):
        per = rounds_ms([make(KINDS[k]) for k in names], args.rounds, args.runs, args.warmup)
        med = {k: statistics.median(t) for k, t in zip(names, per)}
        for k, t in zip(names, per):
          base = "gaussian/2" if k.endswith("/2") else "gaussian/1"
          rows.append({"unit": unit, "shape": shape, "S": S, "N": N, "D": D, "kind": k, "rounds": args.rounds, "runs": args.runs,
                       "ms": med[k], "ms_min": min(t), "ms_max": max(t), "gpairs_per_s": pairs / med[k] * 1e-6,
                       "ms_over_gaussian": med[k] / med[base]})
          print(json.dumps(rows[-1]), flush=True)
  if args.particles:
    R, N, D, steps, h = 2, 16384, 2, 1000, 1e-3
    kinds = {k: (spec_kwargs(*KINDS[k]), 1.0) for k in ("power/log", "gaussian/2")}
    secs = {k: [] for k in kinds}
    for k, (kw, s) in kinds.items():
      particles_seconds(kw, s, R, 256, D, 10, h)                 # (warm-up: a small call)
    for _ in range(args.rounds):
      for k, (kw, s) in kinds.items():
        secs[k].append(particles_seconds(kw, s, R, N, D, steps, h))
    for k, t in secs.items():
      rows.append({"unit": "cnf_mv_particles", "R": R, "N": N, "D": D, "steps": steps, "kind": k, "rounds": args.rounds,
                   "seconds": statistics.median(t), "seconds_min": min(t), "seconds_max": max(t)})
      print(json.dumps(rows[-1]), flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      for r in rows:
        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
  main()
