"""cnf_mv_particles (the interacting particle reference: per step the pair pass of cnf_interaction and one step launch)
against what it replaces and against what it is built from, in one run:
  composed      per step ONE utils.interaction_field call (query mode on the float32 positions, the force a particle
                method would ask for) and a torch float64 update with torch.randn noise
  interaction   n_steps times ONE cnf_interaction call in self mode WITH the force at the same shape: a step of the
                fused stepper is that call with the finish launch replaced by the step launch, so it should cost about
                one such call
Shape: R = 2 replicas of N = 16 384, D = 2 and D = 10, 1 000 steps of h = 1e-3, drift ou, a Gaussian kernel with two
signed terms (--kernel log: the softened log kernel of the power kind); the fused call takes ONE snapshot, at the last step (sums alone).

Timing: HIP events around the whole of each route (all its steps), after --warmup rounds (default 1); the three routes
are timed INTERLEAVED (one run of each in turn, --runs of them, default 5); medians with min and max; buffers are
allocated once where the route allows it (the composition's per-step tensors are torch's own).  One JSON line per D;
--out FILE writes them all to FILE.

  python scripts/probes/mv_particles_probe.py --out profiles/mv_particles/mv_particles_probe.json
"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from interaction_probe import interleaved_ms
from cnf_ot_amd import _capi, utils
from cnf_ot_amd.flows import _stream_ptr

KERNELS = {"gaussian": dict(kind="gaussian", amplitudes=[1.0, -0.5], bandwidths=[1.0, 2.0]),
           "log": dict(kind="power", amplitudes=[1.0], bandwidths=0.1, exponents=[0.0])}
KERNEL = KERNELS["gaussian"]             # (--kernel replaces it)
A, SIGMA, KAPPA, VAR0 = 1.0, 0.5, 1.5, 1.0


def fused_call(dev, R, N, D, h, steps):
  lib, C = _capi.lib(), ctypes
  spec = utils.interaction_spec(**KERNEL)
  nb = C.c_int64(0)
  _capi.check(lib.cnf_mv_particles_workspace(R, N, D, 1, C.byref(nb)), "cnf_mv_particles_workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  ws, state = torch.empty(nb.value // 8, **f64), torch.empty(R, N, D, **f64)
  sums = torch.empty(1, R, 3 + D + D * D, **f64)
  snap = (C.c_int64 * 1)(steps)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_mv_particles(C.byref(spec), KAPPA, _capi.DRIFTS["ou"], D, A, SIGMA, h, steps, VAR0, 7, 0, R, N,
                                     None, snap, 1, None, state.data_ptr(), None, sums.data_ptr(), None, ws.data_ptr(),
                                     nb.value, stream), "cnf_mv_particles")
  return run, sums, nb.value


def composed_call(dev, R, N, D, h, steps):
  sdn = math.sqrt(2.0 * SIGMA * h)
  scale = KAPPA * N / (N - 1.0)            # query mode averages over N sources; the pair i == i adds no force

  def run():
    x = math.sqrt(VAR0) * torch.randn(R, N, D, dtype=torch.float64, device=dev)
    for _ in range(steps):
      x32 = x.float()
      G = utils.interaction_field(x32, x32, **KERNEL)["force"].double()
      x = x + h * (-A * x - scale * G) + sdn * torch.randn_like(x)
    return x
  return run


def interaction_calls(dev, R, N, D, steps):
  lib, C = _capi.lib(), ctypes
  spec = utils.interaction_spec(**KERNEL)
  nb = C.c_int64(0)
  _capi.check(lib.cnf_interaction_workspace(R, N, 0, D, 1, C.byref(nb)), "cnf_interaction_workspace")
  x = math.sqrt(VAR0) * torch.randn(R, N, D, device=dev)
  ws = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
  sums, force = torch.empty(R, dtype=torch.float64, device=dev), torch.empty(R, N, D, device=dev)
  stream = _stream_ptr(dev)

  def run():
    for _ in range(steps):
      _capi.check(lib.cnf_interaction(C.byref(spec), R, x.data_ptr(), N, None, 0, D, sums.data_ptr(), None, force.data_ptr(),
                                      ws.data_ptr(), nb.value, stream), "cnf_interaction")
  return run


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--replicas", type=int, default=2)
  ap.add_argument("--particles", type=int, default=16384)
  ap.add_argument("--steps", type=int, default=1000)
  ap.add_argument("--h", type=float, default=1e-3)
  ap.add_argument("--kernel", default="gaussian", choices=list(KERNELS))
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=1)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "mv_particles_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  global KERNEL
  KERNEL = KERNELS[args.kernel]
  R, N, steps = args.replicas, args.particles, args.steps
  rows = []
  for D in args.dims:
    fused, sums, ws_bytes = fused_call(dev, R, N, D, args.h, steps)
    (f, f_min, f_max), (c, c_min, c_max), (i, i_min, i_max) = interleaved_ms(
      [fused, composed_call(dev, R, N, D, args.h, steps), interaction_calls(dev, R, N, D, steps)], args.runs, args.warmup)
    pairs = float(R) * N * (N - 1.0) * (steps + 1)
    K = 3 + D + D * D
    row = {"R": R, "N": N, "D": D, "steps": steps, "h": args.h, "kernel": KERNEL, "runs": args.runs,
           "fused_ms": f, "fused_ms_min": f_min, "fused_ms_max": f_max, "fused_us_per_step": 1e3 * f / (steps + 1),
           "composed_ms": c, "composed_ms_min": c_min, "composed_ms_max": c_max, "composed_over_fused": c / f,
           "interaction_calls_ms": i, "interaction_calls_ms_min": i_min, "interaction_calls_ms_max": i_max,
           "interaction_us_per_call": 1e3 * i / steps, "step_over_interaction_call": (f / (steps + 1)) / (i / steps),
           "fused_pairs_per_s": pairs / (f * 1e-3), "splits": _capi.lib().cnf_interaction_splits(R, N, 0, D),
           "workspace_bytes": ws_bytes, "bad": float(sums[0, :, 1].sum()),
           "trace_cov_last": float((sums[0, :, 2 + D:K - 1].reshape(R, D, D).diagonal(dim1=1, dim2=2).sum(1) / N).mean())}
    print(json.dumps(row), flush=True)
    rows.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
      json.dump(rows, fh, indent=1)


if __name__ == "__main__":
  main()
