"""cnf_interaction (the interaction energy of all sets, its field and its force: one pair launch and a merge launch)
against its torch composition -- per set a pair matrix from direct differences in float32, reduced in float64, which is
what utils.interaction_energy replaces -- and beside cnf_mmd2 (Gaussian, the same number of terms, with its gradient) on
the same clouds, whose pair loop this one is built from.  Shapes, at D = 2 and D = 10 and for the kinds of KINDS (Gaussian
and exponential with two signed terms, quadratic, and the power kind: exponents 4 and 1, and the log kernel):
  config3   S = 32 sets of N = 4 096 (batch 131 072 // 32 at 32 time slices), with the force: the training term's call
  default   S = 1, N = 64 (batch 2 048 // 32 at one slice), with the force: this measures launch overheads, not pairs
  eval      S = 9, N = 32 768: solvers.evaluate_interaction's shape at n = 65 536; the energy alone
(--shapes also takes config3x2, S = 64 sets of 4 096, and eval_force, the eval shape with the force: what the rates of the
three are read against.)

Timing: HIP events around one call after --warmup rounds (default 2); the fused call, the composition and cnf_mmd2 are
timed INTERLEAVED (one run of each in turn, --runs of them, default 11) and the medians are reported with min and max;
inputs are random, workspaces and outputs are allocated once.  The composition is chunked over rows so that a chunk's
[rows, N, D] differences stay under --chunk-mb (default 1 024 MB); at the eval shape it is timed on ONE of the nine sets
(the sets are independent: the loop over them repeats the same work) and `composed_ms` is that time times S, marked
`composed_scaled_from_one_set`.  Pair counts: S N (N - 1) for cnf_interaction, S (N (N - 1) + M (M - 1) + N M) with M = N
for cnf_mmd2.  One JSON line per case; --out FILE writes them all to FILE.

  python scripts/probes/interaction_probe.py --out profiles/interaction/interaction_probe.json
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

# (S, N, with the force); config3x2: twice config3's sets, for reading fixed costs apart from the pair rate (not a default)
SHAPES = {"config3": (32, 4096, True), "default": (1, 64, True), "eval": (9, 32768, False), "config3x2": (64, 4096, True),
          "eval_force": (9, 32768, True)}
DEFAULT_SHAPES = ["config3", "default", "eval"]
# kind -> (amplitudes, bandwidths); "power" and "power_log" are the spec kind "power" with POWER_EXPONENTS and ONE
# softening length: an attractive-repulsive pair r^4 / 4 - r and the log kernel
KINDS = {"gaussian": ([1.0, -0.5], [1.0, 2.0]), "exponential": ([1.0, -0.5], [0.5, 2.0]), "quadratic": ([1.0], None),
         "power": ([1.0, -1.0], [0.05]), "power_log": ([1.0], [0.1])}
POWER_EXPONENTS = {"power": [4.0, 1.0], "power_log": [0.0]}


def spec_kwargs(kind, amps, bws):
  """utils.interaction_spec's arguments for a kind of KINDS"""
  if kind in POWER_EXPONENTS:
    return dict(kind="power", amplitudes=amps, bandwidths=bws, exponents=POWER_EXPONENTS[kind])
  return dict(kind=kind, amplitudes=amps, bandwidths=bws)


def power_terms(d2, kind, amps, bws):
  """(W, w) of a power kind at the squared distances d2 (torch, float32): grad W = diff w"""
  u = d2 + bws[0] * bws[0]
  W, w = torch.zeros_like(d2), torch.zeros_like(d2)
  for a, p in zip(amps, POWER_EXPONENTS[kind]):
    W = W + (0.5 * a * torch.log(u) if p == 0.0 else (a / p) * u ** (0.5 * p))
    w = w + a * u ** (0.5 * p - 1.0)
  return W, w


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


def fused_call(dev, x, kind, amps, bws, want_force):
  spec = utils.interaction_spec(**spec_kwargs(kind, amps, bws))
  S, N, D = x.shape
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_interaction_workspace(S, N, 0, D, int(want_force), ctypes.byref(nbytes)), "cnf_interaction_workspace")
  ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  sums = torch.empty(S, dtype=torch.float64, device=dev)
  force = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_force else None
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_interaction(ctypes.byref(spec), S, x.data_ptr(), N, None, 0, D, sums.data_ptr(), None,
                                    None if force is None else force.data_ptr(), ws.data_ptr(), nbytes.value, stream),
                "cnf_interaction")
  return run, (sums, force), nbytes.value


def mmd_call(dev, x, y, n_terms):
  spec, _ = utils.mmd_spec([1.0, 2.0, 4.0, 8.0][:n_terms], "gaussian")
  S, N, D = x.shape
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_workspace(S, N, N, D, 1, ctypes.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev)
  stream = _stream_ptr(dev)

  def run():
    _capi.check(lib.cnf_mmd2(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), N, D, sums.data_ptr(), grad.data_ptr(),
                             ws.data_ptr(), nbytes.value, stream), "cnf_mmd2")
  return run


def composed_set(x, kind, amps, bws, want_force, rows):
  """(sum over i != j of W, force [N, D] or None) of ONE set: float32 pair matrices reduced in float64, `rows` rows at
  a time"""
  N = len(x)
  total = torch.zeros((), dtype=torch.float64, device=x.device)
  force = torch.empty_like(x) if want_force else None
  for i0 in range(0, N, rows):
    diff = x[i0:i0 + rows, None, :] - x[None, :, :]
    d2 = (diff * diff).sum(-1)
    if kind == "quadratic":
      W, w = (0.5 * amps[0]) * d2, None
    elif kind in POWER_EXPONENTS:
      W, w = power_terms(d2, kind, amps, bws)
    else:
      W, w = torch.zeros_like(d2), torch.zeros_like(d2)
      r = torch.sqrt(d2) if kind == "exponential" else None
      for a, b in zip(amps, bws):
        e = a * (torch.exp(d2 * (-0.5 / (b * b))) if kind == "gaussian" else torch.exp(r * (-1.0 / b)))
        W = W + e
        if want_force:
          w = w - e * (1.0 / (b * b) if kind == "gaussian" else 1.0 / b)
      if want_force and kind == "exponential":
        w = torch.where(r > 0, w / r, torch.zeros_like(w))
    idx = torch.arange(len(W), device=x.device)
    W[idx, i0 + idx] = 0.0
    total += W.double().sum()
    if want_force:
      f = (diff * (amps[0] if w is None else w[:, :, None])).double().sum(1)
      force[i0:i0 + rows] = (f / (N - 1.0)).float()
  return total, force


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", type=int, nargs="+", default=[2, 10])
  ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=list(KINDS))
  ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, choices=list(SHAPES))
  ap.add_argument("--runs", type=int, default=11)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--chunk-mb", type=int, default=1024)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), "interaction_probe measures on the GPU; there is no fall-back"
  dev = torch.device("cuda", 0)
  rows_out = []
  for name in args.shapes:
    S, N, want_force = SHAPES[name]
    for D in args.dims:
      g = torch.Generator(device=dev).manual_seed(10 * D + len(name))
      x = 1.2 * torch.randn(S, N, D, device=dev, generator=g)
      y = 0.3 + torch.randn(S, N, D, device=dev, generator=g)
      rows = max(1, min(N, args.chunk_mb * (1 << 20) // (4 * N * D)))
      n_sets = 1 if name.startswith("eval") else S
      for kind in args.kinds:
        amps, bws = KINDS[kind]
        n_terms = len(amps)
        run, (sums, force), ws_bytes = fused_call(dev, x, kind, amps, bws, want_force)
        mmd = mmd_call(dev, x, y, n_terms)
        comp = lambda: [composed_set(x[s], kind, amps, bws, want_force, rows) for s in range(n_sets)]
        (f_med, f_min, f_max), (c_med, c_min, c_max), (m_med, m_min, m_max) = interleaved_ms([run, comp, mmd], args.runs,
                                                                                               args.warmup)
        c_scale = S / n_sets
        # the two routes agree (set 0)
        ref_sum, ref_force = composed_set(x[0], kind, amps, bws, want_force, rows)
        run()
        torch.cuda.synchronize()
        d_sum = abs(float(sums[0]) - float(ref_sum)) / (N * (N - 1.0))
        d_force = float((force[0] - ref_force).abs().max()) if want_force else None
        pairs = S * N * (N - 1.0)
        m_pairs = S * (2.0 * N * (N - 1.0) + float(N) * N)
        row = {"shape": name, "S": S, "N": N, "D": D, "kind": kind, "n_terms": n_terms, "force": want_force, "runs": args.runs,
               "fused_ms": f_med, "fused_ms_min": f_min, "fused_ms_max": f_max, "composed_ms": c_med * c_scale,
               "composed_ms_min": c_min * c_scale, "composed_ms_max": c_max * c_scale,
               "composed_scaled_from_one_set": n_sets != S, "composed_chunk_rows": rows, "speedup": c_med * c_scale / f_med,
               "pairs": pairs, "fused_pairs_per_s": pairs / (f_med * 1e-3), "mmd2_ms": m_med, "mmd2_ms_min": m_min,
               "mmd2_ms_max": m_max, "mmd2_pairs": m_pairs, "mmd2_pairs_per_s": m_pairs / (m_med * 1e-3),
               "rate_over_mmd2": (pairs / f_med) / (m_pairs / m_med), "splits": _capi.lib().cnf_interaction_splits(S, N, 0, D),
               "workspace_bytes": ws_bytes, "pair_mean_abs_diff_set0": d_sum, "force_abs_diff_set0": d_force}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
  main()
