"""cnf_score (the exact score, one fused forward + reverse pass) against the two routes to a score there were before:
cnf_logprob_fd (the reference's difference quotient, 2 D data -> base passes per point) and the three-step composition
cnf_inverse_logdet -> negation -> cnf_input_vjp(to_base = 1, ybar = -z, ldbar = 1).  Interleaved rounds in one process
after a warm-up, median of 7 with min-max, a timed window of about 20 ms of engine calls ended by a device synchronise
(DESIGN.md 5.3f).  One JSON line per shape; --out FILE also writes them all to FILE.  The three routes do not compute
the same number: the quotient is the reference's approximation of what the other two evaluate."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnf_ot_amd import FlowConfig, FlowEngine, Params

dev = torch.device("cuda", 0)
REPS, CALLS = 7, 20

def timed(fn, calls=CALLS):
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3 / calls

def shape(name, D, scale, n, conds, shared, out):
  cfg = FlowConfig(dim=D)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, scale, seed=100 + D, device=dev))
  c = torch.tensor(conds, dtype=torch.float32, device=dev)
  S = len(conds)
  pts = eng.normal(1, n) * 1.5 if not shared else \
    torch.cartesian_prod(*[torch.linspace(-2, 2, int(round(n ** (1 / D))), device=dev)] * D).contiguous()
  flat = pts.repeat(S, 1) if shared else pts          # the older entry points take one point per (slice, point)
  ones = torch.ones(flat.shape[0], device=dev)
  def composed():
    z, _ = eng.inverse_logdet(flat, c)
    return eng.input_vjp(flat, c, ybar=-z, ldbar=ones, to_base=True)
  routes = {"score": lambda: eng.score(pts, c, shared=shared), "logprob_fd": lambda: eng.logprob_fd(flat, c, 0.01),
            "composed": composed}
  got = {k: f() for k, f in routes.items()}
  scale_ = float(got["score"].abs().max())
  for _ in range(3):
    for f in routes.values():
      f()
  # a timed window of about 20 ms: a call takes 15 .. 250 us, and 20 of them would measure the clock
  calls = {k: int(min(max(20.0 / timed(f), CALLS), 2000)) for k, f in routes.items()}
  t = {k: [] for k in routes}
  for _ in range(REPS):
    for k, f in routes.items():
      t[k].append(timed(f, calls[k]))
  r = {"dim": D, "points": int(flat.shape[0]), "slices": S, "shared_points": bool(shared), "calls_per_window": calls}
  for k, v in t.items():
    r[k + "_ms"] = float(np.median(v)); r[k + "_min_max"] = [min(v), max(v)]
  r["fd_over_score"] = r["logprob_fd_ms"] / r["score_ms"]
  r["composed_over_score"] = r["composed_ms"] / r["score_ms"]
  r["max_abs_score_minus_composed_over_max"] = float((got["score"] - got["composed"]).abs().max()) / scale_
  out[name] = r
  print(name, json.dumps(r), flush=True)

out = {}
shape("dim2_grid_5x100x100", 2, 0.2, 100 * 100, [0.0, 0.5, 1.0, 1.5, 2.0], True, out)
shape("dim2_1M_points", 2, 0.2, 1 << 20, [0.5], False, out)
shape("dim10_32768_points", 10, 0.12, 32768, [0.5], False, out)
if "--out" in sys.argv:
  with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
    json.dump(out, f, indent=1)
