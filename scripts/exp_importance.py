"""cnf_importance_stats (log Z, KL and ESS of the flow's samples against a closed-form density, one fused launch)
against the composition there was before: model.apply.sample_and_log_prob for every time, then the target's
log-density, the log-weights and their log-sum-exps in torch (float64 from the fp32 samples, as the fused kernel
forms them).  1 M samples x 5 times at dim 2 and dim 10, the noise drawn in the kernel on both routes.  Interleaved
rounds in one process after a warm-up, median of 7 with min-max, a timed window of at least 5 calls and about 40 ms
ended by a device synchronise.  One JSON line per shape; --out FILE also writes them all to FILE."""
import json, math, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnf_ot_amd import FlowConfig, FlowEngine, Params
from cnf_ot_amd import applications as app

dev = torch.device("cuda", 0)
REPS = 7

def timed(fn, calls):
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3 / calls

def shape(name, D, scale, n, conds, tg, out):
  cfg = FlowConfig(dim=D)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, scale, seed=100 + D, device=dev))
  S = len(conds)
  c = torch.tensor(conds, dtype=torch.float32, device=dev)
  mu = torch.from_numpy(tg.means).to(dev)
  W = torch.from_numpy(tg.W).to(dev)
  lw = torch.from_numpy(tg.log_weights).to(dev)
  const = -0.5 * D * math.log(2 * math.pi) + tg.log_det_W
  def fused():
    return eng.importance_stats(tg, t=c, B=n, seed=1)
  def composed():
    y, lq = eng.sample_logprob_seeded(1, S * n, c)          # slice s = samples [s n, (s + 1) n) of the stream: the same draw
    z = (y.double()[:, None, :] - mu[None]) @ W.T            # [S n, M, D]
    lp = torch.logsumexp(lw[None] - 0.5 * (z * z).sum(2), 1) + const
    l = (lp - lq.double()).view(S, n)
    m = l.max(1).values
    e = torch.exp(l - m[:, None])
    return torch.stack([m, e.sum(1), (e * e).sum(1), l.sum(1), torch.full_like(m, n)], 1)
  routes = {"fused": fused, "composed": composed}
  got = {k: app.importance_summary(f()) for k, f in routes.items()}
  for _ in range(3):
    for f in routes.values():
      f()
  calls = {k: int(min(max(40.0 / timed(f, 3), 5), 500)) for k, f in routes.items()}
  t = {k: [] for k in routes}
  for _ in range(REPS):
    for k, f in routes.items():
      t[k].append(timed(f, calls[k]))
  r = {"dim": D, "samples_per_time": n, "times": S, "components": tg.n_comp, "calls_per_window": calls}
  for k, v in t.items():
    r[k + "_ms"] = float(np.median(v)); r[k + "_min_max"] = [min(v), max(v)]
  r["composed_over_fused"] = r["composed_ms"] / r["fused_ms"]
  for k in ("log_Z", "KL", "ess_pct"):
    r[k] = [float(v) for v in got["fused"][k]]
    r[k + "_max_abs_diff"] = float((got["fused"][k] - got["composed"][k]).abs().max())
  out[name] = r
  print(name, json.dumps(r), flush=True)

out = {}
T5 = [0.0, 0.25, 0.5, 0.75, 1.0]
shape("dim2_mixture_5x1M", 2, 0.2, 1 << 20, T5, app.GaussianMixtureTarget(app.MIXTURE_CENTERS.astype(np.float64)), out)
shape("dim10_gaussian_5x1M", 10, 0.12, 1 << 20, T5, app.GaussianMixtureTarget(np.zeros((1, 10)), 1.3), out)
if "--out" in sys.argv:
  with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
    json.dump(out, f, indent=1)
