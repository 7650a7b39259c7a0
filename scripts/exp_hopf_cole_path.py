"""The exact rwpo solution along [0, T]: timings of the default problem at dz 0.01 (median of 7 after a
warm-up, min-max), the energy identity that checks drift_t independently, and evaluate_path's table of the trained
default run.  Prints one JSON line per item:  python scripts/exp_hopf_cole_path.py [--no-train]"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnf_ot_amd import applications as app, solvers

dev = torch.device("cuda", 0)
REPS = 7
cfg = solvers.load_config()
r = cfg["rwpo"]
T, beta, a, sub = r["T"], r["beta"], r["a"], r["pot_type"]
xs, _ = solvers.density_eval_points(dev)

def timed(fn):
  torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3

def bench(fns):
  for fn in fns.values():
    fn(); fn()
  ms = {k: [] for k in fns}
  for _ in range(REPS):                      # interleaved
    for k, fn in fns.items():
      ms[k].append(timed(fn))
  return {k: {"ms": float(np.median(v)), "min_max": [min(v), max(v)]} for k, v in ms.items()}

# 1. 9 times on the 100 x 100 grid
ts9 = np.linspace(0.0, T, 9)
res = bench({
  "path_9_times_one_call": lambda: app.rwpo_reference_path(T, beta, a, sub, ts9, xs),
  "path_9_calls_of_one_time": lambda: [app.rwpo_reference_path(T, beta, a, sub, [t], xs) for t in ts9],
  "path_one_interior_time": lambda: app.rwpo_reference_path(T, beta, a, sub, [0.5 * T], xs),
  "path_8_interior_times": lambda: app.rwpo_reference_path(T, beta, a, sub, np.linspace(0.1 * T, 0.9 * T, 8), xs),
  "solution_at_T_all_fields": lambda: app.rwpo_reference_solution(T, beta, a, sub, xs),
  "value_alone": lambda: app.rwpo_true_value_quadrature(2, T, beta, a, sub),
})
res["per_time_increment_ms"] = (res["path_9_times_one_call"]["ms"] - res["value_alone"]["ms"]) / 9
print("timings", json.dumps(res), flush=True)

# 2. the energy identity: Simpson over 33 times of 1/2 int rho_t |drift_t|^2 dx, plus int rho_T g dx, against true_val
wide = torch.linspace(-3.5, 3.5, 351, dtype=torch.float64, device=dev)
dA = float(wide[1] - wide[0]) ** 2
ts33 = np.linspace(0.0, T, 33)
p = app.rwpo_reference_path(T, beta, a, sub, ts33, wide, fields=("drift",))
rho = torch.exp(p["log_rho"])
mass = (rho.sum((1, 2)) * dA).cpu().numpy()
action = (0.5 * dA * (rho * (p["drift"] ** 2).sum(3)).sum((1, 2))).cpu().numpy()
w = np.ones(33); w[1:-1:2] = 4; w[2:-1:2] = 2
kinetic = float((w * action).sum() * (T / 32) / 3)
X, Y = torch.meshgrid(wide, wide, indexing="xy")
g = ((X - a) ** 2 + (Y - a) ** 2) * ((X + a) ** 2 + (Y + a) ** 2) / 4
potential = float((rho[-1] * g).sum() * dA)
tv = float(p["true_val"])
print("energy_identity", json.dumps({"kinetic": kinetic, "potential": potential, "sum": kinetic + potential, "true_val": tv,
                                     "residual": kinetic + potential - tv, "min_mass": float(mass.min()),
                                     "action_at_0_T": [float(action[0]), float(action[-1])]}), flush=True)

# 3. the trained default run
if "--no-train" not in sys.argv:
  t0 = time.time()
  model, params, _ = solvers.train(cfg, epochs=30000, capture=True)
  ev = solvers.evaluate(cfg, model, params, 7)
  path = solvers.evaluate_path(cfg, model, params)
  print("evaluate", json.dumps(ev), flush=True)
  print("evaluate_path", json.dumps(path), flush=True)
  solvers.print_path_errors(path)
  print(f"({time.time() - t0:.1f} s)")
