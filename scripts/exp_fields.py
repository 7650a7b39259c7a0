"""Fused field calls against their composition from the public flow calls: interleaved A/B in one process, median of 7
after a warm-up, min-max spread.  Prints one JSON line per workload.  Both sides go through the public
functions of cnf_ot_amd.utils (fused=True / fused=False) on grids made once, outside the timed region: the composition
builds and uploads its point tensors on the first (warm-up) call and keeps them with the grid, as a user composing the
arrays from model.apply.* would build XY once."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnf_ot_amd import solvers, utils

dev = torch.device("cuda", 0)
REPS = 7

def timed(fn):
  torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3

def ab(name, fused, composed, out):
  for _ in range(3):
    fused(); composed()
  a, b = [], []
  for _ in range(REPS):
    a.append(timed(fused)); b.append(timed(composed))
  r = {"fused_ms": float(np.median(a)), "fused_min_max": [min(a), max(a)], "composed_ms": float(np.median(b)),
       "composed_min_max": [min(b), max(b)]}
  r["speedup"] = r["composed_ms"] / r["fused_ms"]
  out[name] = r
  print(name, json.dumps(r), flush=True)

out = {}
# 1. the default config's figure
cfg = solvers.load_config()
model, params, _ = solvers.train(cfg, epochs=50)
st = solvers.figure_settings(cfg)
g_fig = utils.field_grid(st["domain_range"], 100)
def fig(fused):
  def run():
    utils.eulerian_fields(model, params, g_fig, st["t_array"], rho=True, fused=fused)
    utils.trajectories(model, params, st["r"].astype(np.float32), st["t_array"], fused=fused)
  return run
ab("default_figure", fig(True), fig(False), out)
# 3. monitoring-sized pass: velocity and score on a 100 x 100 grid at 5 times
g = utils.field_grid(st["domain_range"], 100)
def mon(fused):
  def run():
    utils.eulerian_fields(model, params, g, st["t_array"], rho=True, vel=True, score=True, fused=fused)
  return run
ab("monitoring_pass", mon(True), mon(False), out)
# 2. the Lorenz figure (dim 3)
cfg3 = solvers.load_config(overrides={"general": {"type": "fp", "dim": 3}, "fp": {"velocity_field_type": "lorenz"}})
model3, params3, _ = solvers.train(cfg3, epochs=20)
st3 = solvers.figure_settings(cfg3)
g_slice = utils.field_grid(st3["domain_range"], 100, fixed=[0, 0, 3.0])
g_proj = [utils.field_grid(st3["domain_range"], 100, axes=axes, section=st3["section"], section_axis=sa)
          for axes, sa in st3["directions"].values()]
def lor(fused):
  def run():
    utils.eulerian_fields(model3, params3, g_slice, st3["t_array"], rho=True, fused=fused)
    utils.trajectories(model3, params3, st3["r"].astype(np.float32), st3["t_array"], fused=fused)
    for gp in g_proj:
      utils.eulerian_fields(model3, params3, gp, st3["t_array"], rho=True, fused=fused)
  return run
ab("lorenz_figure", lor(True), lor(False), out)
# train() alone against train() with a monitoring pass every eval_frequency steps
def train_with(kind):
  def run():
    c = solvers.load_config()
    model_, seed = solvers.build_model(c), int(c["general"]["seed"])
    p = model_.init(seed); opt = solvers.Adam(c["train"]["lr"]); stt = opt.init(p)
    upd = solvers.make_update(solvers.bind_loss(c, model_), opt, c["train"]["batch_size"])
    for step in range(1000):
      loss, p, stt = upd(p, (seed + 0x9E3779B97F4A7C15 * (step + 1)) & 0xFFFFFFFFFFFFFFFF, c["train"]["_lambda"], stt)
      if kind is not None and step % c["train"]["eval_frequency"] == 0:
        utils.eulerian_fields(model_, p, g, st["t_array"], rho=True, vel=True, score=True, fused=kind)
  return run
res = {}
for name, k in (("train_alone", None), ("train_fused_monitor", True), ("train_composed_monitor", False)):
  train_with(k)()
for _ in range(REPS):
  for name, k in (("train_alone", None), ("train_fused_monitor", True), ("train_composed_monitor", False)):
    res.setdefault(name, []).append(timed(train_with(k)))
for name, v in res.items():
  out[name + "_1000_steps"] = {"ms": float(np.median(v)), "min_max": [min(v), max(v)]}
  print(name, json.dumps(out[name + "_1000_steps"]), flush=True)
