"""Mirror of cnf_ot/mfc/solvers.py (the caller of the hot path): config keys of
config/mfc.yaml, model construction (:41-56), the loss binding (:58-88),
`update` = value_and_grad + Adam (:90-97), the training loop (:99-127), and the
post-training evaluation (:129-308: `evaluate`, printed by `main`), on the HIP
kernels.  The matplotlib calls (:119-127, 309-493) are out of scope; the arrays they
draw are `figure_data` (`--fields out.npz` saves them).  The double-well
density-vs-interpolator comparison (:178-188, 222-231) reads data files
(data/fcn4a*_interp.pkl) that the reference does not ship; here it compares with
the exact solution computed on the device (rwpo_quadrature_terms).

  python -m cnf_ot_amd.solvers [--config mfc.yaml] [--epochs N] [--capture] [--save params.npz] [--fields out.npz]
                               [--path-errors] [--fit] [--interaction] [--mv-path] [--ksd] [--ksd-test] [--field-errors]
"""
import argparse
import math
import sys
from dataclasses import dataclass, field
from functools import partial
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi, applications, utils
from .distributed import Shard
from .flows import DeviceRng, RQSFlow, FlowModel, _OnDevice, _stream_ptr, mark_updated
from .params import Params

# config/mfc.yaml:6-40 (the checked-in defaults)
DEFAULT_CONFIG: Dict[str, Dict[str, Any]] = {
  "general": {"type": "rwpo", "dim": 2, "dx": 0.01, "dt": 0.01, "t_batch_size": 1, "seed": 42},
  "ot": {"subtype": "free"},
  "rwpo": {"T": 2, "beta": 10, "a": 1, "pot_type": "double_well"},
  "fp": {"T": 1, "a": 1, "sigma": 0.5, "velocity_field_type": "gradient"},
  "cnf": {"flow_num_layers": 2, "mlp_num_layers": 2, "hidden_size": 16, "num_bins": 5},
  "train": {"epochs": 30000, "lr": 0.001, "_lambda": 5000.0, "batch_size": 2048, "eval_frequency": 100},
  # not in the reference: a nonlocal running cost strength * int_0^T F(rho_t) dt for ot and rwpo, F the interaction energy
  # of utils.interaction_energy (kind "none": no such cost; "gaussian", "exponential", "quadratic", "power": utils.interaction_spec;
  # "power" reads the optional key `exponents` and takes `bandwidths` as its one softening length).
  # An optional key `role` (absent: "cost"): "drift" puts -strength grad (W * rho) into fp's drift instead (bind_loss)
  "interaction": {"kind": "none", "strength": 1.0, "amplitudes": [1.0], "bandwidths": [1.0]},
}


def load_config(path: str = None, overrides: Dict[str, Dict[str, Any]] = None) -> Dict[str, Dict[str, Any]]:
  """yaml.safe_load(config/mfc.yaml) (solvers.py:496-500) merged over the
  defaults; the unused `hydra:` block is ignored."""
  cfg = {k: dict(v) for k, v in DEFAULT_CONFIG.items()}
  if path is not None:
    import yaml
    with open(path) as f:
      loaded = yaml.safe_load(f) or {}
    for sec, vals in loaded.items():
      if sec in cfg and isinstance(vals, dict):
        cfg[sec].update(vals)
  for sec, vals in (overrides or {}).items():
    cfg.setdefault(sec, {}).update(vals)
  return cfg


def build_model(config) -> FlowModel:
  """solvers.py:41-48"""
  c = config["cnf"]
  return RQSFlow(event_shape=(config["general"]["dim"],), num_layers=c["flow_num_layers"],
                 hidden_sizes=[c["hidden_size"]] * c["mlp_num_layers"], num_bins=c["num_bins"], periodized=False)


def bind_loss(config, model) -> Callable:
  """solvers.py:58-88: loss_fn(params, rng, _lambda, batch_size).  With an `interaction` section whose kind is not
  "none", the section's optional key `role` says what the interaction is: "cost" (the default when the key is absent), a
  running cost of ot and rwpo (the losses' `interaction=`), which fp does not have: ValueError; "drift", the force
  -strength grad (W * rho) in fp's drift (fp_loss_fn's `interaction=`: the McKean-Vlasov problem whose particle form
  evaluate_mv_reference integrates), which ot and rwpo do not have: ValueError.  Any other role: ValueError."""
  g = config["general"]
  _type, dim, dt, dx, tbs = g["type"], g["dim"], g["dt"], g["dx"], g["t_batch_size"]
  kw = {}
  if _interaction_kind(config) != "none":
    role = _interaction_role(config)
    if _type == "fp" and role != "drift":
      raise ValueError("an interaction COST is defined for ot and rwpo: fp_loss_fn's drifts are compiled into the "
                       "flow-matching kernel; the section's `role: drift` puts the interaction's force into fp's drift")
    if _type != "fp" and role == "drift":
      raise ValueError(f"an interaction with `role: drift` is defined for fp (fp_loss_fn's interaction=), not for {_type}")
    kw["interaction"] = (_interaction_kwargs(config), float(config["interaction"]["strength"]))
  if _type == "rwpo":
    r = config["rwpo"]
    return partial(applications.rwpo_loss_fn, model, dim, r["T"], r["beta"], dt, dx, tbs, r["pot_type"], r["a"], **kw)
  if _type == "fp":
    f = config["fp"]
    return partial(applications.fp_loss_fn, model, dim, f["T"], f["a"], f["sigma"], dt, dx, tbs,
                   f["velocity_field_type"], **kw)
  if _type == "ot":
    return partial(applications.ot_loss_fn, model, dim, 1, dt, tbs, config["ot"]["subtype"], **kw)
  raise Exception(f"Unknown problem type: {_type}...")        # solvers.py:87-88


INTERACTION_ROLES = ("cost", "drift")


def _interaction_role(config) -> str:
  """The `interaction` section's optional key `role` ("cost" when absent; not in DEFAULT_CONFIG) -- ValueError for any
  other value than INTERACTION_ROLES"""
  role = config.get("interaction", {}).get("role", "cost")
  if role not in INTERACTION_ROLES:
    raise ValueError(f"interaction: role is one of {INTERACTION_ROLES}, not {role!r}")
  return role


def _interaction_kind(config) -> str:
  return config.get("interaction", {}).get("kind", "none")


def _interaction_kwargs(config) -> Dict[str, Any]:
  """utils.interaction_spec's arguments from the config's `interaction` section"""
  i = config["interaction"]
  kw = {"kind": i["kind"], "amplitudes": i.get("amplitudes"),
        "bandwidths": None if i["kind"] == "quadratic" else i.get("bandwidths")}
  if i.get("exponents") is not None:       # (the power kind's; utils.interaction_spec refuses it for the others)
    kw["exponents"] = i["exponents"]
  return kw


@dataclass
class AdamState:
  """optax.adam state: step count and the two moment estimates (flat tensors)."""
  step: int
  mu: torch.Tensor
  nu: torch.Tensor


@dataclass
class Adam:
  """optax.adam(lr) (solvers.py:55): b1 = 0.9, b2 = 0.999, eps = 1e-8."""
  lr: float
  b1: float = 0.9
  b2: float = 0.999
  eps: float = 1e-8

  def init(self, params: Params) -> AdamState:
    return AdamState(0, torch.zeros_like(params.flat), torch.zeros_like(params.flat))

  def apply(self, params: Params, grads: Params, state: AdamState, step_state: torch.Tensor = None) -> AdamState:
    """optimizer.update + optax.apply_updates (solvers.py:95-96), in place on
    params.flat (one kernel: cnf_adam_step).  step_state: a DeviceRng's `state` -- the step count is then read on the
    device (cnf_adam_step_dev; cnf_step_begin has already counted this step), as a captured step needs it."""
    lib = _capi.lib()
    state.step += 1
    dev = params.flat.device
    with _OnDevice(dev):
      if step_state is not None:
        _capi.check(lib.cnf_adam_step_dev(params.flat.data_ptr(), grads.flat.data_ptr(), state.mu.data_ptr(),
                                          state.nu.data_ptr(), params.flat.numel(), self.lr, self.b1, self.b2, self.eps,
                                          step_state.data_ptr(), _stream_ptr(dev)), "cnf_adam_step_dev")
      else:
        _capi.check(lib.cnf_adam_step(params.flat.data_ptr(), grads.flat.data_ptr(), state.mu.data_ptr(),
                                      state.nu.data_ptr(), params.flat.numel(), self.lr, self.b1, self.b2, self.eps,
                                      state.step, _stream_ptr(dev)), "cnf_adam_step")
    # the kernel wrote params.flat behind torch's back: engines must re-prepare (FlowEngine.load)
    mark_updated(params.flat)
    return state


class CapturedUpdate:
  """`update` of solvers.py:90-97 as ONE device-side program -- what the reference's jitted step is: value_and_grad
  + Adam captured into a HIP graph on the first calls and replayed afterwards (a default-config step is ~20 small
  launches: launch latency, not kernels).  Everything that changes from step to step is read from device memory:
  the step's key (one 8-byte copy per call), the time batch, the mixture components and the base noise drawn from it
  by kernels, Adam's step count (include/cnf_ot_amd.h, "a training step as one device-side program").

  Same call surface as the eager update: (params, rng, _lambda, opt_state) -> (loss, params, opt_state), with
  `params` / `opt_state` updated in place and `loss` a 0-dim device tensor that the NEXT call overwrites.  The
  graph holds the addresses of `params.flat` and of the optimiser state and the value of `_lambda`: call it with the
  same objects (checked).  `replay=False` runs the very same body eagerly (what the graph is compared with).

  The step count of Adam's bias correction continues the optimiser state it is first called with (`opt_state.step`,
  written to the device state once, before the warm-up), and every later call must find `opt_state.step` where this
  object left it: ValueError for a state that was stepped elsewhere in between.

  The recorded kernels read, by raw address, tensors that were NOT allocated inside the capture and that their owners
  may drop: the uploads of host condition lists ([0], [T]) in the engine's `_cond_cache` (cleared at 32 keys), the
  weight vectors of `applications._WEIGHTS` (cleared at 64 keys) and the engine's `_kp_work` (replaced when a larger
  call arrives).  The object keeps a reference to each of them from the capture on (`_held`), so eager work on the
  same engine between two replays cannot free what the graph reads.  Everything else the body reads is either
  allocated inside the capture (the graph's own pool: draws, time batch, sums, gradient), owned by an object this one
  holds (the device state of `rng`; the model's tables, slabs and statistics, through the loss function), the
  caller's (`params.flat`, the moments: checked by address on every call), or in a cache that is never emptied
  (`applications._CHOL_ROWS`, `_CENTERS_DEV`).  After every replay the engine holds the parameters from BEFORE that
  step's Adam update (the graph loads them first): `mark_updated` follows each replay, so `model.apply.*` reloads even
  with `assume_unchanged_params`."""

  WARMUP = 2       # eager steps before the capture: allocations (gradient slabs, cached weight vectors) happen there

  def __init__(self, loss_fn: Callable, optimizer: Adam, batch_size: int, replay: bool = True):
    self.vg = applications.value_and_grad(loss_fn)
    self.opt, self.B, self.replay = optimizer, batch_size, replay
    self.rng, self.graph, self.loss, self._key, self._calls = None, None, None, None, 0
    self._step = None       # opt_state.step as the next call must find it
    self._held = []         # what the graph reads and did not allocate (class docstring)
    # The warm-up steps run on the stream the graph is captured on: the engine's table workspaces are reserved PER
    # STREAM and cannot grow during a capture (FlowEngine.reserve), so a step warmed up on the caller's stream and
    # captured on torch's side stream found no tables there and recorded the MLP kernels -- correct, and for a
    # large batch several times slower than the eager step (found by the ot_large case of
    # test_captured_step_equals_the_eager_step_bit_for_bit).
    self._stream = None

  def _body(self, params, _lambda, opt_state):
    dev = params.flat.device
    with _OnDevice(dev):
      _capi.check(_capi.lib().cnf_step_begin(self.rng.ptr, _stream_ptr(dev)), "cnf_step_begin")
    loss, grads = self.vg(params, self.rng, _lambda, self.B)
    self.opt.apply(params, grads, opt_state, step_state=self.rng.state)
    return loss

  def __call__(self, params: Params, rng, _lambda, opt_state: AdamState):
    if self.rng is None:
      from .distributed import current_shard
      if self.replay and current_shard().world > 1:
        # (the loss's all-reduce would be recorded into the graph: RCCL can, gloo cannot, and neither has been run here)
        raise NotImplementedError("CapturedUpdate: single rank only -- use the eager update under torch.distributed")
      self.rng = DeviceRng(params.flat.device)
      # Adam's bias corrections read the count from the device state: it continues the optimiser state handed over
      self.rng.state[:1].copy_(torch.tensor([int(opt_state.step)], dtype=torch.int64))
      self._step = int(opt_state.step)
    key = (params.flat.data_ptr(), opt_state.mu.data_ptr(), opt_state.nu.data_ptr(), float(_lambda))
    if self._key is not None and key != self._key:
      raise ValueError("CapturedUpdate was captured for other parameter / optimiser tensors or another _lambda")
    if opt_state.step != self._step:
      raise ValueError(f"CapturedUpdate counts step {self._step} on the device, the optimiser state is at step "
                       f"{opt_state.step}: it was stepped elsewhere in between")
    self._key = key
    self.rng.set_key(rng)
    self._calls += 1
    if not self.replay:
      self.loss = self._body(params, _lambda, opt_state)
    elif self._calls <= self.WARMUP:
      dev = params.flat.device
      if self._stream is None:
        self._stream = torch.cuda.Stream(device=dev)
      cur = torch.cuda.current_stream(dev)
      self._stream.wait_stream(cur)
      with torch.cuda.stream(self._stream):
        self.loss = self._body(params, _lambda, opt_state)
      cur.wait_stream(self._stream)
    elif self.graph is None:
      torch.cuda.synchronize(params.flat.device)
      graph = torch.cuda.CUDAGraph()
      step0 = opt_state.step
      applications._CAPTURED_BACKENDS = used = []
      try:
        with torch.cuda.graph(graph, stream=self._stream):
          self.loss = self._body(params, _lambda, opt_state)
      finally:
        applications._CAPTURED_BACKENDS = None
      opt_state.step = step0            # (the capture only recorded the step)
      # what the recorded kernels read and the capture did not allocate: kept from here on (class docstring)
      self._held = list(applications._WEIGHTS.values())
      for be in used:
        self._held += list(getattr(be, "_cond_cache", {}).values()) + [getattr(be, "_kp_work", None)]
      self.graph = graph
      self._replay(params, opt_state)
    else:
      self._replay(params, opt_state)
    self._step = opt_state.step
    return self.loss, params, opt_state

  def _replay(self, params, opt_state):
    self.graph.replay()
    opt_state.step += 1
    # the graph's Adam wrote params.flat after the graph's own load of it: engines must re-prepare (FlowEngine.load)
    mark_updated(params.flat)


def make_update(loss_fn: Callable, optimizer: Adam, batch_size: int, capture: bool = False) -> Callable:
  """`update` of solvers.py:90-97.  The reference returns new pytrees; here the
  parameters and the optimiser state are updated IN PLACE (the same objects are
  returned), which is what `params, opt_state = update(...)` callers expect.
  capture=True: the step as one replayed HIP graph (CapturedUpdate)."""
  if capture:
    return CapturedUpdate(loss_fn, optimizer, batch_size)
  vg = applications.value_and_grad(loss_fn)

  def update(params: Params, rng, _lambda, opt_state: AdamState) -> Tuple[torch.Tensor, Params, AdamState]:
    loss, grads = vg(params, rng, _lambda, batch_size)
    opt_state = optimizer.apply(params, grads, opt_state)
    return loss, params, opt_state

  return update


def train(config, epochs: int = None, log=None, capture: bool = False):
  """The training loop of solvers.py:99-127 without tqdm/plots: returns
  (params, loss history as a list of 0-dim device tensors).  capture=True: every step after the first two is the
  replay of one HIP graph (CapturedUpdate); ValueError, before any device work, with an interaction term (eager update
  only)."""
  if capture and _interaction_kind(config) != "none":
    raise ValueError("train: an interaction term is for the eager update only (the captured step draws on the device)")
  model = build_model(config)
  seed = int(config["general"]["seed"])
  params = model.init(seed)
  opt = Adam(config["train"]["lr"])
  state = opt.init(params)
  update = make_update(bind_loss(config, model), opt, config["train"]["batch_size"], capture=capture)
  n = config["train"]["epochs"] if epochs is None else epochs
  hist = []
  for step in range(n):
    # update_rng, rng = jax.random.split(rng) (solvers.py:104): an independent Philox key per step
    step_rng = (seed + 0x9E3779B97F4A7C15 * (step + 1)) & 0xFFFFFFFFFFFFFFFF
    loss, params, state = update(params, step_rng, config["train"]["_lambda"], state)
    hist.append(loss.clone() if capture else loss)       # (a captured step overwrites its loss tensor)
    if log is not None and step % config["train"]["eval_frequency"] == 0:
      log(step, float(loss))
  return model, params, hist


# ---- post-training evaluation (solvers.py:129-308) ------------------------------

def evaluate(config, model: FlowModel, params: Params, rng) -> Dict[str, Any]:
  """What solvers.py:129-308 computes after training, without plots, keyed by name.  Every value is a Python float
  (var_T: a list of floats, one per dimension), or None where the reference has no value.
    all:  param_count (:128-129)
    ot:   kinetic_energy_more (65 536 samples x 10 000 slices), kinetic_energy_less (4 096 x 1 000)   (:132-149)
    rwpo: e_kin = T calc_score_kinetic_energy, e_pot = potential_loss_fn(params, T, rng, 65536), total, true_val
          (applications.rwpo_true_value), rel_err_pct = (total - true_val) / true_val * 100          (:150-237)
    fp:   l2_mc: the density L2 error of 1 M samples at cond 1 against the reference's mixture (source variance 4,
          as it prints it, :238-282); l2_grid: the same on the 500 x 500 grid of [-5, 5]^2 (dim 2 only, :284-307);
          l2_mc_ic: l2_mc against the mixture of the training's own initial condition N(0, (T+1)/2 I) (fp_loss_fn's
          reverse KL at beta = 4, applications.py:432: the reference's variance 4 does not match it, so its printed
          error cannot reach 0); var_T: the per-dimension sample variance of 1 M samples at t = T, and
          var_T_closed_form = ou_variance(T, a, (T+1)/2, sigma).
          At dim 2 (None elsewhere), for every potential, from the exact solution (rwpo_quadrature_terms):
          true_val_quadrature, rel_err_pct_quadrature, density_sq_err, ic_mass.
  The reference's double-well density-vs-interpolator comparison (:178-188, 222-231) reads data/fcn4a*_interp.pkl,
  which it does not ship; density_sq_err computes the interpolated solution's source exactly instead, and true_val
  still comes from cost_rwpo."""
  g = config["general"]
  _type, dim = g["type"], g["dim"]
  out: Dict[str, Any] = {"param_count": int(params.flat.numel())}
  if _type == "ot":
    out["kinetic_energy_more"] = float(utils.calc_kinetic_energy(model.apply.sample, params, rng, batch_size=65536,
                                                                 t_size=10000, dim=dim))
    out["kinetic_energy_less"] = float(utils.calc_kinetic_energy(model.apply.sample, params, rng, batch_size=4096,
                                                                 t_size=1000, dim=dim))
  elif _type == "rwpo":
    r = config["rwpo"]
    T, beta, a, sub = r["T"], r["beta"], r["a"], r["pot_type"]
    e_kin = T * float(utils.calc_score_kinetic_energy(model.apply.sample, model.apply.log_prob, params, T, beta, dim,
                                                      rng))
    e_pot = float(applications.potential_loss_fn(model, dim, a, sub, params, T, rng, 65536))
    true_val = applications.rwpo_true_value(dim, T, beta, a, sub, rng) if (sub != "double_well" or dim == 2) else None
    total = e_kin + e_pot
    out.update(e_kin=e_kin, e_pot=e_pot, total=total, true_val=true_val,
               rel_err_pct=None if true_val is None else (total - true_val) / true_val * 100)
    out.update(rwpo_quadrature_terms(model, params, T, beta, a, sub, total) if dim == 2 else
               dict.fromkeys(RWPO_QUADRATURE_KEYS))
  elif _type == "fp":
    f = config["fp"]
    T, a, sigma = f["T"], f["a"], f["sigma"]
    n = 1000000
    var_ic = (T + 1.0) / 2.0
    out["l2_mc"] = float(applications.density_l2_error_fn(model, dim, T, a, params, 1.0, rng, n, var0=4.0))
    out["l2_grid"] = float(applications.density_l2_grid_error_fn(model, T, a, params, 1.0, 500)) if dim == 2 else None
    out["l2_mc_ic"] = float(applications.density_l2_error_fn(model, dim, T, a, params, 1.0, rng, n, var0=var_ic))
    y = model.apply.sample(params, cond=float(T), seed=rng, sample_shape=(n,))
    out["var_T"] = [float(v) for v in y.double().var(dim=0).cpu()]
    out["var_T_closed_form"] = applications.ou_variance(T, a, var_ic, sigma)
  else:
    raise Exception(f"Unknown problem type: {_type}...")        # solvers.py:87-88
  return out


RWPO_QUADRATURE_KEYS = ("true_val_quadrature", "rel_err_pct_quadrature", "density_sq_err", "ic_mass")
DENSITY_GRID = (-2.0, 2.0, 100)       # the reference's XY grid of the double-well density check (solvers.py:182-188)


def density_eval_points(device):
  """The reference's XY: meshgrid(linspace(-2, 2, 100), same) flattened, x fastest, as the float32 points the flow
  sees.  Returns (the 1-D coordinates in float64, the [10 000, 2] float32 points)."""
  lo, hi, n = DENSITY_GRID
  xs = torch.linspace(lo, hi, n, dtype=torch.float64, device=device).to(torch.float32)
  X, Y = torch.meshgrid(xs, xs, indexing="xy")
  return xs.double(), torch.stack([X.reshape(-1), Y.reshape(-1)], 1).contiguous()


def rwpo_quadrature_terms(model: FlowModel, params: Params, T, beta, a, subtype, total) -> Dict[str, Any]:
  """evaluate's rwpo keys from the exact dim-2 solution (applications.rwpo_reference_solution, the reference's
  generator at its own resolution): true_val_quadrature, rel_err_pct_quadrature = (total - it) / it * 100,
  ic_mass, and density_sq_err = sum over the reference's 100 x 100 grid of [-2, 2]^2 of
  (exp(log_prob(XY, cond=T)) - rho_T(XY))^2 -- the statistic solvers.py:222-225 prints, rho_T evaluated exactly at
  the grid points instead of through the generator's bilinear interpolator."""
  xs, pts = density_eval_points(params.flat.device)
  sol = applications.rwpo_reference_solution(T, beta, a, subtype, xs, fields=())
  lp = model.apply.log_prob(params, pts, cond=float(T))
  err = float(((torch.exp(lp.double()) - torch.exp(sol["log_rho_T"].reshape(-1))) ** 2).sum())
  tv = float(sol["true_val"])
  return {"true_val_quadrature": tv, "rel_err_pct_quadrature": (total - tv) / tv * 100, "density_sq_err": err,
          "ic_mass": float(sol["ic_mass"])}


def evaluate_path(config, model: FlowModel, params: Params, times=None, with_score=False) -> Dict[str, Any]:
  """Where along [0, T] the flow departs from the exact rwpo solution (dim 2 only; ValueError otherwise): per time of
  `times` (default: 9 equally spaced in [0, T]) on evaluate's 100 x 100 grid of [-2, 2]^2 with cell area dA, against
  applications.rwpo_reference_path, the flow's rho and velocity from one utils.eulerian_fields call.  Lists of floats:
    times
    density_sq_err    sum (rho_flow - rho_t)^2                          (density_sq_err's measure, at every time)
    velocity_rel_err  sum rho_t |v_flow - vel_t|^2 / sum rho_t |vel_t|^2
    action_exact      1/2 sum rho_t |drift_t|^2 dA                      (the exact solution's kinetic term at t)
    mass              sum rho_t dA                                      (how much of rho_t the grid holds)
  with_score=True adds
    score_rel_err     sum rho_t |s_flow - s_t|^2 / sum rho_t |s_t|^2    (s_t = grad log rho_t of the exact solution,
                                                                         s_flow the flow's exact score, model.apply.score)
  and leaves the other entries as they are."""
  g = config["general"]
  if g["type"] != "rwpo" or g["dim"] != 2:
    raise ValueError(f"evaluate_path: defined for rwpo at dim 2 only, not {g['type']} at dim {g['dim']}")
  r = config["rwpo"]
  T = r["T"]
  ts = np.linspace(0.0, float(T), 9) if times is None else utils._times_of(times)
  xs, pts = density_eval_points(params.flat.device)
  dA = float(xs[1] - xs[0]) ** 2
  ref = applications.rwpo_reference_path(T, r["beta"], r["a"], r["pot_type"], ts, xs,
                                         fields=("score", "drift", "vel") if with_score else ("drift", "vel"))
  flow = utils.eulerian_fields(model, params, pts, ts, rho=True, vel=True, dt=g["dt"])
  S = len(ts)
  rho = torch.exp(ref["log_rho"].reshape(S, -1))
  vel, drift = ref["vel"].reshape(S, -1, 2), ref["drift"].reshape(S, -1, 2)
  dv = ((flow["vel"].double() - vel) ** 2).sum(2)
  res = {"times": [float(t) for t in ts],
         "density_sq_err": ((flow["rho"].double() - rho) ** 2).sum(1).tolist(),
         "velocity_rel_err": ((rho * dv).sum(1) / (rho * (vel ** 2).sum(2)).sum(1)).tolist(),
         "action_exact": (0.5 * dA * (rho * (drift ** 2).sum(2)).sum(1)).tolist(),
         "mass": (dA * rho.sum(1)).tolist()}
  if with_score:
    s_t = ref["score"].reshape(S, -1, 2)
    s_flow = model.apply.score(params, pts, cond=ts).reshape(S, -1, 2)
    ds = ((s_flow.double() - s_t) ** 2).sum(2)
    res["score_rel_err"] = ((rho * ds).sum(1) / (rho * (s_t ** 2).sum(2)).sum(1)).tolist()
  return res


def print_path_errors(res: Dict[str, Any]) -> None:
  """evaluate_path's table, one line per time (the score column where evaluate_path(with_score=True) made it)"""
  score = "score_rel_err" in res
  print("path errors against the exact solution:  t | density sq err | velocity rel err | exact action | mass on grid"
        + (" | score rel err" if score else ""))
  for i, row in enumerate(zip(res["times"], res["density_sq_err"], res["velocity_rel_err"], res["action_exact"],
                              res["mass"])):
    print("  {:.4f} | {:.3e} | {:.3e} | {:.6f} | {:.6f}".format(*row)
          + (" | {:.3e}".format(res["score_rel_err"][i]) if score else ""))


def rwpo_particles_domain(config):
  """The histogram domain of evaluate_rwpo_particles: the figure's where the reference draws one (dim 2), else
  +-3 standard deviations of the initial condition over axes (0, 1)"""
  st = figure_settings(config)
  if st is not None:
    return [float(v) for v in st["domain_range"]]
  r = config["rwpo"]
  half = 3.0 * math.sqrt(applications.rwpo_initial_variance(r["T"], r["beta"]))
  return [-half, half, -half, half]


def evaluate_rwpo_particles(config, model: FlowModel, params: Params, times=None, n_particles=65536, n_inner=4096,
                            seed=0) -> Dict[str, Any]:
  """Where along [0, T] the flow of an rwpo configuration departs from the optimal path measure, at any dimension and
  for every potential (ValueError for another problem type): per time of `times` (default: 5 equally spaced in [0, T]),
  n_particles flow samples (model.apply.sample of `seed`, through utils.point_stats) against the bridges of
  applications.rwpo_reference_particles (same count, n_inner draws each, same seed, run as its two halves), histograms
  of FIGURE_GRID^2 cells on rwpo_particles_domain over axes (0, 1).  Lists of floats, one per time -- times, mean_err,
  cov_rel_err, tv, tv_floor, bad, formed exactly as evaluate_fp_path forms them -- and the floats
    true_val, true_val_se, bias_est, true_val_corrected   the optimal energy -(2 / beta) mean log h, its standard error,
                                                          the self-normalisation bias and the value less the bias
    ess_median, ess_min                                   the effective sample size over the outer particles (of n_inner)
  Single process."""
  g = config["general"]
  if g["type"] != "rwpo":
    raise ValueError(f"evaluate_rwpo_particles: defined for rwpo only, not {g['type']}")
  n_particles = int(n_particles)
  if n_particles < 2 or n_particles % 2:
    raise ValueError(f"evaluate_rwpo_particles: n_particles must be even and >= 2 (two halves are compared), not {n_particles}")
  r, dim = config["rwpo"], g["dim"]
  T, beta, a, sub = r["T"], r["beta"], r["a"], r["pot_type"]
  ts = np.linspace(0.0, float(T), 5) if times is None else utils._times_of(times)
  S, half = len(ts), n_particles // 2
  grid = utils.field_grid(rwpo_particles_domain(config), FIGURE_GRID, axes=(0, 1))
  samples = torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n_particles,)) for t in ts])
  flow = utils.point_stats(samples, grid)
  halves = [applications.rwpo_reference_particles(dim, T, beta, a, sub, ts, half, n_inner, seed, grid=grid, first=k * half)
            for k in (0, 1)]
  ref = applications.stats_from_sums(halves[0]["sums"] + halves[1]["sums"], halves[0]["hist"] + halves[1]["hist"],
                                     n_particles, applications.stats_grid(grid, None, dim), dim)
  p, q = flow["hist"].double() / n_particles, ref["hist"].double() / n_particles
  ha, hb = (hv["hist"].double() / half for hv in halves)
  ess = torch.cat([hv["ess"] for hv in halves])
  val = applications.rwpo_value_of(torch.cat([hv["log_h"] for hv in halves]), ess, beta, n_inner)
  out = {"times": [float(t) for t in ts],
         "mean_err": torch.linalg.norm(flow["mean"] - ref["mean"], dim=1).tolist(),
         "cov_rel_err": (torch.linalg.norm((flow["cov"] - ref["cov"]).reshape(S, -1), dim=1)
                         / torch.linalg.norm(ref["cov"].reshape(S, -1), dim=1)).tolist(),
         "tv": (0.5 * (p - q).abs().sum((1, 2))).tolist(),
         "tv_floor": (0.5 * (ha - hb).abs().sum((1, 2))).tolist(),
         "bad": ref["bad"].tolist()}
  out.update({k: float(v) for k, v in val.items()})
  out.update(ess_median=float(ess.median()), ess_min=float(ess.min()))
  return out


def print_rwpo_particles(res: Dict[str, Any]) -> None:
  """evaluate_rwpo_particles' lines: the value, then one line per time"""
  print("optimal energy from the particle reference: {:.6f} +- {:.1e} | less the bias {:.1e}: {:.6f} | "
        "ess median {:.1f} min {:.1f}".format(res["true_val"], res["true_val_se"], res["bias_est"],
                                              res["true_val_corrected"], res["ess_median"], res["ess_min"]))
  print("path errors against the particle reference:  t | mean err | cov rel err | tv | tv floor | bad")
  for row in zip(res["times"], res["mean_err"], res["cov_rel_err"], res["tv"], res["tv_floor"], res["bad"]):
    print("  {:.4f} | {:.3e} | {:.3e} | {:.4f} | {:.4f} | {:.0f}".format(*row))


def _fp_prelude(name, config, times, n_particles, h, min_particles, start="gaussian"):
  """What the fp evaluators refuse, in `name`'s words, before any device work -- another problem type, (evaluate_fp_path:
  an unknown `start`,) a configuration without figure settings, an n_particles that is odd or below min_particles,
  times that are no multiples of h -- and what they go on with: (figure settings, times, n_particles, (dim, T, a,
  sigma, drift type))."""
  g = config["general"]
  if g["type"] != "fp":
    raise ValueError(f"{name}: defined for fp only, not {g['type']}")
  if start not in ("gaussian", "flow"):
    raise ValueError(f"{name}: start is 'gaussian' or 'flow', not {start!r}")
  st = figure_settings(config)
  if st is None:
    raise ValueError(f"{name}: no figure settings for fp / {config['fp']['velocity_field_type']} at dim {g['dim']}")
  n_particles = int(n_particles)
  if n_particles < min_particles or n_particles % 2:
    raise ValueError(f"{name}: n_particles must be even and >= {min_particles} (two halves are compared), not {n_particles}")
  f = config["fp"]
  # (the figure's own times need not be multiples of h -- linspace(0, 1, 10) at dim 3: the default snaps them to it)
  ts = np.rint(st["t_array"] / float(h)) * float(h) if times is None else utils._times_of(times)
  applications.fp_step_indices(ts, float(h), f["T"])
  return st, ts, n_particles, (g["dim"], f["T"], f["a"], f["sigma"], f["velocity_field_type"])


def _fp_flow_and_halves(model, params, fp, ts, n_particles, h, seed):
  """(flow, half 0, half 1), [S, n_particles / 2, D] each: the flow's samples of `seed` at the times ts, stacked, and
  the positions of the two halves of the Euler-Maruyama ensemble (fp: the problem, as _fp_prelude returns it)."""
  flow = torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n_particles // 2,)) for t in ts])
  h0, h1 = _fp_halves(fp, ts, n_particles, h, seed)
  return flow, h0, h1


def _fp_halves(fp, ts, n_particles, h, seed):
  """The positions of the two halves of the Euler-Maruyama ensemble at the times ts, [S, n_particles / 2, D] each"""
  dim, T, a, sigma, sub = fp
  return tuple(applications.fp_reference_particles(dim, T, a, sigma, sub, ts, n_particles, h, seed, positions=True,
                                                   shard=Shard(r, 2), all_reduce=False)["pos"].float() for r in (0, 1))


def evaluate_fp_path(config, model: FlowModel, params: Params, times=None, n_particles=1 << 20, h=1e-3, seed=0,
                     start="gaussian") -> Dict[str, Any]:
  """Where along [0, T] the flow of an fp configuration departs from the Fokker-Planck solution, for every drift and
  dimension the figures cover (ValueError for another problem type or a configuration without figure settings): per
  time of `times` (default: the figure's, each rounded to a multiple of h), n_particles flow samples (model.apply.sample of `seed`) against the
  Euler-Maruyama ensemble of applications.fp_reference_particles (same count, step h, same seed), histograms on the
  figure's domain with FIGURE_GRID^2 cells over axes (0, 1).  Lists of floats, one per time:
    times
    mean_err        |mean of the flow samples - particle mean|
    cov_rel_err     |cov_flow - cov_particles|_F / |cov_particles|_F
    tv              1/2 sum |p - q| between the flow samples' and the particles' histograms (p = counts / n_particles)
    tv_floor        the same between the two halves of the particle ensemble (each over its n_particles / 2): the
                    Monte-Carlo noise that makes tv readable (two samples of n_particles / 2: sqrt(2) above the noise
                    between two of n_particles)
    density_sq_err  sum (rho_flow(grid points) - density)^2, evaluate_path's measure, the flow's rho from
                    utils.eulerian_fields; dim 2 only (None elsewhere: the histogram is a marginal there)
    bad             particles that were not finite
  start="flow": the ensemble starts from the flow's own samples at t = 0 instead of N(0, (T + 1) / 2 I), which takes
  the initial-condition fit out of the path error.  Single process (the ensemble is run as its two halves)."""
  st, ts, n_particles, (dim, T, a, sigma, sub) = _fp_prelude("evaluate_fp_path", config, times, n_particles, h, 2, start)
  S = len(ts)
  grid = utils.field_grid(st["domain_range"], FIGURE_GRID, axes=(0, 1))
  samples = torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n_particles,)) for t in ts])
  flow = utils.point_stats(samples, grid)
  x0 = model.apply.sample(params, cond=0.0, seed=seed, sample_shape=(n_particles,)).double() if start == "flow" else None
  halves = [applications.fp_reference_particles(dim, T, a, sigma, sub, ts, n_particles, h, seed, x0=x0, grid=grid,
                                                shard=Shard(r, 2), all_reduce=False) for r in (0, 1)]
  ref = applications.stats_from_sums(halves[0]["sums"] + halves[1]["sums"], halves[0]["hist"] + halves[1]["hist"],
                                     n_particles, applications.stats_grid(grid, None, dim), dim)
  p, q = flow["hist"].double() / n_particles, ref["hist"].double() / n_particles
  ha, hb = (hv["hist"].double() / (n_particles // 2) for hv in halves)
  dens = None
  if dim == 2:
    rho = utils.eulerian_fields(model, params, grid, ts, rho=True)["rho"].double()
    dens = ((rho - ref["density"].reshape(S, -1)) ** 2).sum(1).tolist()
  return {"times": [float(t) for t in ts],
          "mean_err": torch.linalg.norm(flow["mean"] - ref["mean"], dim=1).tolist(),
          "cov_rel_err": (torch.linalg.norm((flow["cov"] - ref["cov"]).reshape(S, -1), dim=1)
                          / torch.linalg.norm(ref["cov"].reshape(S, -1), dim=1)).tolist(),
          "tv": (0.5 * (p - q).abs().sum((1, 2))).tolist(),
          "tv_floor": (0.5 * (ha - hb).abs().sum((1, 2))).tolist(),
          "density_sq_err": dens,
          "bad": ref["bad"].tolist()}


def print_fp_path_errors(res: Dict[str, Any]) -> None:
  """evaluate_fp_path's table, one line per time"""
  print("path errors against the particle reference:  t | mean err | cov rel err | tv | tv floor | density sq err | bad")
  dens = res["density_sq_err"] or [float("nan")] * len(res["times"])
  for row in zip(res["times"], res["mean_err"], res["cov_rel_err"], res["tv"], res["tv_floor"], dens, res["bad"]):
    print("  {:.4f} | {:.3e} | {:.3e} | {:.4f} | {:.4f} | {:.3e} | {:.0f}".format(*row))


def evaluate_fp_two_sample(config, model: FlowModel, params: Params, times=None, n_particles=65536, h=1e-3, seed=0,
                           bandwidths=None) -> Dict[str, Any]:
  """How far, in the FULL dimension, the flow's samples are from the Euler-Maruyama ensemble of an fp configuration
  (evaluate_fp_path's histograms are a marginal over axes (0, 1) beyond dim 2): kernel two-sample statistics per time
  of `times` (default and refusals as evaluate_fp_path: fp only, a configuration with figure settings, an even
  n_particles, times that are multiples of h).  The ensemble is run as its two halves
  (fp_reference_particles(positions=True, shard=Shard(r, 2), all_reduce=False)); n_particles / 2 flow samples
  (model.apply.sample of `seed`) are compared with half 0, and half 1 with half 0 -- the same sample sizes and the same
  bandwidths (None: utils.median_bandwidths of half 0's first time).  Lists of floats, one per time:
    times
    mmd2, mmd2_floor      the unbiased Gaussian MMD^2 of flow against half 0, and of half 1 against half 0: the
                          Monte-Carlo level that makes mmd2 readable, as tv_floor does for tv
    energy, energy_floor  the same for the energy distance 2 E|x - y| - E|x - x'| - E|y - y'|
    bandwidths            the bandwidths used
  Two cnf_mmd2 calls per kind over all times (utils.mmd2).  Single process."""
  _, ts, n_particles, fp = _fp_prelude("evaluate_fp_two_sample", config, times, n_particles, h, 4)
  if bandwidths is not None:
    utils.mmd_spec(bandwidths, "gaussian")
  flow, h0, h1 = _fp_flow_and_halves(model, params, fp, ts, n_particles, h, seed)
  bws = utils.median_bandwidths(h0) if bandwidths is None else bandwidths
  out: Dict[str, Any] = {"times": [float(t) for t in ts]}
  for kind, key in (("gaussian", "mmd2"), ("energy", "energy")):
    res = utils.mmd2(flow, h0, bws, kind)
    out[key] = res["mmd2"].tolist()
    out[key + "_floor"] = utils.mmd2(h1, h0, bws, kind)["mmd2"].tolist()
    if kind == "gaussian":
      out["bandwidths"] = res["bandwidths"]
  return out


def print_fp_two_sample(res: Dict[str, Any]) -> None:
  """evaluate_fp_two_sample's table, one line per time"""
  print("two-sample distances to the particle reference (bandwidths " + " ".join(f"{b:.3g}" for b in res["bandwidths"])
        + "):  t | mmd2 | mmd2 floor | energy | energy floor")
  for row in zip(res["times"], res["mmd2"], res["mmd2_floor"], res["energy"], res["energy_floor"]):
    print("  {:.4f} | {:.3e} | {:.3e} | {:.3e} | {:.3e}".format(*row))


def evaluate_fp_permutation(config, model: FlowModel, params: Params, times=None, n_particles=16384, h=1e-3, seed=0,
                            n_perm=255, bandwidths=None) -> Dict[str, Any]:
  """evaluate_fp_two_sample's values as p-values: per time of `times` (default, refusals, halves and bandwidth rule as
  evaluate_fp_two_sample), the permutation test of n_particles / 2 flow samples against half 0 of the Euler-Maruyama
  ensemble, and of half 1 against half 0, under n_perm relabellings of the pooled sample
  (utils.permutation_labels(n_particles / 2, n_particles / 2, n_perm, seed): the same label vectors at every time and
  for both pairs).  Lists of floats, one per time:
    times
    mmd2, p_mmd2                  the unbiased Gaussian MMD^2 of flow against half 0 and its p-value
                                  (1 + #{null >= mmd2}) / (1 + n_perm): can the two samples be told apart, at what level
    energy, p_energy              the same for the energy distance
    mmd2_halves, p_mmd2_halves, energy_halves, p_energy_halves
                                  the same four of half 1 against half 0: two samples of one law, so these p-values are
                                  uniform on (0, 1] -- what shows that the test is calibrated
    bandwidths, n_perm            the bandwidths and the number of relabellings used
  One cnf_mmd_perm call per kind and pair over all times (utils.mmd_permutation_test).  ValueError unless n_perm + 1 is
  a multiple of 32 within 32..1024.  Single process."""
  _, ts, n_particles, fp = _fp_prelude("evaluate_fp_permutation", config, times, n_particles, h, 4)
  if bandwidths is not None:
    utils.mmd_spec(bandwidths, "gaussian")
  labels = utils.permutation_labels(n_particles // 2, n_particles // 2, n_perm, seed)
  flow, h0, h1 = _fp_flow_and_halves(model, params, fp, ts, n_particles, h, seed)
  bws = utils.median_bandwidths(h0) if bandwidths is None else bandwidths
  out: Dict[str, Any] = {"times": [float(t) for t in ts], "n_perm": int(n_perm)}
  for kind, key in (("gaussian", "mmd2"), ("energy", "energy")):
    for first, tail in ((flow, ""), (h1, "_halves")):
      res = utils.mmd_permutation_test(first, h0, bws, kind, labels=labels)
      out[key + tail] = res["mmd2"].tolist()
      out["p_" + key + tail] = res["p_value"].tolist()
      if kind == "gaussian":
        out["bandwidths"] = res["bandwidths"]
  return out


def print_fp_permutation(res: Dict[str, Any]) -> None:
  """evaluate_fp_permutation's table, one line per time"""
  print(f"permutation tests against the particle reference ({res['n_perm']} relabellings, bandwidths "
        + " ".join(f"{b:.3g}" for b in res["bandwidths"])
        + "):  t | mmd2 (p) | energy (p) | halves: mmd2 (p) | halves: energy (p)")
  for row in zip(res["times"], res["mmd2"], res["p_mmd2"], res["energy"], res["p_energy"], res["mmd2_halves"],
                 res["p_mmd2_halves"], res["energy_halves"], res["p_energy_halves"]):
    print("  {:.4f} | {:.3e} ({:.4f}) | {:.3e} ({:.4f}) | {:.3e} ({:.4f}) | {:.3e} ({:.4f})".format(*row))


# ---- the flow's fields against the ensemble's: log-density, score and the velocity the flow-matching term trains -------

FP_FIELD_KEYS = ("times", "bandwidth", "logp_rmse", "logp_rmse_floor", "score_rel_err", "score_rel_err_floor",
                 "velocity_rel_err", "velocity_rel_err_floor", "kde_score_bias", "n", "n_points")


def _rel_err(a, b):
  """sum |a - b|^2 / sum |b|^2 over the points, in float64"""
  a, b = a.double(), b.double()
  return float(((a - b) ** 2).sum() / (b ** 2).sum())


def _rmse(a, b):
  return float(((a.double() - b.double()) ** 2).mean().sqrt())


def evaluate_fp_fields(config, model: FlowModel, params: Params, times=None, n_particles=1 << 18, n_points=4096, h=1e-3,
                       seed=0, bandwidth_factor=1.0) -> Dict[str, Any]:
  """The flow's FIELDS against the particle reference's, in the full dimension and for every drift -- what the
  flow-matching term trains is the velocity, v_flow + sigma grad log rho = drift, and for the drifts without a
  closed-form score the only source of the true right-hand side is the ensemble: its kernel density estimate
  (applications.ensemble_fields, cnf_kde) gives log rho_t, grad log rho_t and the probability-flow velocity
  drift - sigma grad log rho_t [- strength grad(W * rho_t)] at any points.  `times`, and the refusals, as
  evaluate_fp_two_sample.  The ensemble is run as its two halves of n_particles / 2 -- with an `interaction` section of
  `role: drift`, the two replicas of applications.mv_reference_particles(positions=True), the force in the velocity.  Per
  time: the sources are half 0, the evaluation points the first n_points particles of half 1 (points of the law that are
  not sources), ONE bandwidth, utils.kde_bandwidths of that time's sources times bandwidth_factor; the flow's side is
  one utils.eulerian_fields(logp, vel, score with exact_score=True) call.  Lists, one entry per time:
    times, bandwidth
    logp_rmse          root mean square of log rho_flow - log rho_ens over the points
    score_rel_err      sum |s_flow - s_ens|^2 / sum |s_ens|^2
    velocity_rel_err   sum |v_flow - v_ens|^2 / sum |v_ens|^2
    logp_rmse_floor, score_rel_err_floor, velocity_rel_err_floor
                       the same quantities between the ensemble's fields from the two halves of the SOURCE half (one
                       call on two sets, the same bandwidth): the Monte-Carlo noise at half the sources
    kde_score_bias     drift ou without an interaction: sum |s_ens - s_t|^2 / sum |s_t|^2 against the closed form s_t =
                       -x / applications.ou_variance(t, ...): what the bandwidth costs; else None
  and n (sources), n_points.  Two cnf_kde calls per time (the estimate, its floor).  Single process.  ValueError, before
  any device work, for what _fp_prelude refuses (n_particles even and >= 8), an n_points outside 1..n_particles / 2, a
  bandwidth_factor that is not positive and finite and what utils.kde_check_shapes refuses."""
  name = "evaluate_fp_fields"
  _, ts, n_particles, fp = _fp_prelude(name, config, times, n_particles, h, 8)
  dim, T, a, sigma, sub = fp
  n, n_points = n_particles // 2, int(n_points)
  if n % 2:
    raise ValueError(f"{name}: n_particles must be a multiple of 4 (the source half is halved for the floors), not {n_particles}")
  if not 1 <= n_points <= n:
    raise ValueError(f"{name}: n_points must lie in 1..n_particles / 2 = {n}, not {n_points}")
  if not (float(bandwidth_factor) > 0.0 and np.isfinite(float(bandwidth_factor))):
    raise ValueError(f"{name}: the bandwidth factor must be positive and finite, not {bandwidth_factor}")
  utils.kde_check_shapes((1, n, dim), (1, n_points, dim))
  kw, strength = None, 0.0
  if _interaction_kind(config) != "none" and _interaction_role(config) == "drift":
    kw, strength = _interaction_kwargs(config), float(config["interaction"]["strength"])
    utils.interaction_spec(**kw)
    pos = applications.mv_reference_particles(dim, T, a, sigma, sub, kw, strength, ts, n, 2, h, seed, positions=True)["pos"]
    h0, h1 = pos[:, 0].float(), pos[:, 1].float()
  else:
    h0, h1 = _fp_halves(fp, ts, n_particles, h, seed)
  out: Dict[str, Any] = {k: [] for k in FP_FIELD_KEYS[:8]}
  out.update(kde_score_bias=[] if sub == "ou" and kw is None else None, n=n, n_points=n_points)
  var0 = applications.fp_initial_variance(T)
  for i, t in enumerate(ts):
    src, pts = h0[i].contiguous(), h1[i, :n_points].contiguous()
    bw = [float(bandwidth_factor) * utils.kde_bandwidths(src)[0]]
    ens = applications.ensemble_fields(pts, src, sigma, a, sub, bw, kw, strength)
    two = applications.ensemble_fields(torch.stack([pts, pts]), torch.stack([src[:n // 2], src[n // 2:]]), sigma, a, sub, bw,
                                       kw, strength)
    flow = utils.eulerian_fields(model, params, pts, [float(t)], logp=True, vel=True, score=True, exact_score=True,
                                 dt=config["general"]["dt"])
    out["times"].append(float(t))
    out["bandwidth"].append(ens["bandwidths"][0])
    out["logp_rmse"].append(_rmse(flow["logp"][0], ens["log_density"][0]))
    out["score_rel_err"].append(_rel_err(flow["score"][0], ens["score"][0]))
    out["velocity_rel_err"].append(_rel_err(flow["vel"][0], ens["velocity"][0]))
    out["logp_rmse_floor"].append(_rmse(two["log_density"][0, 0], two["log_density"][1, 0]))
    out["score_rel_err_floor"].append(_rel_err(two["score"][0, 0], two["score"][1, 0]))
    out["velocity_rel_err_floor"].append(_rel_err(two["velocity"][0, 0], two["velocity"][1, 0]))
    if out["kde_score_bias"] is not None:
      exact = pts.double() * (-1.0 / applications.ou_variance(float(t), a, var0, sigma))
      out["kde_score_bias"].append(_rel_err(ens["score"][0], exact))
  return out


def print_fp_fields(res: Dict[str, Any]) -> None:
  """evaluate_fp_fields' table, one line per time"""
  bias = res["kde_score_bias"]
  print("field errors against the particle reference's kernel density estimate ({} sources, {} points):  t | bandwidth | "
        "log rho rmse | floor | score rel err | floor | velocity rel err | floor{}"
        .format(res["n"], res["n_points"], " | kde score bias" if bias is not None else ""))
  for i, row in enumerate(zip(res["times"], res["bandwidth"], res["logp_rmse"], res["logp_rmse_floor"], res["score_rel_err"],
                              res["score_rel_err_floor"], res["velocity_rel_err"], res["velocity_rel_err_floor"])):
    print("  {:.4f} | {:.4g} | {:.3e} | {:.3e} | {:.3e} | {:.3e} | {:.3e} | {:.3e}".format(*row)
          + (" | {:.3e}".format(bias[i]) if bias is not None else ""))


# ---- the same comparison in transport units at the full ensemble size: the sliced Wasserstein distance ---------------

FP_SLICED_KEYS = ("times", "sw", "sw_floor", "max_sliced", "max_sliced_floor", "w2_marginal", "w2_marginal_floor", "n",
                  "n_proj")


def evaluate_fp_sliced(config, model: FlowModel, params: Params, times=None, n_particles=1 << 20, h=1e-3, seed=0,
                       n_proj=64) -> Dict[str, Any]:
  """How far, in the FULL dimension and in transport units, the flow's samples are from the Euler-Maruyama ensemble of
  an fp configuration, at the ensemble size of the other evaluators: the sliced Wasserstein distance
  (utils.sliced_wasserstein: cost |.|^2 / 2, N log N per projection, where evaluate_fp_two_sample's pair statistics stop
  at 65 536 particles).  `times`, and the refusals, as evaluate_fp_two_sample.  The ensemble is run as its two halves;
  n_particles / 2 flow samples (model.apply.sample of `seed`) are compared with half 0, and half 1 with half 0 -- the
  same sizes and the same directions, utils.sliced_directions(dim, n_proj, seed).  Per time, lists of floats:
    times
    sw, sw_floor                  the distance of flow against half 0, and of half 1 against half 0: its Monte-Carlo level
    max_sliced, max_sliced_floor  the largest one-dimensional cost over the directions
    w2_marginal, w2_marginal_floor  [D] each: sqrt(2 w) with the coordinate axes as directions, the exact W2 between
                                  the two empirical marginals of every coordinate
    n, n_proj                     the points per set and the directions used
  All times, flow and floor, go into ONE cnf_sliced_w2 call per direction set (2 x len(times) <= 64 sets).  Single
  process."""
  _, ts, n_particles, fp = _fp_prelude("evaluate_fp_sliced", config, times, n_particles, h, 2)
  n, S, dim = n_particles // 2, len(ts), fp[0]
  utils.sliced_check_shapes((2 * S, n, dim), (2 * S, n, dim))
  theta = utils.sliced_directions(dim, 1 if dim == 1 else n_proj, seed)
  axes = utils.sliced_directions(dim, dim, kind="axes")
  flow, h0, h1 = _fp_flow_and_halves(model, params, fp, ts, n_particles, h, seed)
  x, y = torch.cat([flow.float(), h1]), torch.cat([h0, h0])
  rnd = utils.sliced_wasserstein(x, y, theta)
  marg = (2.0 * utils.sliced_wasserstein(x, y, axes)["per_projection"]).sqrt()
  return {"times": [float(t) for t in ts], "sw": rnd["sw"][:S].tolist(), "sw_floor": rnd["sw"][S:].tolist(),
          "max_sliced": rnd["max_sliced"][:S].tolist(), "max_sliced_floor": rnd["max_sliced"][S:].tolist(),
          "w2_marginal": marg[:S].tolist(), "w2_marginal_floor": marg[S:].tolist(), "n": n, "n_proj": int(theta.shape[0])}


def print_fp_sliced(res: Dict[str, Any]) -> None:
  """evaluate_fp_sliced's table, one line per time"""
  print("sliced Wasserstein distance to the particle reference ({} points per set, {} directions; units of W2^2 / 2):  "
        "t | sw | sw floor | max sliced | floor | W2 of each marginal (floor)".format(res["n"], res["n_proj"]))
  for t, sw, fl, mx, mfl, wm, wfl in zip(res["times"], res["sw"], res["sw_floor"], res["max_sliced"], res["max_sliced_floor"],
                                         res["w2_marginal"], res["w2_marginal_floor"]):
    print("  {:.4f} | {:.3e} | {:.3e} | {:.3e} | {:.3e} | ".format(t, sw, fl, mx, mfl)
          + " ".join("{:.3e} ({:.1e})".format(u, v) for u, v in zip(wm, wfl)))


# ---- the same comparison in the unit the flow was trained in: nearest-neighbour KL and entropy, in nats --------------

FP_KNN_KEYS = ("times", "kl", "kl_floor", "kl_reverse", "entropy_knn", "entropy_model", "kl_ensemble_flow", "n", "k")


def evaluate_fp_knn(config, model: FlowModel, params: Params, times=None, n_particles=65536, h=1e-3, seed=0,
                    k=4) -> Dict[str, Any]:
  """How far, in NATS and in the full dimension, the flow is from the Euler-Maruyama ensemble of an fp configuration,
  whose law at t > 0 exists only as particles: the nearest-neighbour estimates of utils.knn_divergence at rank k.
  `times`, and the refusals, as evaluate_fp_two_sample (and what utils.knn_check_shapes refuses).  The ensemble is run as
  its two halves; n_particles / 2 flow samples (model.apply.sample of `seed`) stand beside them.  Per time, lists of floats:
    times
    kl                KL(flow || half 0)
    kl_floor          KL(half 1 || half 0): two samples of one law, so the estimator's own bias and noise -- visibly
                      non-zero at dim 10, and what makes kl readable
    kl_reverse        KL(half 0 || flow samples); biased low where the flow's samples are the narrower cloud (the
                      neighbours of the ensemble's tail points are far): read it beside kl_ensemble_flow
    entropy_knn, entropy_model  the nearest-neighbour entropy of the flow's samples beside -mean log_prob of the same
                      samples: a check of log_prob that never touches the flow's Jacobian
    kl_ensemble_flow  -H_knn(half 0) - mean log_prob_flow(half 0): the forward KL with a single nearest-neighbour
                      estimate in it
    n, k              the points per set and the rank
  The three comparisons of all times are the sets of as few cnf_knn calls as its 64-set limit allows (one for up to 21
  times).  Single process."""
  k = int(k)
  _, ts, n_particles, fp = _fp_prelude("evaluate_fp_knn", config, times, n_particles, h, 4)
  n, S, dim = n_particles // 2, len(ts), fp[0]
  utils.knn_check_shapes((min(3 * S, _capi.MMD_MAX_SETS), n, dim), (min(3 * S, _capi.MMD_MAX_SETS), n, dim), k)
  flow, h0, h1 = _fp_flow_and_halves(model, params, fp, ts, n_particles, h, seed)
  flow = flow.float()
  x, y = torch.cat([flow, h1, h0]), torch.cat([h0, h0, flow])
  parts = [utils.knn_divergence(x[i:i + _capi.MMD_MAX_SETS], y[i:i + _capi.MMD_MAX_SETS], k)
           for i in range(0, 3 * S, _capi.MMD_MAX_SETS)]
  kl, ent = (torch.cat([p[key] for p in parts]) for key in ("kl", "entropy"))
  lp_flow = [model.apply.sample_and_log_prob(params, cond=float(t), seed=seed, sample_shape=(n,))[1].double().mean().item()
             for t in ts]
  lp_h0 = [model.apply.log_prob(params, h0[i], cond=float(t)).double().mean().item() for i, t in enumerate(ts)]
  return {"times": [float(t) for t in ts], "kl": kl[:S].tolist(), "kl_floor": kl[S:2 * S].tolist(),
          "kl_reverse": kl[2 * S:].tolist(), "entropy_knn": ent[:S].tolist(), "entropy_model": [-v for v in lp_flow],
          "kl_ensemble_flow": [-e - v for e, v in zip(ent[2 * S:].tolist(), lp_h0)], "n": n, "k": k}


def print_fp_knn(res: Dict[str, Any]) -> None:
  """evaluate_fp_knn's table, one line per time"""
  print("nearest-neighbour estimates against the particle reference ({} points per set, k = {}; nats):  t | KL(flow||ens) | "
        "floor | KL(ens||flow samples) | H knn | H model | KL(ens||flow), one estimate".format(res["n"], res["k"]))
  for row in zip(res["times"], res["kl"], res["kl_floor"], res["kl_reverse"], res["entropy_knn"], res["entropy_model"],
                 res["kl_ensemble_flow"]):
    print("  {:.4f} | {:.4f} | {:.4f} | {:.4f} | {:.4f} | {:.4f} | {:.4f}".format(*row))


# ---- the flow against the Fokker-Planck equation itself, solved on a grid (fp at dim 2) ------------------------------

# The box the PDE is solved in (no-flux faces), per drift: wide enough that N(0, (T + 1) / 2 I) and the solution leave
# no mass at the faces; the smile's cubic drift makes a wider box only stiffer (the step count grows with |b| dx / sigma)
FP_GRID_DOMAIN = {"ou": [-6.0, 6.0, -6.0, 6.0], "nongradient": [-6.0, 6.0, -6.0, 6.0], "gradient": [-4.0, 4.0, -4.0, 4.0],
                  "smile": [-4.0, 4.0, -4.0, 4.0]}
FP_GRID_KEYS = ("times", "l1", "rel_l2", "max_log_err", "mean_grid", "mean_flow", "trace_cov_grid", "trace_cov_flow",
                "trace_cov_closed_form", "mass", "n_steps", "n", "domain")
FP_GRID_MASS = 0.999     # max_log_err looks at the densest cells that hold this share of the grid solution's mass


def evaluate_fp_grid(config, model: FlowModel, params: Params, times=None, n=257, domain=None, n_samples=1 << 18,
                     seed=0) -> Dict[str, Any]:
  """The flow of an fp configuration at dim 2 against the Fokker-Planck equation itself, solved in float64 on a grid
  (applications.fp_reference_grid: no Monte-Carlo floor): per time of `times` (default: the figure's) the flow's density
  on the grid's points (utils.density_on_grid) beside the grid solution on n (an int or (nx, ny)) points per axis of
  `domain` (default: FP_GRID_DOMAIN of the drift).  Lists, one entry per time:
    times
    l1               sum |rho_flow - rho_grid| dx dy
    rel_l2           |rho_flow - rho_grid|_2 / |rho_grid|_2
    max_log_err      max |log rho_flow - log rho_grid| over the densest cells that hold FP_GRID_MASS of the grid's mass:
                     the tails, where a histogram has nothing to say
    mean_grid, mean_flow            [2] each; the flow's from n_samples samples of `seed` (utils.point_stats)
    trace_cov_grid, trace_cov_flow  tr cov of the same
    trace_cov_closed_form           ou: 2 ou_variance(t); None for the other drifts
    mass, n_steps                   the grid solution's mass and its explicit steps up to that time from the one before
  and n, domain.  ValueError before any device work for another problem type, another dimension, a drift the grid does
  not cover (lorenz), and an interaction in the drift."""
  g = config["general"]
  if g["type"] != "fp":
    raise ValueError(f"evaluate_fp_grid: defined for fp only, not {g['type']}")
  f = config["fp"]
  sub = f["velocity_field_type"]
  if g["dim"] != 2 or sub not in applications.FP_GRID_DRIFTS:
    raise ValueError(f"evaluate_fp_grid: the grid reference is defined at dim 2 for {applications.FP_GRID_DRIFTS}, "
                     f"not for {sub} at dim {g['dim']}")
  if _interaction_kind(config) != "none" and _interaction_role(config) == "drift":
    raise ValueError("evaluate_fp_grid: the grid reference has no interaction term in its drift")
  T, a, sigma = float(f["T"]), f["a"], f["sigma"]
  ts = figure_settings(config)["t_array"] if times is None else utils._times_of(times)
  dom = [float(v) for v in (FP_GRID_DOMAIN[sub] if domain is None else domain)]
  grid = utils.field_grid(dom, n)
  ref = applications.fp_reference_grid(T, a, sigma, sub, ts, grid)
  S = len(ts)
  want = ref["density"]
  rho = utils.density_on_grid(model, params, ts, dom, n).double()
  area = float((ref["x"][1] - ref["x"][0]) * (ref["y"][1] - ref["y"][0]))
  diff = rho - want
  # the densest cells that hold FP_GRID_MASS of the mass: sort descending, keep while the running sum stays below it
  flat = want.reshape(S, -1)
  order = flat.argsort(dim=1, descending=True)
  before = flat.gather(1, order).cumsum(1) - flat.gather(1, order)
  keep = torch.zeros_like(flat, dtype=torch.bool).scatter(1, order, before < FP_GRID_MASS * flat.sum(1, keepdim=True))
  log_err = (rho.reshape(S, -1).clamp_min(1e-300).log() - flat.clamp_min(1e-300).log()).abs()
  samples = torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(int(n_samples),)) for t in ts])
  flow = utils.point_stats(samples)
  return {"times": [float(t) for t in ts],
          "l1": (diff.abs().sum((1, 2)) * area).tolist(),
          "rel_l2": (torch.linalg.norm(diff.reshape(S, -1), dim=1) / torch.linalg.norm(flat, dim=1)).tolist(),
          "max_log_err": torch.where(keep, log_err, torch.zeros_like(log_err)).amax(1).tolist(),
          "mean_grid": ref["mean"].tolist(), "mean_flow": flow["mean"].tolist(),
          "trace_cov_grid": ref["cov"].diagonal(dim1=1, dim2=2).sum(1).tolist(),
          "trace_cov_flow": flow["cov"].diagonal(dim1=1, dim2=2).sum(1).tolist(),
          "trace_cov_closed_form": [2.0 * applications.ou_variance(float(t), a, applications.fp_initial_variance(T), sigma)
                                    for t in ts] if sub == "ou" else None,
          "mass": ref["mass"].tolist(), "n_steps": ref["n_steps"].tolist(),
          "n": [int(v) for v in grid["n"]], "domain": dom}


def print_fp_grid(res: Dict[str, Any]) -> None:
  """evaluate_fp_grid's table, one line per time"""
  print("errors against the grid solution of the Fokker-Planck equation ({} x {} points over {}):  t | L1 | rel L2 | "
        "max |log rho err| ({:.1%} of the mass) | mean grid | mean flow | tr cov grid | tr cov flow | tr cov closed form | "
        "steps".format(res["n"][0], res["n"][1], res["domain"], FP_GRID_MASS))
  closed = res["trace_cov_closed_form"] or [float("nan")] * len(res["times"])
  for row in zip(res["times"], res["l1"], res["rel_l2"], res["max_log_err"], res["mean_grid"], res["mean_flow"],
                 res["trace_cov_grid"], res["trace_cov_flow"], closed, res["n_steps"]):
    t, l1, l2, le, mg, mf, cg, cf, cc, k = row
    print("  {:.4f} | {:.3e} | {:.3e} | {:.3e} | ({:+.4f}, {:+.4f}) | ({:+.4f}, {:+.4f}) | {:.5f} | {:.5f} | {:.5f} | {:d}".format(
      t, l1, l2, le, mg[0], mg[1], mf[0], mf[1], cg, cf, cc, int(k)))


# ---- the nonlocal running cost of a trained flow: its interaction energy along the path ------------------------------

INTERACTION_KEYS = ("times", "energy", "floor", "running_cost", "trace_cov", "kind", "strength", "n")


def evaluate_interaction(config, model: FlowModel, params: Params, times=None, n=8192, seed=0) -> Dict[str, Any]:
  """The interaction energy F(rho_t) (utils.interaction_energy, the kernel of the config's `interaction` section) of the
  flow's samples at `times` (default: 9 times of [0, T]; T = 1 for ot).  Per time n samples are drawn
  (model.apply.sample of `seed`) and read as two halves of n / 2.  Lists of floats, one per time:
    times
    energy        F of the first half
    floor         |F(first half) - F(second half)|: two samples of one law, so the Monte-Carlo level of `energy`
    trace_cov     quadratic kind: amp_0 tr(cov) / 2 of the first half from utils.point_stats (cov: unbiased, the factor
                  N / (N - 1) applied) -- the same number as `energy`; else None
  and running_cost = strength * the trapezoid rule of `energy` over `times` (what the training term estimates by
  strength T mean_t F), kind, strength and n (the points per set).  The 2 x len(times) sets are ONE cnf_interaction
  call (up to 32 times).  ValueError, before any device work, for kind "none", n < 4 and what utils.interaction_spec and
  utils.interaction_check_shapes refuse.  For an fp configuration with an interaction, evaluate_mv_reference gives the
  interacting particle system's own F(t), the ground truth of such a problem."""
  kind = _interaction_kind(config)
  if kind == "none":
    raise ValueError("evaluate_interaction: the config's interaction kind is 'none'")
  _type = config["general"]["type"]
  T = 1.0 if _type == "ot" else float(config[_type]["T"])
  ts = np.linspace(0.0, T, 9) if times is None else utils._times_of(times)
  half, S, dim = int(n) // 2, len(ts), config["general"]["dim"]
  kw, strength = _interaction_kwargs(config), float(config["interaction"]["strength"])
  utils.interaction_spec(**kw)
  utils.interaction_check_shapes((min(2 * S, _capi.MMD_MAX_SETS), half, dim))
  draws = [model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(2 * half,)) for t in ts]
  x = torch.stack([d[:half] for d in draws] + [d[half:] for d in draws]).float()
  F = torch.cat([utils.interaction_energy(x[i:i + _capi.MMD_MAX_SETS], **kw)["energy"]
                 for i in range(0, 2 * S, _capi.MMD_MAX_SETS)])
  energy = F[:S].tolist()
  trace_cov = None
  if kind == "quadratic":
    cov = torch.cat([utils.point_stats(x[i:i + _capi.MMD_MAX_SETS])["cov"] for i in range(0, S, _capi.MMD_MAX_SETS)])[:S]
    amp = float(np.float32(kw["amplitudes"][0] if kw["amplitudes"] is not None else 1.0))
    trace_cov = (0.5 * amp * half / (half - 1.0) * cov.diagonal(dim1=1, dim2=2).sum(1)).tolist()
  return {"times": [float(t) for t in ts], "energy": energy, "floor": (F[:S] - F[S:]).abs().tolist(),
          "running_cost": strength * sum(0.5 * (energy[i] + energy[i + 1]) * float(ts[i + 1] - ts[i]) for i in range(S - 1)),
          "trace_cov": trace_cov,
          "kind": kind, "strength": strength, "n": half}


def print_interaction(res: Dict[str, Any]) -> None:
  """evaluate_interaction's table, one line per time, and the running cost"""
  quad = res["trace_cov"] is not None
  print("interaction energy of the flow's samples ({} kernel, {} points per set):  t | F | floor{}".format(
    res["kind"], res["n"], " | amp tr(cov) / 2" if quad else ""))
  for i, row in enumerate(zip(res["times"], res["energy"], res["floor"])):
    print("  {:.4f} | {:.6e} | {:.2e}".format(*row) + (" | {:.6e}".format(res["trace_cov"][i]) if quad else ""))
  print("running cost strength * int F dt (strength {}): {:.6e}".format(res["strength"], res["running_cost"]))


# ---- the particle reference of an fp problem with an interaction: what the interacting training term is held to ------

MV_REFERENCE_KEYS = ("times", "mean", "trace_cov", "free_mean", "free_trace_cov", "trace_cov_floor", "energy",
                     "energy_floor", "bad", "trace_cov_exact", "second_moment", "second_moment_exact", "kind", "strength",
                     "n", "replicas")


def evaluate_mv_reference(config, times=None, n_particles=16384, replicas=2, h=1e-3, seed=0) -> Dict[str, Any]:
  """The ground truth of an fp configuration whose `interaction` section has a kind: the interacting particle system
  of applications.mv_reference_particles (`replicas` systems of n_particles, step h, the config's drift, sigma and
  kernel, strength as the force's factor) whose law converges to d rho / dt = -div(rho (drift - strength grad(W * rho)))
  + sigma lap rho.  It takes no model: it is what the interacting training term (the section's `role: drift`,
  fp_loss_fn's `interaction=`) is held to, and evaluate_mv_path puts a trained flow beside it.  Per time of `times` (default: the figure's, rounded to multiples of h), lists:
    times
    mean, trace_cov            of the interacting ensemble, pooled over the replicas (mean: [D] per time)
    free_mean, free_trace_cov  the same of applications.fp_reference_particles with the same seed and
                               replicas * n_particles particles: the same normals without the force -- what the
                               interaction does
    trace_cov_floor            the largest replica-to-replica difference of tr cov
    energy, energy_floor       F(t), the mean over the replicas of the interaction energy, and its largest
                               replica-to-replica difference: the Monte-Carlo and finite-N level of both
    bad                        particles that were not finite
    trace_cov_exact            drift ou with the quadratic kernel: dim * applications.mv_quadratic_ou_variance, the
                               mean-field limit (the ensemble's h-bias and 1 / N are not in it); else None
    second_moment_exact        the power kind with a single log term (exponent 0) and no drift (ou with a = 0):
                               applications.mv_log_second_moment, E mean |x|^2 of the UNSOFTENED kernel, exact for every
                               N (the softening lowers the force's share by the pair mean of eps^2 / (d^2 + eps^2));
                               beside it second_moment = tr cov + |mean|^2 of the ensemble; else both None
  and kind, strength, n (particles per replica), replicas.  ValueError, before any device work, for what _fp_prelude
  refuses, an interaction kind "none", fewer than 2 replicas and what mv_reference_particles refuses."""
  name = "evaluate_mv_reference"
  st, ts, n_particles, (dim, T, a, sigma, sub) = _fp_prelude(name, config, times, n_particles, h, 2)
  kind = _interaction_kind(config)
  if kind == "none":
    raise ValueError(f"{name}: defined for fp with an interaction kind, not 'none'")
  replicas = int(replicas)
  if replicas < 2:
    raise ValueError(f"{name}: needs replicas >= 2 (the floors compare them), not {replicas}")
  kw, strength = _interaction_kwargs(config), float(config["interaction"]["strength"])
  mv = applications.mv_reference_particles(dim, T, a, sigma, sub, kw, strength, ts, n_particles, replicas, h, seed)
  free = applications.fp_reference_particles(dim, T, a, sigma, sub, ts, replicas * n_particles, h, seed)
  tr = lambda cov: cov.diagonal(dim1=-2, dim2=-1).sum(-1)
  rep_tr, F = tr(mv["replica_cov"]), mv["energy"]
  exact = None
  if sub == "ou" and kind == "quadratic":
    amp = float(np.float32(kw["amplitudes"][0] if kw["amplitudes"] is not None else 1.0))
    var0 = applications.fp_initial_variance(T)
    exact = [dim * applications.mv_quadratic_ou_variance(float(t), a, sigma, strength, amp, var0) for t in ts]
  m2 = m2_exact = None
  pws = kw.get("exponents")
  if sub == "ou" and float(a) == 0.0 and kind == "power" and pws is not None and [float(p) for p in np.ravel(pws)] == [0.0]:
    amp = float(np.float32(np.ravel(kw["amplitudes"])[0] if kw["amplitudes"] is not None else 1.0))
    m0 = dim * applications.fp_initial_variance(T)
    m2_exact = [applications.mv_log_second_moment(float(t), dim, sigma, strength, amp, m0) for t in ts]
    m2 = (tr(mv["cov"]) + (mv["mean"] ** 2).sum(-1)).tolist()      # (cov is the population's: sum x x^T / n - mean mean^T)
  return {"times": [float(t) for t in ts], "second_moment": m2, "second_moment_exact": m2_exact,
          "mean": mv["mean"].tolist(), "trace_cov": tr(mv["cov"]).tolist(),
          "free_mean": free["mean"].tolist(), "free_trace_cov": tr(free["cov"]).tolist(),
          "trace_cov_floor": (rep_tr.max(1).values - rep_tr.min(1).values).tolist(),
          "energy": F.mean(1).tolist(), "energy_floor": (F.max(1).values - F.min(1).values).tolist(),
          "bad": mv["bad"].tolist(), "trace_cov_exact": exact,
          "kind": kind, "strength": strength, "n": n_particles, "replicas": replicas}


def print_mv_reference(res: Dict[str, Any]) -> None:
  """evaluate_mv_reference's table, one line per time"""
  exact = res["trace_cov_exact"] is not None
  virial = res.get("second_moment_exact") is not None
  print("interacting particle reference ({} kernel, strength {}, {} replicas of {}):  t | |mean| | tr cov | floor | "
        "tr cov without the force | F | floor | bad{}{}".format(
          res["kind"], res["strength"], res["replicas"], res["n"], " | tr cov, mean-field limit" if exact else "",
          " | mean |x|^2 | log kernel's closed form (no softening)" if virial else ""))
  for i, t in enumerate(res["times"]):
    print("  {:.4f} | {:.3e} | {:.6f} | {:.2e} | {:.6f} | {:.6e} | {:.2e} | {:.0f}".format(
      t, float(np.linalg.norm(res["mean"][i])), res["trace_cov"][i], res["trace_cov_floor"][i],
      res["free_trace_cov"][i], res["energy"][i], res["energy_floor"][i], res["bad"][i])
      + (" | {:.6f}".format(res["trace_cov_exact"][i]) if exact else "")
      + (" | {:.6f} | {:.6f}".format(res["second_moment"][i], res["second_moment_exact"][i]) if virial else ""))


# ---- a flow trained on the interacting fp problem beside the particle reference ---------------------------------------

MV_PATH_KEYS = ("times", "flow_mean", "flow_trace_cov", "flow_energy", "mean", "trace_cov", "trace_cov_floor", "energy",
                "energy_floor", "free_trace_cov", "trace_cov_exact", "bad", "kind", "strength", "n", "n_particles", "replicas")


def evaluate_mv_path(config, model: FlowModel, params: Params, times=None, n=8192, n_particles=16384, replicas=2, h=1e-3,
                     seed=0) -> Dict[str, Any]:
  """A flow trained on an fp configuration whose `interaction` section has `role: drift`, beside the interacting particle
  reference: per time of `times` (evaluate_mv_reference's default and rounding), lists
    times
    flow_mean, flow_trace_cov  of n flow samples (model.apply.sample of `seed`; utils.point_stats, cov over n)
    flow_energy                their interaction energy F (utils.interaction_energy, the section's kernel)
    mean, trace_cov, trace_cov_floor, energy, energy_floor, free_trace_cov, bad, trace_cov_exact
                               evaluate_mv_reference's columns for the same arguments: the pooled values, the replica
                               floors, the ensemble without the force and, for drift ou with the quadratic kernel, the
                               mean-field limit (else None)
  and kind, strength, n, n_particles, replicas.  A flow agrees with the reference where its columns differ by the
  floors' order.  ValueError, before any device work, for n < 2, what utils.interaction_check_shapes refuses at n and
  what evaluate_mv_reference refuses."""
  name = "evaluate_mv_path"
  n = int(n)
  _, ts, _, (dim, _, _, _, _) = _fp_prelude(name, config, times, n_particles, h, 2)
  if _interaction_kind(config) == "none":
    raise ValueError(f"{name}: defined for fp with an interaction kind, not 'none'")
  if n < 2:
    raise ValueError(f"{name}: needs n >= 2 flow samples per time, not {n}")
  utils.interaction_check_shapes((1, n, dim))
  kw = _interaction_kwargs(config)
  utils.interaction_spec(**kw)
  ref = evaluate_mv_reference(config, times, n_particles, replicas, h, seed)
  x = torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n,)) for t in ref["times"]]).float()
  chunks = range(0, x.shape[0], _capi.MMD_MAX_SETS)
  stats = [utils.point_stats(x[i:i + _capi.MMD_MAX_SETS]) for i in chunks]
  F = torch.cat([utils.interaction_energy(x[i:i + _capi.MMD_MAX_SETS], **kw)["energy"] for i in chunks])
  out = {"times": ref["times"],
         "flow_mean": torch.cat([s["mean"] for s in stats]).tolist(),
         "flow_trace_cov": torch.cat([s["cov"] for s in stats]).diagonal(dim1=-2, dim2=-1).sum(-1).tolist(),
         "flow_energy": F.tolist(), "n": n, "n_particles": ref["n"]}
  for k in ("mean", "trace_cov", "trace_cov_floor", "energy", "energy_floor", "free_trace_cov", "trace_cov_exact", "bad",
            "kind", "strength", "replicas"):
    out[k] = ref[k]
  return out


def print_mv_path(res: Dict[str, Any]) -> None:
  """evaluate_mv_path's table, one line per time"""
  exact = res["trace_cov_exact"] is not None
  print("flow against the interacting particle reference ({} kernel, strength {}, {} flow samples, {} replicas of {}):  "
        "t | |mean| flow | reference | tr cov flow | reference | floor | without the force{} | F flow | reference | floor"
        .format(res["kind"], res["strength"], res["n"], res["replicas"], res["n_particles"],
                " | mean-field limit" if exact else ""))
  for i, t in enumerate(res["times"]):
    print("  {:.4f} | {:.3e} | {:.3e} | {:.6f} | {:.6f} | {:.2e} | {:.6f}".format(
      t, float(np.linalg.norm(res["flow_mean"][i])), float(np.linalg.norm(res["mean"][i])), res["flow_trace_cov"][i],
      res["trace_cov"][i], res["trace_cov_floor"][i], res["free_trace_cov"][i])
      + (" | {:.6f}".format(res["trace_cov_exact"][i]) if exact else "")
      + " | {:.6e} | {:.6e} | {:.2e}".format(res["flow_energy"][i], res["energy"][i], res["energy_floor"][i]))


# ---- the optimal-transport reference of the ot problems: Sinkhorn divergences between point clouds -------------------

OT_REFERENCE_KEYS = ("coupling_cost", "kinetic_energy", "w2_flow", "gap_flow", "map_rmse", "map_blur", "w2_problem",
                     "w2_closed_form", "fit_0", "fit_T", "floor", "change", "eps", "n", "iterations")


def evaluate_ot_reference(config, model: FlowModel, params: Params, n=8192, eps=0.05, seed=0) -> Dict[str, Any]:
  """What an ot flow is judged against: at the optimum the kinetic energy E|v|^2 / 2 over [0, 1] equals
  W2^2(source, target) / 2, and the flow's own map from t = 0 to t = T is the Monge map between its endpoints.  From
  one base draw z of `seed`: x0 = flow(z, 0) and xT = flow(z, T), the flow's own coupling; src: n draws of the
  configured source (ot.source, the training's own draw), tgt and a second, independent draw: n samples of N(0, I).
  Five Sinkhorn divergences S_eps (utils.sinkhorn: cost |x - y|^2 / 2, so every number is in the units of W2^2 / 2) in
  ONE cnf_sinkhorn call, on one schedule (utils.sinkhorn_schedule over all sets).  Floats:
    coupling_cost   mean |xT - x0|^2 / 2: >= W2^2 / 2 of the flow's own endpoints, <= its kinetic energy
    kinetic_energy  utils.calc_kinetic_energy at batch n, 1 000 slices
    w2_flow         S_eps(x0, xT);  gap_flow = coupling_cost - w2_flow: what the flow's map pays above the optimal one
    map_rmse        the rms of |xT - T_eps(x0)|, T_eps the barycentric map of (x0, xT); beside it
    map_blur        the rms of |x0 - Txx(x0)|, the barycentric map of x0 onto itself: what eps alone smears
    w2_problem      S_eps(src, tgt): the value training aims for
    w2_closed_form  (|m|^2 + tr(A + I - 2 A^(1/2))) / 2 for the Gaussian source N(m, A); None for the mixture
    fit_0, fit_T    S_eps(x0, src) and S_eps(xT, tgt): the boundary fits in transport units
    floor           S_eps between the two target draws: the Monte-Carlo level of n points
    change          [5, 2], cnf_sinkhorn's convergence diagnostic per set (utils.sinkhorn), as lists
    eps, n, iterations
  ValueError before any device work: a problem type other than ot, a dimension other than the sources' 2, n outside
  2..2^20, an eps that is not positive and finite.  Single process."""
  g = config["general"]
  if g["type"] != "ot":
    raise ValueError(f"evaluate_ot_reference: defined for ot only, not {g['type']}")
  dim, source = g["dim"], config["ot"].get("source", "mixture")
  if dim != 2 or source not in ("mixture", "gaussian"):
    raise ValueError(f"evaluate_ot_reference: the ot sources are 2-D ('mixture' or 'gaussian'), not {source!r} at dim {dim}")
  n, eps, seed = int(n), float(eps), int(seed)
  utils.sinkhorn_check_shapes((5, n, dim), (5, n, dim))
  if not (eps > 0.0 and np.isfinite(eps)):
    raise ValueError(f"evaluate_ot_reference: eps must be positive and finite, not {eps}")
  T = 1.0
  ctx = applications._Ctx(model, params, seed + 1, Shard(0, 1))
  be = ctx.be
  z = be.normal(seed, n)
  ends, _ = be.forward_logdet(z.repeat(2, 1), be.slice_conds(np.array([0.0, T], dtype=np.float32)), want_logdet=False)
  x0, xT = ends[:n], ends[n:]
  zs, start, count = ctx.noise(n)
  src = applications._source_samples(ctx, zs, start, count, n, source)
  tgt, tgt2 = be.normal(seed + 2, n), be.normal(seed + 3, n)
  x = torch.stack([x0, src, x0, xT, tgt2])
  y = torch.stack([xT, tgt, src, tgt, tgt])
  res = utils.sinkhorn(x, y, eps, want_grad=True, want_map=True)
  div = res["divergence"].tolist()
  tmap, txx = res["map"][0].double(), res["map"][0].double() + n * res["grad"][0].double()
  coupling = float(0.5 * ((xT - x0).double() ** 2).sum(1).mean())
  closed = None
  if source == "gaussian":
    m, A = np.array([-3.0, -3.0]), np.array([[5.0, 1.0], [1.0, 0.5]])
    w, _ = np.linalg.eigh(A)
    closed = float(0.5 * (m @ m + np.trace(A) + dim - 2.0 * np.sqrt(w).sum()))
  return {"coupling_cost": coupling,
          "kinetic_energy": float(utils.calc_kinetic_energy(model.apply.sample, params, seed, batch_size=n, t_size=1000,
                                                            dim=dim)),
          "w2_flow": div[0], "gap_flow": coupling - div[0],
          "map_rmse": float(((xT.double() - tmap) ** 2).sum(1).mean().sqrt()),
          "map_blur": float(((x0.double() - txx) ** 2).sum(1).mean().sqrt()),
          "w2_problem": div[1], "w2_closed_form": closed, "fit_0": div[2], "fit_T": div[3], "floor": div[4],
          "change": res["change"].tolist(), "eps": eps, "n": n, "iterations": len(res["schedule"])}


def print_ot_reference(res: Dict[str, Any]) -> None:
  """evaluate_ot_reference's lines"""
  print("optimal-transport reference (Sinkhorn divergence, eps {:.3g}, {} points, {} iterations; units of W2^2 / 2):".format(
    res["eps"], res["n"], res["iterations"]))
  closed = "n/a" if res["w2_closed_form"] is None else "{:.4f}".format(res["w2_closed_form"])
  print("  problem: S(source, target) {:.4f} | closed form {} | floor {:.3e}".format(res["w2_problem"], closed, res["floor"]))
  print("  flow: kinetic energy {:.4f} | coupling cost {:.4f} | S(x0, xT) {:.4f} | gap {:.3e}".format(
    res["kinetic_energy"], res["coupling_cost"], res["w2_flow"], res["gap_flow"]))
  print("  map: rms |xT - T(x0)| {:.3e} | blur of eps alone {:.3e}".format(res["map_rmse"], res["map_blur"]))
  print("  boundary fits: S(x0, source) {:.3e} | S(xT, target) {:.3e}".format(res["fit_0"], res["fit_T"]))
  print("  largest change of the final pass: {:.2e}".format(max(max(c) for c in res["change"])))


# ---- the fit to the densities known in closed form (the reference's kl_ess, tests/test_fit_prob.py:50-56) -----------

def evaluate_fit(config, model: FlowModel, params: Params, rng, batch_size: int = 1 << 20) -> Dict[str, Any]:
  """The importance-sampling fit of the trained flow to every closed-form density of the problem
  (applications.known_densities: the boundary densities, and for fp / ou the exact density along the path): lists of
  floats, one entry per time -- times, log_Z, KL, ess, ess_pct, max_log_w -- from batch_size samples per time.  One
  fused launch per target (applications.importance_stats).  A perfect fit has log_Z = KL = 0 and ess_pct = 100."""
  entries = applications.known_densities(config)
  keys = ("log_Z", "KL", "ess", "ess_pct", "max_log_w")
  out: Dict[str, Any] = {"times": [], "batch_size": int(batch_size), **{k: [] for k in keys}}
  i = 0
  while i < len(entries):                       # consecutive times of one target: one call
    j = i
    while j < len(entries) and entries[j][1] is entries[i][1]:
      j += 1
    grp = entries[i:j]
    scale = None if all(e[2] is None for e in grp) else [1.0 if e[2] is None else float(e[2]) for e in grp]
    res = applications.importance_stats(model, params, grp[0][1], [float(e[0]) for e in grp], rng, batch_size, scale=scale)
    out["times"] += [float(e[0]) for e in grp]
    for k in keys:
      out[k] += [float(v) for v in res[k].cpu()]
    i = j
  return out


def print_fit(res: Dict[str, Any]) -> None:
  """evaluate_fit's table, one line per time"""
  print(f"fit to the known densities ({res['batch_size']} samples per time):  t | log Z | KL | ESS % | max log w")
  for row in zip(res["times"], res["log_Z"], res["KL"], res["ess_pct"], res["max_log_w"]):
    print("  {:.4f} | {:+.4e} | {:.4e} | {:.2f} | {:.3f}".format(*row))


# ---- sample sets against a score: the kernel Stein discrepancy in the full dimension, with no binning ----------------

KSD_KEYS = ("times", "flow", "floor", "ensemble", "ensemble_flow", "flow_own", "stationary", "kind", "n")


def target_draws(target, scale, n, seed):
  """n exact draws of a GaussianMixtureTarget with its covariance times `scale` (None: 1), [n, D] float32 on the host:
  numpy's default_rng(seed), the components by their weights."""
  rng = np.random.default_rng(int(seed))
  comp = rng.choice(target.n_comp, size=int(n), p=np.exp(target.log_weights))
  L = np.linalg.inv(target.W) * float(np.sqrt(1.0 if scale is None else float(scale)))
  return torch.from_numpy((target.means[comp] + rng.standard_normal((int(n), target.dim)) @ L.T).astype(np.float32))


def evaluate_ksd(config, model: FlowModel, params: Params, n=8192, seed=0, kind="imq", h=1e-3) -> Dict[str, Any]:
  """The kernel Stein discrepancy KSD^2_U (utils.ksd, `kind`; the bandwidths are utils.median_bandwidths of the set
  named first below, one choice per line) of sample sets against scores.  Lists with one entry per (t, target, scale) of
  applications.known_densities:
    times
    flow            n flow samples (model.apply.sample of `seed`) against the closed-form score
    floor           n exact draws of the target (target_draws of `seed`) against it: two numbers of one size say the
                    flow's samples are as close to the target as the target's own
  for fp also, at those times, from the n particles of applications.fp_reference_particles (step h, `seed`):
    ensemble        the ensemble against the closed-form score (ou: the exact density along the path; else the initial
                    condition at 0)
    ensemble_flow   the ensemble against the flow's exact score model.apply.score at the ensemble's points
    flow_own        the flow's samples against the flow's score at them: the floor of ensemble_flow
  (None for the other types), and, for fp with an `interaction` section of `role: drift` and the ou drift,
    stationary      {"flow": ..., "particles": [...]}: the stationarity residual at T, the KSD of the flow's samples and
                    of every replica of applications.mv_reference_particles (2 replicas of n) against
                    applications.mv_stationary_score at their own points; else None
  and kind, n.  ValueError, before any device work, for what utils.stein_check_shapes refuses at n and an unknown kind."""
  n = int(n)
  g = config["general"]
  _type, dim = g["type"], g["dim"]
  utils.stein_check_shapes((2, n, dim))
  utils.stein_spec(kind, [1.0])
  entries = applications.known_densities(config)
  ts = [float(e[0]) for e in entries]
  dev = params.flat.device
  flow = [model.apply.sample(params, cond=t, seed=seed, sample_shape=(n,)).float() for t in ts]
  one = lambda x, s, bw: float(utils.ksd(x, s, kind, bw)["ksd2"][0])
  out: Dict[str, Any] = {"times": ts, "flow": [], "floor": [], "ensemble": None, "ensemble_flow": None, "flow_own": None,
                         "stationary": None, "kind": kind, "n": n}
  for x, (t, target, scale) in zip(flow, entries):
    exact = target_draws(target, scale, n, seed).to(dev)
    bw = utils.median_bandwidths(exact)[:utils.STEIN_MAX_TERMS]
    both = utils.ksd(torch.stack([x, exact]), torch.stack([target.score(x, scale), target.score(exact, scale)]), kind, bw)
    out["flow"].append(float(both["ksd2"][0]))
    out["floor"].append(float(both["ksd2"][1]))
  if _type != "fp":
    return out
  f = config["fp"]
  T, a, sigma, sub = float(f["T"]), f["a"], f["sigma"], f["velocity_field_type"]
  pos = applications.fp_reference_particles(dim, T, a, sigma, sub, ts, n, h, seed, positions=True)["pos"].float()
  out["ensemble"], out["ensemble_flow"], out["flow_own"] = [], [], []
  for i, (x, (t, target, scale)) in enumerate(zip(flow, entries)):
    bw = utils.median_bandwidths(pos[i])[:utils.STEIN_MAX_TERMS]
    out["ensemble"].append(one(pos[i], target.score(pos[i], scale), bw))
    both = utils.ksd(torch.stack([pos[i], x]), torch.stack([model.apply.score(params, pos[i].contiguous(), cond=t),
                                                            model.apply.score(params, x.contiguous(), cond=t)]), kind, bw)
    out["ensemble_flow"].append(float(both["ksd2"][0]))
    out["flow_own"].append(float(both["ksd2"][1]))
  if _interaction_kind(config) != "none" and _interaction_role(config) == "drift" and sub == "ou":
    kw, strength = _interaction_kwargs(config), float(config["interaction"]["strength"])
    mv = applications.mv_reference_particles(dim, T, a, sigma, sub, kw, strength, [T], n, 2, h, seed, positions=True)["pos"][0]
    xT = model.apply.sample(params, cond=T, seed=seed, sample_shape=(n,)).float()
    sets = torch.cat([xT[None], mv.float()])
    bw = utils.median_bandwidths(sets[1])[:utils.STEIN_MAX_TERMS]
    res = utils.ksd(sets, applications.mv_stationary_score(sets, a, sigma, sub, kw, strength), kind, bw)["ksd2"].tolist()
    out["stationary"] = {"flow": res[0], "particles": res[1:]}
  return out


def print_ksd(res: Dict[str, Any]) -> None:
  """evaluate_ksd's tables, one line per time"""
  fp = res["ensemble"] is not None
  print("kernel Stein discrepancy KSD^2_U ({} kernel, {} points per set):  t | flow against the closed-form score | exact "
        "draws against it{}".format(res["kind"], res["n"], " | ensemble against it | ensemble against the flow's score | "
                                    "flow against its own score" if fp else ""))
  for i, t in enumerate(res["times"]):
    print("  {:.4f} | {:+.4e} | {:+.4e}".format(t, res["flow"][i], res["floor"][i])
          + (" | {:+.4e} | {:+.4e} | {:+.4e}".format(res["ensemble"][i], res["ensemble_flow"][i], res["flow_own"][i]) if fp else ""))
  if res["stationary"] is not None:
    print("stationarity residual at T (KSD^2_U against the zero-current score): flow {:+.4e} | particle replicas {}".format(
      res["stationary"]["flow"], " ".join("{:+.4e}".format(v) for v in res["stationary"]["particles"])))


KSD_TEST_ROWS = ("flow", "floor", "ensemble", "ensemble_flow", "flow_own")


def evaluate_ksd_test(config, model: FlowModel, params: Params, n=8192, seed=0, kind="imq", h=1e-3,
                      n_boot=255) -> Dict[str, Any]:
  """evaluate_ksd's sets against evaluate_ksd's scores, each value of KSD^2_U read as a p-value: the wild-bootstrap test
  (utils.ksd_bootstrap_test, n_boot vectors of fair signs, utils.rademacher_signs(n, n_boot, seed): the same sign vectors
  for every set and time).  The samples, the scores and the bandwidths are evaluate_ksd's at the same arguments.  Lists
  with one entry per (t, target, scale) of applications.known_densities:
    times
    flow, p_flow            n flow samples against the closed-form score: the value and its p-value
    floor, p_floor          n exact draws of the target against it: the null holds, so these p-values are uniform --
                            the printed calibration check
  for fp also (None for the other types), from the n particles of applications.fp_reference_particles:
    ensemble, p_ensemble            the ensemble against the closed-form score
    ensemble_flow, p_ensemble_flow  the ensemble against the flow's exact score at the ensemble's points
    flow_own, p_flow_own            the flow's samples against the flow's own score: the null holds here as well
  and kind, n, n_boot.  evaluate_ksd's `stationary` row is left out: the particles of an interacting ensemble are
  exchangeable, not independent, and the i.i.d. wild bootstrap does not apply to them (a dependent bootstrap is out of
  scope).  ValueError, before any device work, for what utils.stein_boot_check_shapes refuses at n, an
  unknown kind and an n_boot that utils.rademacher_signs refuses."""
  n = int(n)
  g = config["general"]
  _type, dim = g["type"], g["dim"]
  utils.stein_boot_check_shapes((2, n, dim))
  utils.stein_spec(kind, [1.0])
  signs = utils.rademacher_signs(n, n_boot, seed)
  entries = applications.known_densities(config)
  ts = [float(e[0]) for e in entries]
  dev = params.flat.device
  flow = [model.apply.sample(params, cond=t, seed=seed, sample_shape=(n,)).float() for t in ts]
  out: Dict[str, Any] = {"times": ts, "kind": kind, "n": n, "n_boot": int(n_boot)}
  for k in KSD_TEST_ROWS:
    out[k], out["p_" + k] = ([], []) if _type == "fp" or k in ("flow", "floor") else (None, None)

  def test(names, sets, scores, bw):
    res = utils.ksd_bootstrap_test(torch.stack(sets), torch.stack(scores), kind, bw, signs=signs)
    for i, k in enumerate(names):
      out[k].append(float(res["ksd2"][i]))
      out["p_" + k].append(float(res["p_value"][i]))

  for x, (t, target, scale) in zip(flow, entries):
    exact = target_draws(target, scale, n, seed).to(dev)
    bw = utils.median_bandwidths(exact)[:utils.STEIN_MAX_TERMS]
    test(("flow", "floor"), [x, exact], [target.score(x, scale), target.score(exact, scale)], bw)
  if _type != "fp":
    return out
  f = config["fp"]
  T, a, sigma, sub = float(f["T"]), f["a"], f["sigma"], f["velocity_field_type"]
  pos = applications.fp_reference_particles(dim, T, a, sigma, sub, ts, n, h, seed, positions=True)["pos"].float()
  for i, (x, (t, target, scale)) in enumerate(zip(flow, entries)):
    bw = utils.median_bandwidths(pos[i])[:utils.STEIN_MAX_TERMS]
    test(("ensemble",), [pos[i]], [target.score(pos[i], scale)], bw)
    test(("ensemble_flow", "flow_own"), [pos[i], x], [model.apply.score(params, pos[i].contiguous(), cond=t),
                                                      model.apply.score(params, x.contiguous(), cond=t)], bw)
  return out


def print_ksd_test(res: Dict[str, Any]) -> None:
  """evaluate_ksd_test's table, one line per time: every value with its p-value"""
  fp = res["ensemble"] is not None
  print("wild-bootstrap test of KSD^2_U ({} kernel, {} points per set, {} sign vectors), value (p):  t | flow against the "
        "closed-form score | exact draws against it (uniform p: the calibration){}".format(
          res["kind"], res["n"], res["n_boot"], " | ensemble against it | ensemble against the flow's score | flow "
          "against its own score" if fp else ""))
  for i, t in enumerate(res["times"]):
    print("  {:.4f}".format(t) + "".join(" | {:+.4e} ({:.4f})".format(res[k][i], res["p_" + k][i])
                                         for k in KSD_TEST_ROWS if res[k] is not None))


# ---- the arrays behind the figures (solvers.py:309-493 through cnf_ot/utils.py:598-751) ---------------------------
# The reference's seed points r_, domain ranges [x_min, x_max, y_min, y_max] and time arrays, restated as numbers, keyed
# by (type, subtype or None = any, dim).  times: ("linspace", n) = linspace(0, T, n), or the literal list.
FIGURE_SETTINGS: Dict[Tuple[str, Optional[str], int], Dict[str, Any]] = {
  ("ot", None, 2): {                                                              # solvers.py:400-416
    "r": [[-5.0, 0.0], [5.0, 0.0], [0.0, 5.0], [0.0, -5.0], [3.0, 4.0], [3.0, -4.0], [-3.0, 4.0], [-3.0, -4.0]],
    "domain_range": [-7.5, 7.5, -7.5, 7.5], "times": ("linspace", 5)},
  ("rwpo", "quadratic", 2): {                                                     # solvers.py:421-432, 452
    "r": [[-2.0, -2.0], [-2.0, 2.0], [2.0, -2.0], [2.0, 2.0]],
    "domain_range": [-4.0, 4.0, -4.0, 4.0], "times": ("linspace", 5)},
  ("rwpo", "double_well", 2): {                                                   # solvers.py:436-452
    "r": [[-2.0, -2.0], [-2.0, 0.0], [-2.0, 2.0], [0.0, -2.0], [0.0, 2.0], [2.0, -2.0], [2.0, 0.0], [2.0, 2.0]],
    "domain_range": [-2.0, 2.0, -2.0, 2.0], "times": ("linspace", 5)},
  ("fp", None, 2): {                                                              # solvers.py:468-484
    "r": [[-3.0, -3.0], [-3.0, 0.0], [-3.0, 3.0], [0.0, 3.0], [3.0, 3.0], [3.0, 0.0], [3.0, -3.0], [0.0, -3.0]],
    "domain_range": [-3.0, 3.0, -3.0, 3.0], "times": [0.0, 0.05, 0.1, 0.3, 1.0]},
  ("fp", "lorenz", 3): {                                                          # solvers.py:330-376
    "r": [[-1.0, -1.0, 3.0], [-1.0, 1.0, 3.0], [1.0, -1.0, 3.0], [1.0, 1.0, 3.0]],
    "domain_range": [-2.0, 2.0, -2.0, 2.0], "times": ("linspace", 10),
    "slice": 3.0,                                                                 # utils.py:665-669: z = 3
    "section": ("linspace", -5.0, 5.0, 11),                                       # utils.py:714
    # plot_proj_density's hstack order per direction (utils.py:719-742): (grid axes (X, Y), section axis)
    "directions": {"x": ((1, 2), 0), "y": ((0, 2), 1), "z": ((0, 1), 2)}},
}
FIGURE_GRID = 100        # utils.py:615-616, 662-663, 710


def figure_settings(config) -> Optional[Dict[str, Any]]:
  """The FIGURE_SETTINGS entry of a config with its time array made explicit (t_array: float64 numpy), or None where
  the reference draws nothing (any other dimension; fp at dim 3 with another field than lorenz)."""
  g = config["general"]
  _type, dim = g["type"], g["dim"]
  if _type == "rwpo":
    T, sub = config["rwpo"]["T"], config["rwpo"]["pot_type"]
  elif _type == "fp":
    T, sub = config["fp"]["T"], config["fp"]["velocity_field_type"]
  elif _type == "ot":
    T, sub = 1, config["ot"]["subtype"]                   # solvers.py:81
  else:
    raise Exception(f"Unknown problem type: {_type}...")
  entry = FIGURE_SETTINGS.get((_type, sub, dim), FIGURE_SETTINGS.get((_type, None, dim)))
  if entry is None:
    return None
  out = dict(entry)
  times = entry["times"]
  out["t_array"] = np.linspace(0.0, float(T), times[1]) if isinstance(times, tuple) else np.asarray(times, dtype=np.float64)
  out["r"] = np.asarray(entry["r"], dtype=np.float64)
  if "section" in entry:
    out["section"] = np.linspace(*entry["section"][1:3], entry["section"][3])
  return out


def figure_data(config, model: FlowModel, params: Params, dtype=torch.float32) -> Dict[str, torch.Tensor]:
  """The arrays behind the figures solvers.py:309-493 draws for `config` -- device tensors, nothing drawn:
    t_array [S], r0 [N, D], domain_range [4]
    density [S, 100, 100]      exp(log_prob) on the grid (dim 3: the z = `slice` plane), row i = y_i, column j = x_j
    trajectories [S, N, D]     the characteristics through r0 from t0 = 0
    proj_density_x / _y / _z [S, 100, 100]   (fp / lorenz at dim 3) the mean over 11 sections along that axis
  Two fused launches at dim 2, five at dim 3.  Empty dict where the reference draws nothing."""
  st = figure_settings(config)
  if st is None:
    return {}
  dev = params.flat.device
  dim = config["general"]["dim"]
  t_array, dom = st["t_array"], st["domain_range"]
  out = {"t_array": torch.as_tensor(t_array, device=dev), "r0": torch.as_tensor(st["r"], device=dev).to(dtype),
         "domain_range": torch.as_tensor(np.asarray(dom, dtype=np.float64), device=dev)}
  fixed = None if "slice" not in st else [0.0] * (dim - 1) + [st["slice"]]
  out["density"] = utils.density_on_grid(model, params, t_array, dom, n=FIGURE_GRID, fixed=fixed, dtype=dtype)
  out["trajectories"] = utils.trajectories(model, params, out["r0"], t_array, t0=0.0, dtype=dtype)
  for name, (axes, sec_axis) in st.get("directions", {}).items():
    out["proj_density_" + name] = utils.density_on_grid(model, params, t_array, dom, n=FIGURE_GRID, axes=axes,
                                                        section=st["section"], section_axis=sec_axis, dtype=dtype)
  return out


_SOLVING = {"rwpo": "Solving regularized Wasserstein proximal in {dim}D with lambda{lam}...",
            "fp": "Solving Fokker-Planck equation in {dim}D with lambda{lam}...",
            "ot": "Solving optimal transport in {dim}D with lambda{lam}..."}


def _eval_rng(seed, step):
  """eval_rng, rng = jax.random.split(rng) (solvers.py:110,131): a key of its own, apart from the training steps'."""
  return ((int(seed) ^ 0x5DEECE66DA3B9F1B) + 0x9E3779B97F4A7C15 * (step + 1)) & 0xFFFFFFFFFFFFFFFF


def main(config, epochs: Optional[int] = None, capture: bool = False, save: Optional[str] = None,
         fields: Optional[str] = None, path_errors: bool = False, fit: bool = False,
         two_sample: bool = False, ot_reference: bool = False, sliced: bool = False, knn: bool = False,
         interaction: bool = False, mv_path: bool = False, ksd: bool = False, field_errors: bool = False,
         permutation_test: bool = False, ksd_test: bool = False, rwpo_particles: bool = False,
         grid_reference: bool = False) -> Dict[str, Any]:
  """solvers.py:26-308 without plots: train, then print the reference's lines in its wording and return
  `evaluate`'s dict.  For ot, the density-fit KL is printed every eval_frequency steps (:108-116).  path_errors: print
  evaluate_path's table after them (rwpo at dim 2), or evaluate_fp_path's (fp).  fit: print evaluate_fit's table (the
  returned dict is `evaluate`'s either way).  two_sample (fp): print evaluate_fp_two_sample's table.  ot_reference (ot):
  print evaluate_ot_reference's lines.  sliced (fp): print evaluate_fp_sliced's table.  knn (fp): print evaluate_fp_knn's
  table.  interaction (an `interaction` section with a kind): print evaluate_interaction's table.  mv_path (fp with an
  `interaction` section whose role is drift): print evaluate_mv_path's table.  ksd: print evaluate_ksd's tables.
  field_errors (fp): print evaluate_fp_fields' table.  permutation_test (fp): print evaluate_fp_permutation's table.
  ksd_test: print evaluate_ksd_test's table.  rwpo_particles (rwpo, any dim): print evaluate_rwpo_particles' lines.
  grid_reference (fp at dim 2): print evaluate_fp_grid's table."""
  g, tr = config["general"], config["train"]
  _type, dim, seed = g["type"], g["dim"], g["seed"]
  if _type not in _SOLVING:
    raise Exception(f"Unknown problem type: {_type}...")
  if two_sample and _type != "fp":      # (before the training run, not after it)
    raise ValueError(f"--two-sample compares the flow with the fp particle reference: not defined for {_type}")
  if permutation_test and _type != "fp":
    raise ValueError(f"--permutation-test compares the flow with the fp particle reference: not defined for {_type}")
  if sliced and _type != "fp":
    raise ValueError(f"--sliced compares the flow with the fp particle reference: not defined for {_type}")
  if knn and _type != "fp":
    raise ValueError(f"--knn compares the flow with the fp particle reference: not defined for {_type}")
  if field_errors and _type != "fp":
    raise ValueError(f"--field-errors compares the flow's fields with the fp particle reference's: not defined for {_type}")
  if interaction and _interaction_kind(config) == "none":
    raise ValueError("--interaction prints the interaction energy of the config's `interaction` section: its kind is 'none'")
  if mv_path and (_type != "fp" or _interaction_kind(config) == "none" or _interaction_role(config) != "drift"):
    raise ValueError("--mv-path compares an fp flow trained with the interaction in its drift (`role: drift`) with the "
                     "interacting particle reference")
  if rwpo_particles and _type != "rwpo":
    raise ValueError(f"--rwpo-particles compares an rwpo flow with the particle reference of its optimal path: not defined for {_type}")
  if grid_reference and (_type != "fp" or dim != 2):
    raise ValueError(f"--grid-reference compares an fp flow at dim 2 with the grid solution of its Fokker-Planck equation: "
                     f"not defined for {_type} at dim {dim}")
  if ot_reference and _type != "ot":
    raise ValueError(f"--ot-reference compares an ot flow with Sinkhorn divergences of its samples: not defined for {_type}")
  print(_SOLVING[_type].format(dim=dim, lam=tr["_lambda"]), flush=True)

  def log(step, loss):
    desc = f"step {step}: loss={loss:.4e}"
    if _type == "ot":
      # train() hands its callback (step, loss) only; the model and the parameters it is training are its locals
      # (the parameters are updated in place, so they are the current ones)
      f = sys._getframe(1).f_locals
      KL = float(applications.density_fit_kl_loss_fn(f["model"], dim, 1, f["params"], _eval_rng(seed, step),
                                                      tr["batch_size"]))
      desc += f"KL={KL:.4f}"
    print(desc, flush=True)

  model, params, hist = train(config, epochs=epochs, log=log, capture=capture)
  if hist:
    print(f"loss={float(hist[-1]):.4e}")
  if save:
    np.savez(save, params=params.flat.detach().cpu().numpy())
  if fields:
    np.savez(fields, **{k: v.detach().cpu().numpy() for k, v in figure_data(config, model, params).items()})
  res = evaluate(config, model, params, _eval_rng(seed, -1))
  print("Network parameters: {}".format(res["param_count"]))
  if _type == "ot":
    print("kinetic energy with more samples: {:.3e}".format(res["kinetic_energy_more"]))
    print("kinetic energy with less samples: {:.3e}".format(res["kinetic_energy_less"]))
  elif _type == "rwpo":
    print(f"kinetic energy: {res['e_kin']:.3e}")
    print(f"potential energy: {res['e_pot']:.3e}")
    if res["true_val"] is None:
      print(f"total energy: {res['total']:.3e}|relative err: n/a (no reference value for this potential)")
    else:
      print("total energy: {:.3e}|relative err: {:.3e}".format(res["total"], res["rel_err_pct"]))
    if res["true_val_quadrature"] is not None:
      print(f"density squared error against the exact solution: {res['density_sq_err']:.3e}")
      print("total energy: {:.3e}|relative err against the quadrature value {:.6f}: {:.3e}".format(
        res["total"], res["true_val_quadrature"], res["rel_err_pct_quadrature"]))
  else:
    print("L2 error via Monte-Carlo: {:.3e}".format(res["l2_mc"]))
    if res["l2_grid"] is not None:
      print("L2 error on grid: {:.3e}".format(res["l2_grid"]))
    print("L2 error via Monte-Carlo against the initial condition N(0, (T+1)/2 I): {:.3e}".format(res["l2_mc_ic"]))
    print("variance at T: {} | closed form: {:.4f}".format(" ".join(f"{v:.4f}" for v in res["var_T"]),
                                                          res["var_T_closed_form"]))
  if path_errors and _type == "fp":
    print_fp_path_errors(evaluate_fp_path(config, model, params))
  elif path_errors:
    print_path_errors(evaluate_path(config, model, params))
  if fit:
    print_fit(evaluate_fit(config, model, params, _eval_rng(seed, -2)))
  if two_sample:
    print_fp_two_sample(evaluate_fp_two_sample(config, model, params))
  if ot_reference:
    print_ot_reference(evaluate_ot_reference(config, model, params))
  if sliced:
    print_fp_sliced(evaluate_fp_sliced(config, model, params))
  if knn:
    print_fp_knn(evaluate_fp_knn(config, model, params))
  if interaction:
    print_interaction(evaluate_interaction(config, model, params))
  if mv_path:
    print_mv_path(evaluate_mv_path(config, model, params))
  if ksd:
    print_ksd(evaluate_ksd(config, model, params))
  if ksd_test:
    print_ksd_test(evaluate_ksd_test(config, model, params))
  if field_errors:
    print_fp_fields(evaluate_fp_fields(config, model, params))
  if permutation_test:
    print_fp_permutation(evaluate_fp_permutation(config, model, params))
  if rwpo_particles:
    print_rwpo_particles(evaluate_rwpo_particles(config, model, params))
  if grid_reference:
    print_fp_grid(evaluate_fp_grid(config, model, params))
  return res


def _parse(argv):
  p = argparse.ArgumentParser(prog="python -m cnf_ot_amd.solvers",
                              description="Train a cnf_ot configuration on the HIP engine and print its evaluation.")
  p.add_argument("--config", default=None, help="config file (mfc.yaml layout); default: the checked-in defaults")
  p.add_argument("--epochs", type=int, default=None, help="training steps (default: train.epochs)")
  p.add_argument("--capture", action="store_true", help="replay each training step as one captured HIP graph")
  p.add_argument("--save", default=None, help="write the trained flat parameters to this .npz file")
  p.add_argument("--fields", default=None, help="write the arrays behind the reference's figures (figure_data) to this .npz file")
  p.add_argument("--path-errors", action="store_true",
                 help="print the density and velocity errors against the exact solution at 9 times (rwpo at dim 2), or the "
                      "errors against the particle reference at the figure's times (fp)")
  p.add_argument("--fit", action="store_true",
                 help="print log Z, KL and the effective sample size of the flow against every density of the problem that "
                      "is known in closed form (1 M samples per time)")
  p.add_argument("--two-sample", action="store_true",
                 help="print MMD^2 and the energy distance, in the full dimension, between the flow's samples and the "
                      "particle reference at the figure's times, each beside its Monte-Carlo floor (fp)")
  p.add_argument("--ot-reference", action="store_true",
                 help="print the Sinkhorn divergence between source and target samples, the flow's coupling cost and "
                      "kinetic energy beside it, and the distance of the flow's map from the barycentric map (ot)")
  p.add_argument("--sliced", action="store_true",
                 help="print the sliced Wasserstein distance, in the full dimension and at the full ensemble size, between "
                      "the flow's samples and the particle reference, and the exact W2 of every marginal (fp)")
  p.add_argument("--knn", action="store_true",
                 help="print the nearest-neighbour estimates of KL, in nats and in the full dimension, between the flow's "
                      "samples and the particle reference, beside their floor, and the flow's entropy two ways (fp)")
  p.add_argument("--interaction", action="store_true",
                 help="print the interaction energy of the flow's samples along the path, beside its Monte-Carlo floor, and "
                      "the running cost (a config with an `interaction` section whose kind is not none)")
  p.add_argument("--mv-path", action="store_true",
                 help="print the mean, tr cov and interaction energy of the flow's samples beside the interacting particle "
                      "reference and its replica floors (fp with an `interaction` section whose role is drift)")
  p.add_argument("--ksd", action="store_true",
                 help="print the kernel Stein discrepancy of the flow's samples against every closed-form score of the "
                      "problem beside its floor, for fp the particle ensemble against that score and against the flow's "
                      "exact score, and with an interaction in the ou drift the stationarity residual at T")
  p.add_argument("--ksd-test", action="store_true",
                 help="print the same discrepancies (without the stationarity residual) with their wild-bootstrap p-values "
                      "(255 sign vectors): the exact draws' p-values are uniform, the calibration check")
  p.add_argument("--field-errors", action="store_true",
                 help="print the errors of the flow's log-density, score and velocity, in the full dimension, against the "
                      "kernel density estimate of the particle reference, each beside its Monte-Carlo floor (fp)")
  p.add_argument("--permutation-test", action="store_true",
                 help="print MMD^2 and the energy distance between the flow's samples and the particle reference with "
                      "their permutation p-values (255 relabellings), beside the same test between the reference's two "
                      "halves (fp)")
  p.add_argument("--rwpo-particles", action="store_true",
                 help="print the optimal energy from the particle reference of the rwpo problem, its standard error, bias "
                      "and effective sample size, and the flow's mean, covariance and histogram errors against the "
                      "reference's Brownian bridges along the path, beside their floor (rwpo, any dimension)")
  p.add_argument("--grid-reference", action="store_true",
                 help="print the L1, relative L2 and tail log-density errors of the flow's density against the float64 "
                      "finite-volume solution of the Fokker-Planck equation on a grid, and both sets of moments (fp, dim 2)")
  return p.parse_args(argv)


if __name__ == "__main__":
  args = _parse(sys.argv[1:])
  main(load_config(args.config), epochs=args.epochs, capture=args.capture, save=args.save, fields=args.fields,
       path_errors=args.path_errors, fit=args.fit, two_sample=args.two_sample, ot_reference=args.ot_reference,
       sliced=args.sliced, knn=args.knn, interaction=args.interaction, mv_path=args.mv_path, ksd=args.ksd,
       field_errors=args.field_errors, permutation_test=args.permutation_test, ksd_test=args.ksd_test,
       rwpo_particles=args.rwpo_particles, grid_reference=args.grid_reference)
