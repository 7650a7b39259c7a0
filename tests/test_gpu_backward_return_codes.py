"""What the backward entry points that take a model return for a call they do not serve, and in which order they ask.

One table: entry point x state of the model x what is wrong with the call -> the code, and how many of the call's sums
were zeroed on the way.  The order of the host checks decides which code a doubly-wrong call gets (a model without
parameters AND a config the backward does not serve; no gradient slabs AND an empty call ...), and callers branch on
these codes: CNF_ERR_UNSUPPORTED sends solvers.py to another route, CNF_ERR_INVALID raises.  Every pointer passed is a
device allocation of the size a correct call would need; nothing here relies on a bad pointer being caught.

Shapes: dim 2, two flow layers, 128 points in two slices of 64; dim 3 for cnf_score_fd_vjp's drift check.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, INV, UNS = 0, -22, -95
N, COUNT = 128, 64                    # points, points per slice
FILL = 7.25                           # of the sums before every call


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


class Ctx:
  """One model in one state, and valid buffers for every entry point at its dimension."""

  def __init__(self, dev, load, enable, **cfg_kw):
    from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
    from cnf_ot_amd.flows import _stream_ptr
    assert (_capi.CNF_OK, _capi.CNF_ERR_INVALID, _capi.CNF_ERR_UNSUPPORTED) == (OK, INV, UNS)
    self.capi, self.cfg = _capi, FlowConfig(**cfg_kw)
    D = self.D = self.cfg.dim
    params = Params.random(self.cfg, 0.2, seed=11, device=dev)
    self.eng = FlowEngine(self.cfg, dev)
    if load:
      self.eng.load(params)
    self.lib, self.h, self.st = self.eng.lib, self.eng._h, _stream_ptr(dev)
    self.enabled = self.lib.cnf_grad_enable(self.h, 0) if enable else None
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    self.flat = params.flat.contiguous()
    self.grad = torch.zeros(self.cfg.param_count(), device=dev)
    self.pts, self.ybar, self.ldbar, self.gbar = rnd(N, D), rnd(N, D), rnd(N), rnd(N, D)
    self.out, self.lp = torch.zeros(N, D, device=dev), torch.zeros(N, device=dev)
    self.c = torch.linspace(0.2, 0.8, 8, device=dev)
    self.r3, self.rbar3 = rnd(3 * N, D), torch.zeros(3 * N, D, device=dev)
    self.sums = torch.full((4,), FILL, dtype=torch.float64, device=dev)
    self.work = torch.zeros(4 * 6 * COUNT, device=dev)       # kinetic + potential: 3 sets x 2 slices x 64 points, r | rbar

  # ---- the calls: what a correct one looks like, with the arguments a row changes as keywords --------------------------
  def pass_vjp(self, B=N, c_block=COUNT):
    return self.lib.cnf_pass_vjp(self.h, 1, self.pts.data_ptr(), self.c.data_ptr(), c_block, self.ybar.data_ptr(),
                                 self.ldbar.data_ptr(), self.out.data_ptr(), self.grad.data_ptr(), self.flat.data_ptr(), B, self.st)

  def input_vjp(self, B=N, c_block=COUNT):
    return self.lib.cnf_input_vjp(self.h, 1, self.pts.data_ptr(), self.c.data_ptr(), c_block, self.ybar.data_ptr(),
                                  self.ldbar.data_ptr(), self.out.data_ptr(), B, self.st)

  def score(self, n_slices=2, count=COUNT):
    return self.lib.cnf_score(self.h, self.pts.data_ptr(), 0, self.c.data_ptr(), n_slices, count, self.out.data_ptr(),
                              self.lp.data_ptr(), self.st)

  def loss_terms_grad(self, B=COUNT, n_slices=2, kind="kinetic", dt=0.01, dx=0.01):
    kinds = {"kinetic": self.capi.TERM_KINETIC, "kinetic_score": self.capi.TERM_KINETIC_SCORE}
    spec = self.capi.CnfLossSpec(kind=kinds[kind], dt=dt, dx=dx, coef=0.1)
    return self.lib.cnf_loss_terms_grad(self.h, ctypes.byref(spec), self.pts.data_ptr(), 0, self.c.data_ptr(), n_slices, B,
                                        1.0, self.sums.data_ptr(), self.grad.data_ptr(), self.flat.data_ptr(), self.st)

  def logprob_fd_vjp(self, B=N, c_block=COUNT, dx=0.01):
    return self.lib.cnf_logprob_fd_vjp(self.h, self.pts.data_ptr(), self.c.data_ptr(), c_block, dx, self.gbar.data_ptr(),
                                       self.out.data_ptr(), self.grad.data_ptr(), self.flat.data_ptr(), B, self.st)

  def score_fd_vjp(self, n=N, count=COUNT, dt=0.01, dx=0.01, drift="none"):
    code = {"none": -1, "ou": self.capi.DRIFTS["ou"], "smile": self.capi.DRIFTS["smile"], "lorenz": self.capi.DRIFTS["lorenz"]}[drift]
    return self.lib.cnf_score_fd_vjp(self.h, self.r3.data_ptr(), self.c.data_ptr(), count, dt, dx, 0.1, code, 1.0, 1.0,
                                     self.sums.data_ptr(), self.rbar3.data_ptr(), self.grad.data_ptr(), self.flat.data_ptr(), n, self.st)

  def neg_logprob_vjp(self, B=N, c_block=COUNT):
    return self.lib.cnf_neg_logprob_vjp(self.h, self.pts.data_ptr(), self.c.data_ptr(), c_block, 1.0, self.sums.data_ptr(),
                                        self.grad.data_ptr(), self.flat.data_ptr(), B, self.st)

  def kinetic_potential_vjp(self, count=COUNT, S=2, dt=0.1, subtype=0, pot=True, grad=True):
    return self.lib.cnf_kinetic_potential_vjp(self.h, self.pts.data_ptr(), count, self.c.data_ptr(), S, dt, 1.0, subtype, 1.0, 1.0,
                                              self.sums.data_ptr(), self.sums[2:].data_ptr() if pot else None,
                                              self.grad.data_ptr() if grad else None, self.flat.data_ptr(), self.work.data_ptr(), self.st)


# The states of a model: (parameters set, cnf_grad_enable called, config).  cnf_grad_enable declines a config the
# backward does not serve, so such a model never has gradient slabs.
STATES = {
  "ready": (True, True, {}),
  "no slabs": (True, False, {}),
  "no params": (False, True, {}),
  "no params, no slabs": (False, False, {}),
  "hidden 32": (True, True, {"hidden_size": 32}),
  "hidden 32, no params": (False, True, {"hidden_size": 32}),
  "periodized": (True, True, {"periodized": True}),
  "ready, dim 3": (True, True, {"dim": 3}),
  "no params, dim 3": (False, True, {"dim": 3}),
}


@pytest.fixture(scope="module")
def ctxs(dev):
  made = {}

  def get(state):
    if state not in made:
      load, enable, cfg_kw = STATES[state]
      made[state] = Ctx(dev, load, enable, dim=cfg_kw.get("dim", 2), **{k: v for k, v in cfg_kw.items() if k != "dim"})
      served = not cfg_kw or set(cfg_kw) == {"dim"}
      assert made[state].enabled in (None, OK if served else UNS)
    return made[state]
  return get


# (entry point, state, changed arguments, code, sums zeroed).  The rows after the first of a group are the pairs the
# order of the checks tells apart.
TABLE = [
  # ---- cnf_pass_vjp (with a parameter gradient) -------------------------------------------------------------------------
  ("pass_vjp", "no params", {}, INV, 0),
  ("pass_vjp", "no slabs", {}, INV, 0),
  ("pass_vjp", "hidden 32", {}, UNS, 0),
  ("pass_vjp", "periodized", {}, UNS, 0),
  ("pass_vjp", "ready", {"B": -1}, INV, 0),
  ("pass_vjp", "ready", {"c_block": 0}, INV, 0),
  ("pass_vjp", "ready", {"B": 0}, OK, 0),
  ("pass_vjp", "hidden 32, no params", {}, INV, 0),            # the parameters are asked for before the config
  ("pass_vjp", "hidden 32", {"B": -1}, INV, 0),                # the arguments before the config
  ("pass_vjp", "hidden 32", {"B": 0}, UNS, 0),                 # the config before the empty call
  ("pass_vjp", "no params", {"B": 0}, INV, 0),                 # the parameters before the empty call
  ("pass_vjp", "no slabs", {"B": 0}, OK, 0),                   # the empty call before the slabs
  # ---- cnf_input_vjp (no parameter gradient: needs no slabs) ------------------------------------------------------------
  ("input_vjp", "no params", {}, INV, 0),
  ("input_vjp", "no slabs", {}, OK, 0),
  ("input_vjp", "hidden 32", {}, UNS, 0),
  ("input_vjp", "periodized", {}, UNS, 0),
  ("input_vjp", "ready", {"B": -1}, INV, 0),
  ("input_vjp", "ready", {"c_block": 0}, INV, 0),
  ("input_vjp", "ready", {"B": 0}, OK, 0),
  ("input_vjp", "hidden 32, no params", {}, INV, 0),
  ("input_vjp", "hidden 32", {"c_block": 0}, INV, 0),
  ("input_vjp", "hidden 32", {"B": 0}, UNS, 0),
  # ---- cnf_score (needs no slabs) ----------------------------------------------------------------------------------------
  ("score", "no params", {}, INV, 0),
  ("score", "no slabs", {}, OK, 0),
  ("score", "hidden 32", {}, UNS, 0),
  ("score", "periodized", {}, UNS, 0),
  ("score", "ready", {"count": -1}, INV, 0),
  ("score", "ready", {"n_slices": -1}, INV, 0),
  ("score", "ready", {"count": 0}, OK, 0),
  ("score", "ready", {"n_slices": 0}, OK, 0),
  ("score", "hidden 32, no params", {}, INV, 0),
  ("score", "hidden 32", {"count": -1}, INV, 0),
  ("score", "hidden 32", {"count": 0}, UNS, 0),
  ("score", "no params", {"n_slices": 0}, INV, 0),
  # ---- cnf_loss_terms_grad -----------------------------------------------------------------------------------------------
  ("loss_terms_grad", "no params", {}, INV, 0),
  ("loss_terms_grad", "no slabs", {}, INV, 2),                 # the sums are zeroed before the slabs are asked for
  ("loss_terms_grad", "hidden 32", {}, UNS, 0),
  ("loss_terms_grad", "periodized", {}, UNS, 0),
  ("loss_terms_grad", "ready", {"B": -1}, INV, 0),
  ("loss_terms_grad", "ready", {"n_slices": -1}, INV, 0),
  ("loss_terms_grad", "ready", {"dt": 0.0}, INV, 0),
  ("loss_terms_grad", "ready", {"dt": -0.01}, INV, 0),
  ("loss_terms_grad", "ready", {"kind": "kinetic_score", "dx": 0.0}, INV, 0),
  ("loss_terms_grad", "ready", {"B": 0}, OK, 2),
  ("loss_terms_grad", "ready", {"n_slices": 0}, OK, 0),
  ("loss_terms_grad", "hidden 32, no params", {}, INV, 0),
  ("loss_terms_grad", "hidden 32", {"dt": 0.0}, UNS, 0),       # the config before the term's spec
  ("loss_terms_grad", "hidden 32", {"B": 0}, UNS, 0),
  ("loss_terms_grad", "no params", {"dt": 0.0}, INV, 0),
  ("loss_terms_grad", "no slabs", {"dt": 0.0}, INV, 0),        # the spec before the sums: nothing zeroed
  ("loss_terms_grad", "no slabs", {"B": 0}, OK, 2),            # the empty call before the slabs
  # ---- cnf_logprob_fd_vjp ------------------------------------------------------------------------------------------------
  ("logprob_fd_vjp", "no params", {}, INV, 0),
  ("logprob_fd_vjp", "no slabs", {}, INV, 0),
  ("logprob_fd_vjp", "hidden 32", {}, UNS, 0),
  ("logprob_fd_vjp", "periodized", {}, UNS, 0),
  ("logprob_fd_vjp", "ready", {"B": -1}, INV, 0),
  ("logprob_fd_vjp", "ready", {"c_block": 0}, INV, 0),
  ("logprob_fd_vjp", "ready", {"dx": 0.0}, INV, 0),
  ("logprob_fd_vjp", "ready", {"dx": -0.01}, INV, 0),
  ("logprob_fd_vjp", "ready", {"B": 0}, OK, 0),
  ("logprob_fd_vjp", "hidden 32, no params", {}, INV, 0),
  ("logprob_fd_vjp", "hidden 32", {"dx": 0.0}, INV, 0),
  ("logprob_fd_vjp", "hidden 32", {"B": 0}, UNS, 0),
  ("logprob_fd_vjp", "no slabs", {"B": 0}, OK, 0),
  # ---- cnf_score_fd_vjp --------------------------------------------------------------------------------------------------
  ("score_fd_vjp", "no params", {}, INV, 0),
  ("score_fd_vjp", "no slabs", {}, INV, 2),                    # the sums are zeroed before the slabs are asked for
  ("score_fd_vjp", "hidden 32", {}, UNS, 0),
  ("score_fd_vjp", "periodized", {}, UNS, 0),
  ("score_fd_vjp", "ready", {"n": -1}, INV, 0),
  ("score_fd_vjp", "ready", {"count": 0}, INV, 0),
  ("score_fd_vjp", "ready", {"dt": 0.0}, INV, 0),
  ("score_fd_vjp", "ready", {"dx": 0.0}, INV, 0),
  ("score_fd_vjp", "ready", {"n": 0}, OK, 0),
  ("score_fd_vjp", "ready", {"drift": "smile"}, UNS, 0),       # the coupled fields: cnf_loss_terms_grad serves them
  ("score_fd_vjp", "ready, dim 3", {"drift": "lorenz"}, UNS, 0),
  ("score_fd_vjp", "no params, dim 3", {"drift": "lorenz"}, UNS, 0),      # the drift before the parameters
  ("score_fd_vjp", "ready, dim 3", {"drift": "lorenz", "dt": 0.0}, INV, 0),      # the arguments before the drift
  ("score_fd_vjp", "no params, dim 3", {"drift": "ou"}, INV, 0),
  ("score_fd_vjp", "hidden 32, no params", {}, INV, 0),
  ("score_fd_vjp", "hidden 32", {"n": 0}, UNS, 0),
  ("score_fd_vjp", "no params", {"n": 0}, INV, 0),
  ("score_fd_vjp", "no slabs", {"n": 0}, OK, 0),
  # ---- cnf_neg_logprob_vjp: the slabs are asked for with the parameters, before the config and the empty call ------------
  ("neg_logprob_vjp", "no params", {}, INV, 0),
  ("neg_logprob_vjp", "no slabs", {}, INV, 0),
  ("neg_logprob_vjp", "hidden 32", {}, INV, 0),                # (no slabs: cnf_grad_enable declined)
  ("neg_logprob_vjp", "periodized", {}, INV, 0),
  ("neg_logprob_vjp", "ready", {"B": -1}, INV, 0),
  ("neg_logprob_vjp", "ready", {"c_block": 0}, INV, 0),
  ("neg_logprob_vjp", "ready", {"B": 0}, OK, 0),
  ("neg_logprob_vjp", "no slabs", {"B": 0}, INV, 0),
  ("neg_logprob_vjp", "hidden 32", {"B": 0}, INV, 0),
  # ---- cnf_kinetic_potential_vjp -----------------------------------------------------------------------------------------
  ("kinetic_potential_vjp", "no params", {}, INV, 0),
  ("kinetic_potential_vjp", "no slabs", {}, INV, 0),
  ("kinetic_potential_vjp", "hidden 32", {}, INV, 0),          # (no slabs) ...
  ("kinetic_potential_vjp", "hidden 32", {"grad": False}, UNS, 0),      # ... and without a gradient: no table route
  ("kinetic_potential_vjp", "periodized", {"grad": False}, UNS, 0),
  ("kinetic_potential_vjp", "ready", {"count": 0}, INV, 0),
  ("kinetic_potential_vjp", "ready", {"S": 0}, INV, 0),
  ("kinetic_potential_vjp", "ready", {"dt": 0.0}, INV, 0),
  ("kinetic_potential_vjp", "ready", {"subtype": 3}, INV, 0),
  ("kinetic_potential_vjp", "ready", {"subtype": -1}, INV, 0),          # no potential asked for, but its sums given
  ("kinetic_potential_vjp", "ready", {"pot": False}, INV, 0),           # a potential asked for, but no sums
  ("kinetic_potential_vjp", "hidden 32, no params", {"grad": False}, INV, 0),
  ("kinetic_potential_vjp", "hidden 32", {"grad": False, "dt": 0.0}, INV, 0),
]


def test_the_table_covers_every_entry_point_and_reason():
  entries = {row[0] for row in TABLE}
  assert entries == {"pass_vjp", "input_vjp", "score", "loss_terms_grad", "logprob_fd_vjp", "score_fd_vjp", "neg_logprob_vjp",
                     "kinetic_potential_vjp"}
  for e in entries:
    states = {row[1] for row in TABLE if row[0] == e}
    assert {"no params", "no slabs", "hidden 32", "periodized"} <= states, e
  assert len(set((e, s, tuple(sorted(kw.items()))) for e, s, kw, _, _ in TABLE)) == len(TABLE)


def test_backward_entry_points_return_the_tabled_codes(ctxs):
  """Every row of TABLE, in one pass (the models are made once per state); all mismatches are reported together."""
  wrong = []
  for entry, state, kw, code, zeroed in TABLE:
    ctx = ctxs(state)
    ctx.sums.fill_(FILL)
    rc = getattr(ctx, entry)(**kw)
    torch.cuda.synchronize()
    sums = ctx.sums.cpu().tolist()
    # (the only rows that launch a kernel are cnf_input_vjp and cnf_score without slabs: they take no sums)
    if rc != code or sums != [0.0] * zeroed + [FILL] * (4 - zeroed):
      wrong.append((entry, state, kw, f"got {rc} want {code}", sums))
  print(f"{len(TABLE)} rows, {len(wrong)} wrong")
  assert not wrong, "\n".join(map(str, wrong))
