"""Differentiable flow passes for torch.autograd.

`flow_forward(engine, flat_params, x, c)` / `flow_inverse(...)` return
(points, log|det J|) and are differentiable w.r.t. the parameters and the input
points: forward = the fused HIP flow kernel, backward = `cnf_pass_vjp` (the
backward kernels of cnf_grad.hip and cnf_grad_pwl.hip).  Any loss composed
from these on the host gets the gradients jax.value_and_grad gives the reference
(cnf_ot/mfc/solvers.py:94) -- the fused loss kernels of
`cnf_ot_amd.applications` are the fast path for the reference's own losses,
this is the general one (and the one that parallelises the 2*dim log_prob
evaluations of the score terms over the whole GPU at large dim).

The condition `c` is not differentiated (the reference differentiates w.r.t.
the parameters only; its time derivatives are finite differences).
"""
import torch

from . import _capi, interaction, stein, two_sample
from .flows import FlowEngine, _stream_ptr


class _FlowPass(torch.autograd.Function):

  @staticmethod
  def forward(ctx, flat, x, c, engine: FlowEngine, to_base: bool):
    engine.load(flat)
    x = x.contiguous()
    out, ld = (engine.inverse_logdet if to_base else engine.forward_logdet)(x, c)
    ctx.save_for_backward(flat, x, c)
    ctx.engine, ctx.to_base = engine, to_base
    return out, ld

  @staticmethod
  def backward(ctx, g_out, g_ld):
    flat, x, c = ctx.saved_tensors
    eng = ctx.engine
    eng.load(flat)
    need_p, need_x = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    grad = torch.zeros_like(flat) if need_p else None
    xbar = eng.pass_vjp(x, c, g_out, g_ld, ctx.to_base, grad=grad, want_xbar=need_x)
    return grad, xbar, None, None, None


def flow_forward(engine: FlowEngine, flat_params: torch.Tensor, x: torch.Tensor, c):
  """base -> data: (y, log|det J|), differentiable in flat_params and x."""
  return _FlowPass.apply(flat_params, x, _cond_tensor(engine, c), engine, False)


def flow_inverse(engine: FlowEngine, flat_params: torch.Tensor, y: torch.Tensor, c):
  """data -> base: (x, log|det J^-1|), differentiable in flat_params and y."""
  return _FlowPass.apply(flat_params, y, _cond_tensor(engine, c), engine, True)


def log_prob(engine: FlowEngine, flat_params: torch.Tensor, value: torch.Tensor, c):
  """ConditionalTransformed.log_prob (conditional.py:316-321), differentiable."""
  x, ildj = flow_inverse(engine, flat_params, value, c)
  return (-0.5 * x * x).sum(1) - 0.5 * x.shape[1] * 1.8378770664093453 + ildj


class _LogProbFD(torch.autograd.Function):
  """score[i, d] = (log_prob(r_i + dx/2 e_d) - log_prob(r_i - dx/2 e_d)) / dx (applications.py:264-273):
  forward cnf_logprob_fd, backward cnf_logprob_fd_vjp -- the 2 D evaluation points per sample exist only inside
  the kernels."""

  @staticmethod
  def forward(ctx, flat, pts, c, engine: FlowEngine, dx: float):
    engine.load(flat)
    pts = pts.contiguous()
    score = engine.logprob_fd(pts, c, dx)
    ctx.save_for_backward(flat, pts, c)
    ctx.engine, ctx.dx = engine, dx
    return score

  @staticmethod
  def backward(ctx, gbar):
    flat, pts, c = ctx.saved_tensors
    eng = ctx.engine
    eng.load(flat)
    grad = torch.zeros_like(flat)
    pts_bar = eng.logprob_fd_vjp(pts, c, ctx.dx, gbar.contiguous(), grad, want_pts_bar=ctx.needs_input_grad[1])
    return (grad if ctx.needs_input_grad[0] else None), pts_bar, None, None, None


def logprob_fd(engine: FlowEngine, flat_params: torch.Tensor, pts: torch.Tensor, c, dx: float):
  """Central-difference score of log_prob, differentiable in flat_params and pts."""
  return _LogProbFD.apply(flat_params, pts, _cond_tensor(engine, c), engine, float(dx))


def _cond_tensor(engine, c):
  if not torch.is_tensor(c):
    c = torch.as_tensor(c, dtype=torch.float32)
  return c.to(device=engine.device, dtype=torch.float32).reshape(-1)



class _PointSetStat(torch.autograd.Function):
  """A symmetric statistic of two point sets whose call returns the value and its gradient in x (two_sample.mmd2,
  sinkhorn, sliced_wasserstein): the gradient in x from the forward call, in y from a second call with the roles
  swapped.  stat(x, y, want_grad, first) returns the statistic's dict; `first` is None in the forward call and the
  forward call's dict in the swapped one.  key: the value's entry."""

  @staticmethod
  def forward(ctx, x, y, stat, key):
    need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    res = stat(x.detach(), y.detach(), need_x, None)
    gy = stat(y.detach(), x.detach(), True, res)["grad"] if need_y else None
    ctx.save_for_backward(res.get("grad"), gy)
    return res[key]

  @staticmethod
  def backward(ctx, gbar):
    gx, gy = ctx.saved_tensors
    w = gbar.to(torch.float32)
    scale = lambda g: None if g is None else (g * w[:, None, None] if g.dim() == 3 else g * w[0])
    return scale(gx), scale(gy), None, None


def mmd2(x: torch.Tensor, y: torch.Tensor, bandwidths, kind: str = "gaussian"):
  """The unbiased MMD^2 (kind="gaussian", up to 8 bandwidths) or energy distance (kind="energy") between the sample
  sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D], [S] float64 ([1] for 2-D inputs), differentiable in x and y:
  with `flow_forward` a flow trains on samples through ordinary autograd (applications.mmd_loss_fn is the hand-written
  fast path).  The bandwidths are constants (utils.median_bandwidths(y) gives the usual choice)."""
  return _PointSetStat.apply(x, y, lambda a, b, want_grad, first: two_sample.mmd2(a, b, bandwidths, kind, want_grad),
                             "mmd2")


def sinkhorn_divergence(x: torch.Tensor, y: torch.Tensor, eps: float = 0.05, schedule=None):
  """The Sinkhorn divergence S_eps (cost |x - y|^2 / 2, uniform weights) between the sample sets x [N, D] or [S, N, D]
  and y [M, D] or [S, M, D], [S] float64 ([1] for 2-D inputs), differentiable in x (and in y, by a second call) through
  the ENVELOPE gradient of cnf_sinkhorn: the potentials are held fixed, which is exact at the fixed point of the
  recursion (utils.sinkhorn's `change` says how far the schedule stopped from it).  The schedule is a constant
  (None: utils.sinkhorn_schedule(x, y, eps)).  With `flow_forward` a flow trains on target samples in transport units
  through ordinary autograd (applications.sinkhorn_loss_fn is the hand-written fast path)."""
  # (the swapped call runs on the schedule the forward call resolved)
  stat = lambda a, b, want_grad, first: two_sample.sinkhorn(a, b, eps, schedule if first is None else first["schedule"],
                                                            want_grad=want_grad)
  return _PointSetStat.apply(x, y, stat, "divergence")


def sliced_wasserstein(x: torch.Tensor, y: torch.Tensor, directions):
  """The sliced Wasserstein distance (cost |.|^2 / 2, uniform weights) between the sample sets x [N, D] or [S, N, D] and
  y [M, D] or [S, M, D] over the directions [P, D] (constants: utils.sliced_directions gives the usual choice), [S]
  float64 ([1] for 2-D inputs), differentiable in x (and in y, by a second call): backward is the gradient cnf_sliced_w2
  stored times the incoming scalar.  With `flow_forward` a flow trains on target samples through ordinary autograd
  (applications.sliced_loss_fn is the hand-written fast path)."""
  stat = lambda a, b, want_grad, first: two_sample.sliced_wasserstein(a, b, directions, want_grad=want_grad)
  return _PointSetStat.apply(x, y, stat, "sw")


class _InteractionEnergy(torch.autograd.Function):
  """The interaction energy of one point set: the forward call stores dF / dx, backward is it times the incoming scalar."""

  @staticmethod
  def forward(ctx, x, kind, amplitudes, bandwidths, exponents):
    res = interaction.interaction_energy(x.detach(), kind, amplitudes, bandwidths, want_grad=ctx.needs_input_grad[0],
                                         exponents=exponents)
    ctx.save_for_backward(res.get("grad"))
    return res["energy"]

  @staticmethod
  def backward(ctx, gbar):
    g, = ctx.saved_tensors
    w = gbar.to(torch.float32)
    return (None if g is None else g * w[:, None, None] if g.dim() == 3 else g * w[0]), None, None, None, None


def interaction_energy(x: torch.Tensor, kind: str, amplitudes=None, bandwidths=None, exponents=None):
  """The mean-field interaction energy F = sum_{i != j} W(x_i - x_j) / (2 N (N - 1)) of the sample sets x [N, D] or
  [S, N, D] (utils.interaction_energy: a signed Gaussian, exponential, quadratic or softened power-law / log pair
  kernel), [S] float64 ([1] for a 2-D input), differentiable in x: backward is the gradient cnf_interaction stored times
  the incoming scalar.  The kernel's amplitudes, bandwidths and exponents are constants.  With `flow_forward` a flow
  trains on the energy through ordinary autograd (applications.interaction_loss_fn is the hand-written fast path)."""
  return _InteractionEnergy.apply(x, kind, amplitudes, bandwidths, exponents)


class _Ksd(torch.autograd.Function):
  """The kernel Stein discrepancy of point sets against a score: the forward call stores both gradients, backward is
  each times the incoming scalar."""

  @staticmethod
  def forward(ctx, x, score, kind, bandwidths, beta, weights):
    need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    res = stein.ksd(x.detach(), score.detach(), kind, bandwidths, beta, weights, want_grad=need)
    ctx.save_for_backward(res["grad_x"], res["grad_score"])
    return res["ksd2"]

  @staticmethod
  def backward(ctx, gbar):
    gx, gs = ctx.saved_tensors
    w = gbar.to(torch.float32)
    scale = lambda g, need: None if g is None or not need else (g * w[:, None, None] if g.dim() == 3 else g * w[0])
    return scale(gx, ctx.needs_input_grad[0]), scale(gs, ctx.needs_input_grad[1]), None, None, None, None


def ksd(x: torch.Tensor, score: torch.Tensor, kind: str = "imq", bandwidths=None, beta: float = -0.5, weights=None):
  """The kernel Stein discrepancy KSD^2_U (utils.ksd) of the sample sets x [N, D] or [S, N, D] against the law whose
  score at those points is `score`, [S] float64 ([1] for 2-D inputs), differentiable in x AND in score: with
  score = f(x) built from torch ops the chain rule runs through both, so a target known up to its constant trains a
  flow through ordinary autograd (applications.ksd_loss_fn is the hand-written fast path).  Backward is the gradients
  cnf_stein stored times the incoming scalar.  The kernel's bandwidths (None: utils.median_bandwidths(x), held
  constant), beta and weights are constants."""
  return _Ksd.apply(x, score, kind, bandwidths, beta, weights)


class _InteractionForce(torch.autograd.Function):
  """The self-mode force of point sets: forward is cnf_interaction's force, backward cnf_interaction_vjp on the incoming
  adjoint."""

  @staticmethod
  def forward(ctx, x, kind, amplitudes, bandwidths, exponents):
    x3 = interaction._sets("interaction", x, "x")
    interaction.interaction_check_shapes((min(x3.shape[0], _capi.MMD_MAX_SETS),) + tuple(x3.shape[1:]))
    spec = interaction.interaction_vjp_check_spec(
        interaction.interaction_spec(kind, amplitudes, bandwidths, exponents))
    _, one, (x3, _) = interaction._stage(x, x3, x3[:, :0])
    ctx.spec, ctx.one = spec, one
    ctx.save_for_backward(x3)
    return interaction._unstack(interaction.force_of_sets(spec, x3), one)

  @staticmethod
  def backward(ctx, fbar):
    x3, = ctx.saved_tensors
    g3 = fbar.detach().to(device=x3.device, dtype=torch.float32).reshape(x3.shape).contiguous()
    return interaction._unstack(interaction.force_vjp_of_sets(ctx.spec, x3, g3), ctx.one), None, None, None, None


def interaction_force(x: torch.Tensor, kind: str, amplitudes=None, bandwidths=None, exponents=None):
  """The mean-field force f_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j) of the sample sets x [N, D] or [S, N, D]
  (cnf_interaction in self mode; the pair kernel of utils.interaction_spec), float32 of x's shape, differentiable in x:
  backward is ONE cnf_interaction_vjp call per 64 sets (utils.interaction_force_vjp) -- the second pair sum, with the
  pair Hessian of W, that a loss needs when the force sits inside a square, as in the interacting Fokker-Planck residual
  (applications.fp_loss_fn(interaction=...) is the hand-written fast path).  The backward is the exact gradient of the
  discrete force: for the exponential kind in dimension 1 it does not contain the delta term of the kink of W at 0.
  The kernel's amplitudes, bandwidths and exponents are constants."""
  return _InteractionForce.apply(x, kind, amplitudes, bandwidths, exponents)
