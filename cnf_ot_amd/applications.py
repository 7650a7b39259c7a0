"""Mirror of cnf_ot/mfc/applications.py on the fused MI355X loss kernels.

Same function names and positional arguments as the reference
(`ot_loss_fn(model, dim, T, dt, t_batch_size, subtype, params, rng, _lambda,
batch_size)` ...), so `functools.partial(applications.ot_loss_fn, model, dim, T,
dt, t_batch_size, subtype)` from cnf_ot/mfc/solvers.py:58-88 works unchanged.
Every term is ONE kernel launch that returns per-slice sums (no [B,D]
intermediate reaches HBM); a composite loss stacks the partial sums of all its
terms and does ONE sum all-reduce when samples are sharded over GPUs.

Random draws: the reference reuses one `rng` for every draw inside a loss
(applications.py:36-67,81-82,233-239,392).  Here `rng` is a seed for the
build's Philox stream: base noise is element (global sample index, dim) of
that stream -- so the `batch_size // 32` draw is the first rows of the full
draw and sharding does not change results -- and `t_batch` / mixture
components come from a host generator keyed by the same seed.

Reference quirks kept on purpose: `batch_size // 32`
per-slice batches; the obstacle potential is summed, not averaged, over slices
(applications.py:397-400); RWPO/FP kinetic scaled by T / t_batch_size;
flow_matching overrides dt = dx = 0.01 (:286,301); fp beta = 4 (:432).
"""
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _capi, stein, two_sample
from . import kde as kd           # (ensemble_fields returns a key of that name's kind)
from . import interaction as ia      # (the composites take a keyword of that name)
from .distributed import Shard, all_reduce_sums, current_shard, shard_range
from .flows import DeviceRng, FlowEngine, _OnDevice, _stream_ptr, seed_to_u64

# Cholesky factor L (lower: A = L L^T, applied as z @ L like oracle/losses.py) of the Gaussian source's covariance A = [[5, 1], [1, .5]]
# (applications.py:28-32), computed once: torch.linalg.cholesky of a 2 x 2 CPU tensor costs ~20 ms PER CALL on a
# 256-thread host (LAPACK thread start-up) -- it was 35 of the 41 ms of config 5's value_and_grad.
GAUSSIAN_SOURCE_CHOL = np.linalg.cholesky(np.array([[5.0, 1.0], [1.0, 0.5]])).astype(np.float32)
_CHOL_ROWS = {}        # device -> the factor's rows on that device
_CENTERS_DEV = {}      # device -> MIXTURE_CENTERS on that device
MIXTURE_R = 5.0
# applications.py:34-67: centres of the 8-mode mixture source
MIXTURE_CENTERS = MIXTURE_R * np.array(
  [[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0],
   [0.6, 0.8], [0.6, -0.8], [-0.6, -0.8], [-0.6, 0.8]], dtype=np.float32)


def _spec(kind, subtype=0, dt=0.0, dx=0.0, coef=0.0, a=0.0, T=1.0, beta=1.0):
  return _capi.CnfLossSpec(kind, subtype, dt, dx, coef, a, T, beta)


def host_rng(rng, stream: int) -> np.random.Generator:
  """The host generator of a loss's non-Gaussian draws (time batch: stream 1, mixture components: stream 2), keyed by
  the loss's `rng`.  (One integer seed into PCG64: np.random.default_rng on a 4-word list costs 40 us per call -- a
  third of the host time of a config-3 loss evaluation.)"""
  seed, off = seed_to_u64(rng)
  return np.random.Generator(np.random.PCG64((seed << 72) | ((off & ((1 << 64) - 1)) << 8) | stream))


def draw_t_batch(rng, t_batch_size: int, scale: float = 1.0):
  """jax.random.uniform(rng, (t_batch_size,)) * T (applications.py:392,414,434): a host array, or -- for a DeviceRng --
  a device tensor drawn by cnf_fill_uniform_dev from the key in device memory."""
  if isinstance(rng, DeviceRng):
    out = torch.empty(t_batch_size, dtype=torch.float32, device=rng.device)
    with _OnDevice(rng.device):
      _capi.check(_capi.lib().cnf_fill_uniform_dev(rng.ptr, 0, t_batch_size, float(scale), out.data_ptr(),
                                                   _stream_ptr(rng.device)), "cnf_fill_uniform_dev")
    return out
  return (host_rng(rng, 1).uniform(0.0, 1.0, size=t_batch_size) * scale).astype(np.float32)


def _conds(t):
  """time-slice conditions as the term functions pass them on: a device tensor stays one, the rest a float32 array"""
  return t.reshape(-1) if torch.is_tensor(t) else np.atleast_1d(np.asarray(t, dtype=np.float32)).reshape(-1)


def _n_conds(t) -> int:
  return int(t.numel()) if torch.is_tensor(t) else int(np.atleast_1d(t).size)


def _cat_conds(parts):
  return torch.cat(list(parts)) if torch.is_tensor(parts[0]) else np.concatenate(list(parts))


def draw_components(rng, n: int) -> np.ndarray:
  """jax.random.choice(seed, a=8, shape=(n,)) (applications.py:36-38).  One byte per draw: the default int64 draw took
  5 ms per million on the GPU box's host and its [n, 2] table of centres another 5 plus a 16 MB copy -- an eager
  large-batch step with the mixture source was 15 ms of host work around 0.5 ms of kernels."""
  return host_rng(rng, 2).integers(0, 8, size=n, dtype=np.uint8)


class _Ctx:
  """Backend (loaded engine) + shard + local noise cache for one loss call.
  With `grad` (a zeroed flat float32 tensor) every term also accumulates
  coef * d(term sum)/d(params) into it (cnf_loss_terms_grad)."""

  def __init__(self, model, params, rng, shard: Optional[Shard], grad: Optional[torch.Tensor] = None):
    self.be = model.terms_backend(params)
    # the HIP engine, or a stand-in that has `normal`, `loss_terms` and `loss_terms_grad` alone (the CPU tests'): the
    # one place that asks; every route below that needs more than those three reads this flag
    self.hip = isinstance(self.be, FlowEngine)
    if _CAPTURED_BACKENDS is not None:
      _CAPTURED_BACKENDS.append(self.be)
    self.rng = rng
    self.shard = shard if shard is not None else current_shard()
    self.grad = grad
    if self.hip and grad is not None:
      self.be.grad_ready(grad)      # (cnf_grad_enable: what `_on_tables` asks about exists from here on)
    self._noise = {}
    self._passes = []       # base -> data backward passes waiting for ONE launch (defer_pass_vjp)
    self._jobs = []         # fused loss terms waiting for ONE launch (cnf_loss_terms_grad_multi)
    self._grad64 = None     # the reduced gradient of the last `reduce`, in float64
    # the terms' per-slice sums land side by side in one buffer: `reduce` needs no concatenation kernel
    self._sumbuf = torch.empty(256, dtype=torch.float64, device=self.be.device) if self.hip else None
    self._sumpos = 0

  def new_sums(self, n: int):
    if self._sumbuf is None or self._sumpos + n > self._sumbuf.numel():
      return None
    v = self._sumbuf[self._sumpos:self._sumpos + n]
    self._sumpos += n
    return v

  def noise(self, n_global: int) -> torch.Tensor:
    """This rank's rows of the first n_global samples of the seed's stream."""
    if n_global not in self._noise:
      start, count = shard_range(n_global, self.shard)
      if self.shard.world == 1:      # one rank: a smaller draw is the first rows of a larger one already made
        for n_have, v in self._noise.items():      # (the ("source", ...) entries hold one tensor, not a triple)
          if isinstance(n_have, int) and n_have >= n_global:
            self._noise[n_global] = (v[0][:n_global], 0, n_global)
            return self._noise[n_global]
      self._noise[n_global] = (self.be.normal(self.rng, count, first_sample=start), start, count)
    return self._noise[n_global]

  def terms(self, spec, pts, t, B_local, coef, shared=True):
    """per-slice sums of one term; `coef` = d(loss)/d(sum) (the same for every slice)."""
    t = _conds(t)
    kw = {}
    if self._sumbuf is not None:
      s = self.new_sums(_n_conds(t))
      if s is not None:
        kw["sums"] = s
    if self.grad is not None:
      if "sums" in kw and self.hip:
        # value_and_grad: the term is QUEUED -- the terms of a loss go out as one launch whose grid their tiles share
        # (flush_terms, at the latest in `reduce`); nobody reads a term's sums before the collective
        self._jobs.append((spec, pts, t, B_local, shared, coef, kw["sums"]))
        return kw["sums"]
      return self.be.loss_terms_grad(spec, pts, t, B_local, shared, coef, self.grad, **kw)
    return self.be.loss_terms(spec, pts, t, B_local, shared, **kw)

  def flush_terms(self):
    jobs, self._jobs = self._jobs, []
    if jobs:
      self.be.loss_terms_grad_multi(jobs, self.grad)

  def defer_pass_vjp(self, z, conds, count: int, ybar, ldbar):
    """Queue the backward of a base -> data pass (points z [S * count, D], one condition per slice of `count`
    points) instead of launching it: the passes of a loss's terms go out as ONE cnf_pass_vjp launch in `reduce`.
    A rank's share of a term is often too small to fill the GPU on its own (config 4: 512 and 1 536 waves for 2 048
    wave slots, each wave one tile -- two launches took two tile times, the merged one takes one)."""
    self._passes.append((z, _conds(conds), int(count), ybar, ldbar))

  def flush_passes(self):
    self.flush_terms()
    passes, self._passes = self._passes, []
    if not passes:
      return
    be = self.be
    if len(passes) == 1:
      z, conds, count, ybar, ldbar = passes[0]
      be.pass_vjp(z, be.slice_conds(conds), ybar, ldbar, False, grad=self.grad, want_xbar=False)
      return
    g = 0
    for _, _, count, _, _ in passes:
      g = int(np.gcd(g, count))
    dev = any(torch.is_tensor(c) for _, c, _, _, _ in passes)
    rep = []
    for _, c, count, _, _ in passes:
      if dev:
        # (the cached upload of slice_conds: a fresh host-to-device copy is not permitted inside a graph capture -- the
        # captured step failed from dim 6 up, where the reverse-KL pass [cond 0] is merged with the score term's)
        c = c if torch.is_tensor(c) else be.slice_conds(c)
        rep.append(c.repeat_interleave(count // g))
      else:
        rep.append(np.repeat(c, count // g))
    conds = _cat_conds(rep)
    z = torch.cat([p[0] for p in passes])
    ybar = torch.cat([p[3] if p[3] is not None else torch.zeros_like(p[0]) for p in passes])
    ldbar = None
    if any(p[4] is not None for p in passes):
      ldbar = torch.cat([p[4] if p[4] is not None else torch.zeros(p[0].shape[0], device=z.device) for p in passes])
    be.pass_vjp(z, be.slice_conds(conds), ybar, ldbar, False, grad=self.grad, want_xbar=False)

  def _stack(self, sums: Sequence[torch.Tensor]):
    """The partial sums of some terms as one float64 vector (a view of the sums buffer when they sit side by side)."""
    parts = [s.reshape(-1).to(torch.float64) for s in sums]
    n = sum(p.numel() for p in parts)
    if self._sumbuf is not None and len(parts) > 1:
      base = self._sumbuf.data_ptr()
      off = parts[0].data_ptr() - base
      ptr, ok = parts[0].data_ptr(), 0 <= off and off + 8 * n <= 8 * self._sumbuf.numel()
      for q in parts:
        ok = ok and q.data_ptr() == ptr
        ptr += 8 * q.numel()
      if ok:
        return self._sumbuf[off // 8:off // 8 + n], n
    return (torch.cat(parts) if len(parts) > 1 else parts[0]), n

  def reduce(self, sums: Sequence[torch.Tensor]) -> torch.Tensor:
    """The ONE collective of a loss evaluation: partial sums (+ the gradient)."""
    self.flush_passes()
    flat, n = self._stack(sums)
    if self.grad is not None and self.shard.world > 1:
      flat = all_reduce_sums(torch.cat([flat, self.grad.to(torch.float64)]), self.shard)
      self._grad64 = flat[n:]
      self.grad.copy_(flat[n:].to(self.grad.dtype))
      return flat[:n]
    return all_reduce_sums(flat, self.shard)

  # -- the collective of the FIRST terms under the compute of the later ones (config 5: BASELINE.json configs[4]) -----
  def reduce_begin(self, sums: Sequence[torch.Tensor]):
    """Start the sum all-reduce of the terms evaluated so far -- their partial sums and the gradient accumulated so
    far -- WITHOUT waiting for it (async_op: RCCL runs it on its own stream behind an event, gloo on a worker thread);
    the terms that follow accumulate into a fresh gradient buffer, and `reduce_end` folds the two.  With one rank
    nothing is started."""
    self.flush_passes()
    flat, n = self._stack(sums)
    work, g0 = None, self.grad
    if self.shard.world > 1:
      import torch.distributed as dist
      flat = torch.cat([flat, g0.to(torch.float64)]) if g0 is not None else flat.clone()
      work = dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.shard.group, async_op=True)
      if g0 is not None:
        self.grad = torch.zeros_like(g0)
    return flat, work, n, g0

  def reduce_end(self, handle) -> torch.Tensor:
    """Wait for `reduce_begin`'s collective (call it after the `reduce` of the later terms): the reduced sums of the
    first terms; the caller's gradient tensor receives first-phase + later-phase gradient."""
    flat, work, n, g0 = handle
    if work is not None:
      work.wait()
      if g0 is not None:      # first-phase + later-phase gradient, added in float64 and rounded once
        g0.copy_((flat[n:] + self._grad64).to(g0.dtype))
        self.grad = g0
    return flat[:n]

  def weighted(self, flat: torch.Tensor, sums: Sequence[torch.Tensor], coefs: Sequence[float]) -> torch.Tensor:
    """sum_i coefs[i] * (reduced) sums[i].sum(): one dot product with a cached weight vector instead of a slice /
    sum / multiply / add chain of tiny kernels per term (each costs a launch: 4-5 us on the stream)."""
    key = (tuple((float(c), int(s.numel())) for c, s in zip(coefs, sums)), str(flat.device))
    w = _WEIGHTS.get(key)
    if w is None:
      if len(_WEIGHTS) >= 64:
        _WEIGHTS.clear()
      w = _WEIGHTS[key] = torch.tensor(np.concatenate([np.full(n, c, dtype=np.float64) for c, n in key[0]]),
                                       dtype=torch.float64, device=flat.device)
    if flat.is_cuda:       # one block, fixed order, no BLAS call (and nothing a stream capture could not record)
      out = torch.empty(1, dtype=torch.float64, device=flat.device)
      with _OnDevice(flat.device):
        _capi.check(_capi.lib().cnf_weighted_sum(flat.data_ptr(), w.data_ptr(), flat.numel(), out.data_ptr(),
                                                 _stream_ptr(flat.device)), "cnf_weighted_sum")
      return out[0]
    return torch.dot(flat, w)

  def combine(self, sums: Sequence[torch.Tensor], coefs: Sequence[float]) -> torch.Tensor:
    """The loss from all its terms' partial sums, after the one collective."""
    return self.weighted(self.reduce(sums), sums, coefs)

  def combine_overlapped(self, first: Sequence[torch.Tensor], c_first: Sequence[float], later, c_later):
    """`combine` with the collective of the `first` terms already in flight while `later()` -- a callable that
    evaluates the remaining terms and returns their sums -- runs; a second, blocking collective for those."""
    h = self.reduce_begin(first)
    late = later()
    flat_late = self.reduce(late)
    flat_first = self.reduce_end(h)
    return self.weighted(torch.cat([flat_first, flat_late]), list(first) + list(late), list(c_first) + list(c_later))


# Sample-sharded value_and_grad of ot_loss_fn: start the all-reduce of the two density-fit terms (sums + their share
# of the gradient) as soon as they are done and run the t_batch_size kinetic / obstacle slices under it (BASELINE.json
# configs[4] "allreduce/compute overlap"); a second collective carries the rest.  False: ONE blocking collective at the
# end.  Both give the same loss and gradient (tests/test_distributed_cpu.py); see DESIGN.md 7 for what each costs.
OVERLAP_ALLREDUCE = True


_WEIGHTS = {}
# A list while solvers.CapturedUpdate records its graph: the backends of the loss evaluations made meanwhile (_Ctx), whose
# cached tensors the recorded kernels read by address
_CAPTURED_BACKENDS = None


# ---- local partial sums of each term ----------------------------------------

def _source_samples(ctx, z, start, count, n_global, source):
  if source == "mixture":      # applications.py:34-71 (live code)
    if z.shape[1] != 2:
      raise ValueError("the mixture source of kl_loss_fn is 2-D (applications.py:40-67)")
    if isinstance(ctx.rng, DeviceRng):
      out = torch.empty_like(z)
      with _OnDevice(z.device):
        _capi.check(_capi.lib().cnf_mixture_source_dev(ctx.rng.ptr, start, count, z.data_ptr(), out.data_ptr(), None,
                                                       _stream_ptr(z.device)), "cnf_mixture_source_dev")
      return out
    comp = draw_components(ctx.rng, n_global)[start:start + count]
    cdev = _CENTERS_DEV.get(z.device)
    if cdev is None:
      cdev = _CENTERS_DEV[z.device] = torch.from_numpy(MIXTURE_CENTERS).to(z.device)
    return z + cdev[torch.from_numpy(np.ascontiguousarray(comp)).to(z.device).long()]      # (the bytes cross, not the centres)
  if source == "gaussian":     # applications.py:28-32 (commented Gaussian source; BASELINE configs)
    if z.shape[1] != 2:
      raise ValueError("the Gaussian source N(-3, A) is 2-D (applications.py:28-32)")
    # z @ L - 3 for the 2 x 2 factor L, as three elementwise kernels: the rocBLAS GEMM torch picks for a [B, 2] x [2, 2]
    # product took 0.22 ms at B = 4.2 M (28 % of config 5's loss evaluation)
    rows = _CHOL_ROWS.get(z.device)
    if rows is None:
      rows = _CHOL_ROWS[z.device] = torch.from_numpy(np.concatenate([GAUSSIAN_SOURCE_CHOL, np.full((1, 2), -3.0, GAUSSIAN_SOURCE_CHOL.dtype)])).to(z.device)
    return torch.addcmul(torch.addcmul(rows[2], z[:, :1], rows[0]), z[:, 1:], rows[1])      # (two kernels, not three)
  raise ValueError(f"unknown source {source!r}")


# ---- dim 2, value_and_grad of large batches: the terms composed from table-path launches ---------------------------
# The fused gradient kernel evaluates the conditioner MLP per sample and multiplies per-sample weight gradients on
# the matrix cores (4 G flow passes/s); cnf_pass_vjp on the conditioner tables needs neither (per-piece sufficient
# statistics: DESIGN.md 5.4, 9 G passes/s).  So when the library's table kernels will take a rank's share of a term
# (cnf_model_term_on_tables: the network, the set_pwl mode and the size thresholds, stated once in cnf_common.h) the
# term is ONE forward launch on the tables, a few elementwise kernels for its value and adjoints, and ONE table
# backward launch.  The same composition serves the loss WITHOUT its gradient (table forward + term epilogue: 70 G
# flow passes/s where the fused loss kernel, three table sets in LDS, does 39 -- config 5's share 0.54 -> 0.3 ms).

def _on_tables(ctx, count, n_slices, passes=1):
  """Whether the term -- `passes` flow passes over n_slices slices of `count` points -- is composed from table launches:
  the library's answer, for the value alone or (ctx.grad) for value and gradient."""
  return ctx.hip and ctx.be.term_on_tables(count, count * n_slices * passes, ctx.grad is not None)


def _neg_logprob_tables(ctx, samples, cond, coef):
  """-sum log_prob(samples; cond) and its gradient: data -> base pass, log_prob = base(x) + ildj."""
  be = ctx.be
  c = be.slice_conds([cond])
  # value and gradient from ONE launch over the data (cnf_neg_logprob_vjp: the backward kernel seeds itself)
  total = be.neg_logprob_vjp(samples, c, coef, ctx.grad) if ctx.grad is not None else None
  if total is not None:
    return total
  # (the value alone; or the call declined for what `_on_tables` does not cover: no table reservation or slab room)
  # plain fp32 positions, like the fused loss kernel: a mean over the batch does not need the float64 position path
  # that makes single log_prob values good to 1e-5 (1.75 x the time of this launch)
  was = be._precise
  be.set_precise(False)
  try:
    x, ildj = be.inverse_logdet(samples, c)
  finally:
    be.set_precise(was)
  # d(-sum lp) scaled by coef: lp_bar = -coef; x_bar = lp_bar * d base/dx = coef * x; ld_bar = -coef
  total, xbar, ldbar = be.term_residual(_capi.TERM_NEG_LOGPROB, x, ildj, x.shape[0], loss_coef=coef,
                                        want_adjoints=ctx.grad is not None)
  if ctx.grad is not None:
    be.pass_vjp(samples, c, xbar, ldbar, True, grad=ctx.grad, want_xbar=False)
  return total


def _kinetic_tables(ctx, z, conds, count, dt, coef):
  """per-slice sums of |(r2 - r1) / dt|^2 with r1, r2 the same draw pushed to t -+ dt/2 (applications.py:220-242)."""
  be = ctx.be
  th = _conds(conds)
  S = _n_conds(th)
  half = np.float32(0.5 * dt)
  c2 = be.slice_conds(_cat_conds([th - half, th + half]))
  done = be.kinetic_potential_vjp(z, c2, S, dt, coef, ctx.grad)
  if done is not None:      # (one call: no repeated copy of z, one table build, no adjoint scan)
    return done[0]
  # (declined for what `_on_tables` does not cover: more than 128 slice sets, an odd slice length, no reservation or slab room)
  z2 = z.repeat(2 * S, 1)
  r, _ = be.forward_logdet(z2, c2, want_logdet=False)
  sums, rbar, _ = be.term_residual(_capi.TERM_KINETIC, r, None, count, p0=dt, loss_coef=coef, want_adjoints=ctx.grad is not None)
  if ctx.grad is not None:
    be.pass_vjp(z2, c2, rbar, None, False, grad=ctx.grad, want_xbar=False)
  return sums


def _potential_tables(ctx, z, conds, count, subtype, a, coef):
  """per-slice sums of the potential at the samples pushed to the slices' times (applications.py:176-205)."""
  be = ctx.be
  th = _conds(conds)
  S = _n_conds(th)
  c = be.slice_conds(th)
  zr = z.repeat(S, 1) if S > 1 else z
  r, _ = be.forward_logdet(zr, c, want_logdet=False)
  sums, rbar, _ = be.term_residual(_capi.TERM_POTENTIAL, r, None, count, subtype=_capi.POTENTIALS[subtype], p0=a,
                                   loss_coef=coef, want_adjoints=ctx.grad is not None)
  if ctx.grad is not None:
    be.pass_vjp(zr, c, rbar, None, False, grad=ctx.grad, want_xbar=False)
  return sums


def _kinetic_potential_tables(ctx, z, conds, count, dt, c_kin, subtype, a, c_pot):
  """The kinetic and the potential term of ot_loss_fn's obstacle case (applications.py:392-400: the same draw pushed to
  t -+ dt/2 and to t) from ONE forward and ONE backward launch over the 3 S slices -- they were two of each."""
  be = ctx.be
  th = _conds(conds)
  S = _n_conds(th)
  n = S * count
  half = np.float32(0.5 * dt)
  c3 = be.slice_conds(_cat_conds([th - half, th + half, th]))
  done = be.kinetic_potential_vjp(z, c3, S, dt, c_kin, ctx.grad, subtype=_capi.POTENTIALS[subtype], a=a, c_pot=c_pot)
  if done is not None:
    return done
  # (declined for what `_on_tables` does not cover: more than 128 slice sets, an odd slice length, no reservation or slab room)
  z3 = z.repeat(3 * S, 1)
  r, _ = be.forward_logdet(z3, c3, want_logdet=False)
  if ctx.grad is None:
    kin, _, _ = be.term_residual(_capi.TERM_KINETIC, r[:2 * n], None, count, p0=dt, loss_coef=c_kin, want_adjoints=False)
    pot, _, _ = be.term_residual(_capi.TERM_POTENTIAL, r[2 * n:], None, count, subtype=_capi.POTENTIALS[subtype], p0=a,
                                 loss_coef=c_pot, want_adjoints=False)
    return kin, pot
  rbar = torch.empty_like(r)
  kin, _, _ = be.term_residual(_capi.TERM_KINETIC, r[:2 * n], None, count, p0=dt, loss_coef=c_kin, rbar_out=rbar[:2 * n])
  pot, _, _ = be.term_residual(_capi.TERM_POTENTIAL, r[2 * n:], None, count, subtype=_capi.POTENTIALS[subtype], p0=a,
                               loss_coef=c_pot, rbar_out=rbar[2 * n:])
  be.pass_vjp(z3, c3, rbar, None, False, grad=ctx.grad, want_xbar=False)
  return kin, pot


def _kl_sum(ctx, T, cond, batch_size, source, coef):
  z, start, count = ctx.noise(batch_size)
  key = ("source", batch_size, source)       # the same key draws the same source samples for every condition
  s1 = ctx._noise.get(key)
  if s1 is None:
    s1 = ctx._noise[key] = _source_samples(ctx, z, start, count, batch_size, source)
  if cond == 0.0:
    samples = s1
  elif cond == T:
    samples = z
  else:
    samples = s1 * ((T - cond) / T) + z * (cond / T)      # target N(0,I) drawn from the same key
  if _on_tables(ctx, count, 1):
    return _neg_logprob_tables(ctx, samples.contiguous(), cond, coef)
  return ctx.terms(_spec(_capi.TERM_NEG_LOGPROB), samples.contiguous(), [cond], count, coef)


def _reverse_kl_sum(ctx, T, beta, cond, batch_size, coef):
  z, _, count = ctx.noise(batch_size)
  # (the gradient form alone: without a gradient the term stays on the fused kernel)
  if (_use_unfused(ctx, z.shape[1]) and count <= UNFUSED_RKL_MAX_BATCH) or (ctx.grad is not None and _on_tables(ctx, count, 1)):
    return _reverse_kl_unfused(ctx, T, beta, cond, batch_size, coef)
  return ctx.terms(_spec(_capi.TERM_REVERSE_KL, T=T, beta=beta), z, [cond], count, coef)


def _potential_sum(ctx, a, subtype, conds, batch_size, coef):
  if subtype not in _capi.POTENTIALS:
    raise ValueError(f"unknown potential {subtype!r}")
  z, _, count = ctx.noise(batch_size)
  if _on_tables(ctx, count, _n_conds(conds)):
    return _potential_tables(ctx, z, conds, count, subtype, a, coef)
  return ctx.terms(_spec(_capi.TERM_POTENTIAL, subtype=_capi.POTENTIALS[subtype], a=a), z, conds, count, coef)


def _kinetic_sum(ctx, dt, conds, batch_size, coef):
  z, _, count = ctx.noise(batch_size)
  if _on_tables(ctx, count, _n_conds(conds), passes=2):
    return _kinetic_tables(ctx, z, conds, count, dt, coef)
  return ctx.terms(_spec(_capi.TERM_KINETIC, dt=dt), z, conds, count, coef)


# From this dimension on, the score terms run UNFUSED: the fused kernel runs a
# sample's 3 + 2*dim flow passes back to back on one lane, which starves the GPU
# when a rank has few samples (dim 10: 32 768 samples = 512 waves, 23 passes
# each).  Unfused, the 2*dim log_prob evaluations at r3 +- dx/2 e_d are just
# 2*dim*B more points for the fast flow kernel, and the gradient comes from
# torch.autograd over the differentiable flow passes (cnf_ot_amd.autograd).
UNFUSED_SCORE_MIN_DIM = 6
# ... and the reverse-KL term too while the rank's batch is small (the fused kernel runs one sample per lane:
# 131 072 samples are 2 waves per SIMD)
UNFUSED_RKL_MAX_BATCH = 131072


def _score_terms_unfused(ctx, conds, batch_size, dt, dx, coef_score, loss_coef, drift=-1, a=0.0, interaction=None):
  """per-slice sums of  sum_d ((r2-r1)/dt + coef_score * score_d(r3) - drift_d(r3))^2  from three launches:
  ONE base -> data pass over the 3 x S x count points (conditions t -+ dt/2 and t; at this size the
  wave-per-dimension kernel), ONE central-difference score launch over the S x count points r3 (its 2 D
  evaluation points per sample exist only inside the kernel) and ONE epilogue (cnf_score_residual).  With ctx.grad
  the epilogue also emits the adjoints, and two backward launches (cnf_logprob_fd_vjp, cnf_pass_vjp) accumulate
  the parameter gradient -- the reverse sweep written out by hand: no autograd graph, a dozen host calls.
  interaction = (spec, strength): the residual gains strength * f(r3), f the self-mode interaction force of each time's
  `count` samples (ONE cnf_interaction call per 64 times, between the forward pass and the score launch); the epilogue
  is cnf_score_residual_force, and its fbar goes through ONE cnf_interaction_vjp call per 64 times (the pair Hessian of
  W against fbar) into the adjoint of r3, before cnf_logprob_fd_vjp.  Always this composed route: the launch that fuses
  value and backward has no force."""
  be = ctx.be
  z, _, count = ctx.noise(batch_size)
  S = _n_conds(conds)
  n = S * count
  # conditions per SLICE (the engine broadcasts a slice's value over its `count` samples): 3 S floats, built on the
  # host and uploaded once per distinct time batch -- not per-sample tensors assembled by a chain of small kernels
  th = _conds(conds)
  half = np.float32(0.5 * dt)
  tt = be.slice_conds(th)
  c3 = be.slice_conds(_cat_conds([th - half, th + half, th]))
  z3 = z.repeat(3 * S, 1)                                     # the same draw for every slice and condition
  want = ctx.grad is not None
  r, _ = be.forward_logdet(z3, c3, want_logdet=False)
  if interaction is not None:
    ia_spec, strength = interaction
    r3 = r[2 * n:]
    sets = r3.view(S, count, -1)
    force = ia.force_of_sets(ia_spec, sets).view(n, -1)
    score = be.logprob_fd(r3, tt, dx)
    sums, rbar, sbar, fbar = be.score_residual_force(r, score, force, strength, count, dt, coef_score, drift, a, loss_coef,
                                                     want)
    if want:
      rbar[2 * n:] += ia.force_vjp_of_sets(ia_spec, sets, fbar.view(S, count, -1)).view(n, -1)
      rbar[2 * n:] += be.logprob_fd_vjp(r3, tt, dx, sbar, ctx.grad)
      ctx.defer_pass_vjp(z3, _cat_conds([th - half, th + half, th]), count, rbar, None)
    return sums
  if want and drift in (-1, _capi.DRIFTS["ou"]):
    # value AND backward of the score term in one launch: the kernel that differentiates the 2 D evaluation points
    # forms the score from its own forward passes (no separate forward launch over them)
    sums, rbar = be.score_fd_vjp(r, tt, count, dt, dx, coef_score, drift, a, loss_coef, ctx.grad)
    ctx.defer_pass_vjp(z3, _cat_conds([th - half, th + half, th]), count, rbar, None)
    return sums
  r3 = r[2 * n:]
  score = be.logprob_fd(r3, tt, dx)
  sums, rbar, sbar = be.score_residual(r, score, count, dt, coef_score, drift, a, loss_coef, want)
  if want:
    r3bar = be.logprob_fd_vjp(r3, tt, dx, sbar, ctx.grad)     # adjoint of r3 through the score; + parameter gradient
    rbar[2 * n:] += r3bar
    ctx.defer_pass_vjp(z3, _cat_conds([th - half, th + half, th]), count, rbar, None)
  return sums


def _reverse_kl_unfused(ctx, T, beta, cond, batch_size, coef):
  """reverse_kl_loss_fn from one base -> data launch + an epilogue (+ one backward launch): the form for
  dimensions where a rank's share of the batch cannot fill the GPU from inside the fused kernel."""
  be = ctx.be
  z, _, count = ctx.noise(batch_size)
  c = be.slice_conds([cond])
  y, lp = be.sample_logprob(z, c)
  want = ctx.grad is not None
  total, ybar, lpbar = be.rkl_residual(y, lp, cond, T, beta, coef, want)
  if want:      # lp = base(noise) - fldj: the adjoint of the pass's log-det output is -lpbar
    if ctx.grad is not None and _on_tables(ctx, count, 1):      # (dim 2, large batch: the table form, on its own)
      be.pass_vjp(z, c, ybar, -lpbar, False, grad=ctx.grad, want_xbar=False)
    else:
      ctx.defer_pass_vjp(z, [cond], count, ybar, -lpbar)
  return total


def _use_unfused(ctx, dim):
  return dim >= UNFUSED_SCORE_MIN_DIM and ctx.hip


def _kinetic_score_sum(ctx, beta, dt, dx, conds, batch_size, coef):
  z, _, count = ctx.noise(batch_size)
  if _use_unfused(ctx, z.shape[1]):
    return _score_terms_unfused(ctx, conds, batch_size, dt, dx, 1.0 / beta, coef)
  return ctx.terms(_spec(_capi.TERM_KINETIC_SCORE, dt=dt, dx=dx, coef=1.0 / beta), z, conds, count, coef)


def _flow_matching_check(dim, subtype):
  if subtype not in _capi.DRIFTS:
    raise ValueError(f"unknown velocity field {subtype!r}")
  if subtype in ("nongradient",) and dim != 2:
    raise Exception("nongradient case is only implemented for 2D!")        # applications.py:359-360
  if subtype == "lorenz" and dim != 3:
    raise Exception("Lorenz dynamics is only defined for 3 dim!")          # applications.py:365-366
  if subtype == "gradient" and dim != 2:
    raise ValueError("the reference's 'gradient' target is a 2-D field (applications.py:353-357); "
                     "use subtype='ou' for the documented drift -a*r in other dimensions")


def _flow_matching_sum(ctx, dim, a, sigma, subtype, conds, batch_size, coef, interaction=None):
  _flow_matching_check(dim, subtype)
  z, _, count = ctx.noise(batch_size)
  if interaction is not None:      # (the composed route at every dimension and for every drift)
    return _score_terms_unfused(ctx, conds, batch_size, 0.01, 0.01, sigma, coef, _capi.DRIFTS[subtype], a, interaction)
  if _use_unfused(ctx, dim) and subtype in ("ou", "lorenz"):
    return _score_terms_unfused(ctx, conds, batch_size, 0.01, 0.01, sigma, coef, _capi.DRIFTS[subtype], a)
  # dt and dx are overridden to 0.01 inside the reference function (:286,301)
  return ctx.terms(_spec(_capi.TERM_FLOW_MATCHING, subtype=_capi.DRIFTS[subtype], dt=0.01, dx=0.01,
                         coef=sigma, a=a), z, conds, count, coef)


# ---- public term functions (reference signatures) ----------------------------
# Every function takes two extra keywords: `shard` (cnf_ot_amd.distributed.Shard,
# default: the torch.distributed world) and `grad` (a zeroed flat float32 tensor
# that receives d loss / d params: see `value_and_grad`).

def kl_loss_fn(model, dim, T, params, cond, rng, batch_size, source="mixture", shard=None, grad=None):
  """applications.py:11-86: -mean log_prob of samples interpolated between the
  source and the target draw."""
  ctx = _Ctx(model, params, rng, shard, grad)
  return ctx.reduce([_kl_sum(ctx, T, float(cond), batch_size, source, 1.0 / batch_size)])[0] / batch_size


def density_fit_kl_loss_fn(model, dim, T, params, rng, batch_size, source="mixture", shard=None, grad=None):
  """applications.py:166-173"""
  ctx = _Ctx(model, params, rng, shard, grad)
  c = 1.0 / batch_size
  s = ctx.reduce([_kl_sum(ctx, T, 0.0, batch_size, source, c), _kl_sum(ctx, T, float(T), batch_size, source, c)])
  return (s[0] + s[1]) * c


def reverse_kl_loss_fn(model, dim, T, beta, params, cond, rng, batch_size, shard=None, grad=None):
  """applications.py:129-163"""
  ctx = _Ctx(model, params, rng, shard, grad)
  return ctx.reduce([_reverse_kl_sum(ctx, T, beta, float(cond), batch_size, 1.0 / batch_size)])[0] / batch_size


def potential_loss_fn(model, dim, a, subtype, params, cond, rng, batch_size, shard=None, grad=None):
  """applications.py:176-205"""
  ctx = _Ctx(model, params, rng, shard, grad)
  return ctx.reduce([_potential_sum(ctx, a, subtype, [float(cond)], batch_size, 1.0 / batch_size)])[0] / batch_size


def kinetic_loss_fn(model, dim, dt, params, cond, rng, batch_size, shard=None, grad=None):
  """applications.py:220-242: mean(v^2) * dim / 2 with v by finite differences in c."""
  ctx = _Ctx(model, params, rng, shard, grad)
  c = 0.5 / batch_size       # mean over batch*dim, times dim / 2
  return ctx.reduce([_kinetic_sum(ctx, dt, [float(cond)], batch_size, c)])[0] * c


def kinetic_with_score_loss_fn(model, dim, beta, dt, dx, params, cond, rng, batch_size, shard=None, grad=None):
  """applications.py:245-276"""
  ctx = _Ctx(model, params, rng, shard, grad)
  c = 0.5 / batch_size
  return ctx.reduce([_kinetic_score_sum(ctx, beta, dt, dx, [float(cond)], batch_size, c)])[0] * c


def flow_matching_loss_fn(model, dim, a, sigma, subtype, dt, dx, params, cond, rng, batch_size, shard=None,
                          grad=None):
  """applications.py:279-374 (dt, dx arguments are ignored, as in the reference)."""
  ctx = _Ctx(model, params, rng, shard, grad)
  c = 0.5 / batch_size
  return ctx.reduce([_flow_matching_sum(ctx, dim, a, sigma, subtype, [float(cond)], batch_size, c)])[0] * c


# ---- post-training evaluation (cnf_ot/mfc/solvers.py:129-308) -------------------
# The density errors are one fused launch each (CNF_TERM_DENSITY_L2 / _DATA: per-slice sums of
# (exp(log_prob) - p_mix)^2, no [B, D] samples in HBM); the caller takes the root of the mean.

def ou_variance(t, a, var0, sigma=0.5):
  """Per-dimension variance at time t under the flow-matching dynamics v = -a r - sigma grad log rho, started from
  variance var0: exp(-2 a t) (var0 - sigma / a) + sigma / a.  At sigma = 1/2 this is the reference's 1/(2a) form
  (solvers.py:246-252), which hard-codes that value -- and so does the density-error kernel's mixture."""
  return math.exp(-2.0 * a * t) * (var0 - sigma / a) + sigma / a


def density_l2_error_fn(model, dim, T, a, params, cond, rng, batch_size, var0=4.0, shard=None):
  """rmse_mc_loss_fn (solvers.py:254-279): sqrt(mean (exp(log_prob) - p_mix)^2) over batch_size samples drawn at
  `cond`, p_mix(y) = (1 - cond) N(y; 0, var0 I) + cond N(y; 0, vT I), vT = ou_variance(T, a, var0).  One
  cnf_loss_terms_seeded launch (the noise is drawn in the kernel); this rank's block of the samples, one sum
  all-reduce."""
  shard = shard if shard is not None else current_shard()
  be = model.terms_backend(params)
  start, count = shard_range(batch_size, shard)
  spec = _spec(_capi.TERM_DENSITY_L2, coef=var0, a=a, T=T)
  total = all_reduce_sums(be.loss_terms_seeded(spec, rng, [float(cond)], count, first_sample=start), shard)
  return torch.sqrt(total[0] / batch_size)


def density_grid(grid_size, lo, hi, rows, device):
  """Rows `rows` (a range of y indices) of jnp.meshgrid(linspace(lo, hi, n), linspace(lo, hi, n)) flattened to
  [len(rows) * n, 2] points (x fastest), as rmse_grid_loss_fn builds them (solvers.py:288-293)."""
  xs = torch.linspace(lo, hi, grid_size, dtype=torch.float64, device=device)
  X, Y = torch.meshgrid(xs, xs[rows.start:rows.stop], indexing="xy")
  return torch.stack([X.reshape(-1), Y.reshape(-1)], 1).to(torch.float32).contiguous()


def density_l2_grid_error_fn(model, T, a, params, cond, grid_size=500, lo=-5.0, hi=5.0, var0=4.0, shard=None):
  """rmse_grid_loss_fn (solvers.py:284-305): the density error of density_l2_error_fn on the grid_size^2 points of
  [lo, hi]^2.  Dim 2 only, as the reference only calls it there.  The grid is built once on the device, then ONE
  cnf_loss_terms launch (CNF_TERM_DENSITY_L2_DATA); a rank takes its block of grid rows."""
  if model.cfg.dim != 2:
    raise ValueError(f"density_l2_grid_error_fn: the grid error is defined at dim 2 only, not {model.cfg.dim}")
  shard = shard if shard is not None else current_shard()
  be = model.terms_backend(params)
  start, rows = shard_range(grid_size, shard)
  pts = density_grid(grid_size, lo, hi, range(start, start + rows), be.device)
  spec = _spec(_capi.TERM_DENSITY_L2_DATA, coef=var0, a=a, T=T)
  total = all_reduce_sums(be.loss_terms(spec, pts, [float(cond)], pts.shape[0], True), shard)
  return torch.sqrt(total[0] / (grid_size * grid_size))


def cost_rwpo_terms(x, y, beta, a):
  """The double-well cost_rwpo of solvers.py:190-220 from its draws, scaled: x [nx, 2], y [nx, ny, 2] (float64)."""
  nx, ny = y.shape[0], y.shape[1]
  r = y.reshape(-1, 2)
  v = (torch.linalg.norm(r - a, dim=1) * torch.linalg.norm(r + a, dim=1) / 2) ** 2
  return (-2.0 / beta * torch.log(torch.exp(v.reshape(nx, ny) * (-beta / 2)).mean(1))).mean()


def rwpo_true_value(dim, T, beta, a, subtype, rng=None):
  """The reference value of the rwpo energy (solvers.py:164-235).  quadratic: the closed form dim (1 + log(T + 1)) /
  beta (:170-172, quadratic potential and Gaussian initial condition).  double_well: cost_rwpo(rng, 100, 1000)
  (:190-220, 232), dim 2 only as in the reference: x ~ N(0, 2/beta (T+1) I) [100], y = x + N(0, 2/beta T I)
  [100 x 1000], both from the cnf_fill_normal stream of `rng` (x: samples 0-99, y: the next 100 000), in float64 on
  the device.  obstacle: None (the reference has no value: it raises NameError at :234-235)."""
  if subtype == "quadratic":
    return dim * (1.0 + math.log(T + 1.0)) / beta
  if subtype == "obstacle":
    return None
  if subtype != "double_well":
    raise ValueError(f"unknown potential {subtype!r}")
  if dim != 2:
    raise ValueError(f"rwpo_true_value: cost_rwpo is defined at dim 2 only, not {dim}")
  seed, off = seed_to_u64(0 if rng is None else rng)
  nx, ny = 100, 1000
  dev = torch.device("cuda", torch.cuda.current_device())
  z = torch.empty(nx * (1 + ny) * 2, dtype=torch.float32, device=dev)
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_fill_normal(seed, off * 2, z.numel(), z.data_ptr(), _stream_ptr(dev)),
                "cnf_fill_normal")
  z = z.double()
  x = z[:nx * 2].reshape(nx, 2) * math.sqrt(2.0 / beta * (T + 1))
  y = z[nx * 2:].reshape(nx, ny, 2) * math.sqrt(2.0 / beta * T) + x.reshape(nx, 1, 2)
  return float(cost_rwpo_terms(x, y, beta, a))


# The exact rwpo solution at dim 2 (the reference's offline generator, cnf_ot/mfc/2d_WPO_ref_solution.py:60-187): one
# cnf_hopf_cole_2d call, float64 separable log-sum-exp passes on the device (include/cnf_ot_amd.h).
HOPF_COLE_FIELDS = ("score_T", "w0", "wT")


def rwpo_initial_variance(T, beta):
  """The per-dimension variance 2 (T + 1) / beta of the initial condition the rwpo training fits: the source of its
  reverse-KL term at cond 0 (reverse_kl_loss_fn, applications.py:137-143)."""
  return 2.0 * (T + 1.0) / beta


def rwpo_reference_solution(T, beta, a, subtype, x1, x2=None, var0=None, dz=0.01, window=6.0, y_range=4.0,
                            fields=HOPF_COLE_FIELDS):
  """The regularized Wasserstein proximal solution at time T on the tensor grid x1 [n1] x x2 [n2] (x2 = x1 if None),
  by the generator's Hopf-Cole quadrature with eps = 1/beta, g = the potential `subtype` (a as float32, as the loss
  spec carries it), rho0 = N(0, var0 I) (default: rwpo_initial_variance(T, beta); the generator hard-codes N(0, I)),
  a y grid of step dz over [-y_range, y_range]^2 and the z window |z_i - y_i| <= window.  Returns a dict of float64
  device tensors: log_rho_T [n2, n1] (x1 fastest, meshgrid(x1, x2, indexing="xy")), the requested `fields` among
  score_T, w0, wT [n2, n1, 2], and the 0-dim true_val (the optimal energy) and ic_mass (sum rho0 dz^2)."""
  fields = tuple(fields)
  bad = [f for f in fields if f not in HOPF_COLE_FIELDS]
  if bad:
    raise ValueError(f"rwpo_reference_solution: unknown fields {bad} (known: {HOPF_COLE_FIELDS})")
  dev = torch.device("cuda", torch.cuda.current_device())
  x1 = torch.as_tensor(x1, dtype=torch.float64).to(dev).reshape(-1).contiguous()
  x2 = x1 if x2 is None else torch.as_tensor(x2, dtype=torch.float64).to(dev).reshape(-1).contiguous()
  n1, n2 = x1.numel(), x2.numel()
  if n1 == 0 or n2 == 0:
    raise ValueError("rwpo_reference_solution: the output grid is empty")
  return _hopf_cole(dev, T, beta, a, subtype, var0, dz, window, y_range, x1, x2, fields)


def rwpo_true_value_quadrature(dim, T, beta, a, subtype, var0=None, dz=0.01, window=6.0, y_range=4.0):
  """The optimal rwpo energy -2 eps sum_y rho0(y) (log h(y) - log(4 pi eps T)) dy^2 from the same quadrature as
  rwpo_reference_solution (deterministic; for the quadratic potential it approaches rwpo_true_value's closed form
  as the ranges grow).  Dim 2 only."""
  if dim != 2:
    raise ValueError(f"rwpo_true_value_quadrature: the quadrature is defined at dim 2 only, not {dim}")
  dev = torch.device("cuda", torch.cuda.current_device())
  return float(_hopf_cole(dev, T, beta, a, subtype, var0, dz, window, y_range, None, None, ())["true_val"])


def _hopf_cole(dev, T, beta, a, subtype, var0, dz, window, y_range, x1, x2, fields):
  if subtype not in _capi.POTENTIALS:
    raise ValueError(f"unknown potential {subtype!r}")
  var0 = rwpo_initial_variance(T, beta) if var0 is None else var0
  lib = _capi.lib()
  n1, n2 = (0, 0) if x1 is None else (x1.numel(), x2.numel())
  nbytes = _capi.ctypes.c_int64(0)
  _capi.check(lib.cnf_hopf_cole_workspace(float(dz), float(window), float(y_range), n1, n2, _capi.ctypes.byref(nbytes)),
              "cnf_hopf_cole_workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  ws = torch.empty(-(-nbytes.value // 8), **f64)
  scalars = torch.empty(2, **f64)
  out = {}
  if n1:
    out["log_rho_T"] = torch.empty(n2, n1, **f64)
    for f in fields:
      out[f] = torch.empty(n2, n1, 2, **f64)

  def ptr(name):
    return out[name].data_ptr() if name in out else None

  with _OnDevice(dev):
    _capi.check(lib.cnf_hopf_cole_2d(_capi.POTENTIALS[subtype], float(a), float(T), float(beta), float(var0), float(dz),
                                     float(window), float(y_range), None if x1 is None else x1.data_ptr(), n1,
                                     None if x2 is None else x2.data_ptr(), n2, ptr("log_rho_T"), ptr("score_T"),
                                     ptr("w0"), ptr("wT"), scalars.data_ptr(), scalars.data_ptr() + 8, ws.data_ptr(),
                                     ws.numel() * 8, _stream_ptr(dev)), "cnf_hopf_cole_2d")
  out["true_val"], out["ic_mass"] = scalars[0], scalars[1]
  return out


HOPF_COLE_PATH_FIELDS = ("score", "drift", "vel")


def rwpo_reference_path(T, beta, a, subtype, times, x1, x2=None, var0=None, dz=0.01, window=6.0, y_range=4.0,
                        fields=HOPF_COLE_PATH_FIELDS):
  """The regularized Wasserstein proximal solution at every time of `times` (0 <= t <= T) on the tensor grid x1 [n1] x
  x2 [n2], from the quadrature of rwpo_reference_solution (same arguments) in one cnf_hopf_cole_path_2d call: h and the
  value once, the times in chunks of 8 per launch.  Returns a dict of float64 device tensors: log_rho [S, n2, n1], the
  requested `fields` [S, n2, n1, 2] among score (grad log rho_t), drift (the optimal control 2 eps grad log eta_t;
  -grad g at T) and vel (drift - eps score, the velocity the flow's must equal), and the 0-dim true_val and ic_mass.
  The slab of t = T equals rwpo_reference_solution's log_rho_T, score_T and wT bit for bit; t = 0 is rho0 itself.  A
  time closer to an endpoint than (1.5 dz)^2 beta / 2, or outside [0, T], is refused (CnfError)."""
  fields = tuple(fields)
  bad = [f for f in fields if f not in HOPF_COLE_PATH_FIELDS]
  if bad:
    raise ValueError(f"rwpo_reference_path: unknown fields {bad} (known: {HOPF_COLE_PATH_FIELDS})")
  if subtype not in _capi.POTENTIALS:
    raise ValueError(f"unknown potential {subtype!r}")
  dev = torch.device("cuda", torch.cuda.current_device())
  x1 = torch.as_tensor(x1, dtype=torch.float64).to(dev).reshape(-1).contiguous()
  x2 = x1 if x2 is None else torch.as_tensor(x2, dtype=torch.float64).to(dev).reshape(-1).contiguous()
  ts = np.ascontiguousarray(np.asarray(times.cpu() if torch.is_tensor(times) else times, dtype=np.float64).reshape(-1))
  n1, n2, S = x1.numel(), x2.numel(), ts.size
  if n1 == 0 or n2 == 0 or S == 0:
    raise ValueError("rwpo_reference_path: the output grid or the time array is empty")
  var0 = rwpo_initial_variance(T, beta) if var0 is None else var0
  lib, C = _capi.lib(), _capi.ctypes
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_hopf_cole_path_workspace(float(dz), float(window), float(y_range), n1, n2, C.byref(nbytes)),
              "cnf_hopf_cole_path_workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  ws = torch.empty(-(-nbytes.value // 8), **f64)
  scalars = torch.empty(2, **f64)
  out = {"log_rho": torch.empty(S, n2, n1, **f64)}
  for f in fields:
    out[f] = torch.empty(S, n2, n1, 2, **f64)

  def ptr(name):
    return out[name].data_ptr() if name in out else None

  with _OnDevice(dev):
    _capi.check(lib.cnf_hopf_cole_path_2d(_capi.POTENTIALS[subtype], float(a), float(T), float(beta), float(var0),
                                          float(dz), float(window), float(y_range),
                                          ts.ctypes.data_as(C.POINTER(C.c_double)), S, x1.data_ptr(), n1, x2.data_ptr(),
                                          n2, ptr("log_rho"), ptr("score"), ptr("drift"), ptr("vel"), scalars.data_ptr(),
                                          scalars.data_ptr() + 8, ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)),
                "cnf_hopf_cole_path_2d")
  out["true_val"], out["ic_mass"] = scalars[0], scalars[1]
  return out


# ---- the particle reference of the fp problems --------------------------------------------------------------------
# flow_matching_loss_fn (applications.py:279-374) fits v_flow + sigma grad log rho = drift: the continuity form of
# d rho / dt = -div(rho drift) + sigma lap rho, the law of dX = drift(X) dt + sqrt(2 sigma) dW.  An Euler-Maruyama
# ensemble of that SDE (the reference's tests/test_lorenz.py sketches one) is a ground truth for every drift and every
# dimension: cnf_fp_particles (include/cnf_ot_amd.h), float64 state, one particle per lane.
FP_DRIFT_DIM = {"gradient": 2, "smile": 2, "nongradient": 2, "lorenz": 3}       # ou: any dimension
FP_MAX_SNAPSHOTS = 64


def fp_initial_variance(T):
  """The per-dimension variance (T + 1) / 2 of the initial condition the fp training fits: fp_loss_fn's reverse KL at
  beta = 4 (applications.py:432, reverse_kl_loss_fn :137-143)."""
  return (T + 1.0) / 2.0


def stats_grid(grid, axes, dim):
  """The histogram grid of fp_reference_particles / utils.point_stats as a CnfFieldGrid: `grid` is a utils.field_grid
  (its own axes count) or (domain_range, n) over the event axes `axes`; cell j is centred on the grid point
  lo + j (hi - lo) / (n - 1), density_on_grid's points.  None for grid = None."""
  if grid is None:
    return None
  if isinstance(grid, dict):
    dom, n, axes = grid["domain_range"], grid["n"], grid["axes"]
  else:
    dom, n = grid
  x_min, x_max, y_min, y_max = (float(v) for v in dom)
  nx, ny = (int(n), int(n)) if np.ndim(n) == 0 else (int(n[0]), int(n[1]))
  ax, ay = int(axes[0]), int(axes[1])
  if nx < 2 or ny < 2 or not (x_max > x_min and y_max > y_min):
    raise ValueError(f"histogram grid: needs n >= 2 points per axis over a non-empty range, not {n} over {dom}")
  if ax == ay or not (0 <= ax < dim and 0 <= ay < dim):
    raise ValueError(f"histogram grid: axes {(ax, ay)} are equal or outside an event of dimension {dim}")
  return _capi.CnfFieldGrid(x_min, y_min, (x_max - x_min) / (nx - 1), (y_max - y_min) / (ny - 1), nx, ny, ax, ay, -1, 1,
                            None, None)


def stats_from_sums(sums, hist, n_total, g, dim):
  """The dictionary of fp_reference_particles / utils.point_stats from raw sums [S, 2 + D + D D] (float64) and counts
  hist [S, ny, nx] (or None): count and bad [S] (finite / non-finite points), mean [S, D] and cov [S, D, D] =
  sum x x^T / count - mean mean^T over the finite ones, hist (int64), density = hist / (n_total cell area), and the raw
  sums (those of two shards add)."""
  S = sums.shape[0]
  n = sums[:, 0]
  mean = sums[:, 2:2 + dim] / n[:, None]
  cov = sums[:, 2 + dim:].reshape(S, dim, dim) / n[:, None, None] - mean[:, :, None] * mean[:, None, :]
  out = {"count": n, "bad": sums[:, 1], "mean": mean, "cov": cov, "sums": sums, "hist": None, "density": None}
  if hist is not None:
    out["hist"] = hist.to(torch.int64)
    out["density"] = out["hist"].double() / (float(n_total) * g.step_x * g.step_y)
  return out


def _stats_buffers(dev, N, dim, S, g, want_sums=True):
  """(sums, hist, workspace) device buffers of one cnf_fp_particles / cnf_point_stats call"""
  lib, C = _capi.lib(), _capi.ctypes
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_fp_particles_workspace(N, dim, S, C.byref(nbytes)), "cnf_fp_particles_workspace")
  sums = torch.empty(S, 2 + dim + dim * dim, dtype=torch.float64, device=dev) if want_sums else None
  ws = torch.empty(-(-nbytes.value // 8), dtype=torch.float64, device=dev) if want_sums else None
  hist = None if g is None else torch.empty(S, g.ny, g.nx, dtype=torch.int32, device=dev)      # (uint32 counts < 2^31)
  return sums, hist, ws


def fp_step_indices(times, h, T):
  """times -> Euler-Maruyama step indices; ValueError for a time that is not a multiple of h to within 1e-9 T, is
  negative, or for times that do not ascend or are more than 64."""
  ts = np.asarray(times.cpu() if torch.is_tensor(times) else times, dtype=np.float64).reshape(-1)
  if not (h > 0.0 and math.isfinite(h)):
    raise ValueError(f"fp_reference_particles: the step h must be positive, not {h}")
  if ts.size < 1 or ts.size > FP_MAX_SNAPSHOTS or not np.isfinite(ts).all():
    raise ValueError(f"fp_reference_particles: between 1 and {FP_MAX_SNAPSHOTS} finite times, not {ts.size}")
  steps = np.rint(ts / h).astype(np.int64)
  if (np.abs(steps * h - ts) > 1e-9 * float(T)).any():
    raise ValueError(f"fp_reference_particles: every time must be a multiple of h = {h} (to within 1e-9 T): {ts.tolist()}")
  if steps[0] < 0 or (np.diff(steps) <= 0).any():
    raise ValueError(f"fp_reference_particles: the times must be >= 0 and ascend: {ts.tolist()}")
  return ts, steps


def fp_reference_particles(dim, T, a, sigma, subtype, times, n_particles=1 << 20, h=1e-3, seed=0, var0=None, x0=None,
                           grid=None, axes=(0, 1), positions=False, shard=None, all_reduce=True):
  """The fp problem's density along `times` from an Euler-Maruyama ensemble of dX = drift(X) dt + sqrt(2 sigma) dW
  (drift `subtype` with parameter a, as flow_matching_loss_fn evaluates it) started from N(0, var0 I) -- var0 = None:
  fp_initial_variance(T), the training's own initial condition -- or from the given x0 [n_particles, dim]: n_particles
  float64 paths of step h in one cnf_fp_particles launch, the normals drawn in the kernel from the cnf_fill_normal
  stream of `seed`.  Particle p's draws depend on (seed, p) alone: the ranks of `shard` split the particles by
  first_particle and the sums and counts are all-reduced (all_reduce=False: this rank's block alone, e.g. one half of
  an ensemble), so the result does not depend on the number of ranks beyond the sums' last bits.
  Returns a dict of device tensors, as stats_from_sums: times [S]; count, bad [S]; mean [S, D]; cov [S, D, D]; sums;
  with `grid` (a utils.field_grid or (domain_range, n), over `axes`) hist [S, ny, nx] and density = hist / (n_particles
  cell area), cell j centred on grid point j -- density_on_grid's points; with positions=True pos [S, count, D], this
  rank's particles.  ValueError before any device work for an unknown drift or one for another dimension, a time that is
  not a multiple of h (1e-9 T), and the C ABI's other refusals."""
  if subtype not in _capi.DRIFTS:
    raise ValueError(f"unknown drift {subtype!r}")
  dim, n_particles = int(dim), int(n_particles)
  if not 1 <= dim <= 14 or FP_DRIFT_DIM.get(subtype, dim) != dim:
    raise ValueError(f"fp_reference_particles: drift {subtype!r} is not defined at dim {dim}")
  ts, steps = fp_step_indices(times, float(h), T)
  var0 = fp_initial_variance(T) if var0 is None else float(var0)
  if n_particles < 1 or not (var0 > 0.0 and math.isfinite(var0)) or not (sigma >= 0.0):
    raise ValueError(f"fp_reference_particles: needs n_particles >= 1, var0 > 0 and sigma >= 0")
  g = stats_grid(grid, axes, dim)
  shard = shard if shard is not None else current_shard()
  start, count = shard_range(n_particles, shard)
  if count < 1:
    raise ValueError(f"fp_reference_particles: {n_particles} particles leave rank {shard.rank} of {shard.world} none")
  dev = torch.device("cuda", torch.cuda.current_device())
  if x0 is not None:
    x0 = torch.as_tensor(x0)
    if tuple(x0.shape) != (n_particles, dim):
      raise ValueError(f"fp_reference_particles: x0 must be [{n_particles}, {dim}], not {tuple(x0.shape)}")
    x0 = x0[start:start + count].to(device=dev, dtype=torch.float64).contiguous()
  u64, off = seed_to_u64(seed)
  S = len(steps)
  # the stream's stride per particle follows n_steps: T / h steps (or the last time's, beyond T), so that every choice
  # of times in [0, T] looks at the same paths; nothing is integrated past the last time
  n_steps = max(int(round(float(T) / float(h))), int(steps[-1]))
  lib, C = _capi.lib(), _capi.ctypes
  sums, hist, ws = _stats_buffers(dev, count, dim, S, g)
  pos = torch.empty(S, count, dim, dtype=torch.float64, device=dev) if positions else None
  snap = (C.c_int64 * S)(*[int(k) for k in steps])
  with _OnDevice(dev):
    _capi.check(lib.cnf_fp_particles(_capi.DRIFTS[subtype], dim, float(a), float(sigma), float(h), n_steps, var0,
                                     u64, off + start, count, None if x0 is None else x0.data_ptr(), snap, S,
                                     None if g is None else C.byref(g), None if pos is None else pos.data_ptr(),
                                     sums.data_ptr(), None if hist is None else hist.data_ptr(), ws.data_ptr(),
                                     ws.numel() * 8, _stream_ptr(dev)), "cnf_fp_particles")
  hist = None if hist is None else hist.to(torch.int64)
  if all_reduce:
    sums = all_reduce_sums(sums, shard)
    hist = None if hist is None else all_reduce_sums(hist, shard)
  out = stats_from_sums(sums, hist, n_particles, g, dim)
  out["times"] = torch.as_tensor(ts, device=dev)
  if positions:
    out["pos"] = pos
  return out


# ---- the grid reference of the 2-D fp problems ----------------------------------------------------------------------
# The same PDE solved on density_on_grid's points by a Scharfetter-Gummel finite-volume scheme in float64: no noise
# floor (cnf_fp_grid, include/cnf_ot_amd.h).
FP_GRID_DRIFTS = ("ou", "gradient", "smile", "nongradient")
FP_GRID_K = (1, 2, 4, 8)
FP_GRID_STEPS_PER_LAUNCH = 8       # the fastest measured at 513 x 513


def fp_grid_initial(g, var0) -> np.ndarray:
  """Exact cell averages [ny, nx] of N(0, var0 I) on the cells of `g` (a CnfFieldGrid): a product of erf differences"""
  s = math.sqrt(2.0 * var0)

  def avg(lo, d, n):
    c = lo + np.arange(n) * d
    e = np.array([math.erf((v - 0.5 * d) / s) for v in c] + [math.erf((c[-1] + 0.5 * d) / s)])
    return 0.5 * (e[1:] - e[:-1]) / d

  return avg(g.lo_y, g.step_y, g.ny)[:, None] * avg(g.lo_x, g.step_x, g.nx)[None, :]


def fp_grid_step_count(delta, rate, safety=0.9) -> int:
  """Explicit steps between two output times `delta` apart: ceil(delta rate / safety), so that dt rate <= safety"""
  return 0 if delta == 0.0 else max(1, int(math.ceil(delta * rate / safety)))


def fp_reference_grid(T, a, sigma, subtype, times, grid, var0=None, rho0=None, safety=0.9, steps_per_launch=None):
  """The 2-D fp problem's density at `times`, d rho / dt = -div(b rho) + sigma lap rho with the drift `subtype` (ou,
  gradient = smile, nongradient; parameter a as float32), solved in float64 on `grid` -- a utils.field_grid or
  (domain_range, n), as stats_grid takes it: cell (j, i) centred on grid point (x_i, y_j), density_on_grid's points --
  by the Scharfetter-Gummel finite-volume scheme of cnf_fp_grid with no-flux box faces.  Start: exact cell averages of
  N(0, var0 I) (var0 = None: fp_initial_variance(T)) or the given rho0 [ny, nx] >= 0.  Between consecutive times Delta
  apart it takes ceil(Delta rate / safety) explicit steps, rate the largest outflow rate: each step is a convex
  combination, so rho stays >= 0 and its sum is kept to rounding.  steps_per_launch in {1, 2, 4, 8} (None:
  FP_GRID_STEPS_PER_LAUNCH) changes the launches, not one bit of the result.
  Returns a dict of device tensors: times [S]; density [S, ny, nx] (float64); mass, min [S]; mean [S, 2]; cov [S, 2, 2];
  n_steps [S] (int64); rate (0-dim); x [nx], y [ny].  The rate is read back once (8 bytes): not for graph capture.
  ValueError before any device work for an unknown drift or one of another dimension, sigma <= 0, safety outside
  (0, 1], times that are negative, do not ascend or are more than FP_MAX_SNAPSHOTS, a rho0 of the wrong shape or with a
  negative entry, and steps_per_launch outside {1, 2, 4, 8}."""
  if subtype not in _capi.DRIFTS:
    raise ValueError(f"unknown drift {subtype!r}")
  if subtype not in FP_GRID_DRIFTS:
    raise ValueError(f"fp_reference_grid: drift {subtype!r} is not defined at dim 2")
  sigma, safety = float(sigma), float(safety)
  if not (sigma > 0.0 and math.isfinite(sigma)):
    raise ValueError(f"fp_reference_grid: sigma must be positive, not {sigma}")
  if not 0.0 < safety <= 1.0:
    raise ValueError(f"fp_reference_grid: safety must lie in (0, 1], not {safety}")
  K = FP_GRID_STEPS_PER_LAUNCH if steps_per_launch is None else steps_per_launch
  if K not in FP_GRID_K:
    raise ValueError(f"fp_reference_grid: steps_per_launch must be one of {FP_GRID_K}, not {steps_per_launch!r}")
  ts = np.asarray(times.cpu() if torch.is_tensor(times) else times, dtype=np.float64).reshape(-1)
  if ts.size < 1 or ts.size > FP_MAX_SNAPSHOTS or not np.isfinite(ts).all():
    raise ValueError(f"fp_reference_grid: between 1 and {FP_MAX_SNAPSHOTS} finite times, not {ts.size}")
  if ts[0] < 0.0 or (np.diff(ts) <= 0.0).any():
    raise ValueError(f"fp_reference_grid: the times must be >= 0 and ascend: {ts.tolist()}")
  if grid is None:
    raise ValueError("fp_reference_grid: needs a grid")
  g = stats_grid(grid, (0, 1), 2)
  nx, ny, S = g.nx, g.ny, int(ts.size)
  if rho0 is None:
    var0 = fp_initial_variance(T) if var0 is None else float(var0)
    if not (var0 > 0.0 and math.isfinite(var0)):
      raise ValueError(f"fp_reference_grid: var0 must be positive, not {var0}")
    start = fp_grid_initial(g, var0)
  else:
    start = np.asarray(rho0.detach().cpu() if torch.is_tensor(rho0) else rho0, dtype=np.float64)
    if start.shape != (ny, nx):
      raise ValueError(f"fp_reference_grid: rho0 must be [{ny}, {nx}], not {list(start.shape)}")
    if not np.isfinite(start).all() or (start < 0.0).any():
      raise ValueError("fp_reference_grid: rho0 must be finite and >= 0")
  dev = torch.device("cuda", torch.cuda.current_device())
  lib, C = _capi.lib(), _capi.ctypes
  f64 = dict(dtype=torch.float64, device=dev)
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_fp_grid_coeffs_bytes(nx, ny, C.byref(nbytes)), "cnf_fp_grid_coeffs_bytes")
  coef = torch.empty(nbytes.value // 8, **f64)
  _capi.check(lib.cnf_fp_grid_steps_workspace(nx, ny, C.byref(nbytes)), "cnf_fp_grid_steps_workspace")
  ws = torch.empty(nbytes.value // 8, **f64)
  rate = torch.empty((), **f64)
  density = torch.empty(S, ny, nx, **f64)
  stats = torch.empty(S, 7, **f64)
  cur = torch.as_tensor(np.ascontiguousarray(start)).to(dev)
  n_steps = []
  with _OnDevice(dev):
    st = _stream_ptr(dev)
    _capi.check(lib.cnf_fp_grid_coeffs(_capi.DRIFTS[subtype], 2, float(a), sigma, C.byref(g), coef.data_ptr(),
                                       coef.numel() * 8, rate.data_ptr(), st), "cnf_fp_grid_coeffs")
    R = float(rate)                                  # the one read-back
    t_prev = 0.0
    for s in range(S):
      delta = float(ts[s]) - t_prev
      n = fp_grid_step_count(delta, R, safety)
      density[s].copy_(cur)
      cur = density[s]
      if n:
        _capi.check(lib.cnf_fp_grid_steps(coef.data_ptr(), nx, ny, delta / n, n, K, cur.data_ptr(), ws.data_ptr(),
                                          ws.numel() * 8, st), "cnf_fp_grid_steps")
      n_steps.append(n)
      t_prev = float(ts[s])
    _capi.check(lib.cnf_fp_grid_stats(C.byref(g), density.data_ptr(), S, stats.data_ptr(), st), "cnf_fp_grid_stats")
  mass = stats[:, 0]
  mean = stats[:, 2:4] / mass[:, None]
  second = torch.stack([stats[:, 4], stats[:, 5], stats[:, 5], stats[:, 6]], -1).reshape(S, 2, 2) / mass[:, None, None]
  return {"times": torch.as_tensor(ts, device=dev), "density": density, "mass": mass, "min": stats[:, 1], "mean": mean,
          "cov": second - mean[:, :, None] * mean[:, None, :], "stats": stats,
          "n_steps": torch.as_tensor(n_steps, dtype=torch.int64, device=dev), "rate": rate,
          "x": g.lo_x + g.step_x * torch.arange(nx, **f64), "y": g.lo_y + g.step_y * torch.arange(ny, **f64)}


def fp_grid_coefficients(a, sigma, subtype, grid):
  """The face coefficients of fp_reference_grid on `grid` as float64 device tensors (cxL, cxR [ny, nx + 1], cyL, cyR
  [ny + 1, nx]) and the 0-dim rate: the probes' and the tests' view of cnf_fp_grid_coeffs."""
  if subtype not in FP_GRID_DRIFTS:
    raise ValueError(f"fp_grid_coefficients: drift {subtype!r} is not defined at dim 2")
  g = stats_grid(grid, (0, 1), 2)
  nx, ny = g.nx, g.ny
  dev = torch.device("cuda", torch.cuda.current_device())
  lib, C = _capi.lib(), _capi.ctypes
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_fp_grid_coeffs_bytes(nx, ny, C.byref(nbytes)), "cnf_fp_grid_coeffs_bytes")
  coef = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
  rate = torch.empty((), dtype=torch.float64, device=dev)
  with _OnDevice(dev):
    _capi.check(lib.cnf_fp_grid_coeffs(_capi.DRIFTS[subtype], 2, float(a), float(sigma), C.byref(g), coef.data_ptr(),
                                       coef.numel() * 8, rate.data_ptr(), _stream_ptr(dev)), "cnf_fp_grid_coeffs")
  nxf, nyf = ny * (nx + 1), (ny + 1) * nx
  return (coef[:nxf].view(ny, nx + 1), coef[nxf:2 * nxf].view(ny, nx + 1), coef[2 * nxf:2 * nxf + nyf].view(ny + 1, nx),
          coef[2 * nxf + nyf:].view(ny + 1, nx), rate)


# ---- the particle reference of the rwpo problems --------------------------------------------------------------------
# The Hopf-Cole formula read as an expectation (the reference's cost_rwpo, solvers.py:190-220, is its nested Monte-Carlo
# at dim 2): with eps = 1 / beta the optimal path measure is Brownian motion of variance 2 eps t from rho0, reweighted by
# exp(-g(X_T) / (2 eps)) / h(X_0).  cnf_rwpo_particles (include/cnf_ot_amd.h) draws the inner ensembles
# from a two-centre Gaussian proposal, one wave per outer particle, and the Brownian bridges to the selected endpoints.
RWPO_MAX_INNER = 1 << 20


def rwpo_proposal(dim, T, beta, a, subtype) -> dict:
  """The inner proposal z = shrink y +- centre + sqrt(prop_var) xi of rwpo_reference_particles for a potential:
  quadratic: the exact posterior of X_T given y (every weight equal); double_well: the Gaussians that the Brownian
  kernel and the well's curvature beta a^2 dim at +-a 1 give, P = beta a^2 dim + beta / (2 T) their precision;
  obstacle: the plain Brownian kernel.  dict(shrink, prop_var, centre: [dim] float64 or None)."""
  if subtype not in _capi.POTENTIALS:
    raise ValueError(f"unknown potential {subtype!r}")
  dim, T, beta, a = int(dim), float(T), float(beta), float(a)
  if subtype == "quadratic":
    return {"shrink": 1.0 / (1.0 + T), "prop_var": 2.0 * T / (beta * (1.0 + T)), "centre": None}
  if subtype == "double_well":
    curv = beta * a * a * dim
    P = curv + beta / (2.0 * T)
    return {"shrink": (beta / (2.0 * T)) / P, "prop_var": 1.0 / P, "centre": np.full(dim, a * curv / P)}
  return {"shrink": 1.0, "prop_var": 2.0 * T / beta, "centre": None}


def rwpo_selection_uniforms(n_total, seed) -> np.ndarray:
  """The float64 uniforms in [0, 1) that pick every outer particle's endpoint among its inner draws, particle p's at
  index p: a host Philox generator keyed by `seed`.  They are an input of cnf_rwpo_particles, so that a result is a
  function of its arguments."""
  u64, off = seed_to_u64(seed)
  return np.random.Generator(np.random.Philox(key=u64)).random(int(off) + int(n_total))[int(off):]


def rwpo_reference_particles(dim, T, beta, a, subtype, times, n_particles=65536, n_inner=4096, seed=0, var0=None,
                             proposal=None, grid=None, first=0, want_pos=False):
  """The rwpo problem's optimal value, endpoint law and path density at any dimension from one cnf_rwpo_particles call:
  n_particles outer particles y ~ N(0, var0 I) (var0 = None: rwpo_initial_variance(T, beta)), n_inner weighted draws of
  X_T each from `proposal` (None: rwpo_proposal's), one endpoint per particle selected by rwpo_selection_uniforms and a
  Brownian bridge through `times` (ascending, in [0, T], at most 64).  Global particle first + i depends on (seed,
  first + i) alone.  Returns a dict of device tensors: stats_from_sums' keys of the bridge's positions (count, bad [S];
  mean [S, D]; cov [S, D, D]; sums; with `grid` -- a utils.field_grid or (domain_range, n) over axes (0, 1) -- hist and
  density), times [S], and
    log_h, ess [N], mean_T [N, D], sel [N]   log h(y_i), the effective sample size, E[X_T | y_i], the selected draw
    y [N, D], drift0 = (mean_T - y) / T      the outer particles (from the stream) and the optimal control at time 0
    true_val = -(2 / beta) mean log_h        the optimal energy; true_val_se: its standard error from the sample
    bias_est = (2 / beta) mean((1 / ess - 1 / K) / 2)   the first-order self-normalisation bias: true_val lies above the
                                             limit by it; true_val_corrected = true_val - bias_est
  (0-dim tensors), and with want_pos=True pos [S, N, D].  ValueError before any device work for an unknown potential,
  sizes or times out of range; the C ABI's other refusals raise CnfError."""
  if subtype not in _capi.POTENTIALS:
    raise ValueError(f"unknown potential {subtype!r}")
  dim, N, K, first = int(dim), int(n_particles), int(n_inner), int(first)
  ts = np.ascontiguousarray(np.asarray(times.cpu() if torch.is_tensor(times) else times, dtype=np.float64).reshape(-1))
  S = ts.size
  if not 1 <= dim <= 14 or N < 1 or not 1 <= K <= RWPO_MAX_INNER or first < 0:
    raise ValueError(f"rwpo_reference_particles: needs 1 <= dim <= 14, n_particles >= 1, 1 <= n_inner <= 2^20, first >= 0")
  if not 1 <= S <= FP_MAX_SNAPSHOTS or not np.isfinite(ts).all() or ts[0] < 0.0 or ts[-1] > T or (np.diff(ts) <= 0).any():
    raise ValueError(f"rwpo_reference_particles: between 1 and {FP_MAX_SNAPSHOTS} ascending times in [0, T]: {ts.tolist()}")
  var0 = rwpo_initial_variance(T, beta) if var0 is None else float(var0)
  prop = rwpo_proposal(dim, T, beta, a, subtype) if proposal is None else proposal
  centre = prop.get("centre")
  centre = None if centre is None else np.ascontiguousarray(np.broadcast_to(np.asarray(centre, dtype=np.float64), (dim,)))
  g = stats_grid(grid, (0, 1), dim)
  dev = torch.device("cuda", torch.cuda.current_device())
  u64, off = seed_to_u64(seed)
  lib, C = _capi.lib(), _capi.ctypes
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_rwpo_particles_workspace(N, dim, S, C.byref(nbytes)), "cnf_rwpo_particles_workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  ws = torch.empty(-(-nbytes.value // 8), **f64)
  u = torch.as_tensor(rwpo_selection_uniforms(first + N, seed)[first:]).to(dev)
  out = {"log_h": torch.empty(N, **f64), "ess": torch.empty(N, **f64), "mean_T": torch.empty(N, dim, **f64),
         "sel": torch.empty(N, dtype=torch.int32, device=dev)}
  sums = torch.empty(S, 2 + dim + dim * dim, **f64)
  hist = None if g is None else torch.empty(S, g.ny, g.nx, dtype=torch.int32, device=dev)
  pos = torch.empty(S, N, dim, **f64) if want_pos else None
  dptr = C.POINTER(C.c_double)
  with _OnDevice(dev):
    _capi.check(lib.cnf_rwpo_particles(_capi.POTENTIALS[subtype], dim, float(a), float(T), float(beta), var0,
                                       float(prop["shrink"]), float(prop["prop_var"]),
                                       None if centre is None else centre.ctypes.data_as(dptr), K, u64, off + first, N,
                                       u.data_ptr(), ts.ctypes.data_as(dptr), S, None if g is None else C.byref(g),
                                       out["log_h"].data_ptr(), out["ess"].data_ptr(), out["mean_T"].data_ptr(),
                                       out["sel"].data_ptr(), None if pos is None else pos.data_ptr(), sums.data_ptr(),
                                       None if hist is None else hist.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                       _stream_ptr(dev)), "cnf_rwpo_particles")
    # y again from the stream: the first dim elements of each particle's R
    R = rwpo_stream_stride(dim, K, S)
    head = -(-dim // 4) * 4
    y = torch.empty(N, head, dtype=torch.float32, device=dev)
    if R <= 4096:                             # whole strides, a block of particles at a time
      block = max(1, (1 << 26) // R)
      z = torch.empty(min(N, block) * R, dtype=torch.float32, device=dev)
      for i0 in range(0, N, block):
        n = min(block, N - i0)
        _capi.check(lib.cnf_fill_normal(u64, (off + first + i0) * R, n * R, z.data_ptr(), _stream_ptr(dev)),
                    "cnf_fill_normal")
        y[i0:i0 + n].copy_(z[:n * R].reshape(n, R)[:, :head])
    else:                                     # the head of each stride alone
      for i in range(N):
        _capi.check(lib.cnf_fill_normal(u64, (off + first + i) * R, head, y.data_ptr() + 4 * head * i, _stream_ptr(dev)),
                    "cnf_fill_normal")
    y = y[:, :dim]
  out.update(stats_from_sums(sums, None if hist is None else hist.to(torch.int64), N, g, dim))
  out["times"] = torch.as_tensor(ts, device=dev)
  out["y"] = y.double() * math.sqrt(var0)
  out["drift0"] = (out["mean_T"] - out["y"]) / float(T)
  out.update(rwpo_value_of(out["log_h"], out["ess"], beta, K))
  if want_pos:
    out["pos"] = pos
  return out


def rwpo_stream_stride(dim, n_inner, n_times) -> int:
  """R: the elements of the cnf_fill_normal stream that a particle of cnf_rwpo_particles owns"""
  return 4 * (-(-dim // 4) + n_inner * (-(-(dim + 1) // 4)) + -(-n_times * dim // 4))


def rwpo_value_of(log_h, ess, beta, n_inner) -> dict:
  """true_val, true_val_se, bias_est and true_val_corrected (0-dim tensors) from the outer particles' log_h and ess"""
  c = 2.0 / float(beta)
  n = log_h.numel()
  val = -c * log_h.mean()
  se = c * (log_h.std(unbiased=True) / math.sqrt(n) if n > 1 else torch.full_like(val, float("nan")))
  bias = c * ((1.0 / ess - 1.0 / float(n_inner)) / 2.0).mean()
  return {"true_val": val, "true_val_se": se, "bias_est": bias, "true_val_corrected": val - bias}


# ---- the particle reference of the interacting (McKean-Vlasov) fp problem -------------------------------------------
# d rho / dt = -div(rho (drift - strength grad (W * rho))) + sigma lap rho is the mean-field limit of N particles that
# feel, beside the drift and the noise, the force of the other N - 1 through the pair kernel W: cnf_mv_particles
# (include/cnf_ot_amd.h) steps R independent replicas of such a system, the pair force by
# cnf_interaction's own kernel, the step, stream and statistics cnf_fp_particles'.

def mv_quadratic_ou_variance(t, a, sigma, strength, amp, var0):
  """Per-coordinate variance at time t of the mean-field limit for the drift "ou" (-a x) and the quadratic kernel
  W = amp r^2 / 2, started from N(0, var0 I): the force strength amp (x - mean) adds to the drift's pull, so with
  lam = a + strength amp the variance obeys v' = -2 lam v + 2 sigma: v_inf + (var0 - v_inf) exp(-2 lam t), v_inf =
  sigma / lam (ou_variance with a -> lam); for lam = 0, var0 + 2 sigma t."""
  lam = float(a) + float(strength) * float(amp)
  if lam == 0.0:
    return var0 + 2.0 * sigma * t
  v_inf = sigma / lam
  return v_inf + (var0 - v_inf) * math.exp(-2.0 * lam * t)


def mv_log_second_moment(t, dim, sigma, strength, amp, m0):
  """E mean_i |x_i|^2 at time t of the interacting system with the log kernel W = amp ln r (utils.interaction_spec's
  kind "power", one exponent 0, no softening), no drift and noise sigma, started at E mean |x|^2 = m0:
    m0 + (2 dim sigma - strength amp) t,
  exact in every dimension and for EVERY N, not only in the mean-field limit (the Keller-Segel virial identity).  With
  G_i = (1 / (N - 1)) sum_{j != i} amp (x_i - x_j) / |x_i - x_j|^2, antisymmetry of the pair force gives
  sum_i x_i . G_i = (amp / (N - 1)) sum_{i < j} |x_i - x_j|^2 / |x_i - x_j|^2 = amp N / 2, so Ito's formula for
  dx_i = -strength G_i dt + sqrt(2 sigma) dB reads d E mean |x|^2 / dt = -2 strength amp / 2 + 2 dim sigma.  A softening
  length eps replaces each pair's 1 by d^2 / (d^2 + eps^2) (the drift term shrinks by the pair mean of eps^2 / (d^2 +
  eps^2)), and Euler-Maruyama with step h adds h strength^2 mean |G|^2 per unit time: neither is in this form."""
  return float(m0) + (2.0 * float(dim) * float(sigma) - float(strength) * float(amp)) * float(t)


def mv_reference_particles(dim, T, a, sigma, subtype, interaction, strength, times, n_particles=16384, replicas=2,
                           h=1e-3, seed=0, var0=None, x0=None, grid=None, axes=(0, 1), positions=False):
  """The interacting fp problem's density along `times` from `replicas` independent systems of n_particles particles
    x_i <- x_i + h (drift(x_i) - strength G_i) + sqrt(2 sigma h) z,  G_i = mean_{j != i} grad W(x_i - x_j),
  drift `subtype` with parameter a as in fp_reference_particles, W the pair kernel of `interaction` (the keyword
  arguments of utils.interaction_spec), in ONE cnf_mv_particles call: float64 state, the pair force by cnf_interaction's
  kernel on the float32 rounding of the positions (self mode), two launches per step.  Start, stream and times as
  fp_reference_particles (global particle r n_particles + i); x0: [replicas, n_particles, dim].  strength = 0 gives
  fp_reference_particles' paths bit for bit.  A particle that is not finite is counted in `bad` and is not masked out
  of the pair sums: from the next step on its whole replica is not finite.
  Returns fp_reference_particles' dictionary over the POOLED replicas (count, bad, mean, cov, times, hist and density
  with `grid`) and, per replica, energy [S, R] = F = sum_{i != j} W / (2 N (N - 1)) of the step's own pair pass,
  replica_mean [S, R, D], replica_cov [S, R, D, D], the raw sums [S, R, 3 + D + D D] (their last column: the W sum; the
  pooled moments are the other columns added over R) and, with positions=True, pos [S, R, N, D].
  ValueError before any device work for what fp_reference_particles, utils.interaction_spec and
  utils.interaction_check_shapes refuse, a strength that is not finite, and more than one rank (pairs across ranks need
  an all-gather of the positions per step)."""
  name = "mv_reference_particles"
  if subtype not in _capi.DRIFTS:
    raise ValueError(f"unknown drift {subtype!r}")
  dim, N, R = int(dim), int(n_particles), int(replicas)
  if not 1 <= dim <= 14 or FP_DRIFT_DIM.get(subtype, dim) != dim:
    raise ValueError(f"{name}: drift {subtype!r} is not defined at dim {dim}")
  ts, steps = fp_step_indices(times, float(h), T)
  var0 = fp_initial_variance(T) if var0 is None else float(var0)
  if not (var0 > 0.0 and math.isfinite(var0)) or not (sigma >= 0.0 and math.isfinite(sigma)) or not math.isfinite(a):
    raise ValueError(f"{name}: needs var0 > 0, sigma >= 0 and a finite a")
  if not math.isfinite(float(strength)):
    raise ValueError(f"{name}: the strength must be finite, not {strength}")
  spec = ia.interaction_spec(**dict(interaction))
  ia.interaction_check_shapes((R, N, dim))
  g = stats_grid(grid, axes, dim)
  if current_shard().world > 1:
    raise ValueError(f"{name}: single rank only (pairs across ranks need an all-gather of the positions per step)")
  if x0 is not None:
    x0 = torch.as_tensor(x0)
    if tuple(x0.shape) != (R, N, dim):
      raise ValueError(f"{name}: x0 must be [{R}, {N}, {dim}], not {tuple(x0.shape)}")
  u64, off = seed_to_u64(seed)
  S = len(steps)
  n_steps = max(int(round(float(T) / float(h))), int(steps[-1]))      # (the stream's stride: fp_reference_particles')
  if n_steps > 1 << 30 or (off + R * N) > ((1 << 63) - 1) // 4 // (-(-(n_steps + 1) * dim // 4)):
    raise ValueError(f"{name}: more than 2^30 steps, or the normals' stream index does not fit")
  dev = torch.device("cuda", torch.cuda.current_device())
  if x0 is not None:
    x0 = x0.to(device=dev, dtype=torch.float64).contiguous()
  lib, C = _capi.lib(), _capi.ctypes
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_mv_particles_workspace(R, N, dim, S, C.byref(nbytes)), "cnf_mv_particles_workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  K = 3 + dim + dim * dim
  ws = torch.empty(-(-nbytes.value // 8), **f64)
  state, sums = torch.empty(R, N, dim, **f64), torch.empty(S, R, K, **f64)
  pos = torch.empty(S, R, N, dim, **f64) if positions else None
  hist = None if g is None else torch.empty(S, g.ny, g.nx, dtype=torch.int32, device=dev)
  snap = (C.c_int64 * S)(*[int(k) for k in steps])
  with _OnDevice(dev):
    _capi.check(lib.cnf_mv_particles(C.byref(spec), float(strength), _capi.DRIFTS[subtype], dim, float(a), float(sigma),
                                     float(h), n_steps, var0, u64, off, R, N, None if x0 is None else x0.data_ptr(),
                                     snap, S, None if g is None else C.byref(g), state.data_ptr(),
                                     None if pos is None else pos.data_ptr(), sums.data_ptr(),
                                     None if hist is None else hist.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                     _stream_ptr(dev)), "cnf_mv_particles")
  out = stats_from_sums(sums[:, :, :K - 1].sum(1), hist, R * N, g, dim)
  per = stats_from_sums(sums[:, :, :K - 1].reshape(S * R, K - 1), None, N, None, dim)
  out["times"] = torch.as_tensor(ts, device=dev)
  out["energy"] = sums[:, :, K - 1] / (2.0 * N * (N - 1.0))
  out["replica_mean"], out["replica_cov"] = per["mean"].reshape(S, R, dim), per["cov"].reshape(S, R, dim, dim)
  out["sums"] = sums
  if positions:
    out["pos"] = pos
  return out


def mv_stationary_score(x, a, sigma, subtype, interaction, strength):
  """The score a stationary law of the interacting fp equation has at its own points x [N, D] or [S, N, D]: zero
  current, sigma grad log rho = drift - strength grad (W * rho), with the empirical measure of x for rho:
    (drift(x_i) - strength mean_{j != i} grad W(x_i - x_j)) / sigma,
  the drift "ou" (-a x), the force by autograd.interaction_force (self mode, the pair kernel of `interaction`: the
  keyword arguments of utils.interaction_spec), so the result is differentiable in x.  float32 on x's device.  The KSD
  of x against it (utils.ksd) is a stationarity residual of an ensemble, or of the flow's samples at a large time.
  ValueError before any device work for an unknown drift, a drift other than "ou" (the zero-current identity needs a
  gradient drift; the other drifts' stationary laws carry a current), a sigma that is not positive and finite, an a or a
  strength that is not finite and what utils.interaction_spec refuses."""
  from . import autograd
  name = "mv_stationary_score"
  if subtype not in _capi.DRIFTS:
    raise ValueError(f"unknown drift {subtype!r}")
  if subtype != "ou":
    raise ValueError(f"{name}: only the drift 'ou': the zero-current identity needs a gradient drift, not {subtype!r}")
  if not (float(sigma) > 0.0 and math.isfinite(float(sigma))) or not math.isfinite(float(a)):
    raise ValueError(f"{name}: needs sigma > 0 and a finite a, not {sigma}, {a}")
  if not math.isfinite(float(strength)):
    raise ValueError(f"{name}: the strength must be finite, not {strength}")
  kw = dict(interaction)
  ia.interaction_vjp_check_spec(ia.interaction_spec(**kw))
  x = torch.as_tensor(x)
  force = autograd.interaction_force(x, **kw)
  return (-float(a) * x.to(device=force.device, dtype=torch.float32) - float(strength) * force) * (1.0 / float(sigma))


# ---- an ensemble as fields: density, score and probability-flow velocity at given points ------------------------------
# The flow trains v_flow + sigma grad log rho = drift (flow_matching_loss_fn).  For the drifts without a closed-form
# score the only source of the true right-hand side is the particle reference; its kernel density estimate (cnf_kde,
# DESIGN.md 5.3r) gives log rho_t and grad log rho_t at any points in the full dimension.

_C28_9, _C8_3 = float(np.float32(28.0) / np.float32(9.0)), float(np.float32(8.0) / np.float32(3.0))


def fp_drift(x, a, subtype):
  """The drifts of drift_field (csrc/cnf_terms.h) at x [..., D] in torch, in x's dtype: "ou" -a x at any D, "gradient"
  (= "smile") and "nongradient" at D = 2, "lorenz" at D = 3; a and the Lorenz constants 28 / 9 and 8 / 3 as float32.
  ValueError for an unknown drift and for a drift at another dimension."""
  if subtype not in _capi.DRIFTS:
    raise ValueError(f"unknown drift {subtype!r}")
  x = torch.as_tensor(x)
  D = x.shape[-1]
  if FP_DRIFT_DIM.get(subtype, D) != D:
    raise ValueError(f"fp_drift: drift {subtype!r} is not defined at dim {D}")
  a = float(np.float32(a))
  if subtype == "ou":
    return x * -a
  if subtype in ("gradient", "smile"):
    X, Y = x[..., 0], x[..., 1]
    q = X * X + Y * Y - 4.0
    return torch.stack([(-q * X) * a, (-q * Y - (Y - 1.0) * 2.0) * a], -1)
  if subtype == "nongradient":
    X, Y = x[..., 0], x[..., 1]
    return torch.stack([X * -a - Y * 0.5, Y * -a + X * 0.5], -1)
  X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
  return torch.stack([(Y - X) * 10.0, X * 9.0 * (_C28_9 - Z) - Y, X * 9.0 * Y - Z * _C8_3], -1)


def ensemble_fields(points, particles, sigma, a, subtype, bandwidths=None, interaction=None, strength=0.0) -> dict:
  """What an ensemble `particles` ([N, D] or [S, N, D]) of the fp problem (drift `subtype` with parameter a, diffusion
  sigma) says at `points` ([Q, D] or [S, Q, D]), by its kernel density estimate (utils.kde, ONE cnf_kde call):
    log_density [S, B, Q], score [S, B, Q, D]   the estimate's, per bandwidth (None: kde_bandwidths(particles))
    velocity [S, B, Q, D]  the probability-flow velocity drift(q) - sigma score [- strength force], with `interaction`
                           (the keyword arguments of utils.interaction_spec) force = grad (W * rho)(q) from
                           utils.interaction_field(points, particles, ...): the mean over ALL particles
    bandwidths
  float32 on the device; the leading axis is dropped for 2-D points.  ValueError before any device work for what
  fp_drift, utils.kde and utils.interaction_field refuse and for a sigma or strength that is not finite."""
  if not math.isfinite(float(sigma)) or not math.isfinite(float(strength)):
    raise ValueError(f"ensemble_fields: sigma and the strength must be finite, not {sigma}, {strength}")
  fp_drift(torch.zeros(1, int(np.shape(points)[-1])), a, subtype)      # (its refusals, before any device work)
  if interaction is not None:
    ia.interaction_spec(**dict(interaction))
  est = kd.kde(points, particles, bandwidths, want_score=True, loo=False)
  score = est["score"]
  q = torch.as_tensor(points).detach().to(device=score.device, dtype=torch.float32)
  vel = fp_drift(q, a, subtype).unsqueeze(-3) - float(sigma) * score
  if interaction is not None:
    force = ia.interaction_field(points, particles, want_force=True, **dict(interaction))["force"]
    vel = vel - float(strength) * force.unsqueeze(-3)
  return {"log_density": est["log_density"], "score": score, "velocity": vel, "bandwidths": est["bandwidths"]}


# ---- importance-sampling diagnostics against the densities known in closed form -------------------------------------
# The reference's kl_ess (tests/test_fit_prob.py:50-56, "metrics used in the tori paper"): draw y from the flow, weight
# w = p_target(y) / q_flow(y), report Z = mean w, KL = mean(log q - log p) + log Z, ESS = (sum w)^2 / sum w^2.  It
# divides in linear space, where sum w underflows to 0 as soon as the flow is far from its target; here one fused
# launch (cnf_importance_stats) returns, per time, the raw state of the LOG-weights l = log p - log q,
#   (m, s1, s2, c, n) = (max l, sum exp(l - m), sum exp(2 (l - m)), sum l, count),
# which merges exactly across ranks and calls (merge_importance_stats) and gives the three numbers in log space.

class GaussianMixtureTarget:
  """The packer of CnfTargetSpec: sum_m weights[m] N(means[m], scale * cov), up to 8 components and dim 14.  means
  [n_comp, D] (or [D]: one component); cov: None = I, a scalar v = v I, or a symmetric positive definite [D, D]
  matrix; weights: None = uniform, else positive numbers (normalised here).  `scale` is a per-time factor of the
  covariance given with the call, not part of the target.  ValueError for a covariance that is not positive definite,
  more than 8 components or dim > 14."""

  def __init__(self, means, cov=None, weights=None):
    mu = np.atleast_2d(np.asarray(means, dtype=np.float64))
    if mu.ndim != 2 or mu.shape[0] < 1 or mu.shape[1] < 1:
      raise ValueError(f"GaussianMixtureTarget: means must be [n_comp, D], got {np.shape(means)}")
    n, D = mu.shape
    if n > _capi.TARGET_MAX_COMP:
      raise ValueError(f"GaussianMixtureTarget: {n} components, at most {_capi.TARGET_MAX_COMP}")
    if D > _capi.TARGET_MAX_DIM:
      raise ValueError(f"GaussianMixtureTarget: dim {D}, at most {_capi.TARGET_MAX_DIM}")
    if cov is None:
      A = np.eye(D)
    elif np.ndim(cov) == 0:
      A = float(cov) * np.eye(D)
    else:
      A = np.asarray(cov, dtype=np.float64)
      if A.shape != (D, D) or not np.allclose(A, A.T, rtol=1e-12, atol=0.0):
        raise ValueError(f"GaussianMixtureTarget: cov must be a symmetric [{D}, {D}] matrix")
    if not np.all(np.isfinite(A)) or not np.all(np.isfinite(mu)):
      raise ValueError("GaussianMixtureTarget: means and cov must be finite")
    try:
      L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
      raise ValueError("GaussianMixtureTarget: cov is not positive definite") from None
    # cov = L L^T, so cov^-1 = W^T W with the lower-triangular W = L^-1
    W = np.tril(np.linalg.solve(L, np.eye(D)))
    w = np.full(n, 1.0 / n) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (n,) or not np.all(np.isfinite(w)) or not np.all(w > 0.0):
      raise ValueError(f"GaussianMixtureTarget: weights must be {n} positive numbers")
    self.dim, self.n_comp = D, n
    self.means, self.cov, self.W = mu, A, W
    self.log_weights = np.log(w / w.sum())
    self.log_det_W = -float(np.log(np.diag(L)).sum())
    s = self.spec = _capi.CnfTargetSpec()
    s.n_comp = n
    for i in range(n):
      s.log_weight[i] = self.log_weights[i]
      for d in range(D):
        s.mean[i][d] = mu[i, d]
    for i in range(n, _capi.TARGET_MAX_COMP):
      s.log_weight[i] = -math.inf
    for i in range(_capi.TARGET_MAX_DIM):      # (identity past D: the struct is valid at any dimension's checks)
      s.W[i][i] = 1.0
    for i in range(D):
      for j in range(i + 1):
        s.W[i][j] = W[i, j]
    s.log_det_W = self.log_det_W
    s.scale = None

  def score(self, x, scale=None):
    """grad log p at the points x [..., D], in torch and differentiable in x, in x's dtype and on its device: with the
    responsibilities r_m(x) of the components, -sum_m r_m cov^-1 (x - means[m]) / scale (scale: the covariance's factor,
    None = 1).  What `ksd` compares a point set against."""
    x = torch.as_tensor(x)
    if x.shape[-1] != self.dim:
      raise ValueError(f"GaussianMixtureTarget.score: points of dimension {self.dim}, not {tuple(x.shape)}")
    kw = dict(dtype=x.dtype, device=x.device)
    inv = 1.0 if scale is None else 1.0 / float(scale)
    W, mu = torch.as_tensor(self.W, **kw), torch.as_tensor(self.means, **kw)
    y = (x[..., None, :] - mu) @ W.T                                    # [..., n_comp, D]: W (x - mu_m)
    r = torch.softmax(torch.as_tensor(self.log_weights, **kw) - 0.5 * inv * (y * y).sum(-1), dim=-1)
    return -inv * ((r[..., None] * y).sum(-2) @ W)


# the times of the fp figure (solvers.FIGURE_SETTINGS[("fp", None, 2)]): where fp / ou reports its fit along the path
FP_FIT_TIMES = (0.0, 0.05, 0.1, 0.3, 1.0)


def known_densities(config):
  """[(t, target, scale)]: every density of `config`'s problem that is known in closed form, as a target of
  `importance_stats` at condition t (scale: the variance factor of the target's covariance at that time, or None).
    ot:   the configured source (ot.source, default "mixture": the 8-mode mixture of applications.py:34-71, or
          "gaussian": N(-3 1, A); both dim 2) at 0 and N(0, I) at T = 1
    rwpo: the initial condition N(0, 2 (T + 1) / beta I) at 0
    fp:   the initial condition N(0, (T + 1) / 2 I) at 0; with the OU drift the exact density
          N(0, ou_variance(t) I) at the figure's times (one unit-covariance target, the variances as scales)"""
  g = config["general"]
  _type, dim = g["type"], g["dim"]
  zero = np.zeros((1, dim))
  if _type == "ot":
    out = []
    source = config["ot"].get("source", "mixture")
    if dim == 2 and source == "mixture":
      out.append((0.0, GaussianMixtureTarget(MIXTURE_CENTERS.astype(np.float64)), None))
    elif dim == 2 and source == "gaussian":
      out.append((0.0, GaussianMixtureTarget([[-3.0, -3.0]], np.array([[5.0, 1.0], [1.0, 0.5]])), None))
    return out + [(1.0, GaussianMixtureTarget(zero), None)]
  if _type == "rwpo":
    r = config["rwpo"]
    return [(0.0, GaussianMixtureTarget(zero, rwpo_initial_variance(r["T"], r["beta"])), None)]
  if _type == "fp":
    f = config["fp"]
    T, var0 = float(f["T"]), fp_initial_variance(f["T"])
    if f["velocity_field_type"] != "ou":
      return [(0.0, GaussianMixtureTarget(zero, var0), None)]
    unit = GaussianMixtureTarget(zero)
    times = sorted({t for t in FP_FIT_TIMES if t < T} | {T})
    return [(t, unit, ou_variance(t, f["a"], var0, f["sigma"])) for t in times]
  raise Exception(f"Unknown problem type: {_type}...")


def merge_importance_stats(parts) -> torch.Tensor:
  """Merges raw [S, 5] blocks (m, s1, s2, c, n) of disjoint sample sets into the block of their union, in float64, part
  by part in the order given: the scaled sums are brought to the common maximum, c and n add.  An empty block
  (m = -inf, zeros) is a no-op; a slice that is NaN in one block stays NaN."""
  parts = [torch.as_tensor(p, dtype=torch.float64) for p in parts]
  if not parts:
    raise ValueError("merge_importance_stats: nothing to merge")
  out = parts[0].clone()
  for p in parts[1:]:
    p = p.to(out.device)
    m = torch.maximum(out[:, 0], p[:, 0])
    empty = m == -math.inf
    ea = torch.where(empty, torch.zeros_like(m), torch.exp(out[:, 0] - m))
    eb = torch.where(empty, torch.zeros_like(m), torch.exp(p[:, 0] - m))
    out = torch.stack([m, out[:, 1] * ea + p[:, 1] * eb, out[:, 2] * ea * ea + p[:, 2] * eb * eb, out[:, 3] + p[:, 3],
                       out[:, 4] + p[:, 4]], 1)
  return out


def importance_summary(raw: torch.Tensor):
  """The numbers of a raw [S, 5] block, each a float64 [S] tensor: log_Z = log mean w, KL = mean(log q - log p) + log_Z,
  ess = (sum w)^2 / sum w^2 (in [1, n]), ess_pct = 100 ess / n, max_log_w; and the block itself as `raw`."""
  raw = torch.as_tensor(raw, dtype=torch.float64)
  m, s1, s2, c, n = raw.unbind(1)
  log_Z = torch.log(s1) + m - torch.log(n)
  ess = torch.exp(2.0 * torch.log(s1) - torch.log(s2))
  return {"log_Z": log_Z, "KL": -c / n + log_Z, "ess": ess, "ess_pct": 100.0 * ess / n, "max_log_w": m, "n": n, "raw": raw}


def importance_stats(model, params, target, conds, rng, batch_size, scale=None, shard=None):
  """The importance-sampling fit of the flow at the times `conds` against `target` (GaussianMixtureTarget; scale: the
  covariance factor per time, or None): `importance_summary` of batch_size samples per time, time s drawing samples
  [s batch_size, (s + 1) batch_size) of the stream of `rng` inside the kernel -- ONE fused launch, nothing but 5
  doubles per time returned.  Sharded (shard, default: the torch.distributed world): a rank takes its shard_range of
  every time's samples, the raw blocks are all-gathered and merged in rank order, so every rank returns the same
  numbers, independent of the rank count beyond rounding.  A shard given without an initialised process group cannot
  gather: the rank's own block comes back, to be merged by the caller (merge_importance_stats on `raw`)."""
  if target.dim != model.cfg.dim:
    raise ValueError(f"importance_stats: a target of dim {target.dim} for a flow of dim {model.cfg.dim}")
  shard = shard if shard is not None else current_shard()
  be = model.terms_backend(params)
  start, count = shard_range(batch_size, shard)
  raw = be.importance_stats(target, t=_conds(conds), B=count, seed=rng, first_sample=start, slice_stride=int(batch_size),
                            scale=scale)
  if shard.world > 1:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
      blocks = [torch.empty_like(raw) for _ in range(shard.world)]
      dist.all_gather(blocks, raw, group=shard.group)
      raw = merge_importance_stats(blocks)
  return importance_summary(raw)


# ---- sample-only fitting terms: a distance between the flow's samples and given target samples ----------------------

def _sample_term(name, why, model, params, target, cond, rng, batch_size, shard, grad, refuse, stat):
  """The mean over the times of `cond` of a point-set statistic (two_sample, interaction) of batch_size flow samples
  per time -- the same base draw of `rng` for every time -- against `target`, [M, D] or one set per time, or (target
  None) of the samples alone; with `grad` its parameter gradient, by ONE cnf_pass_vjp call seeded with the statistic's
  gradient in the samples / S.  The term supplies
  refuse(S, target shape [S, M, D] or None): its own ValueErrors, returning what its checks resolved; and
  stat(samples [S, B, D], target [S, M, D] or None, what refuse returned, want_grad) -> (values [S], gradient [S, B, D]
  or None).  Every refusal, the term's included, comes before the backend is touched; a term without a target also
  refuses a terms backend that is not the HIP engine, before it is used.  `why`: the subject of the single-rank
  refusal."""
  shard = shard if shard is not None else current_shard()
  if shard.world > 1:
    raise ValueError(f"{name}: single rank only ({why} an all-gather of the samples)")
  conds = _conds(cond)
  S = _n_conds(conds)
  tgt = None
  if target is not None:
    tgt = target if torch.is_tensor(target) else torch.as_tensor(np.asarray(target))
    if tgt.dim() == 2:
      tgt = tgt[None].expand(S, -1, -1)
    if tgt.dim() != 3 or tgt.shape[0] != S:
      raise ValueError(f"{name}: target must be [M, D] or [{S}, M, D] (one set per time), not {tuple(tgt.shape)}")
  checked = refuse(S, None if tgt is None else tgt.shape)
  ctx = _Ctx(model, params, rng, shard, grad)
  if tgt is None and not ctx.hip:
    raise ValueError(f"{name}: the terms backend must be the HIP engine, not {type(ctx.be).__name__}")
  be = ctx.be
  z, _, count = ctx.noise(batch_size)
  zs = z.repeat(S, 1)                                         # the same draw for every time
  c = be.slice_conds(conds)
  samples, _ = be.forward_logdet(zs, c, want_logdet=False)
  values, xgrad = stat(samples.view(S, count, -1),
                       None if tgt is None else tgt.to(device=samples.device, dtype=torch.float32), checked,
                       grad is not None)
  if grad is not None:
    be.pass_vjp(zs, c, (xgrad * (1.0 / S)).view(S * count, -1), None, False, grad=grad, want_xbar=False)
  return values.sum() / S


# ---- MMD^2 / energy distance ------------------------------------------------------------------------------------------

def mmd_loss_fn(model, dim, params, target, cond, rng, batch_size, bandwidths=None, kind="gaussian", shard=None,
                grad=None):
  """The mean over the times of `cond` of the unbiased MMD^2 (kind="gaussian"; bandwidths=None:
  utils.median_bandwidths(target)) or energy distance (kind="energy") between batch_size flow samples at that time --
  the same base draw of `rng` for every time, as the other terms -- and the samples `target`: [M, D], or [S, M, D] with
  one set per time.  A fitting term for a target known by its samples alone.  With `grad` (the convention of the
  other term functions; `value_and_grad` supplies it) the parameter gradient is accumulated by ONE cnf_mmd2 call
  (value and d / d samples) and ONE cnf_pass_vjp call.  Single rank: the pairs across ranks would need an all-gather of
  the samples, so a shard (or a torch.distributed world) of more than one rank raises ValueError."""
  def refuse(S, tgt_shape):
    two_sample.mmd_check_shapes((S, int(batch_size), int(dim)), tgt_shape)
    if kind == "gaussian" and bandwidths is not None:
      two_sample.mmd_spec(bandwidths, kind)
    elif kind not in _capi.MMD_KINDS:
      raise ValueError(f"mmd_loss_fn: kind is 'gaussian' or 'energy', not {kind!r}")

  def stat(samples, tgt, checked, want_grad):      # (the median bandwidths: of the target where the samples are)
    bws = two_sample.median_bandwidths(tgt) if kind == "gaussian" and bandwidths is None else bandwidths
    res = two_sample.mmd2(samples, tgt, bws, kind, want_grad=want_grad)
    return res["mmd2"], res.get("grad")
  return _sample_term("mmd_loss_fn", "pairs across ranks need", model, params, target, cond, rng, batch_size, shard, grad,
                      refuse, stat)


# ---- the same in transport units: the Sinkhorn divergence between the flow's samples and given target samples --------

def sinkhorn_loss_fn(model, dim, params, target, cond, rng, batch_size, eps=0.05, schedule=None, shard=None, grad=None):
  """The mean over the times of `cond` of the Sinkhorn divergence S_eps (utils.sinkhorn: cost |x - y|^2 / 2, an
  estimate of W2^2 / 2) between batch_size flow samples at that time -- the same base draw of `rng` for every time, as
  the other terms -- and the samples `target`: [M, D], or [S, M, D] with one set per time.  schedule: the eps of every
  iteration (None: utils.sinkhorn_schedule of the samples and the target at `eps`, which reads the samples' bounding
  box back from the device; a fixed schedule does not).  With `grad` (the convention of the other term functions;
  `value_and_grad` supplies it) the parameter gradient is accumulated by ONE cnf_sinkhorn call (value and the envelope
  gradient d / d samples) and ONE cnf_pass_vjp call.  Single rank: the pairs across ranks would need an all-gather of the
  samples, so a shard (or a torch.distributed world) of more than one rank raises ValueError."""
  def refuse(S, tgt_shape):      # -> the checked schedule, or None
    two_sample.sinkhorn_check_shapes((S, int(batch_size), int(dim)), tgt_shape)
    if schedule is not None:
      return two_sample.sinkhorn_check_schedule(schedule)
    if not (float(eps) > 0.0 and np.isfinite(float(eps))):
      raise ValueError(f"sinkhorn_loss_fn: eps must be positive and finite, not {eps}")

  def stat(samples, tgt, sched, want_grad):
    res = two_sample.sinkhorn(samples, tgt, eps, sched, want_grad=want_grad)
    return res["divergence"], res["grad"]
  return _sample_term("sinkhorn_loss_fn", "pairs across ranks need", model, params, target, cond, rng, batch_size, shard,
                      grad, refuse, stat)


# ---- the same at any batch size: the sliced Wasserstein distance between the flow's samples and target samples ------

def sliced_loss_fn(model, dim, params, target, cond, rng, batch_size, directions=None, n_proj=64, seed=0, shard=None,
                   grad=None):
  """The mean over the times of `cond` of the sliced Wasserstein distance (utils.sliced_wasserstein: cost |.|^2 / 2)
  between batch_size flow samples at that time -- the same base draw of `rng` for every time, as the other terms -- and
  the samples `target`: [M, D], or [S, M, D] with one set per time.  directions: [P, dim], constants (None:
  utils.sliced_directions(dim, n_proj, seed)).  N log N per projection, so the term is usable at the flow's own
  training batch sizes, where the pair statistics are not.  With `grad` (the convention of the other term functions;
  `value_and_grad` supplies it) the parameter gradient is accumulated by ONE cnf_sliced_w2 call (value and the
  envelope gradient d / d samples) and ONE cnf_pass_vjp call.  Single rank: the sort would need an all-gather of the
  samples, so a shard (or a torch.distributed world) of more than one rank raises ValueError."""
  def refuse(S, tgt_shape):      # -> the directions as a tensor
    th = two_sample.sliced_directions(int(dim), 1 if int(dim) == 1 else n_proj, seed) if directions is None else directions
    th = th if torch.is_tensor(th) else torch.as_tensor(np.asarray(th))
    two_sample.sliced_check_shapes((S, int(batch_size), int(dim)), tgt_shape, tuple(th.shape))
    return th

  def stat(samples, tgt, th, want_grad):
    res = two_sample.sliced_wasserstein(samples, tgt, th, want_grad=want_grad)
    return res["sw"], res["grad"]
  return _sample_term("sliced_loss_fn", "the sort across ranks needs", model, params, target, cond, rng, batch_size, shard,
                      grad, refuse, stat)


# ---- the nonlocal cost of a mean-field control problem: the interaction energy of the flow's own samples --------------

def interaction_loss_fn(model, dim, params, cond, rng, batch_size, kind, amplitudes=None, bandwidths=None, shard=None,
                        grad=None, exponents=None):
  """The mean over the times of `cond` of the interaction energy F = sum_{i != j} W(x_i - x_j) / (2 N (N - 1))
  (utils.interaction_energy: kind, amplitudes, bandwidths and exponents are utils.interaction_spec's) of batch_size flow
  samples at that time -- the same base draw of `rng` for every time, as the other sample terms.  W > 0 is congestion, W < 0 or
  quadratic W aggregation, a Morse W swarming.  With `grad` (the convention of the other term functions;
  `value_and_grad` supplies it) the parameter gradient is accumulated by ONE cnf_interaction call (value and
  d / d samples) and ONE cnf_pass_vjp call; more than 64 times go in chunks of 64 sets.  Single rank: the pairs across
  ranks would need an all-gather of the samples, so a shard (or a torch.distributed world) of more than one rank raises
  ValueError, as does a terms backend that is not the HIP engine."""
  def refuse(S, _):      # -> the spec
    ia.interaction_check_shapes((min(S, _capi.MMD_MAX_SETS), int(batch_size), int(dim)))
    return ia.interaction_spec(kind, amplitudes, bandwidths, exponents)

  def stat(samples, _, spec, want_grad):
    return ia.energy_of_sets(spec, samples, want_grad)
  return _sample_term("interaction_loss_fn", "pairs across ranks need", model, params, None, cond, rng, batch_size, shard,
                      grad, refuse, stat)


# ---- a target known through its score alone: the kernel Stein discrepancy of the flow's own samples -------------------

def ksd_loss_fn(model, dim, params, target, cond, rng, batch_size, kind="imq", bandwidths=None, beta=-0.5, weights=None,
                scale=None, shard=None, grad=None):
  """The mean over the times of `cond` of the kernel Stein discrepancy KSD^2_U (utils.ksd: kind, bandwidths, beta and
  weights are utils.stein_spec's; bandwidths=None: utils.median_bandwidths of the first time's samples) of batch_size
  flow samples at that time -- the same base draw of `rng` for every time, as the other sample terms -- against the law
  whose score `target` gives: an object with .score(x, scale) (GaussianMixtureTarget; `scale` is passed on) or a
  callable x [S, B, D] -> the score at x, built from torch ops where it depends on x.  A fitting term for a target
  known up to its constant, from no samples of it.  With `grad` (the convention of the other term functions;
  `value_and_grad` supplies it) the sample gradient is cnf_stein's grad_x plus the score's vector-Jacobian product of
  its grad_score, taken by torch autograd, and the parameter gradient is accumulated by ONE cnf_stein call per 64 times
  and ONE cnf_pass_vjp call.  Single rank: the pairs across ranks would need an all-gather of the samples, so a shard
  (or a torch.distributed world) of more than one rank raises ValueError, as do a DeviceRng (the captured step) and a
  terms backend that is not the HIP engine."""
  name = "ksd_loss_fn"
  if isinstance(rng, DeviceRng):
    raise ValueError(f"{name}: for the eager update only (the captured step draws on the device)")
  if hasattr(target, "score"):
    score_fn = lambda x: target.score(x, scale)
  elif callable(target):
    score_fn = target
  else:
    raise ValueError(f"{name}: target must have a .score(x, scale) or be a callable x -> score, not {type(target).__name__}")

  def refuse(S, _):      # -> the spec, or None while the bandwidths wait for the samples
    stein.stein_check_shapes((min(S, _capi.MMD_MAX_SETS), int(batch_size), int(dim)))
    # (kind, beta and the weights are checked either way: the median heuristic gives STEIN_MAX_TERMS bandwidths)
    spec = stein.stein_spec(kind, [1.0] * stein.STEIN_MAX_TERMS if bandwidths is None else bandwidths, beta, weights)
    return None if bandwidths is None else spec

  def stat(samples, _, spec, want_grad):
    if spec is None:
      spec = stein.stein_spec(kind, two_sample.median_bandwidths(samples)[:stein.STEIN_MAX_TERMS], beta, weights)
    xs = samples.detach().requires_grad_(want_grad)
    with torch.enable_grad():
      sc = score_fn(xs)
    if tuple(sc.shape) != tuple(xs.shape):
      raise ValueError(f"{name}: the score must have the samples' shape {tuple(xs.shape)}, not {tuple(sc.shape)}")
    s3 = sc.detach().to(dtype=torch.float32).contiguous()
    values, gx, gs = stein.ksd_of_sets(spec, samples.detach().contiguous(), s3, want_grad)
    if want_grad and sc.requires_grad:
      gx = gx + torch.autograd.grad(sc, xs, gs.to(sc.dtype))[0]
    return values, gx
  return _sample_term(name, "pairs across ranks need", model, params, None, cond, rng, batch_size, shard, grad, refuse, stat)


def _interaction_refuse(name, given, rng, shard, sub, dim):
  """(spec, strength) of a composite loss's `interaction=(spec_kwargs, strength)` -- ValueError, before any device work,
  for what the interaction part refuses: a captured step, more than one rank, fewer than 2 samples per time, a bad
  spec."""
  spec_kwargs, strength = given
  if isinstance(rng, DeviceRng):
    raise ValueError(f"{name}: an interaction term is for the eager update only (the captured step draws on the device)")
  if (shard if shard is not None else current_shard()).world > 1:
    raise ValueError(f"{name}: an interaction term is single rank only (pairs across ranks need an all-gather of the "
                     "samples)")
  if sub < 2:
    raise ValueError(f"{name}: an interaction term needs batch_size // 32 >= 2 samples per time, not {sub}")
  ia.interaction_check_shapes((1, int(sub), int(dim)))
  return ia.interaction_spec(**spec_kwargs), float(strength)


def _interaction_values(ctx, spec, conds, sub, coef):
  """F [S] (float64) of the first `sub` samples of the loss's draw at the times `conds` (a host array), by ONE
  cnf_interaction call per 64 times; with ctx.grad, coef / S times the gradient of their sum is queued as one base ->
  data backward pass (defer_pass_vjp: it leaves with the loss's other passes, in `reduce`)."""
  if not ctx.hip:
    raise ValueError(f"an interaction term needs the HIP engine as the terms backend, not {type(ctx.be).__name__}")
  be = ctx.be
  z, _, count = ctx.noise(sub)
  th = _conds(conds)
  S = _n_conds(th)
  zs = z.repeat(S, 1)                                         # the same draw for every time
  samples, _ = be.forward_logdet(zs, be.slice_conds(th), want_logdet=False)
  values, xgrad = ia.energy_of_sets(spec, samples.view(S, count, -1), ctx.grad is not None)
  if ctx.grad is not None:
    ctx.defer_pass_vjp(zs, th, count, (xgrad * (coef / S)).view(S * count, -1), None)
  return values


# ---- composite losses ---------------------------------------------------------

def ot_loss_fn(model, dim, T, dt, t_batch_size, subtype, params, rng, _lambda, batch_size,
               source="mixture", shard=None, grad=None, overlap=None, interaction=None):
  """applications.py:377-402.  overlap (sharded value_and_grad only; default OVERLAP_ALLREDUCE): the density-fit
  terms' all-reduce runs under the kinetic / obstacle slices.  interaction=(spec_kwargs, strength): the loss gains
  strength T mean_t F(rho_t), the interaction energy (interaction_loss_fn; spec_kwargs: utils.interaction_spec's
  arguments) at the time batch the loss drew, on the batch_size // 32 samples of the kinetic term -- no extra host
  draw; its gradient lands in `grad`.  Eager, single rank."""
  if interaction is not None:
    ia_spec, ia_strength = _interaction_refuse("ot_loss_fn", interaction, rng, shard, batch_size // 32, dim)
  ctx = _Ctx(model, params, rng, shard, grad)
  t_batch = draw_t_batch(rng, t_batch_size)
  sub = batch_size // 32
  c_kl, c_kin = _lambda / batch_size, 0.5 / (sub * t_batch_size)
  first = [_kl_sum(ctx, T, 0.0, batch_size, source, c_kl), _kl_sum(ctx, T, float(T), batch_size, source, c_kl)]
  if interaction is not None:      # (after the full draw: its samples are that draw's first rows)
    ia_values = _interaction_values(ctx, ia_spec, t_batch, sub, ia_strength * T)

  def later():
    if subtype == "obstacle":      # summed, not averaged, over slices (applications.py:397-400)
      z, _, count = ctx.noise(sub)
      if _on_tables(ctx, count, _n_conds(t_batch), passes=2):      # one forward + one backward launch for both
        return list(_kinetic_potential_tables(ctx, z, t_batch, count, dt, c_kin, "obstacle", 0.0, 1.0 / sub))
      return [_kinetic_sum(ctx, dt, t_batch, sub, c_kin), _potential_sum(ctx, 0.0, "obstacle", t_batch, sub, 1.0 / sub)]
    return [_kinetic_sum(ctx, dt, t_batch, sub, c_kin)]

  c_later = [c_kin] + ([1.0 / sub] if subtype == "obstacle" else [])
  if (OVERLAP_ALLREDUCE if overlap is None else overlap) and ctx.shard.world > 1 and ctx.grad is not None:
    return ctx.combine_overlapped(first, [c_kl, c_kl], later, c_later)
  loss = ctx.combine(first + later(), [c_kl, c_kl] + c_later)
  # (one addition, in the float64 `combine` returns; the part's backward pass left with the others, in `reduce`)
  return loss if interaction is None else loss + (ia_strength * T) * (ia_values.sum() / t_batch_size)


def rwpo_loss_fn(model, dim, T, beta, dt, dx, t_batch_size, subtype, a, params, rng, _lambda, batch_size,
                 shard=None, grad=None, interaction=None):
  """applications.py:405-421.  interaction=(spec_kwargs, strength): as ot_loss_fn's."""
  if interaction is not None:
    ia_spec, ia_strength = _interaction_refuse("rwpo_loss_fn", interaction, rng, shard, batch_size // 32, dim)
  ctx = _Ctx(model, params, rng, shard, grad)
  t_batch = draw_t_batch(rng, t_batch_size, T)
  sub = batch_size // 32
  c_rkl, c_pot, c_kin = _lambda / batch_size, 1.0 / batch_size, 0.5 * T / (sub * t_batch_size)
  sums = [_reverse_kl_sum(ctx, T, beta, 0.0, batch_size, c_rkl),
          _potential_sum(ctx, a, subtype, [float(T)], batch_size, c_pot),
          _kinetic_score_sum(ctx, beta, dt, dx, t_batch, sub, c_kin)]
  if interaction is not None:      # (after the full draw: its samples are that draw's first rows)
    ia_values = _interaction_values(ctx, ia_spec, t_batch, sub, ia_strength * T)
  loss = ctx.combine(sums, [c_rkl, c_pot, c_kin])
  return loss if interaction is None else loss + (ia_strength * T) * (ia_values.sum() / t_batch_size)


def fp_loss_fn(model, dim, T, a, sigma, dt, dx, t_batch_size, subtype, params, rng, _lambda, batch_size,
               shard=None, grad=None, interaction=None):
  """applications.py:424-441 (beta = 4: the initial Gaussian has variance 1, :432).  interaction=(spec_kwargs, strength):
  the interacting (McKean-Vlasov) problem d rho / dt = -div(rho (drift - strength grad (W * rho))) + sigma lap rho, whose
  particle form is mv_reference_particles: the flow-matching residual gains strength * f, f the self-mode force of the
  batch_size // 32 samples of each time (utils.interaction_energy's, spec_kwargs: utils.interaction_spec's arguments).
  The force sits inside the square, so its backward is the pair-Hessian pass cnf_interaction_vjp; the term takes the
  composed route at every dimension (`_score_terms_unfused`).  The gradient is the exact one of the discrete objective
  (for the exponential kind in dimension 1 it has no delta term from the kink of W).  Eager, single rank, the HIP engine
  as the terms backend: ValueError otherwise, before any device work.  None: the code as it was."""
  if interaction is not None:
    ia_spec, ia_strength = _interaction_refuse("fp_loss_fn", interaction, rng, shard, batch_size // 32, dim)
    ia.interaction_vjp_check_spec(ia_spec)
    if not np.isfinite(ia_strength):
      raise ValueError(f"fp_loss_fn: the interaction's strength must be finite, not {ia_strength}")
    _flow_matching_check(dim, subtype)
  ctx = _Ctx(model, params, rng, shard, grad)
  if interaction is not None and not ctx.hip:
    raise ValueError(f"fp_loss_fn: an interaction term needs the HIP engine as the terms backend, not {type(ctx.be).__name__}")
  t_batch = draw_t_batch(rng, t_batch_size, T)
  sub = batch_size // 32
  c_rkl, c_fm = _lambda / batch_size, 0.5 * T / (sub * t_batch_size)
  given = None if interaction is None else (ia_spec, ia_strength)
  return ctx.combine([_reverse_kl_sum(ctx, T, 4.0, 0.0, batch_size, c_rkl),
                      _flow_matching_sum(ctx, dim, a, sigma, subtype, t_batch, sub, c_fm, given)], [c_rkl, c_fm])


def value_and_grad(loss_fn):
  """jax.value_and_grad(loss_fn) of cnf_ot/mfc/solvers.py:94 for the loss
  functions of this module (bound with functools.partial like the reference
  does): returns f(params, *args, **kw) -> (loss, grads) with `grads` a
  `Params` tree (haiku names) over one flat gradient tensor."""
  from .params import Params

  def wrapped(params, *args, **kw):
    if not isinstance(params, Params) or not params.flat.is_cuda:
      raise TypeError("value_and_grad needs device-resident cnf_ot_amd.Params")
    g = torch.zeros_like(params.flat)
    loss = loss_fn(params, *args, grad=g, **kw)
    return loss, Params(params.cfg, g)

  return wrapped
