"""The analytic float64 adjoint of tests/flow_adjoint_f64.py against what it must agree with before the GPU kernels
are held to it: central differences of the C oracle (the other, independently written restatement of the flow) over
ALL parameters and all inputs, oracle.pwl_grad's conditioner backward, the transpose identity, forward and inverse
Jacobians as mutual inverses, its own float32 run, and -- for every case of test_gpu_flow_adjoint.py -- the cap on the
share of drawn points that the kink margins may remove.

The difference quotient's own error.  g_h = (f(p + h) - f(p - h)) / 2h = f' + h^2 f''' / 6 + O(h^4) + r, with the
rounding term |r| <= 8 eps F / h for F = the sum of the magnitudes of f's summands (float64 eps = 2.2e-16; 8: a
summand is itself a sum of the base term and L D spline terms, each the end of a dozen rounded operations, and the
two evaluations' errors add).  The truncation term is measured, not guessed: g_3h - g_h = 8 h^2 f''' / 6 + O(h^4), so
|g_h - f'| <= |g_3h - g_h| / 8 + 8 eps F / h up to O(h^4).  At h = 1e-6 and F ~ 1e2 the rounding term is ~2e-7 absolute,
the truncation term below 1e-9: about 1e-9 .. 1e-7 of a block's largest entry.  Asserted per tensor: the derived bound
(x 2 for the O(h^4) remainder and the 3h quotient's own rounding), and -- so that a quotient straddling a kink, which inflates the measured truncation term,
cannot loosen the check unnoticed -- 1e-6 of the block's largest entry (1e-3 of the whole gradient's for a block that
is all but zero).  The difference terms divide differences of O(1) values by dt = dx = 0.01 before they square them:
F, and with it the quotient's rounding term, is 1 / dt larger for the same gradient, and their cap is 1e-5."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import flow_adjoint_f64 as fa  # noqa: E402

H_STEP, EPS = 1e-6, 2.2e-16
SHAPES = [(D, L, 16, 2, 5) for D in (1, 2, 3) for L in (1, 2, 3)] + [(14, 2, 16, 2, 5), (2, 2, 8, 3, 4), (3, 1, 32, 1, 8)]


def _points(cfg, flat, rng, B, to_base):
  """(B points, a quarter of them beyond |x| > 10, their conditions): none within 1e-3 of a knot or a ReLU -- a
  parameter step of 3e-6 moves neither that far.  (At dim 14 one point in ten is that far from all 832 ReLUs.)"""
  n = B * (6 if cfg.D <= 5 else 80)
  pool, c = fa.draw_points(rng, n, cfg.D), rng.random(n)
  knot, relu = fa.margins(cfg, flat, pool, c, to_base)
  ok = (knot >= 1e-3) & (relu >= 1e-3)
  tail = (np.abs(pool) > 10).any(1)
  keep = np.sort(np.concatenate([np.flatnonzero(ok & tail)[:B // 4], np.flatnonzero(ok & ~tail)[:B - B // 4]]))
  assert keep.size == B, keep.size
  return pool[keep].astype(np.float64), c[keep]


def _fd_all(f, p, h):
  g = np.zeros(p.size)
  for i in range(p.size):
    q = p.copy(); q[i] += h; fp = f(q); q[i] -= 2 * h
    g[i] = (fp - f(q)) / (2 * h)
  return g


def _assert_blocks(cfg, g, g_h, g_3h, F, what, cap=1e-6):
  worst = 0.0
  top = np.abs(g_h).max()
  for name, off, n in fa.param_blocks(cfg):
    s = slice(off, off + n)
    err = np.abs(g[s] - g_h[s]).max()
    bound = 2 * (np.abs(g_3h[s] - g_h[s]).max() / 8 + 8 * EPS * F / H_STEP)
    scale = max(np.abs(g_h[s]).max(), 1e-3 * top)
    worst = max(worst, err / scale)
    assert err <= bound and err <= cap * scale, (what, name, err, bound, scale)
  return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-L%d-H%d-M%d-K%d" % s)
def test_pass_vjp_against_central_differences_of_the_oracle(shape):
  """pass_vjp, both directions, every parameter and every input coordinate, ybar and ldbar both set."""
  D, L, H, M, K = shape
  cfg = oracle.OracleConfig(D=D, L=L, H=H, M=M, K=K)
  rng = np.random.default_rng(10 * D + L)
  flat = fa.random_params(cfg, 0.2 if D <= 3 else 0.25 / np.sqrt(D), 7 * D + L).astype(np.float64)
  B = 32
  for to_base in (False, True):
    pts, c = _points(cfg, flat, rng, B, to_base)
    yb, lb = rng.normal(size=(B, D)), rng.normal(size=B)
    fn = oracle.inverse_logdet if to_base else oracle.forward_logdet
    out, ld, xbar, grad = fa.pass_vjp(cfg, flat, pts, c, yb, lb, to_base)
    o_ref, l_ref = fn(cfg, flat, pts, c)
    assert np.abs(out - o_ref).max() <= 1e-12 and np.abs(ld - l_ref).max() <= 1e-12
    assert (np.abs(pts) > 10).any(1).sum() == B // 4

    def f(p, x=pts):
      y, l = fn(cfg, p, x, c)
      return float((y * yb).sum() + (l * lb).sum())

    F = float(np.abs(o_ref * yb).sum() + np.abs(l_ref * lb).sum())
    g_h, g_3h = _fd_all(f, flat, H_STEP), _fd_all(f, flat, 3 * H_STEP)
    worst = _assert_blocks(cfg, grad, g_h, g_3h, F, (shape, to_base))
    xfd = []
    for h in (H_STEP, 3 * H_STEP):
      q = np.zeros((B, D))
      for e in range(D):
        xp, xm = pts.copy(), pts.copy(); xp[:, e] += h; xm[:, e] -= h
        (yp, lp), (ym, lm) = fn(cfg, flat, xp, c), fn(cfg, flat, xm, c)
        q[:, e] = (((yp - ym) * yb).sum(1) + (lp - lm) * lb) / (2 * h)
      xfd.append(q)
    ex = np.abs(xbar - xfd[0]).max()
    assert ex <= 2 * (np.abs(xfd[1] - xfd[0]).max() / 8 + 8 * EPS * F / H_STEP) and ex <= 1e-6 * np.abs(xfd[0]).max()
    print(f"[pass_vjp {shape} to_base={to_base}] worst block {worst:.1e}  xbar {ex / np.abs(xfd[0]).max():.1e}")


def _ns(kind, subtype=0, dt=0.01, dx=0.01, coef=0.5, a=1.0, T=1.0, beta=4.0):
  return SimpleNamespace(kind=kind, subtype=subtype, dt=dt, dx=dx, coef=coef, a=a, T=T, beta=beta)


TERMS = [(2, _ns(fa.KINETIC)), (2, _ns(fa.KINETIC_SCORE)), (2, _ns(fa.FLOW_MATCHING, 0)), (2, _ns(fa.FLOW_MATCHING, 1)),
         (2, _ns(fa.FLOW_MATCHING, 2)), (3, _ns(fa.FLOW_MATCHING, 3)), (2, _ns(fa.POTENTIAL, 0)),
         (2, _ns(fa.POTENTIAL, 1, a=1.5)), (2, _ns(fa.POTENTIAL, 2)), (2, _ns(fa.REVERSE_KL)), (3, _ns(fa.REVERSE_KL)),
         (2, _ns(fa.NEG_LOGPROB)), (1, _ns(fa.NEG_LOGPROB))]


@pytest.mark.parametrize("D,spec", TERMS, ids=lambda v: f"{v.kind}.{v.subtype}" if hasattr(v, "kind") else f"D{v}")
def test_term_grad_against_the_oracle_losses(D, spec):
  """term_grad: the values equal oracle_backend.OracleBackend.loss_terms to 1e-10, the gradient its central differences
  over every parameter."""
  from oracle_backend import OracleBackend
  from cnf_ot_amd import FlowConfig
  cfg = FlowConfig(dim=D)
  rng = np.random.default_rng(50 + spec.kind)
  flat = fa.random_params(cfg, 0.2, 60 + spec.kind).astype(np.float64)
  t = np.array([0.3, 0.7])
  B, shared = 32, spec.kind % 2 == 0
  pool = fa.draw_points(rng, 6 * B, D, 1.5, 0.3) if spec.kind == fa.NEG_LOGPROB else rng.normal(size=(6 * B, D)).astype(np.float32)
  knot, relu = fa.term_margins(cfg, flat, spec, pool, t)
  keep = np.flatnonzero((knot.min(0) >= 1e-3) & (relu.min(0) >= 1e-3))[:B if shared else 2 * B]
  pts = pool[keep].astype(np.float64)
  assert pts.shape[0] == (B if shared else 2 * B)
  sums, grad = fa.term_grad(cfg, flat, spec, pts, t, B, shared)
  ref = OracleBackend(cfg, flat).loss_terms(spec, pts, t, B, shared).numpy()
  assert np.abs(sums - ref).max() <= 1e-10 * np.abs(ref).max(), (sums, ref)
  f = lambda p: float(OracleBackend(cfg, p).loss_terms(spec, pts, t, B, shared).sum())
  # F: the summands of a difference term are squares of differences over dt, each formed from values of size ~|r| / dt
  amp = 1.0 / spec.dt if spec.kind <= fa.FLOW_MATCHING else 1.0
  F = float(np.abs(ref).sum()) * amp + B * len(t) * amp * amp
  g_h, g_3h = _fd_all(f, flat, H_STEP), _fd_all(f, flat, 3 * H_STEP)
  worst = _assert_blocks(fa._cfg(cfg), grad, g_h, g_3h, F, (D, spec.kind, spec.subtype), 1e-5 if amp > 1 else 1e-6)
  print(f"[term_grad D={D} kind={spec.kind}.{spec.subtype}] |g|inf {np.abs(grad).max():.3g}  worst block {worst:.1e}")


def test_conditioner_block_against_pwl_grad():
  """The dim-2 conditioner's backward (the one MLP of a one-layer flow) == oracle.pwl_grad.grad_per_sample for the
  theta adjoints this module's spline backward hands it, and its input adjoint."""
  from oracle import pwl_grad
  cfg = oracle.OracleConfig(D=2, L=1)
  rng = np.random.default_rng(3)
  flat = fa.random_params(cfg, 0.3, 4).astype(np.float64)
  B = 200
  pts = fa.draw_points(rng, B, 2).astype(np.float64)
  net = fa._Net(cfg, flat, np.float64)
  c = np.full(B, 0.37)
  out, _, recs, _, _ = fa._forward(net, pts, c, True)
  crec, tab, srec = recs[0][2][1]
  yb, lb = rng.normal(size=B), rng.normal(size=B)
  _, xkb, ykb, dlb = fa._spline_bwd(net, srec, tab, yb, lb)
  g = net.tables_bwd(tab, xkb, ykb, dlb)
  grad = np.zeros(net.n)
  kb = net.theta_bwd(0, 1, crec, g, grad)
  want, du = pwl_grad.grad_per_sample(flat[16:], 0.37, out[:, 0], g)
  assert np.abs(grad[16:] - want).max() <= 1e-12 * np.abs(want).max()
  assert np.abs(kb[:, 0] - du).max() <= 1e-12 * np.abs(du).max()


@pytest.mark.parametrize("D,L", [(2, 2), (3, 3), (5, 2)])
def test_transpose_identity_and_mutually_inverse_jacobians(D, L):
  """<ybar, J v> + ldbar (d logdet . v) == <xbar, v> for random v (J v by central differences of this module's own
  forward), and the Jacobians of the two directions, row by row from pass_vjp, are inverses of each other; their
  log-determinants are the passes' logdet."""
  cfg = oracle.OracleConfig(D=D, L=L)
  rng = np.random.default_rng(D + L)
  flat = fa.random_params(cfg, 0.2, D).astype(np.float64)
  B = 24
  c = rng.random(B)
  for to_base in (False, True):
    pts, cc = _points(cfg, flat, rng, B, to_base)
    yb, lb, v = rng.normal(size=(B, D)), rng.normal(size=B), rng.normal(size=(B, D))
    _, _, xbar, _ = fa.pass_vjp(cfg, flat, pts, cc, yb, lb, to_base)
    h = 1e-6
    yp, lp, _, _ = fa.pass_vjp(cfg, flat, pts + h * v, cc, None, None, to_base)
    ym, lm, _, _ = fa.pass_vjp(cfg, flat, pts - h * v, cc, None, None, to_base)
    lhs = ((yp - ym) / (2 * h) * yb).sum(1) + lb * (lp - lm) / (2 * h)
    rhs = (xbar * v).sum(1)
    assert np.abs(lhs - rhs).max() <= 1e-7 * max(np.abs(rhs).max(), 1.0)
  x = rng.normal(size=(B, D)) * 1.3
  y, ld_f, _, _ = fa.pass_vjp(cfg, flat, x, c, None, None, False)
  eye = np.eye(D)
  Jf = np.stack([fa.pass_vjp(cfg, flat, x, c, np.tile(eye[i], (B, 1)), None, False)[2] for i in range(D)], 1)
  Ji = np.stack([fa.pass_vjp(cfg, flat, y, c, np.tile(eye[i], (B, 1)), None, True)[2] for i in range(D)], 1)
  assert np.abs(Jf @ Ji - eye).max() <= 1e-9
  x_back, ld_i, _, _ = fa.pass_vjp(cfg, flat, y, c, None, None, True)
  assert np.abs(x_back - x).max() <= 1e-10 and np.abs(ld_f + ld_i).max() <= 1e-10
  assert np.abs(np.log(np.abs(np.linalg.det(Jf))) - ld_f).max() <= 1e-9


def test_float32_run_is_finite_and_at_float32_level():
  """The same statements in float32 (the noise floor the GPU bounds are measured with): finite everywhere, every
  result float32, and within 1e-4 of a tensor's largest float64 entry -- ~1e-6 is typical; the cases' tails (|x| up
  to 13) and 1 / bin width factors take the rest."""
  worst = 0.0
  for case in fa.PASS_CASES[:32]:
    r = fa.pass_case(case)
    for a32, a64 in zip(r.r32, r.r64):
      assert a32.dtype == np.float32 and np.isfinite(a32).all()
    for name, off, n in fa.param_blocks(r.cfg):
      s = slice(off, off + n)
      e = np.abs(r.r32[3][s] - r.r64[3][s]).max() / max(np.abs(r.r64[3][s]).max(), 1e-3 * np.abs(r.r64[3]).max(), 1e-30)
      worst = max(worst, e)
    ex = np.abs(r.r32[2] - r.r64[2]).max() / max(np.abs(r.r64[2]).max(), 1e-30)
    worst = max(worst, ex)
  print(f"[float32 run] worst tensor {worst:.1e}")
  assert worst <= 1e-4


def test_no_gpu_case_drops_more_than_five_percent_of_its_points():
  """The selection rule of the GPU module (knot margin >= 1e-4 of the bin, ReLU margin >= 1e-5) removes at most 5 % of
  the points drawn, in every case."""
  shares = {}
  for case in fa.PASS_CASES:
    shares[("pass",) + case] = fa.pass_case(case).dropped
  for case in fa.TERM_CASES:
    shares[("term", fa.term_case_id(case))] = fa.term_case(case).dropped
  shares[("multi",)] = fa.multi_case().dropped
  for case in fa.SCORE_CASES:
    shares[("score",) + case] = fa.score_case(case).dropped
  for case in fa.TABLE_CASES:
    for k, v in fa.table_case(case).dropped.items():
      shares[("table", k) + case] = v
  worst = max(shares, key=shares.get)
  print(f"[dropped] mean {np.mean(list(shares.values())):.2%}  worst {shares[worst]:.2%} {worst}")
  assert shares[worst] <= fa.MAX_DROPPED, (worst, shares[worst])
