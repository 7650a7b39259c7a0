"""The particle reference of the rwpo problems without a GPU: the float64 restatement (tests/rwpo_particles_f64.py)
against the closed forms of the quadratic potential, the selection rule, the stream layout, applications.rwpo_proposal,
and every refusal of cnf_rwpo_particles from the built library with no device call."""
import ctypes
import math

import numpy as np

import rwpo_particles_f64 as rw
from cnf_ot_amd import _capi


def _normals(N, D, K, S, seed):
  return np.random.default_rng(seed).standard_normal(N * rw.stream_stride(D, K, S))


def test_matched_quadratic_proposal_is_exact():
  """With the posterior of X_T given y as the proposal every weight is equal: log h is its closed form and ess = K"""
  D, T, beta, K, N = 5, 1.0, 2.0, 64, 512
  p = rw.proposal(D, T, beta, 0.0, "quadratic")
  ref = rw.reference(_normals(N, D, K, 1, 1), None, N, D, K, [T], "quadratic", 0.0, T, beta, 2.0 * (T + 1.0) / beta, **p)
  err = np.abs(ref["log_h"] - rw.quadratic_log_h(ref["y"], T, beta)).max()
  ess_err = np.abs(ref["ess"] - K).max()
  print(f"[matched quadratic] log_h error {err:.2e} (bound 1e-13), ess error {ess_err:.2e} (bound {1e-9 * K:.1e})")
  assert err <= 1e-13
  assert ess_err <= 1e-9 * K


def test_plain_proposal_meets_the_closed_form_value():
  D, T, beta, N, K = 2, 1.0, 1.0, 4096, 1024
  p = rw.proposal(D, T, beta, 0.0, "obstacle")            # the plain Brownian proposal
  ref = rw.reference(_normals(N, D, K, 1, 2), None, N, D, K, [T], "quadratic", 0.0, T, beta, 2.0 * (T + 1.0) / beta, **p)
  val, se, bias, corrected = rw.value(ref["log_h"], ref["ess"], beta, K)
  want = D * (1.0 + math.log(T + 1.0)) / beta
  # -2 eps E log h from log h's closed form, E |y|^2 = D var0: the same number
  exact = -(2.0 / beta) * (-0.5 * D * math.log(1.0 + T) - beta * D * (2.0 * (T + 1.0) / beta) / (4.0 * (1.0 + T)))
  print(f"[plain quadratic] corrected {corrected:.6f}, -2 eps E log h exact {exact:.6f}, closed form {want:.6f}: "
        f"{(corrected - exact) / se:+.2f} standard errors (se {se:.2e}, bias {bias:.2e})")
  assert abs(exact - want) <= 1e-12 * want
  assert abs(corrected - want) <= 5.0 * se


def test_bridge_variance_law():
  """Quadratic: the per-coordinate variance of the optimal path at t is 2 (T + 1 - t) / beta"""
  D, T, beta, K, N = 2, 1.0, 2.0, 8, 65536
  times = [0.0, 0.3 * T, 0.7 * T, T]
  p = rw.proposal(D, T, beta, 0.0, "quadratic")
  u = np.random.default_rng(3).random(N)
  ref = rw.reference(_normals(N, D, K, 4, 4), u, N, D, K, times, "quadratic", 0.0, T, beta, 2.0 * (T + 1.0) / beta, **p)
  assert np.array_equal(ref["pos"][0], ref["y"]) and np.array_equal(ref["pos"][3], ref["z_sel"])
  for s, t in enumerate(times):
    var = 2.0 * (T + 1.0 - t) / beta
    got = ref["pos"][s].var(0, ddof=1)
    bound = 5.0 * var * math.sqrt(2.0 / N)
    print(f"[bridge law t={t:.1f}] variance {got} against {var:.4f}: {np.abs(got - var).max() / (bound / 5):.2f} standard errors")
    assert (np.abs(got - var) <= bound).all()


def test_selection_rule():
  l = np.log(np.array([[1.0, 2.0, 3.0, 4.0], [4.0, 3.0, 2.0, 1.0], [1.0, 1.0, 1.0, 1.0]]))
  for u, want in ((0.0, [0, 0, 0]), (0.05, [0, 0, 0]), (0.1, [1, 0, 0]), (0.29, [1, 0, 1]), (0.31, [2, 0, 1]),
                  (0.5, [2, 1, 2]), (0.65, [3, 1, 2]), (0.95, [3, 3, 3]), (0.999999, [3, 3, 3])):
    sel, gap = rw.select(l, np.full(3, u))
    assert sel.tolist() == want, (u, sel.tolist(), want)
  sel, gap = rw.select(l[:1], np.array([0.1 + 1e-13]))
  assert gap[0] <= 2e-13
  # a constant shift of l changes nothing; a cumulative sum that rounding leaves under u times the total: the last draw
  assert rw.select(l + 700.0, np.full(3, 0.5))[0].tolist() == [2, 1, 2]
  assert rw.select(np.zeros((1, 3)), np.array([1.0]))[0].tolist() == [2]


def test_proposals():
  from cnf_ot_amd import applications as app
  T, beta, a = 2.0, 10.0, 1.5
  q = app.rwpo_proposal(3, T, beta, a, "quadratic")
  assert q["shrink"] == 1.0 / (1.0 + T) and q["prop_var"] == 2.0 * T / (beta * (1.0 + T)) and q["centre"] is None
  o = app.rwpo_proposal(3, T, beta, a, "obstacle")
  assert o["shrink"] == 1.0 and o["prop_var"] == 2.0 * T / beta and o["centre"] is None
  for dim in (2, 6):
    d = app.rwpo_proposal(dim, T, beta, a, "double_well")
    P = beta * a * a * dim + beta / (2.0 * T)
    assert abs(d["shrink"] - (beta / (2.0 * T)) / P) <= 1e-15 and abs(d["prop_var"] - 1.0 / P) <= 1e-15
    assert d["centre"].shape == (dim,) and np.abs(d["centre"] - a * beta * a * a * dim / P).max() <= 1e-15
    # shrink y + centre is the mean of the product of the Brownian kernel around y and the well's Gaussian around a 1
    assert abs(d["shrink"] + beta * a * a * dim / P - 1.0) <= 1e-15
    r = rw.proposal(dim, T, beta, a, "double_well")
    assert r["shrink"] == d["shrink"] and r["prop_var"] == d["prop_var"] and np.array_equal(r["centre"], d["centre"])
  try:
    app.rwpo_proposal(2, T, beta, a, "cubic")
  except ValueError:
    pass
  else:
    raise AssertionError("an unknown potential was accepted")
  u = app.rwpo_selection_uniforms(1000, 5)
  assert u.dtype == np.float64 and u.shape == (1000,) and (u >= 0.0).all() and (u < 1.0).all()
  assert np.array_equal(u, app.rwpo_selection_uniforms(1000, 5)) and not np.array_equal(u, app.rwpo_selection_uniforms(1000, 6))
  assert np.array_equal(u[:400], app.rwpo_selection_uniforms(400, 5))


def test_stream_stride():
  from cnf_ot_amd import applications as app
  K, S = 10, 3
  # D: y blocks, blocks per draw, bridge blocks
  for D, (by, bd, bs) in {1: (1, 1, 1), 3: (1, 1, 3), 4: (1, 2, 3), 7: (2, 2, 6)}.items():
    assert rw.stream_stride(D, K, S) == 4 * (by + K * bd + bs) == app.rwpo_stream_stride(D, K, S)
  zy, xi, sign, zeta = rw.particle_normals(np.arange(2 * rw.stream_stride(3, 2, 2), dtype=np.float64), 2, 3, 2, 2)
  R = rw.stream_stride(3, 2, 2)
  assert R == 4 * (1 + 2 + 2)
  assert zy[1].tolist() == [R, R + 1, R + 2] and xi[0, 1].tolist() == [8, 9, 10] and sign[0].tolist() == [7, 11]
  assert zeta[0].tolist() == [[12, 13, 14], [15, 16, 17]]


def test_refusals_before_any_device_call():
  """Every refusal of cnf_rwpo_particles comes back CNF_ERR_INVALID on a machine without a device; the buffers are host
  memory that no refused call may read or write"""
  lib, INV = _capi.lib(), _capi.CNF_ERR_INVALID
  f64, i32 = np.full(4096, 7.25, np.float64), np.full(64, 7, np.int32)
  d, si = f64.ctypes.data, i32.ctypes.data
  dptr = ctypes.POINTER(ctypes.c_double)
  good_grid = _capi.CnfFieldGrid(-3.0, -3.0, 0.1, 0.1, 8, 8, 0, 1, -1, 1, None, None)

  def call(subtype=1, D=2, a=1.0, T=1.0, beta=4.0, var0=1.0, shrink=1.0, prop_var=0.5, centre=None, K=8, first=0, N=16,
           u=d, times=(0.0, 0.5, 1.0), S=None, grid=None, log_h=d, ess=d, mean_T=d, sel=si, pos=d, sums=d, hist=None, ws=d,
           ws_bytes=4096 * 8):
    ts = None if times is None else np.asarray(times, dtype=np.float64)
    c = None if centre is None else np.asarray(centre, dtype=np.float64)
    return lib.cnf_rwpo_particles(subtype, D, a, T, beta, var0, shrink, prop_var, None if c is None else c.ctypes.data_as(dptr),
                                  K, 1, first, N, u, None if ts is None else ts.ctypes.data_as(dptr),
                                  (0 if ts is None else len(ts)) if S is None else S,
                                  None if grid is None else ctypes.byref(grid), log_h, ess, mean_T, sel, pos, sums, hist, ws,
                                  ws_bytes, None)

  def grid(**kw):
    g = _capi.CnfFieldGrid(-3.0, -3.0, 0.1, 0.1, 8, 8, 0, 1, -1, 1, None, None)
    for k, v in kw.items():
      setattr(g, k, v)
    return g

  nan, inf = float("nan"), float("inf")
  none = dict(log_h=None, ess=None, mean_T=None, sel=None, pos=None, sums=None, hist=None)
  bad = {"subtype=-1": call(subtype=-1), "subtype=3": call(subtype=3), "D=0": call(D=0), "D=15": call(D=15)}
  for name in ("T", "beta", "var0", "prop_var"):
    for v in (0.0, -1.0, nan, inf):
      bad[f"{name}={v}"] = call(**{name: v})
  for name in ("shrink", "a"):
    for v in (nan, inf):
      bad[f"{name}={v}"] = call(**{name: v})
  bad.update({"centre nan": call(centre=[0.5, nan]), "centre inf": call(centre=[inf, 0.5]),
              "K=0": call(K=0), "K>2^20": call(K=(1 << 20) + 1), "N=0": call(N=0), "N>2^31": call(N=(1 << 31) + 1),
              "first<0": call(first=-1), "element index": call(first=(1 << 62)), "element index 2": call(first=(1 << 63) - 8),
              "S=0 with pos": call(times=None, S=0), "S=65": call(times=np.linspace(0.0, 1.0, 65)),
              "S=0 with hist": call(times=None, S=0, pos=None, sums=None, hist=d, grid=good_grid),
              "S=0 with sums": call(times=None, S=0, pos=None),
              "S<0": call(times=None, S=-1, pos=None, sums=None),
              "times NULL": call(times=None, S=3), "times descend": call(times=(0.0, 0.6, 0.5)),
              "times repeat": call(times=(0.0, 0.5, 0.5)), "times nan": call(times=(0.0, nan, 1.0)),
              "times<0": call(times=(-0.1, 0.5)), "times>T": call(times=(0.0, 1.0 + 1e-12)),
              "pos without u": call(u=None, sums=None, sel=None), "sums without u": call(u=None, pos=None, sel=None),
              "hist without u": call(u=None, pos=None, sums=None, sel=None, hist=d, grid=good_grid),
              "sel without u": call(u=None, pos=None, sums=None),
              "hist without grid": call(hist=d), "hist nx=0": call(hist=d, grid=grid(nx=0)),
              "hist step=0": call(hist=d, grid=grid(step_x=0.0)), "hist cells": call(hist=d, grid=grid(nx=1 << 13, ny=1 << 12)),
              "hist axes equal": call(hist=d, grid=grid(axis_y=0)), "hist axis outside": call(hist=d, grid=grid(axis_y=2)),
              "hist lo nan": call(hist=d, grid=grid(lo_x=nan)),
              "workspace NULL": call(ws=None), "workspace small": call(ws_bytes=16 * 2 * 8 + 3 * 8 * 8 - 1),
              "workspace NULL, pos alone": call(ws=None, sums=None),
              "no output": call(**none)})
  assert len(bad) == 4 + 16 + 4 + 35
  wrong = {k: v for k, v in bad.items() if v != INV}
  assert not wrong, wrong
  assert (f64 == 7.25).all() and (i32 == 7).all()
  # the workspace: the chunks' partials and z*
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_rwpo_particles_workspace(1000, 3, 4, ctypes.byref(nbytes)) == _capi.CNF_OK
  assert nbytes.value == 8 * (4 * (2 + 3 + 9) * 4 + 1000 * 3)
  assert lib.cnf_rwpo_particles_workspace(16, 2, 3, ctypes.byref(nbytes)) == _capi.CNF_OK
  assert nbytes.value == 16 * 2 * 8 + 3 * 8 * 8
  for args in ((0, 3, 4), (1000, 0, 4), (1000, 15, 4), (1000, 3, -1), (1000, 3, 65), ((1 << 31) + 1, 3, 4)):
    assert lib.cnf_rwpo_particles_workspace(*args, ctypes.byref(nbytes)) == INV, args
  assert lib.cnf_rwpo_particles_workspace(1000, 3, 4, None) == INV
