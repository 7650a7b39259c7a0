"""GPU tests of cnf_mv_particles, the interacting (McKean-Vlasov) particle reference, and of what stands on it
(applications.mv_reference_particles, solvers.evaluate_mv_reference), against the float64 restatement
(tests/mv_particles_f64.py) fed the device's own normals.

Shapes: R = 2 replicas; N = 300 (one partly filled row group of the pair pass, two chunks of 256) and N = 1100 (three row
groups, so the diagonal tiles lie in different workgroups; five chunks); h = 0.01, 12 steps, snapshots (0, 1, 5, 12).

What is held to what:
  kappa = 0           positions and the first 2 + D + D D sums equal cnf_fp_particles' bit for bit (replica r particle i
                      is its particle first + r N + i).
  one step            |x - restatement| <= h |kappa| 4 EPS32 tau + 1e-13 max(1, |x|): the pair force's float32 floor
                      (test_gpu_interaction.py's, EPS32 = 5e-6, tau = interaction_ref.tau) times h |kappa|, and the
                      float64 update's rounding.
  12 steps            e_fused <= 2 e_composed + floor, elementwise in the floor: e_composed is the error, against the
                      restatement, of the same steps with the pair force composed in NumPy float32 throughout (float64
                      state, mv_particles_f64.force_f32); floor = 64 times the restatement's divergence when every start
                      coordinate moves by one ulp, at least 1e-13 max(1, |x|) (test_gpu_fp_particles.py's).
  statistics          sums and histogram against NumPy on the kernel's own positions (1e-12 of sum |term|, counts
                      exact); energy against interaction_ref.energy of the float32-rounded positions within
                      2 EPS32 k_max.
  replicas, calls     one R = 2 call equals two R = 1 calls bit for bit; two calls are bit-identical; a NaN in replica 1
                      leaves replica 0 bit-identical and makes every particle of replica 1 bad from the next snapshot on.
  closed form         ou + quadratic, D = 2, R = 2, N = 4096, 50 steps: the pooled per-coordinate variance of the
                      deviations from the replica means within 5 standard errors v sqrt(2 / (R N D)) of the EXACT discrete
                      expectation v_{k+1} = c^2 v_k + 2 sigma h (1 - 1 / N) = 0.2324 (NumPy with another generator:
                      0.2286, z = -1.5; without the force 0.868).  The continuum value 0.2330 (trace_cov_exact / D)
                      differs from it by the step's bias, 6e-4: a quarter of one standard error here.

Measured on one MI355X (every test prints its figures: run with -s); 12-step paths: the worst ratio over the snapshots
of e_fused / (2 e_composed + floor), then e_fused / e_composed / floor at step 12, then the largest one-step error:
  ou       D = 1  Gaussian x 2  N = 300    0.709   1.7e-9  / 1.2e-9 / 3.1e-13   one step 4.5e-10 (bound 2.9e-7)
  ou       D = 2  Morse         N = 1100   0.121   4.9e-10 / 2.1e-9 / 3.3e-13   one step 7.7e-11 (bound 6.8e-7)
  gradient D = 2  Gaussian x 2  N = 300    0.137   9.0e-10 / 3.3e-9 / 2.5e-13   one step 2.5e-10 (bound 2.9e-7)
  lorenz   D = 3  quadratic     N = 300    0.120   2.6e-8  / 1.1e-7 / 9.8e-13   one step 3.3e-9  (bound 1.4e-6)
  ou       D = 3  Morse         N = 300    0.152   3.6e-10 / 1.2e-9 / 2.8e-13   one step 6.9e-11 (bound 6.8e-7)
  ou       D = 5  quadratic     N = 1100   0.042   6.7e-9  / 1.6e-7 / 3.4e-13   one step 2.9e-9  (bound 1.9e-6)
  ou       D = 5  Gaussian x 2  N = 300    0.155   5.7e-10 / 1.8e-9 / 3.4e-13   one step 1.2e-10 (bound 2.9e-7)
F within 5.5e-9 (bounds 1.5e-5 .. 5.9e-4); sums within 3.1e-15 of sum |term|; closed form: 0.23344 against 0.23237,
z = +0.41.  More: profiles/mv_particles/README.md.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp_particles_f64 as fp
import interaction_ref as ir
import mv_particles_f64 as mv

pytestmark = pytest.mark.gpu

SPECS = {"gaussian/2": ir.spec("gaussian", [1.0, -0.5], [0.75, 2.0]),
         "morse": ir.spec("exponential", [1.0, -0.5], [0.5, 2.0]),
         "quadratic": ir.spec("quadratic", [0.75])}
CASES = [("ou", 1, "gaussian/2", 300), ("ou", 2, "morse", 1100), ("gradient", 2, "gaussian/2", 300),
         ("lorenz", 3, "quadratic", 300), ("ou", 3, "morse", 300), ("ou", 5, "quadratic", 1100),
         ("ou", 5, "gaussian/2", 300)]
R, H, STEPS, SNAPS = 2, 0.01, 12, (0, 1, 5, 12)
A, SIGMA, VAR0, KAPPA, SEED, FIRST = 1.0, 0.5, 1.0, 1.5, 13, 1000
GRID = dict(lo=(-1.5, -1.0), step=(0.5, 0.5), n=(7, 5), axes=(0, 1))      # leaves particles outside on every side


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _c_grid(g):
  from cnf_ot_amd import _capi
  return _capi.CnfFieldGrid(g["lo"][0], g["lo"][1], g["step"][0], g["step"][1], g["n"][0], g["n"][1], g["axes"][0],
                            g["axes"][1], -1, 1, None, None)


def run_mv(dev, subtype, D, name, N, kappa=KAPPA, reps=R, first=FIRST, x0=None, snaps=SNAPS, steps=STEPS):
  """One cnf_mv_particles call with every output (the histogram where the event has two axes): numpy pos [S, R, N, D],
  sums [S, R, K], hist [S, ny, nx] or None, state [R, N, D]"""
  from cnf_ot_amd import _capi, utils
  lib, C = _capi.lib(), _capi.ctypes
  spec = utils.interaction_spec(**ir.kwargs(SPECS[name]))
  S, K = len(snaps), 3 + D + D * D
  nb = C.c_int64(0)
  _capi.check(lib.cnf_mv_particles_workspace(reps, N, D, S, C.byref(nb)), "workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  pos, sums = torch.full((S, reps, N, D), 7.25, **f64), torch.full((S, reps, K), 7.25, **f64)
  state = torch.full((reps, N, D), 7.25, **f64)
  ws = torch.full((nb.value // 8,), float("nan"), **f64)
  g = _c_grid(GRID) if D >= 2 else None
  hist = None if g is None else torch.full((S, GRID["n"][1], GRID["n"][0]), 77, dtype=torch.int32, device=dev)
  x0d = None if x0 is None else torch.as_tensor(x0, **f64).contiguous()
  snap = (C.c_int64 * S)(*snaps)
  rc = lib.cnf_mv_particles(C.byref(spec), kappa, fp.DRIFTS[subtype], D, A, SIGMA, H, steps, VAR0, SEED, first, reps, N,
                            None if x0d is None else x0d.data_ptr(), snap, S, None if g is None else C.byref(g),
                            state.data_ptr(), pos.data_ptr(), sums.data_ptr(), None if hist is None else hist.data_ptr(),
                            ws.data_ptr(), nb.value, None)
  assert rc == _capi.CNF_OK, rc
  torch.cuda.synchronize()
  return (pos.cpu().numpy(), sums.cpu().numpy(), None if hist is None else hist.cpu().numpy().astype(np.int64),
          state.cpu().numpy())


def run_fp(dev, subtype, D, N, first, snaps=SNAPS, steps=STEPS):
  """cnf_fp_particles on the same stream: numpy pos [S, N, D], sums [S, 2 + D + D D]"""
  from cnf_ot_amd import _capi
  lib, C = _capi.lib(), _capi.ctypes
  S = len(snaps)
  nb = C.c_int64(0)
  _capi.check(lib.cnf_fp_particles_workspace(N, D, S, C.byref(nb)), "workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  pos, sums = torch.empty(S, N, D, **f64), torch.empty(S, 2 + D + D * D, **f64)
  ws = torch.empty(nb.value // 8, **f64)
  snap = (C.c_int64 * S)(*snaps)
  rc = lib.cnf_fp_particles(fp.DRIFTS[subtype], D, A, SIGMA, H, steps, VAR0, SEED, first, N, None, snap, S, None,
                            pos.data_ptr(), sums.data_ptr(), None, ws.data_ptr(), nb.value, None)
  assert rc == _capi.CNF_OK, rc
  torch.cuda.synchronize()
  return pos.cpu().numpy(), sums.cpu().numpy()


def device_normals(dev, D, N, reps=R, first=FIRST, steps=STEPS):
  """The replicas' own normals from cnf_fill_normal, widened: z [reps, N, steps + 1, D]"""
  from cnf_ot_amd import _capi
  stride = fp.stream_stride(steps, D)
  out = torch.empty(reps * N * stride, dtype=torch.float32, device=dev)
  _capi.check(_capi.lib().cnf_fill_normal(SEED, first * stride, reps * N * stride, out.data_ptr(), None), "cnf_fill_normal")
  torch.cuda.synchronize()
  return mv.replica_normals(out.cpu().numpy().astype(np.float64), reps, N, steps, D)


class _Runs(dict):
  """Per case, computed on first use and left unchanged: the kernel's outputs, the restatement's positions and W sums,
  the float32 composition's positions and the restatement's one-ulp divergence per snapshot"""

  def __init__(self, dev):
    super().__init__()
    self.dev = dev

  def __missing__(self, case):
    subtype, D, name, N = case
    sp = SPECS[name]
    z = device_normals(self.dev, D, N)
    want, wsum = mv.integrate(z, subtype, A, SIGMA, H, VAR0, KAPPA, sp, SNAPS)
    comp, _ = mv.integrate(z, subtype, A, SIGMA, H, VAR0, KAPPA, sp, SNAPS, force=mv.force_f32)
    moved, _ = mv.integrate(z, subtype, A, SIGMA, H, VAR0, KAPPA, sp, SNAPS, x0=np.nextafter(want[0], np.inf))
    div = np.abs(moved - want).reshape(len(SNAPS), -1).max(1)
    self[case] = dict(got=run_mv(self.dev, subtype, D, name, N), want=want, wsum=wsum, comp=comp, div=div)
    return self[case]


@pytest.fixture(scope="module")
def runs(dev):
  return _Runs(dev)


@pytest.mark.parametrize("subtype,D,name,N", CASES)
def test_without_the_force_it_is_cnf_fp_particles_bit_for_bit(dev, subtype, D, name, N):
  pos, sums, _, state = run_mv(dev, subtype, D, name, N, kappa=0.0)
  K0 = 2 + D + D * D
  for r in range(R):
    fpos, fsums = run_fp(dev, subtype, D, N, FIRST + r * N)
    assert np.array_equal(pos[:, r], fpos) and np.array_equal(sums[:, r, :K0], fsums)
  assert np.array_equal(state, pos[-1]) and np.isfinite(sums).all()


@pytest.mark.parametrize("subtype,D,name,N", CASES)
def test_one_step_is_sharp(runs, subtype, D, name, N):
  r_ = runs[(subtype, D, name, N)]
  pos, want = r_["got"][0], r_["want"]
  assert SNAPS[1] == 1 and np.array_equal(pos[0], want[0])                # the start is one exact product
  for r in range(R):
    tau = ir.tau(mv.rounded(want[0, r]), SPECS[name])
    tol = H * abs(KAPPA) * 4.0 * mv.EPS32 * tau + 1e-13 * np.maximum(1.0, np.abs(want[1, r]))
    err = np.abs(pos[1, r] - want[1, r])
    print(f"[{subtype} D={D} {name} N={N} replica {r}] tau {tau:.3g}  one-step error {err.max():.3e}  (bound {tol.min():.3e})")
    assert (err <= tol).all(), (subtype, D, name, N, r, float(err.max()))
    # and the force does move the particles: its share of the step is far above the bound
    assert H * abs(KAPPA) * np.abs(mv.force_f64(want[0, r], SPECS[name])[0]).max() > 100.0 * tol.max()


@pytest.mark.parametrize("subtype,D,name,N", CASES)
def test_paths_against_the_restatement(runs, subtype, D, name, N):
  r_ = runs[(subtype, D, name, N)]
  pos, want, comp = r_["got"][0], r_["want"], r_["comp"]
  assert pos.shape == want.shape == (len(SNAPS), R, N, D) and np.isfinite(pos).all()
  worst = 0.0
  for s, k in enumerate(SNAPS):
    e_fused, e_comp = np.abs(pos[s] - want[s]), float(np.abs(comp[s] - want[s]).max())
    floor = np.maximum(64.0 * r_["div"][s], 1e-13 * np.maximum(1.0, np.abs(want[s])))
    bound = 2.0 * e_comp + floor
    worst = max(worst, float((e_fused / bound).max()))
    print(f"[{subtype} D={D} {name} N={N} step {k}] max |x| {np.abs(want[s]).max():.3g}  e_fused {e_fused.max():.3e}  "
          f"e_composed {e_comp:.3e}  floor {floor.max():.3e} (one-ulp divergence {r_['div'][s]:.3e})  "
          f"e_fused / bound {float((e_fused / bound).max()):.3f}")
    assert (e_fused <= bound).all(), (subtype, D, name, N, k, float(e_fused.max()), e_comp, float(floor.max()))
  print(f"[{subtype} D={D} {name} N={N}] worst e_fused / (2 e_composed + floor): {worst:.3f}")
  assert np.array_equal(r_["got"][3], pos[-1])                            # the state left behind is the last snapshot's


@pytest.mark.parametrize("subtype,D,name,N", CASES)
def test_statistics_of_the_kernels_own_positions(runs, subtype, D, name, N):
  pos, sums, hist, _ = runs[(subtype, D, name, N)]["got"]
  sp, K0 = SPECS[name], 2 + D + D * D
  grid = GRID if D >= 2 else None
  pooled = None
  for r in range(R):
    want_sums, want_hist = fp.stats(pos[:, r], grid)
    scale = np.maximum(fp.abs_sums(pos[:, r]), 1e-300)
    assert np.array_equal(sums[:, r, :2], want_sums[:, :2]) and (sums[:, r, 0] == N).all()
    rel = float((np.abs(sums[:, r, :K0] - want_sums) / scale).max())
    assert rel <= 1e-12, rel
    if grid is not None:
      pooled = want_hist if pooled is None else pooled + want_hist
    for s, k in enumerate(SNAPS):
      x32 = mv.rounded(pos[s, r])
      F, want_F, k_max = sums[s, r, K0] / (2.0 * N * (N - 1.0)), ir.energy(x32, sp), ir.k_max(x32, sp)
      print(f"[{subtype} D={D} {name} N={N} replica {r} step {k}] sums {rel:.2e} of sum |term|  F {F:.6e}  "
            f"error {abs(F - want_F):.2e}  (bound {2.0 * mv.EPS32 * k_max:.2e})")
      assert abs(F - want_F) <= 2.0 * mv.EPS32 * k_max
  if grid is not None:
    assert np.array_equal(hist, pooled)
    inside = pooled.sum((1, 2))
    assert (inside > 0).all() and (inside < R * N).all()                  # some particles lie outside the grid


@pytest.mark.parametrize("subtype,D,name,N", [CASES[1], CASES[3]])
def test_replicas_are_independent_and_calls_reproducible(dev, runs, subtype, D, name, N):
  got = runs[(subtype, D, name, N)]["got"]
  again = run_mv(dev, subtype, D, name, N)
  for x, y in zip(again, got):
    assert np.array_equal(x, y)
  singles = [run_mv(dev, subtype, D, name, N, reps=1, first=FIRST + r * N) for r in range(R)]
  for r in range(R):
    assert np.array_equal(singles[r][0][:, 0], got[0][:, r]) and np.array_equal(singles[r][1][:, 0], got[1][:, r])
    assert np.array_equal(singles[r][3][0], got[3][r])
  assert np.array_equal(singles[0][2] + singles[1][2], got[2])
  # the drawn start given back: the same paths; then one NaN in replica 1
  x0 = got[0][0].copy()
  base = run_mv(dev, subtype, D, name, N, x0=x0)
  for x, y in zip(base, got):
    assert np.array_equal(x, y)
  x0[1, 137, D - 1] = np.nan
  pos, sums, hist, _ = run_mv(dev, subtype, D, name, N, x0=x0)
  assert np.array_equal(pos[:, 0], got[0][:, 0]) and np.array_equal(sums[:, 0], got[1][:, 0])
  assert sums[0, 1, 0] == N - 1 and sums[0, 1, 1] == 1
  assert (sums[1:, 1, 0] == 0).all() and (sums[1:, 1, 1] == N).all() and not np.isfinite(pos[1:, 1]).all(-1).any()
  assert np.array_equal(hist[1:], fp.stats(got[0][1:, 0], GRID)[1])       # replica 0 alone is left in the histogram


def test_closed_form_on_the_device(dev):
  from cnf_ot_amd import applications as app
  D, N, a, strength, amp, sigma, var0, h, steps = 2, 4096, 1.0, 4.0, 0.5, 0.5, 1.5, 0.01, 50
  T = steps * h
  kw = dict(n_particles=N, replicas=R, h=h, seed=3, var0=var0)
  res = app.mv_reference_particles(D, T, a, sigma, "ou", {"kind": "quadratic", "amplitudes": [amp]}, strength, [0.0, T], **kw)
  assert set(res) == {"count", "bad", "mean", "cov", "sums", "hist", "density", "times", "energy", "replica_mean",
                      "replica_cov"}
  assert res["sums"].shape == (2, R, 3 + D + D * D) and res["energy"].shape == (2, R) and not bool(res["bad"].any())
  assert (res["count"] == R * N).all() and res["replica_cov"].shape == (2, R, D, D) and res["replica_mean"].shape == (2, R, D)
  # replica_cov is sum x x^T / N - mean mean^T: the variance of the deviations from the replica's own mean
  got = float(res["replica_cov"][1].diagonal(dim1=-2, dim2=-1).mean())
  want = mv.em_deviation_variance(var0, a, strength * amp, sigma, h, N, steps)
  free = fp.em_ou_variance(var0, a, sigma, h, steps)
  se = want * math.sqrt(2.0 / (R * N * D))
  cont = app.mv_quadratic_ou_variance(T, a, sigma, strength, amp, var0)
  print(f"[closed form] deviation variance {got:.5f}  exact discrete expectation {want:.5f}  z = {(got - want) / se:+.2f}  "
        f"(continuum {cont:.5f}: the step's bias is {(cont - want) / se:+.2f} standard errors; without the force {free:.4f})")
  assert abs(want - 0.2324) < 5e-5 and abs(cont - 0.2330) < 5e-5 and abs(free - 0.868) < 5e-4
  assert abs(got - want) <= 5.0 * se
  # strength 0: fp_reference_particles' paths bit for bit
  none = app.mv_reference_particles(D, T, a, sigma, "ou", {"kind": "quadratic", "amplitudes": [amp]}, 0.0, [0.0, T],
                                    positions=True, **kw)
  ref = app.fp_reference_particles(D, T, a, sigma, "ou", [0.0, T], n_particles=R * N, h=h, seed=3, var0=var0, positions=True)
  assert none["pos"].reshape(2, R * N, D).equal(ref["pos"])


def test_evaluate_mv_reference_equals_its_composition(dev):
  from cnf_ot_amd import applications as app, solvers
  ia = {"kind": "gaussian", "strength": 2.0, "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]}
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "gradient"},
                                          "interaction": ia})
  f = config["fp"]
  n, h, seed, ts = 512, 0.01, 5, [0.0, 0.05, 0.1]
  res = solvers.evaluate_mv_reference(config, times=ts, n_particles=n, replicas=3, h=h, seed=seed)
  assert set(res) == set(solvers.MV_REFERENCE_KEYS) and res["trace_cov_exact"] is None
  assert (res["kind"], res["strength"], res["n"], res["replicas"], res["times"]) == ("gaussian", 2.0, n, 3, ts)
  kw = {"kind": "gaussian", "amplitudes": [1.0, -0.5], "bandwidths": [0.5, 2.0]}
  m = app.mv_reference_particles(2, f["T"], f["a"], f["sigma"], "gradient", kw, 2.0, ts, n, 3, h, seed)
  free = app.fp_reference_particles(2, f["T"], f["a"], f["sigma"], "gradient", ts, 3 * n, h, seed)
  tr = lambda c: c.diagonal(dim1=-2, dim2=-1).sum(-1)
  rep = tr(m["replica_cov"])
  want = {"mean": m["mean"].tolist(), "trace_cov": tr(m["cov"]).tolist(), "free_mean": free["mean"].tolist(),
          "free_trace_cov": tr(free["cov"]).tolist(), "trace_cov_floor": (rep.max(1).values - rep.min(1).values).tolist(),
          "energy": m["energy"].mean(1).tolist(),
          "energy_floor": (m["energy"].max(1).values - m["energy"].min(1).values).tolist(), "bad": m["bad"].tolist()}
  for k, v in want.items():
    assert res[k] == v, k
  assert res["free_trace_cov"][0] == pytest.approx(res["trace_cov"][0], rel=1e-12)      # the same start
  assert res["trace_cov"][2] != res["free_trace_cov"][2] and all(v > 0.0 for v in res["trace_cov_floor"])
  solvers.print_mv_reference(res)
  # ou with the quadratic kernel: the mean-field limit beside it
  quad = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"},
                                        "interaction": {"kind": "quadratic", "strength": 2.0, "amplitudes": [1.0]}})
  q = solvers.evaluate_mv_reference(quad, times=ts, n_particles=n, h=h, seed=seed)
  fq = quad["fp"]
  var0 = app.fp_initial_variance(fq["T"])
  assert q["trace_cov_exact"] == [2 * app.mv_quadratic_ou_variance(t, fq["a"], fq["sigma"], 2.0, 1.0, var0) for t in ts]
  assert q["trace_cov_exact"][0] == 2 * var0 and q["trace_cov_exact"][2] < q["free_trace_cov"][2]


def test_evaluate_mv_reference_is_for_fp_with_an_interaction_only(dev):
  from cnf_ot_amd import solvers
  ia = {"kind": "quadratic", "strength": 2.0, "amplitudes": [1.0], "bandwidths": [1.0]}
  with pytest.raises(ValueError):
    solvers.evaluate_mv_reference(solvers.load_config(overrides={"interaction": ia}))                    # rwpo
  with pytest.raises(ValueError):
    solvers.evaluate_mv_reference(solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}}))  # kind "none"
