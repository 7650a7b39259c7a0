"""cnf_mv_particles with the power kind on the GPU (it reaches the kind through cnf_interaction's pair pass), against the
float64 restatement (tests/mv_particles_f64.py's integrator with interaction_power_ref's forces) fed the device's own
normals, under test_gpu_mv_particles.py's bounds:
  one step   |x - restatement| <= h |kappa| 4 EPS32 tau + 1e-13 max(1, |x|), tau = sum_b max |W_b'| over the start's pairs
  12 steps   e_fused <= 2 e_composed + floor, elementwise in the floor: e_composed the same steps with the pair force
             composed in NumPy float32 throughout, floor = 64 times the restatement's divergence when every start
             coordinate moves by one ulp, at least 1e-13 max(1, |x|).
and the log kernel's virial identity (applications.mv_log_second_moment): with no drift,
  E mean |x|^2(t) - E mean |x|^2(0) = (2 D sigma - kappa amp) t
for every N, in dimension 2 and 3.  The softening (each pair's 1 becomes d^2 / (d^2 + eps^2)) and Euler's h^2 kappa^2 mean
|G|^2 per step are computed in float64 from the restatement's own path (interaction_power_ref.
log_second_moment_increments: the conditional expectation of every step's increment), and the ensemble is held to the
sum within 5 standard errors, the standard error read from the restatement's per-particle increments minus their
conditional expectations -- the convention of test_gpu_mv_particles.py's closed form.  The same check on the restatement
alone, with NumPy's normals: test_interaction_power_cpu.py.

Every test prints its figures (run with -s).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp_particles_f64 as fp
import interaction_power_ref as pr
import mv_particles_f64 as mv

pytestmark = pytest.mark.gpu

SPECS = {"log": pr.spec([0.0], [1.0], 0.1), "coulomb3": pr.spec([-1.0], [-1.0], 0.1),
         "attractive-repulsive": pr.spec([4.0, 1.0], [1.0, -1.0], 0.05), "mixed/4": pr.spec([4.0, 1.0, 0.0, -1.0], [0.5, -1.0, 0.75, -0.25], 0.2)}
CASES = [("ou", 2, "log", 300), ("ou", 3, "coulomb3", 600), ("gradient", 2, "attractive-repulsive", 300), ("ou", 5, "mixed/4", 300)]
R, H, STEPS, SNAPS = 2, 0.01, 12, (0, 1, 5, 12)
A, SIGMA, VAR0, KAPPA, SEED, FIRST = 1.0, 0.5, 1.0, 1.5, 13, 1000


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def run_mv(dev, subtype, D, sp, N, kappa=KAPPA, reps=R, first=FIRST, snaps=SNAPS, steps=STEPS, a=A, sigma=SIGMA, h=H,
           var0=VAR0, seed=SEED, positions=True):
  """One cnf_mv_particles call: numpy pos [S, R, N, D] (or None), sums [S, R, K]"""
  from cnf_ot_amd import _capi, utils
  lib, C = _capi.lib(), _capi.ctypes
  spec = utils.interaction_spec(**pr.kwargs(sp))
  S, K = len(snaps), 3 + D + D * D
  nb = C.c_int64(0)
  _capi.check(lib.cnf_mv_particles_workspace(reps, N, D, S, C.byref(nb)), "workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  pos = torch.full((S, reps, N, D), 7.25, **f64) if positions else None
  sums, state = torch.full((S, reps, K), 7.25, **f64), torch.full((reps, N, D), 7.25, **f64)
  ws = torch.full((nb.value // 8,), float("nan"), **f64)
  snap = (C.c_int64 * S)(*snaps)
  rc = lib.cnf_mv_particles(C.byref(spec), kappa, fp.DRIFTS[subtype], D, a, sigma, h, steps, var0, seed, first, reps, N, None,
                            snap, S, None, state.data_ptr(), None if pos is None else pos.data_ptr(), sums.data_ptr(), None,
                            ws.data_ptr(), nb.value, None)
  assert rc == _capi.CNF_OK, rc
  torch.cuda.synchronize()
  return None if pos is None else pos.cpu().numpy(), sums.cpu().numpy()


def device_normals(dev, D, N, reps=R, first=FIRST, steps=STEPS, seed=SEED):
  """The replicas' own normals from cnf_fill_normal, widened: z [reps, N, steps + 1, D]"""
  from cnf_ot_amd import _capi
  stride = fp.stream_stride(steps, D)
  out = torch.empty(reps * N * stride, dtype=torch.float32, device=dev)
  _capi.check(_capi.lib().cnf_fill_normal(seed, first * stride, reps * N * stride, out.data_ptr(), None), "cnf_fill_normal")
  torch.cuda.synchronize()
  return mv.replica_normals(out.cpu().numpy().astype(np.float64), reps, N, steps, D)


@pytest.mark.parametrize("subtype,D,name,N", CASES)
def test_paths_against_the_restatement(dev, subtype, D, name, N):
  sp = SPECS[name]
  z = device_normals(dev, D, N)
  want, wsum = mv.integrate(z, subtype, A, SIGMA, H, VAR0, KAPPA, sp, SNAPS, force=pr.force_f64)
  comp, _ = mv.integrate(z, subtype, A, SIGMA, H, VAR0, KAPPA, sp, SNAPS, force=pr.force_f32)
  moved, _ = mv.integrate(z, subtype, A, SIGMA, H, VAR0, KAPPA, sp, SNAPS, x0=np.nextafter(want[0], np.inf), force=pr.force_f64)
  div = np.abs(moved - want).reshape(len(SNAPS), -1).max(1)
  pos, sums = run_mv(dev, subtype, D, sp, N)
  assert pos.shape == want.shape == (len(SNAPS), R, N, D) and np.isfinite(pos).all() and np.array_equal(pos[0], want[0])
  # one step
  for r in range(R):
    tau = pr.scales(mv.rounded(want[0, r]), sp)[1]
    tol = H * abs(KAPPA) * 4.0 * mv.EPS32 * tau + 1e-13 * np.maximum(1.0, np.abs(want[1, r]))
    err = np.abs(pos[1, r] - want[1, r])
    print(f"[{subtype} D={D} {name} N={N} replica {r}] tau {tau:.3g}  one-step error {err.max():.3e}  (bound {tol.min():.3e})")
    assert (err <= tol).all(), (subtype, D, name, N, r, float(err.max()))
    assert H * abs(KAPPA) * np.abs(pr.force_f64(want[0, r], sp)[0]).max() > 100.0 * tol.max()      # the force does move them
  # 12 steps
  worst = 0.0
  for s, k in enumerate(SNAPS):
    e_fused, e_comp = np.abs(pos[s] - want[s]), float(np.abs(comp[s] - want[s]).max())
    floor = np.maximum(64.0 * div[s], 1e-13 * np.maximum(1.0, np.abs(want[s])))
    bound = 2.0 * e_comp + floor
    worst = max(worst, float((e_fused / bound).max()))
    print(f"[{subtype} D={D} {name} N={N} step {k}] max |x| {np.abs(want[s]).max():.3g}  e_fused {e_fused.max():.3e}  "
          f"e_composed {e_comp:.3e}  floor {floor.max():.3e}  e_fused / bound {float((e_fused / bound).max()):.3f}")
    assert (e_fused <= bound).all(), (subtype, D, name, N, k, float(e_fused.max()), e_comp, float(floor.max()))
  print(f"[{subtype} D={D} {name} N={N}] worst e_fused / (2 e_composed + floor): {worst:.3f}")
  # the energy of the step's own pair pass
  K0 = 2 + D + D * D
  for s in range(len(SNAPS)):
    for r in range(R):
      x32 = mv.rounded(pos[s, r])
      F, want_F, k_max = sums[s, r, K0] / (2.0 * N * (N - 1.0)), pr.energy(x32, sp), pr.scales(x32, sp)[0]
      assert abs(F - want_F) <= 2.0 * mv.EPS32 * k_max, (s, r, F, want_F)
  # two calls give the same bits
  again = run_mv(dev, subtype, D, sp, N)
  assert np.array_equal(again[0], pos) and np.array_equal(again[1], sums)


@pytest.mark.parametrize("D,amp", [(2, -1.0), (3, 1.0)])
def test_the_virial_identity_of_the_log_kernel(dev, D, amp):
  """No drift (ou with a = 0), the log kernel at eps = 0.1: repulsive in dimension 2 (the log gas), attractive in
  dimension 3 (Keller-Segel's sign, strong enough that mean |x|^2 shrinks: 2 D sigma - kappa amp = -0.5)"""
  from cnf_ot_amd import applications as app
  reps, N, steps, h, sigma, kappa, eps, var0, seed, first = 8, 128, 200, 0.005, 0.25, 3.0 if amp < 0 else 2.0, 0.1, 1.0, 29, 500
  sp = pr.spec([0.0], [amp], eps)
  T = steps * h
  _, sums = run_mv(dev, "ou", D, sp, N, kappa=kappa, reps=reps, first=first, snaps=(0, steps), steps=steps, a=0.0, sigma=sigma, h=h,
                   var0=var0, seed=seed, positions=False)
  assert (sums[:, :, 0] == N).all() and (sums[:, :, 1] == 0).all()
  m2 = np.trace(sums[:, :, 2 + D:2 + D + D * D].reshape(2, reps, D, D), axis1=-2, axis2=-1) / N      # mean |x|^2 [2, reps]
  got = float((m2[1] - m2[0]).mean())
  z = device_normals(dev, D, N, reps=reps, first=first, steps=steps, seed=seed)
  rm2, expected, resid = pr.log_second_moment_increments(z, sigma, h, var0, kappa, sp, steps)
  closed = app.mv_log_second_moment(T, D, sigma, kappa, amp, 0.0)
  assert abs(closed - (2.0 * D * sigma - kappa * amp) * T) <= 1e-15 * abs(closed)
  corrections = float(expected.mean()) - closed
  se = float(resid.std(ddof=1)) / math.sqrt(reps * N)
  print(f"\n[log kernel D={D} amp={amp} R={reps} N={N} {steps} steps] mean |x|^2 grew by {got:.5f} (the restatement's path: "
        f"{float((rm2[-1] - rm2[0]).mean()):.5f}); closed form {closed:.5f} + softening and Euler terms {corrections:+.5f}; standard "
        f"error {se:.5f}: z = {(got - closed - corrections) / se:+.2f} (without the force: {2.0 * D * sigma * T:.3f})")
  assert abs(got - (closed + corrections)) <= 5.0 * se
  assert 5.0 * se < 0.5 * abs(kappa * amp * T)                # the check can see the force
  # the python entry gives the same ensemble
  res = app.mv_reference_particles(D, T, 0.0, sigma, "ou", pr.kwargs(sp), kappa, [0.0, T], n_particles=N, replicas=reps, h=h,
                                   seed=seed, var0=var0)
  tr = res["cov"].diagonal(dim1=-2, dim2=-1).sum(-1) + (res["mean"] ** 2).sum(-1)
  assert res["energy"].shape == (2, reps) and bool(torch.isfinite(tr).all())


def test_evaluate_mv_reference_prints_the_closed_form(dev, capsys):
  from cnf_ot_amd import applications as app, solvers
  ia = {"kind": "power", "strength": 3.0, "amplitudes": [-1.0], "bandwidths": 0.1, "exponents": [0.0]}
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou", "a": 0.0, "sigma": 0.25},
                                          "interaction": ia})
  res = solvers.evaluate_mv_reference(config, times=[0.0, 0.1, 0.2], n_particles=256, replicas=2, h=0.005, seed=5)
  assert set(res) == set(solvers.MV_REFERENCE_KEYS) and res["trace_cov_exact"] is None
  m0 = 2 * app.fp_initial_variance(config["fp"]["T"])
  assert res["second_moment_exact"] == [app.mv_log_second_moment(t, 2, 0.25, 3.0, -1.0, m0) for t in (0.0, 0.1, 0.2)]
  got, want = np.array(res["second_moment"]), np.array(res["second_moment_exact"])
  # 512 particles: the Monte-Carlo level of mean |x|^2 is m0 sqrt(2 / (512 D)) = 0.06 m0; the closed form's growth is 0.8
  assert (np.abs(got - want) <= 0.25 * m0).all() and got[2] > got[0]
  solvers.print_mv_reference(res)
  assert "closed form" in capsys.readouterr().out
  other = solvers.evaluate_mv_reference(solvers.load_config(overrides={
    "general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}, "interaction": ia}), times=[0.0, 0.1], n_particles=64,
    replicas=2, h=0.01)
  assert other["second_moment_exact"] is None and other["second_moment"] is None      # (a = 1: a drift)
