"""Checks of tests/flow_fields_f64.py itself -- the float64 restatement the GPU field kernels are held to -- and of the
table of figure settings in cnf_ot_amd.solvers.  No GPU."""
import numpy as np
import pytest

import flow_fields_f64 as ff
import oracle

T_ARRAY = np.linspace(0.0, 2.0, 5)


def _flows(D, scale, seed=3):
  ocfg = oracle.OracleConfig(D=D)
  n = oracle.param_count(ocfg)
  params = np.zeros(n) if scale == 0 else np.random.default_rng(seed).normal(0.0, scale, n).astype(np.float32)
  return ff.OracleFlow(ocfg, params), ff.NumpyOracleFlow(params, D=D)


@pytest.mark.parametrize("D", [2, 3])
def test_identity_flow_gives_the_base_density_and_no_motion(oracle_lib, D):
  for flow in _flows(D, 0):
    dom = [-3.0, 3.0, -2.0, 2.0]
    fixed = [0.0] * (D - 1) + [0.5] if D > 2 else None
    rho = ff.density_on_grid(flow, T_ARRAY, dom, n=(7, 5), fixed=fixed)
    pts = ff.grid_points(dom, (7, 5), D, fixed=fixed)
    want = np.exp(-0.5 * (pts ** 2).sum(1) - 0.5 * D * np.log(2 * np.pi)).reshape(5, 7)
    assert rho.shape == (5, 5, 7)
    assert np.abs(rho - want[None]).max() <= 1e-14
    assert np.abs(ff.velocity_field(flow, pts, T_ARRAY)).max() <= 1e-12
    assert np.abs(ff.score_field(flow, pts, T_ARRAY) + pts[None]).max() <= 1e-10      # central difference of a quadratic
    traj = ff.trajectories(flow, pts, T_ARRAY, t0=0.3)
    assert np.abs(traj - pts[None]).max() <= 1e-13
    assert np.abs(ff.trajectory_velocity(flow, pts, T_ARRAY)).max() <= 1e-12


@pytest.mark.parametrize("D", [2, 3])
def test_trajectory_returns_to_its_start_at_t0(oracle_lib, D):
  r0 = np.random.default_rng(5).uniform(-3, 3, (64, D))
  for flow in _flows(D, 0.2):
    traj = ff.trajectories(flow, r0, [0.0, 0.7, 1.3], t0=0.7)
    assert np.abs(traj[1] - r0).max() <= 1e-10
    assert np.abs(traj[0] - r0).max() > 1e-3          # (the flow does move)


def test_c_and_numpy_oracles_agree_on_every_field(oracle_lib):
  c_flow, np_flow = _flows(3, 0.2)
  dom = [-2.0, 2.0, -2.0, 2.0]
  sec = np.linspace(-5, 5, 11)
  pts = np.random.default_rng(2).uniform(-3, 3, (50, 3))
  for fn, args in ((ff.density_on_grid, (T_ARRAY, dom, 9, (0, 2), None, sec, 1)),
                   (ff.trajectories, (pts, T_ARRAY)), (ff.velocity_field, (pts, T_ARRAY)),
                   (ff.score_field, (pts, T_ARRAY)), (ff.trajectory_velocity, (pts, T_ARRAY))):
    a, b = fn(c_flow, *args), fn(np_flow, *args)
    assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max()), fn.__name__


def test_section_mean_is_the_mean_of_the_slices(oracle_lib):
  flow, _ = _flows(3, 0.2)
  dom = [-2.0, 2.0, -1.0, 1.0]
  sec = np.linspace(-5, 5, 11)
  for axes, sec_axis in (((1, 2), 0), ((0, 2), 1), ((0, 1), 2)):
    mean = ff.density_on_grid(flow, T_ARRAY[:2], dom, (6, 4), axes, None, sec, sec_axis)
    fixed = lambda v: [v if d == sec_axis else 0.0 for d in range(3)]
    slices = np.stack([ff.density_on_grid(flow, T_ARRAY[:2], dom, (6, 4), axes, fixed(v)) for v in sec])
    assert mean.shape == (2, 4, 6)
    assert np.abs(mean - slices.mean(0)).max() <= 1e-15


def test_grid_ordering_is_the_references_hstack_layout():
  """Index i * nx + j is (x_j, y_i) for nx != ny, whatever axes the grid spans."""
  dom = [-1.0, 2.0, 10.0, 14.0]
  nx, ny = 4, 3
  X, Y = np.meshgrid(np.linspace(-1.0, 2.0, nx), np.linspace(10.0, 14.0, ny))
  want = np.hstack([X.reshape(nx * ny, 1), Y.reshape(nx * ny, 1), np.ones((nx * ny, 1)) * 3])     # utils.py:665-669
  got = ff.grid_points(dom, (nx, ny), 3, fixed=[0.0, 0.0, 3.0])
  assert np.array_equal(got, want)
  for i in range(ny):
    for j in range(nx):
      assert got[i * nx + j, 0] == np.linspace(-1.0, 2.0, nx)[j] and got[i * nx + j, 1] == np.linspace(10.0, 14.0, ny)[i]
  # plot_proj_density, direction 'x' (utils.py:719-726): [section, X, Y]
  gx = ff.grid_points(dom, (nx, ny), 3, axes=(1, 2), section_value=-5.0, section_axis=0)
  assert np.array_equal(gx, np.hstack([np.ones((nx * ny, 1)) * -5.0, X.reshape(-1, 1), Y.reshape(-1, 1)]))
  # the product's own grid: the same points, and lo + index * step reproduces linspace to the last bit but one
  from cnf_ot_amd import utils
  g = utils.field_grid(dom, (nx, ny), fixed=[0.0, 0.0, 3.0])
  assert np.array_equal(utils.field_grid_points(g, 3), want)
  eg = utils._engine_grid(g, 3)
  xs = eg["lo"][0] + np.arange(nx) * eg["step"][0]
  assert np.abs(xs - np.linspace(-1.0, 2.0, nx)).max() <= 4e-16


def test_figure_settings_have_the_shapes_the_reference_draws():
  from cnf_ot_amd import solvers
  seen = 0
  for (_type, sub, dim), entry in solvers.FIGURE_SETTINGS.items():
    over = {"general": {"type": _type, "dim": dim}}
    if _type == "rwpo":
      over["rwpo"] = {"pot_type": sub}
    if _type == "fp" and sub is not None:
      over["fp"] = {"velocity_field_type": sub}
    st = solvers.figure_settings(solvers.load_config(overrides=over))
    assert st is not None
    seen += 1
    assert st["r"].shape == (len(entry["r"]), dim)
    assert len(st["domain_range"]) == 4 and st["domain_range"][0] < st["domain_range"][1]
    # plt.subplots(t_array.shape[0] // 5, 5) (utils.py:609-611): a whole number of rows of five
    assert len(st["t_array"]) % 5 == 0 and len(st["t_array"]) > 0
    assert st["t_array"][0] == 0.0
    if dim == 3:
      assert st["slice"] == 3.0 and all(p[2] == 3.0 for p in entry["r"])
      assert np.array_equal(st["section"], np.linspace(-5, 5, 11))
      assert {k: v[1] for k, v in st["directions"].items()} == {"x": 0, "y": 1, "z": 2}
      for axes, sec_axis in st["directions"].values():
        assert sorted(axes + (sec_axis,)) == [0, 1, 2] and axes[0] < axes[1]
  assert seen == 5
  # the default config is the rwpo double well: 8 seeds on [-2, 2]^2, linspace(0, T = 2, 5)
  st = solvers.figure_settings(solvers.load_config())
  assert st["r"].shape == (8, 2) and st["domain_range"] == [-2.0, 2.0, -2.0, 2.0]
  assert np.array_equal(st["t_array"], np.linspace(0.0, 2.0, 5))
  # nothing is drawn at other dimensions
  assert solvers.figure_settings(solvers.load_config(overrides={"general": {"dim": 10}})) is None
