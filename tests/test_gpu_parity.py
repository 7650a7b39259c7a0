"""GPU parity tests proper: the HIP path, called through the C ABI, against the
float64 oracle and the committed golden vectors.

Tolerances (fp32 kernels vs float64 oracle; DESIGN.md "Numerics" derives them):
  base -> data  (forward / sample / sample_and_log_prob):
      |dy| <= 2e-5, |d logdet|, |d log_prob| <= 1e-5   (BASELINE.json's bar)
  data -> base  (inverse / log_prob), the default "precise position path"
  (softmax terms to 1e-9, knot prefix sums / bin corner / result / base term
  in float64; include/cnf_ot_amd.h cnf_model_set_precise):
      |dx| <= 2e-5, |d logdet| <= 1e-5, |d log_prob| <= 1e-5  (BASELINE.json's bar)
  and with cnf_model_set_precise(0), plain fp32:
      |d log_prob| <= 5e-5 max and <= 2e-5 at the 99.9th percentile: the base
      term -x^2/2 multiplies the ~2e-6 position error of fp32 softmax-normalised
      knots by |x| <= 5.
These hold on the well-conditioned parameter sets (zeros; N(0, s^2) with the s
recorded in each fixture).  The scale-0.5 `wild` set has local slopes up to
e^16: no fp32 evaluation can meet an absolute bound there, so the kernel is
required to be at least as accurate as the plain fp32 C port of the oracle.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MLP_PATHS = ("mlp1", "mlp2", "mfma")      # the kernels that evaluate the conditioner MLP (mfma: small launches)
TOL_Y = 2e-5
TOL_LD = 1e-5
TOL_LP_SAMPLE = 1e-5
TOL_LP_DATA_MAX = 1e-5
TOL_LP_FP32_MAX = 5e-5       # cnf_model_set_precise(0)
TOL_LP_FP32_P999 = 2e-5


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  return torch.device("cuda", 0)


def _cfg_pair(D=2, L=2, H=16, M=2, K=5):
  import oracle
  from cnf_ot_amd import FlowConfig
  return (FlowConfig(dim=D, num_layers=L, hidden_size=H, mlp_num_layers=M, num_bins=K),
          oracle.OracleConfig(D=D, L=L, H=H, M=M, K=K))


def _engine(fcfg, params64, dev):
  from cnf_ot_amd import FlowEngine
  eng = FlowEngine(fcfg, dev)
  eng.load(torch.from_numpy(np.asarray(params64, dtype=np.float32)).to(dev))
  return eng


def _t(a, dev):
  return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)


RTOL = 2.5e-7   # ~2 fp32 ulps: only matters where |value| >> 1 (tail samples, |log_prob| ~ 700)


def _err(gpu, ref):
  """|gpu - ref| with the fp32 representation floor of large values removed:
  err = max(0, |d| - RTOL*|ref|)."""
  d = np.abs(gpu.detach().cpu().numpy().astype(np.float64) - ref)
  return np.maximum(d - RTOL * np.abs(ref), 0.0)


GOLDEN = {
  "flow_d1.npz": dict(D=1),
  "flow_d2.npz": dict(D=2),
  "flow_d10.npz": dict(D=10),
  "flow_d3_k8_h32_m3_l3.npz": dict(D=3, L=3, H=32, M=3, K=8),
}


@pytest.mark.parametrize("variant", ["mfma2", "mfma1", "packed2", "fast1", "ocml1", "pwl"])
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_vectors(golden_dir, dev, name, variant):
  """Every kernel variant: MFMA conditioner with two / one samples per lane,
  packed-VALU conditioner with two samples per lane (the MLP kernels' default),
  one sample per lane, ocml expf/logf + IEEE division instead of the hardware
  transcendentals, and the piecewise-linear conditioner tables (dim 2 with a
  uniform condition; every other case must fall through to the MLP kernel)."""
  fcfg, _ = _cfg_pair(**GOLDEN[name])
  g = np.load(os.path.join(golden_dir, name))
  eng = _engine(fcfg, g["params"], dev)
  eng.set_fast_math(variant != "ocml1")
  eng.set_mfma(variant.startswith("mfma"))       # only takes effect for hidden 16 / 5 bins
  eng.set_samples_per_lane(2 if variant.endswith("2") else 1)
  eng.set_pwl(2 if variant == "pwl" else 0)
  x = _t(g["noise"], dev)
  for tag, c in (("u", g["c_uniform"]), ("p", g["c_per"])):
    ct = _t(c, dev)
    y, fldj = eng.forward_logdet(x, ct)
    assert _err(y, g[f"y_{tag}"]).max() <= TOL_Y
    assert _err(fldj, g[f"fldj_{tag}"]).max() <= TOL_LD
    y2, lp = eng.sample_logprob(x, ct)
    assert torch.equal(y, y2)
    assert _err(lp, g[f"lp_sample_{tag}"]).max() <= TOL_LP_SAMPLE
    # data -> base on the oracle's (float32-rounded) samples
    y_in = g[f"y_{tag}"].astype(np.float32)
    import oracle
    _, ocfg = _cfg_pair(**GOLDEN[name])
    xb_ref, ildj_ref = oracle.inverse_logdet(ocfg, g["params"], y_in.astype(np.float64), c)
    lp_ref = oracle.log_prob(ocfg, g["params"], y_in.astype(np.float64), c)
    xb, ildj = eng.inverse_logdet(_t(y_in, dev), ct)
    assert _err(xb, xb_ref).max() <= TOL_Y
    assert _err(ildj, ildj_ref).max() <= TOL_LD
    assert _err(eng.log_prob(_t(y_in, dev), ct), lp_ref).max() <= TOL_LP_DATA_MAX
  lpv = eng.log_prob(_t(g["value"], dev), _t(g["c_uniform"], dev))
  assert _err(lpv, g["lp_value_u"]).max() <= TOL_LP_DATA_MAX


@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "valu"])
@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("params_kind", ["zeros", "random"])
@pytest.mark.parametrize("t", [0.0, 0.5, 1.0])
def test_config2_batch_65536_vs_oracle(dev, params_kind, t, spl, mfma):
  """BASELINE config 2 / SURVEY.md 8(d): D=2, B=65 536, base noise N(0,I), c
  uniform t in {0, .5, 1}; params (i) zeros (identity), (ii) N(0, 0.2^2) seed 42."""
  import oracle
  fcfg, ocfg = _cfg_pair(D=2)
  rng = np.random.default_rng(42)
  n = oracle.param_count(ocfg)
  params = np.zeros(n) if params_kind == "zeros" else rng.normal(0, 0.2, n).astype(np.float32).astype(np.float64)
  noise = rng.normal(size=(65536, 2)).astype(np.float32)
  eng = _engine(fcfg, params, dev)
  eng.set_samples_per_lane(spl)
  eng.set_mfma(mfma)
  y, lp = eng.sample_logprob(_t(noise, dev), torch.tensor([t], device=dev))
  y_ref, lp_ref = oracle.sample_logprob(ocfg, params, noise.astype(np.float64), [t])
  ey, elp = _err(y, y_ref), _err(lp, lp_ref)
  print(f"\n[cfg2 {params_kind} t={t} spl={spl} mfma={mfma}] max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e} "
        f"p99.9={np.quantile(elp, 0.999):.2e} median={np.median(elp):.2e}")
  assert ey.max() <= TOL_Y
  assert elp.max() <= TOL_LP_SAMPLE
  if params_kind == "zeros":       # identity at init (flows.py:48,71-76): fp32 rounding only
    assert (y.cpu() - torch.from_numpy(noise)).abs().max().item() <= 1e-6
  # log_prob direction on the kernel's own samples
  y32 = y.cpu().numpy()
  lpd_ref = oracle.log_prob(ocfg, params, y32.astype(np.float64), [t])
  elpd = _err(eng.log_prob(y, torch.tensor([t], device=dev)), lpd_ref)
  print(f"[cfg2 {params_kind} t={t}] log_prob dir: max={elpd.max():.2e} p99.9={np.quantile(elpd, 0.999):.2e}")
  assert elpd.max() <= TOL_LP_DATA_MAX
  eng.set_precise(False)         # plain fp32 stays selectable
  elpd = _err(eng.log_prob(y, torch.tensor([t], device=dev)), lpd_ref)
  print(f"[cfg2 {params_kind} t={t}] log_prob dir, fp32 positions: max={elpd.max():.2e} p99.9={np.quantile(elpd, 0.999):.2e}")
  assert elpd.max() <= TOL_LP_FP32_MAX and np.quantile(elpd, 0.999) <= TOL_LP_FP32_P999


def _zigzag_params(rng, n, L=2):
  """Conditioners whose second-layer units are triangle waves of u crossing
  zero in every first-layer interval: ~256 linear pieces per table (the bound
  is 289), far past the 112 rows the windowed kernels keep in LDS."""
  params = np.zeros(n)
  params[:16] = rng.normal(0, 0.3, 16)
  for l in range(L):
    w = params[16 + 592 * l: 16 + 592 * (l + 1)]
    w[16:32] = 1.0                                  # W0[u row]; the c row stays 0
    w[32:48] = -np.linspace(-7.5, 7.5, 16)          # b0: breakpoints at -7.5 .. 7.5
    slopes = np.array([1.0] + [-2.0, 2.0] * 7 + [-2.0])
    w[48:304] = (slopes[:, None] * (1.0 + 0.01 * np.arange(16))[None, :]).reshape(-1)      # W1[j][k]
    w[304:320] = -0.5 + 0.02 * (np.arange(16) - 8)  # b1
    w[320:576] = rng.normal(0, 0.3, 256)            # Wout
    w[576:592] = rng.normal(0, 0.3, 16)             # bout
  return params.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("params_kind", ["zeros", "random", "first_only", "zigzag", "wide_pieces"])
def test_config2_piecewise_linear_tables(dev, params_kind):
  """The dim-2 fast path (cnf_pwl.h): conditioner read from exact piecewise-
  linear tables built per (slice, layer).  Same bars as the MLP kernels, on
  slices of ragged (even) length with a partial last slice; `zeros` and
  `first_only` (all conditioner weights zero) are the degenerate one-piece
  tables, `zigzag` the near-worst-case piece count, `wide_pieces` breakpoints
  far outside the data."""
  import oracle
  fcfg, ocfg = _cfg_pair(D=2)
  rng = np.random.default_rng(11)
  n = oracle.param_count(ocfg)
  params = np.zeros(n)
  if params_kind == "random":
    params = rng.normal(0, 0.2, n).astype(np.float32).astype(np.float64)
  elif params_kind == "first_only":
    params[:16] = rng.normal(0, 0.5, 16).astype(np.float32)
  elif params_kind == "zigzag":
    params = _zigzag_params(rng, n)
  elif params_kind == "wide_pieces":
    # half of the first-layer units barely depend on u: their breakpoints sit at |u| ~ 1e3, so the pieces
    # that serve the samples are thousands wide (the affine maps must be referred to a point near the samples)
    params = rng.normal(0, 0.2, n)
    for l in range(2):
      params[16 + 592 * l + 16: 16 + 592 * l + 24] *= 1e-3
    params = params.astype(np.float32).astype(np.float64)
  S, Bs = 7, 9998                      # 7 slices of 9 998 = 4 tiles of 2 048 + a partial one
  B = S * Bs - 4000                    # the last slice is short
  noise = rng.normal(size=(S * Bs, 2)).astype(np.float32)
  noise[0] = [11.0, -12.5]             # linear tails
  noise[1] = [-17.0, 12.0]             # outside the coarse grid of the tables (far tails amplify fp32
  noise[2] = [16.5, -11.0]             # rounding through the tail slopes: kept moderate)
  ts = np.linspace(0.0, 1.0, S)
  eng = _engine(fcfg, params, dev)
  eng.set_pwl(2)
  c_host = np.repeat(ts, Bs)
  y, lp = eng.sample_logprob(_t(noise, dev), _t(ts, dev))
  y_ref, lp_ref = oracle.sample_logprob(ocfg, params, noise.astype(np.float64), c_host)
  ey, elp = _err(y, y_ref), _err(lp, lp_ref)
  print(f"\n[pwl {params_kind}] max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e}")
  if params_kind == "zigzag":
    # second-layer slopes of +-2 x 16 units: ill-conditioned like the `wild` set, so the bar is the plain
    # fp32 C port of the oracle (measured: port 9e-4 / 5e-4, tables 4e-4 / 1.6e-4), and agreement with the
    # MLP kernel on the same inputs
    y32, lp32 = oracle.sample_logprob(ocfg, params.astype(np.float32), noise, c_host.astype(np.float32), dtype=np.float32)
    assert ey.max() <= np.abs(y32 - y_ref).max() + TOL_Y and elp.max() <= np.abs(lp32 - lp_ref).max() + TOL_LP_SAMPLE
    assert np.median(elp) <= 2 * np.median(np.abs(lp32 - lp_ref)) + 1e-6
    eng.set_pwl(0)
    y0, lp0 = eng.sample_logprob(_t(noise, dev), _t(ts, dev))
    e0 = _err(y0, y_ref)
    print(f"[mlp zigzag] max|dy|={e0.max():.2e} max|dlogp|={_err(lp0, lp_ref).max():.2e}")
    return
  assert ey.max() <= TOL_Y and elp.max() <= TOL_LP_SAMPLE
  # the short batch: c given per slice with an explicit c_block through the generic per-sample form
  yb, lpb = eng.sample_logprob(_t(noise[:B], dev), _t(c_host[:B], dev)[:, None])      # per sample: MLP kernel
  assert _err(yb, y_ref[:B]).max() <= TOL_Y and _err(lpb, lp_ref[:B]).max() <= TOL_LP_SAMPLE
  # data -> base through the tables, single condition, ragged odd batch
  Bo = 50001
  y_in = y_ref[:Bo].astype(np.float32)
  xb_ref, ildj_ref = oracle.inverse_logdet(ocfg, params, y_in.astype(np.float64), [0.37])
  lp_ref1 = oracle.log_prob(ocfg, params, y_in.astype(np.float64), [0.37])
  xb, ildj = eng.inverse_logdet(_t(y_in, dev), torch.tensor([0.37], device=dev))
  ex = _err(xb, xb_ref)
  # `first_only`/`random` samples in the far tail ( |y| = 30, 40 ) carry the fp32 floor of their magnitude
  assert eng.last_path() == "tables"
  assert ex.max() <= TOL_Y and _err(ildj, ildj_ref).max() <= TOL_LD
  elpd = _err(eng.log_prob(_t(y_in, dev), torch.tensor([0.37], device=dev)), lp_ref1)
  print(f"[pwl {params_kind}] log_prob dir (precise): max={elpd.max():.2e} p99.9={np.quantile(elpd, 0.999):.2e}")
  assert elpd.max() <= TOL_LP_DATA_MAX
  eng.set_precise(False)
  elpd = _err(eng.log_prob(_t(y_in, dev), torch.tensor([0.37], device=dev)), lp_ref1)
  print(f"[pwl {params_kind}] log_prob dir (fp32): max={elpd.max():.2e} p99.9={np.quantile(elpd, 0.999):.2e}")
  assert elpd.max() <= TOL_LP_FP32_MAX and np.quantile(elpd, 0.999) <= TOL_LP_FP32_P999
  eng.set_precise(True)
  # and the tables agree with the MLP kernel far below the oracle tolerance
  eng.set_pwl(0)
  y0, lp0 = eng.sample_logprob(_t(noise, dev), _t(ts, dev))
  # (an ulp of |log_prob| ~ 200 in the far tail is 1.5e-5: allow 2 ulps on top of the absolute bound)
  # two fp32 evaluations, each within ~6e-6 of the float64 value (asserted against the oracle above)
  assert ((y0 - y).abs() - RTOL * y.abs()).max().item() <= 1.5e-5
  assert ((lp0 - lp).abs() - RTOL * lp.abs()).max().item() <= 1.5e-5


@pytest.mark.parametrize("L", [1, 3, 4])
def test_table_path_other_depths(dev, L):
  """The table path with 1, 3 and 4 flow layers (L tables of 21 KB in LDS;
  the layer permutation alternates), both directions, vs the oracle."""
  import oracle
  fcfg, ocfg = _cfg_pair(D=2, L=L)
  rng = np.random.default_rng(20 + L)
  params = rng.normal(0, 0.2, oracle.param_count(ocfg)).astype(np.float32).astype(np.float64)
  S, Bs = 3, 6000
  noise = rng.normal(size=(S * Bs, 2)).astype(np.float32)
  ts = np.array([0.1, 0.5, 0.9])
  c_host = np.repeat(ts, Bs)
  eng = _engine(fcfg, params, dev)
  eng.set_pwl(2)
  y, lp = eng.sample_logprob(_t(noise, dev), _t(ts, dev))
  y_ref, lp_ref = oracle.sample_logprob(ocfg, params, noise.astype(np.float64), c_host)
  assert _err(y, y_ref).max() <= TOL_Y and _err(lp, lp_ref).max() <= TOL_LP_SAMPLE * max(1, L / 2)
  y_in = y_ref.astype(np.float32)
  lpd_ref = oracle.log_prob(ocfg, params, y_in.astype(np.float64), c_host)
  elpd = _err(eng.log_prob(_t(y_in, dev), _t(ts, dev)), lpd_ref)
  assert elpd.max() <= TOL_LP_DATA_MAX * max(1, L / 2)
  eng.set_pwl(0)
  y0, lp0 = eng.sample_logprob(_t(noise, dev), _t(ts, dev))
  assert (y0 - y).abs().max().item() <= 2e-5 and (lp0 - lp).abs().max().item() <= 2e-5


def test_table_rows_past_the_lds_window(dev):
  """With L <= 3 the flow kernel stages every row of its tables; with L = 4 it keeps the first 112 rows of each
  in LDS and reads the rest from the global table -- `zigzag` tables have ~256.  Both row paths must give the
  same function: the L = 4 table result is compared with the MLP kernel and with the fp32 port of the oracle
  (the set is ill-conditioned: see test_config2_piecewise_linear_tables)."""
  import oracle
  L = 4
  fcfg, ocfg = _cfg_pair(D=2, L=L)
  rng = np.random.default_rng(77)
  params = _zigzag_params(rng, oracle.param_count(ocfg), L)
  S, Bs = 3, 6000
  noise = rng.normal(size=(S * Bs, 2)).astype(np.float32)
  ts = np.array([0.2, 0.5, 0.8])
  c_host = np.repeat(ts, Bs)
  eng = _engine(fcfg, params, dev)
  eng.set_pwl(2)
  y, lp = eng.sample_logprob(_t(noise, dev), _t(ts, dev))
  assert eng.last_path() == "tables"
  y_ref, lp_ref = oracle.sample_logprob(ocfg, params, noise.astype(np.float64), c_host)
  y32, lp32 = oracle.sample_logprob(ocfg, params.astype(np.float32), noise, c_host.astype(np.float32), dtype=np.float32)
  ey, elp = _err(y, y_ref), _err(lp, lp_ref)
  print(f"\n[rows past the window, L=4 zigzag] tables max|dy|={ey.max():.2e} max|dlogp|={elp.max():.2e}; "
        f"fp32 port {np.abs(y32 - y_ref).max():.2e} / {np.abs(lp32 - lp_ref).max():.2e}")
  assert ey.max() <= 2 * np.abs(y32 - y_ref).max() + TOL_Y and elp.max() <= 2 * np.abs(lp32 - lp_ref).max() + TOL_LP_SAMPLE
  assert np.median(elp) <= 2 * np.median(np.abs(lp32 - lp_ref)) + 1e-6
  # data -> base through the same rows (precise positions), round trip to the noise
  xb, _ = eng.inverse_logdet(y, _t(ts, dev))
  assert eng.last_path() == "tables"
  rt = (xb - _t(noise, dev)).abs()
  print(f"[rows past the window] round trip median {rt.median().item():.2e} max {rt.max().item():.2e}")
  assert rt.median().item() <= 5e-5      # (measured 1.1e-5: four ill-conditioned layers in fp32)


def test_table_path_randomised_against_mlp_kernel_and_oracle(dev):
  """A small fixed-seed cut of scripts/soak_pwl.py: parameter sets of scale
  0.05 .. 1.5 with sparse / tied / far-breakpoint weights, inputs of spread
  1 .. 8.  Ill-conditioned sets have large fp32 errors in BOTH kernels, so the
  criterion is relative: the table path is never further from the float64 oracle
  than 3x the MLP kernel (+ the fp32 floor), for samples, log_prob and the
  data->base log_prob."""
  import oracle
  fcfg, ocfg = _cfg_pair(D=2)
  rng = np.random.default_rng(123)
  for case in range(18):
    scale = float(rng.choice([0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.5]))
    w = rng.normal(0, scale, 1200)
    kind = case % 6
    if kind == 1:
      w[rng.random(1200) < 0.5] = 0.0
    elif kind == 2:
      for l in range(2):
        blk = w[16 + 592 * l: 16 + 592 * (l + 1)]
        blk[16:24] = blk[24:32]; blk[0:8] = blk[8:16]; blk[32:40] = blk[40:48]
    elif kind == 3:
      for l in range(2):
        w[16 + 592 * l + 16: 16 + 592 * l + 24] *= 1e-3
    elif kind == 4:
      for l in range(2):
        w[16 + 592 * l + 32: 16 + 592 * l + 48] *= 40.0
    params = w.astype(np.float32)
    S, Bs = 3, 3000
    ts = rng.uniform(-0.5, 1.5, S).astype(np.float32)
    noise = (rng.normal(size=(S * Bs, 2)) * float(rng.choice([1.0, 3.0, 8.0]))).astype(np.float32)
    c64 = np.repeat(ts.astype(np.float64), Bs)
    y64, lp64 = oracle.sample_logprob(ocfg, params.astype(np.float64), noise.astype(np.float64), c64)
    y_in = np.clip(y64, -1e6, 1e6).astype(np.float32)
    lpd64 = oracle.log_prob(ocfg, params.astype(np.float64), y_in.astype(np.float64), c64)
    eng = _engine(fcfg, params, dev)
    err = {}
    for mode in (0, 2):
      eng.set_pwl(mode)
      y, lp = eng.sample_logprob(_t(noise, dev), _t(ts, dev))
      lpd = eng.log_prob(_t(y_in, dev), _t(ts, dev))
      err[mode] = [np.abs(y.cpu().double().numpy() - y64).max(1), np.abs(lp.cpu().double().numpy() - lp64),
                   np.abs(lpd.cpu().double().numpy() - lpd64)]
    for q, (e_mlp, e_tab) in enumerate(zip(err[0], err[2])):
      fin = np.isfinite(e_mlp) & np.isfinite(e_tab)
      assert (np.isfinite(e_mlp) == np.isfinite(e_tab)).all(), (case, q)
      e_mlp, e_tab = e_mlp[fin], e_tab[fin]
      assert np.median(e_tab) <= 3 * np.median(e_mlp) + 1e-6, (case, kind, scale, q)
      assert np.quantile(e_tab, 0.999) <= 3 * np.quantile(e_mlp, 0.999) + 5e-5, (case, kind, scale, q)


def test_entry_points_are_graph_capturable(dev):
  """include/cnf_ot_amd.h: compute entry points only enqueue work on the given
  stream -- no allocation, no synchronisation.  Capture a sampling call of each
  kernel family into a HIP graph WITHOUT any warm-up call on the capturing
  stream (the table workspace comes from cnf_model_reserve, outside capture),
  replay it on new inputs, compare with eager calls."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=8, device=dev))
  S, Bs = 4, 4096
  x = eng.normal(1, S * Bs)
  t = torch.linspace(0.2, 0.8, S, device=dev)
  y = torch.empty(S * Bs, 2, device=dev); lp = torch.empty(S * Bs, device=dev)
  torch.cuda.synchronize()
  for mode in (0, 2):
    eng.set_pwl(mode)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
      assert eng.reserve(S) >= S                               # NOT a compute call; nothing has run on `side` yet
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      eng.sample_logprob(x, t, out=y, logp_out=lp)
      assert eng.last_path() == ("tables" if mode == 2 else "mfma")       # 16 384 samples: the small-launch kernel
    x.copy_(eng.normal(2 + mode, S * Bs))                      # new inputs in the captured buffers
    t.copy_(torch.linspace(0.3, 0.9, S, device=dev))
    graph.replay()
    torch.cuda.synchronize()
    y_g, lp_g = y.clone(), lp.clone()
    y_e, lp_e = eng.sample_logprob(x, t)
    assert torch.equal(y_g, y_e) and torch.equal(lp_g, lp_e), mode
  eng.set_pwl(1)


@pytest.mark.parametrize("D", [2, 3, 10])
def test_seeded_sampling_is_fill_normal_plus_sample_logprob(dev, D):
  """cnf_sample_logprob_seeded (model.apply.sample / sample_and_log_prob(seed=), conditional.py:376-402: the base draw
  inside the call) == cnf_fill_normal + cnf_sample_logprob bit for bit, on every kernel path: tables and MLP kernels
  at 65 536 x 7 slices (dim 2), the small-launch MFMA kernel, the wave-per-dimension kernel (dim >= 3), per-sample
  conditions, ragged sizes, a stream offset, and every slice reusing one draw (slice_stride = 0)."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  cfg = FlowConfig(dim=D); model = FlowModel(cfg)
  params = Params.random(cfg, 0.2 if D == 2 else 0.12, seed=70 + D, device=dev)
  eng = model.engine(dev).load(params)
  cases = [(7, 65536 if D == 2 else 8192, 2), (7, 65536 if D == 2 else 8192, 0), (1, 65536, 1), (5, 1001, 1), (3, 4096, 1)]
  for S, Bs, mode in cases:
    if D != 2 and mode == 0:
      continue
    eng.set_pwl(mode)
    t = torch.linspace(0.05, 0.95, S, device=dev)
    for first in (0, 12345):
      noise = eng.normal(99, S * Bs, first_sample=first)
      y0, lp0 = eng.sample_logprob(noise, t)
      path = eng.last_path()
      y1, lp1 = eng.sample_logprob_seeded(99, S * Bs, t, first_sample=first)
      assert eng.last_path() == path
      assert torch.equal(y0, y1) and torch.equal(lp0, lp1), (D, S, Bs, mode, first, path)
    # every slice the same draw (the reused rng of applications.py:392-400)
    one = eng.normal(5, Bs)
    y0, lp0 = eng.sample_logprob(one.repeat(S, 1), t)
    y1, lp1 = eng.sample_logprob_seeded(5, S * Bs, t, slice_stride=0)
    assert torch.equal(y0, y1) and torch.equal(lp0, lp1), (D, S, Bs, mode, "stride 0")
  eng.set_pwl(1)
  # per-sample conditions cond[B, 1] (the reference's literal form), uniform and not: through model.apply
  B = 65536 if D == 2 else 4096
  for cond in (torch.full((B, 1), 0.4, device=dev), torch.linspace(0.0, 1.0, B, device=dev)[:, None].contiguous()):
    ya, lpa = model.apply.sample_and_log_prob(params, cond=cond, seed=31, sample_shape=(B,))
    yb, lpb = model.apply.sample_and_log_prob(params, cond=cond, noise=eng.normal(31, B), sample_shape=(B,))
    assert torch.equal(ya, yb) and torch.equal(lpa, lpb)
    assert torch.equal(model.apply.sample(params, cond=cond, seed=31, sample_shape=(B,)), ya)


def test_graph_replay_survives_a_larger_reservation(dev):
  """A HIP graph captured on the table path has the workspace address baked into its kernel arguments.  Growing the
  stream's reservation afterwards (an eager call with more slices) must not free that block: the replay that follows
  would read and write freed memory (cnf_model_reserve retires outgrown blocks instead of freeing them)."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=9, device=dev))
  eng.set_pwl(2)
  S, Bs = 4, 4096
  x = eng.normal(1, S * Bs)
  t = torch.linspace(0.2, 0.8, S, device=dev)
  y = torch.empty(S * Bs, 2, device=dev); lp = torch.empty(S * Bs, device=dev)
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  with torch.cuda.stream(side):
    small = eng.reserve(S)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    eng.sample_logprob(x, t, out=y, logp_out=lp)
    assert eng.last_path() == "tables"
  graph.replay(); torch.cuda.synchronize()
  y0, lp0 = y.clone(), lp.clone()
  # an eager call on the SAME stream with many more slices: the engine grows the reservation
  with torch.cuda.stream(side):
    S2 = 8 * small
    x2 = eng.normal(3, S2 * 1024)
    eng.sample_logprob(x2, torch.linspace(0.0, 1.0, S2, device=dev))
    assert eng.lib.cnf_model_reserved(eng._h, side.cuda_stream) > small
    # churn the allocator so that a freed block would have been handed out again and overwritten
    junk = [torch.full((1 << 20,), float("nan"), device=dev) for _ in range(8)]
  torch.cuda.synchronize()
  y.zero_(); lp.zero_()
  graph.replay(); torch.cuda.synchronize()
  assert torch.equal(y, y0) and torch.equal(lp, lp0)
  del junk
  eng.set_pwl(1)


def test_load_reprepares_unless_told_the_parameters_are_unchanged(dev):
  """FlowEngine.load prepares the parameters on every call: writers torch does not see (collectives, `.data`, other
  libraries' kernels) leave the version counter alone, and an engine that skipped "unchanged" parameters would go on
  computing with the old weights.  The skip is opt-in (assume_unchanged=True) and `mark_updated` is its escape hatch."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  from cnf_ot_amd.flows import mark_updated
  cfg = FlowConfig(dim=2)
  params = Params.random(cfg, 0.2, seed=3, device=dev)
  x = torch.randn(4096, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
  c = torch.tensor([0.4], device=dev)
  model = FlowModel(cfg)
  lp0 = model.apply.log_prob(params, x, c).clone()
  v = params.flat._version
  params.flat.data.mul_(1.5)                       # a write torch's version counter does not record
  assert params.flat._version == v
  lp1 = model.apply.log_prob(params, x, c).clone()
  assert (lp1 - lp0).abs().max().item() > 1e-3     # default: re-prepared, the new weights are used
  fast = FlowModel(cfg, assume_unchanged_params=True)
  a0 = fast.apply.log_prob(params, x, c).clone()
  assert torch.equal(a0, lp1)
  params.flat.data.mul_(1.0 / 1.5)
  stale = fast.apply.log_prob(params, x, c).clone()
  assert torch.equal(stale, a0)                    # the documented hazard of the opt-in ...
  mark_updated(params.flat)
  fresh = fast.apply.log_prob(params, x, c).clone()
  assert (fresh - lp0).abs().max().item() <= 1e-5  # ... and its escape hatch


def test_compute_calls_never_allocate(dev):
  """A compute call never grows the table workspace: on a stream WITHOUT a
  reservation, captured into a graph (where an allocation would fail the
  capture), a call that asks for the table path runs the MLP kernels and gives
  their result; with a reservation smaller than the call's slice count it is
  processed in chunks of the reservation."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=9, device=dev))
  S, Bs = 40, 2048
  x = eng.normal(1, S * Bs)
  t = torch.linspace(0.0, 1.0, S, device=dev)
  eng.set_pwl(0)
  y_mlp, lp_mlp = eng.sample_logprob(x, t)
  eng.set_pwl(2)
  y = torch.empty_like(y_mlp); lp = torch.empty_like(lp_mlp)
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):                   # FlowEngine.reserve is a no-op while capturing
    eng.sample_logprob(x, t, out=y, logp_out=lp)
    assert eng.last_path() in MLP_PATHS
  assert eng.lib.cnf_model_reserved(eng._h, side.cuda_stream) == 0
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(y, y_mlp) and torch.equal(lp, lp_mlp)
  # a reservation of 16 sets for a 40-slice call: chunks of 16, 16, 8 -- same numbers as one big workspace
  with torch.cuda.stream(side):
    _capi.check(eng.lib.cnf_model_reserve(eng._h, side.cuda_stream, 16), "cnf_model_reserve")
    eng._reserved[side.cuda_stream] = 1 << 20                  # keep the engine from growing it
    y_c, lp_c = eng.sample_logprob(x, t)
    assert eng.last_path() == "tables"
  torch.cuda.synchronize()
  assert eng.lib.cnf_model_reserved(eng._h, side.cuda_stream) == 16
  y_t, lp_t = eng.sample_logprob(x, t)                         # current stream: engine reserves 64 sets, one chunk
  assert eng.last_path() == "tables"
  torch.cuda.synchronize()
  assert torch.equal(y_c, y_t) and torch.equal(lp_c, lp_t)
  assert (y_t - y_mlp).abs().max().item() <= 2e-5 and (lp_t - lp_mlp).abs().max().item() <= 2e-5
  eng.set_pwl(1)


def test_per_sample_uniform_condition_is_detected_on_device(dev):
  """The reference's literal call form: one time broadcast to cond[B,1]
  (applications.py:153,226,231) is per-sample in form and uniform in content.
  For a launch large enough for the table path the library checks uniformity
  on the device and runs the table kernels, with the MLP kernel enqueued behind
  them as the gated alternative: a uniform cond[B,1] gives the scalar-condition
  table result bit for bit, a cond[B,1] with one different entry gives the MLP
  kernel's per-sample result bit for bit -- no host synchronisation either way."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=12, device=dev))
  B = 1 << 21
  x = eng.normal(5, B)
  for fn in ("sample_logprob", "log_prob"):
    call = (lambda c: eng.sample_logprob(x, c)) if fn == "sample_logprob" else (lambda c: (eng.log_prob(x, c),))
    ref_tab = call(torch.tensor([0.3], device=dev))
    assert eng.last_path() == "tables"
    c_uni = torch.full((B, 1), 0.3, device=dev)
    got = call(c_uni)
    assert eng.last_path() == "detect"
    for a, b in zip(got, ref_tab):
      assert torch.equal(a, b), fn
    c_mix = c_uni.clone()
    c_mix[B - 7, 0] = 0.31
    got = call(c_mix)
    assert eng.last_path() == "detect"
    eng.set_pwl(0)
    ref_mlp = call(c_mix)
    assert eng.last_path() in MLP_PATHS
    eng.set_pwl(1)
    for a, b in zip(got, ref_mlp):
      assert torch.equal(a, b), fn
  # a single 65 536-sample batch stays on the MLP kernel (the tables do not pay there): no check is enqueued
  eng.sample_logprob(x[:65536], c_uni[:65536])
  assert eng.last_path() in MLP_PATHS


def test_table_path_many_slices(dev):
  """More slices than one build + flow kernel pair takes (2 048): the call is
  processed in chunks against a bounded workspace; same numbers as the MLP
  kernel, chunk boundaries included."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, applications as app, _capi
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=6, device=dev))
  S, Bs = 2048 * 2 + 77, 64
  x = eng.normal(3, S * Bs)
  t = torch.rand(S, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
  res = {}
  for mode in (0, 2):
    eng.set_pwl(mode)
    y, lp = eng.sample_logprob(x, t)
    kin = eng.loss_terms_seeded(app._spec(_capi.TERM_KINETIC, dt=0.01), 11, t.cpu().numpy(), Bs, first_sample=5, slice_stride=Bs)
    res[mode] = (y, lp, kin)
  # two fp32 evaluations, each within ~5e-6 of the float64 value
  assert (res[0][0] - res[2][0]).abs().max().item() <= 2e-5
  assert (res[0][1] - res[2][1]).abs().max().item() <= 2e-5
  # a slice sums only 64 finite-difference velocities (fp32 noise ~1e-3 each): loose per slice, tight in total
  rel = ((res[0][2] - res[2][2]).abs() / res[0][2].abs().clamp_min(1e-6)).max().item()
  tot = abs(float(res[0][2].sum() - res[2][2].sum())) / float(res[0][2].sum())
  assert rel <= 5e-3 and tot <= 1e-5, (rel, tot)
  eng.set_pwl(1)


def test_table_path_chunked_by_a_small_reservation(dev):
  """A reservation smaller than the slice count, together with several table sets per slice: 7 slices of 4 098 samples
  (two full 2 048-sample tiles and a 2-sample tail tile) on 3 reserved sets run as flow chunks of 3, 3 and 1 slices,
  and the kinetic term (2 sets per slice) as one slice per chunk.  Per-sample results do not depend on the chunking:
  bit for bit those of a 7-set reservation.  The per-slice kinetic sums are accumulated in an order that depends on
  the grid: the one-chunk result (14 sets) to the 5e-5 that test_gpu_losses.py grants two evaluations of that term."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, applications as app, _capi
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=14, device=dev))
  eng.set_pwl(2)
  S, Bs = 7, 4098
  x = eng.normal(8, S * Bs)
  t = torch.linspace(0.05, 0.95, S, device=dev)
  kinetic = app._spec(_capi.TERM_KINETIC, dt=0.01)
  torch.cuda.synchronize()

  def reserved(n_sets, calls):
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
      _capi.check(eng.lib.cnf_model_reserve(eng._h, side.cuda_stream, n_sets), "cnf_model_reserve")
      eng._reserved[side.cuda_stream] = 1 << 20                # keep the engine from growing it
      out = []
      for call, path in calls:
        out.append(call())
        assert eng.last_path() == path
    torch.cuda.synchronize()
    assert eng.lib.cnf_model_reserved(eng._h, side.cuda_stream) == n_sets
    return out

  flow = [(lambda: eng.sample_logprob(x, t), "tables"), (lambda: eng.log_prob(x, t), "tables")]
  loss = [(lambda: eng.loss_terms_seeded(kinetic, 11, t, Bs, first_sample=5, slice_stride=Bs), "loss_tables")]
  (y3, lp3), lq3, kin3 = reserved(3, flow + loss)
  (y7, lp7), lq7 = reserved(7, flow)
  kin14, = reserved(14, loss)
  assert torch.equal(y3, y7) and torch.equal(lp3, lp7) and torch.equal(lq3, lq7)
  rel = ((kin3 - kin14).abs() / kin14.abs().clamp_min(1e-30)).max().item()
  print(f"\n[chunked kinetic] 1 slice per chunk vs one chunk: max relative difference over {S} slices {rel:.2e}")
  assert torch.isfinite(kin14).all() and (kin14 > 0).all() and rel <= 5e-5
  eng.set_pwl(1)


def test_table_path_on_two_streams(dev):
  """The conditioner tables live in a workspace per (model, stream): calls of
  one model issued on two streams, with different slice counts (one grows its
  workspace mid-way), give the single-stream results."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=5, device=dev))
  eng.set_pwl(2)
  Bs = 4096
  jobs = []
  for i, S in enumerate((3, 9, 5, 17)):
    x = eng.normal(100 + i, S * Bs)
    t = torch.linspace(0.1, 0.9, S, device=dev)
    jobs.append((x, t, eng.sample_logprob(x, t)))
  torch.cuda.synchronize()
  streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
  outs = []
  for rep in range(3):
    for i, (x, t, _) in enumerate(jobs):
      with torch.cuda.stream(streams[i % 2]):
        outs.append((i, eng.sample_logprob(x, t)))
  torch.cuda.synchronize()
  for i, (y, lp) in outs:
    assert torch.equal(y, jobs[i][2][0]) and torch.equal(lp, jobs[i][2][1])


def test_dim10_batch_vs_oracle(dev):
  """BASELINE config 4 shape: D=10 (per-GPU shard 32 768), N(0, 0.12^2) params."""
  import oracle
  fcfg, ocfg = _cfg_pair(D=10)
  rng = np.random.default_rng(4)
  params = rng.normal(0, 0.12, oracle.param_count(ocfg)).astype(np.float32).astype(np.float64)
  noise = rng.normal(size=(32768, 10)).astype(np.float32)
  eng = _engine(fcfg, params, dev)
  eng.set_samples_per_lane(2)
  y, lp = eng.sample_logprob(_t(noise, dev), torch.tensor([0.3], device=dev))
  y_ref, lp_ref = oracle.sample_logprob(ocfg, params, noise.astype(np.float64), [0.3])
  print(f"\n[d10] max|dy|={_err(y, y_ref).max():.2e} max|dlogp|={_err(lp, lp_ref).max():.2e}")
  assert _err(y, y_ref).max() <= TOL_Y
  assert _err(lp, lp_ref).max() <= 2e-5      # 20 splines summed instead of 4


@pytest.mark.parametrize("D,B", [(3, 5000), (10, 32768 + 77), (24, 700)])
def test_wave_per_dimension_kernel(dev, D, B):
  """flow_dpar_kernel (base -> data at dim >= 3, one wave per conditioned
  dimension; D = 24 strides 23 conditioners over 16 waves): both lane widths,
  uniform and per-sample conditions, ragged batch, vs the oracle and vs the
  one-sample-per-lane kernel; forward / sample_and_log_prob / sample."""
  import oracle
  fcfg, ocfg = _cfg_pair(D=D)
  rng = np.random.default_rng(100 + D)
  params = rng.normal(0, 0.12 if D <= 10 else 0.05, oracle.param_count(ocfg)).astype(np.float32).astype(np.float64)
  noise = rng.normal(size=(B, D)).astype(np.float32)
  c_per = rng.uniform(0, 1, B).astype(np.float32)
  eng = _engine(fcfg, params, dev)
  for cond, c_host, c_block in ((torch.tensor([0.3], device=dev), [0.3], B), (_t(c_per, dev), c_per.astype(np.float64), 1)):
    y_ref, lp_ref = oracle.sample_logprob(ocfg, params, noise.astype(np.float64), c_host)     # c of length B: per sample
    eng.set_dpar(0)
    y0, lp0 = eng.sample_logprob(_t(noise, dev), cond)
    assert eng.last_path() in MLP_PATHS
    eng.set_dpar(2)
    for spl in (1, 2):
      eng.set_samples_per_lane(spl)
      y, lp = eng.sample_logprob(_t(noise, dev), cond)
      assert eng.last_path() == "dpar"
      assert _err(y, y_ref).max() <= TOL_Y and _err(lp, lp_ref).max() <= (2e-5 if D <= 10 else 5e-5)
      assert (y - y0).abs().max().item() <= 2e-5 and (lp - lp0).abs().max().item() <= 2e-5
      yf, fldj = eng.forward_logdet(_t(noise, dev), cond)
      assert torch.equal(yf, y)
      ys, _ = eng.sample_logprob(_t(noise, dev), cond, want_logp=False)
      assert torch.equal(ys, y)
    eng.set_samples_per_lane(0)
  eng.set_dpar(1)                       # default: by batch size -- these batches are small
  eng.sample_logprob(_t(noise, dev), torch.tensor([0.3], device=dev))
  assert eng.last_path() == "dpar"


@pytest.mark.parametrize("pwl", [0, 2], ids=["mlp", "pwl"])
def test_wild_params_no_worse_than_fp32_port(dev, golden_dir, pwl):
  """SURVEY.md 8(d) cfg 2 (ii) literal: N(0, 0.5^2) on every tensor, seed 42
  (with the piecewise-linear tables too: many breakpoints inside the range)."""
  import oracle
  fcfg, ocfg = _cfg_pair(D=2)
  rng = np.random.default_rng(42)
  params = rng.normal(0, 0.5, oracle.param_count(ocfg)).astype(np.float32)
  noise = rng.normal(size=(65536, 2)).astype(np.float32)
  eng = _engine(fcfg, params, dev)
  eng.set_pwl(pwl)
  _, lp = eng.sample_logprob(_t(noise, dev), torch.tensor([0.5], device=dev))
  _, lp64 = oracle.sample_logprob(ocfg, params.astype(np.float64), noise.astype(np.float64), [0.5])
  _, lp32 = oracle.sample_logprob(ocfg, params, noise, [0.5], dtype=np.float32)
  e_gpu, e_port = _err(lp, lp64), np.abs(lp32.astype(np.float64) - lp64)
  print(f"\n[wild] gpu: median={np.median(e_gpu):.2e} p99={np.quantile(e_gpu, .99):.2e} max={e_gpu.max():.2e} | "
        f"fp32 C port: median={np.median(e_port):.2e} p99={np.quantile(e_port, .99):.2e} max={e_port.max():.2e}")
  assert np.median(e_gpu) <= 2 * np.median(e_port) + 1e-6
  assert np.quantile(e_gpu, 0.99) <= 2 * np.quantile(e_port, 0.99) + 1e-5


@pytest.mark.parametrize("D", [2, 3])
def test_non_finite_points_come_out_non_finite(dev, D):
  """data -> base (log_prob / inverse, conditional.py:299-321): a NaN or infinite coordinate must not come back as a
  finite number -- the splines' clamps and bin searches used to turn a NaN into the point -10 and log_prob(NaN) into
  -58.9, where the reference's arithmetic (and the float64 oracle: NaN / -inf) propagates it.  Every kernel that serves
  the direction (tables, MLP at 1 and 2 samples per lane, MFMA, the precise and the plain position path), and the
  samples around the bad ones unchanged."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  from oracle import capi as ocapi
  cfg = FlowConfig(dim=D)
  params = Params.random(cfg, 0.2, seed=5, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  B = 1 << 18
  g = torch.Generator(device="cpu").manual_seed(D)
  x = torch.randn(B, D, generator=g).to(dev)
  bad_rows = [5, 70001, B - 1]
  ocfg = ocapi.OracleConfig(D=D)
  pnp = params.flat.cpu().numpy().astype(np.float64)
  for bad in (float("nan"), float("inf"), -float("inf")):
    x2 = x.clone()
    for k, r in enumerate(bad_rows):
      x2[r, k % D] = bad
    want = ocapi.log_prob(ocfg, pnp, x2[bad_rows].cpu().numpy().astype(np.float64), np.full((len(bad_rows), 1), 0.3))
    assert not np.isfinite(want).any()
    for mode in ((0, 2) if D == 2 else (0,)):
      eng.set_pwl(mode)
      for precise in (True, False):
        eng.set_precise(precise)
        for n in (B, 4096):      # (small launches: the MFMA kernel)
          lp_clean = eng.log_prob(x[:n], 0.3)
          lp = eng.log_prob(x2[:n], 0.3)
          z, ild = eng.inverse_logdet(x2[:n], 0.3)
          rows = [r for r in bad_rows if r < n]
          for r in rows:
            assert not torch.isfinite(lp[r]), (bad, mode, precise, n, r, lp[r].item(), eng.last_path())
            assert not torch.isfinite(ild[r]) or not torch.isfinite(z[r]).all(), (bad, mode, precise, n, r)
          keep = torch.ones(n, dtype=torch.bool, device=dev); keep[rows] = False
          # (not bit for bit: a wave evaluates the general form of a spline when ANY of its lanes needs it)
          torch.testing.assert_close(lp[keep], lp_clean[keep], rtol=0, atol=2e-5)
  eng.set_precise(True); eng.set_pwl(1)


def test_roundtrip_and_consistency_at_full_size(dev):
  """Size-independent properties at BASELINE sizes (no oracle needed):
  inverse(forward(x)) == x, logdets antisymmetric, log_prob(sample) equals the
  log_prob returned with the sample."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  for D, B, scale in ((2, 1 << 20, 0.2), (10, 262144, 0.12)):
    cfg = FlowConfig(dim=D)
    eng = FlowEngine(cfg, dev).load(Params.random(cfg, scale, seed=7, device=dev))
    x = eng.normal(123, B)
    c = torch.tensor([0.6], device=dev)
    y, fldj = eng.forward_logdet(x, c)
    xb, ildj = eng.inverse_logdet(y, c)
    assert (xb - x).abs().max().item() <= 1e-4
    assert (fldj + ildj).abs().max().item() <= 1e-4
    _, lp_s = eng.sample_logprob(x, c)
    assert (eng.log_prob(y, c) - lp_s).abs().max().item() <= 2e-4
    assert torch.isfinite(y).all() and torch.isfinite(lp_s).all()


def test_condition_layouts_agree(dev):
  """uniform / per-sample / per-slice / ragged c_block forms give the same
  numbers, and tails + ragged batch sizes are handled."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=3, device=dev))
  for spl in (1, 2):
    eng.set_samples_per_lane(spl)
    _check_condition_layouts(eng, dev)


def _check_condition_layouts(eng, dev):
  S, Bs = 6, 768                       # 6 slices of 768 (multiple of the 256 / not of the 512 tile)
  x = eng.normal(5, S * Bs)
  ts = torch.linspace(0, 1, S, device=dev)
  y_sl, lp_sl = eng.sample_logprob(x, ts)                              # c_block = 768
  y_ps, lp_ps = eng.sample_logprob(x, ts.repeat_interleave(Bs)[:, None])   # per sample
  assert torch.equal(y_sl, y_ps) and torch.equal(lp_sl, lp_ps)
  for s in range(S):
    y_u, lp_u = eng.sample_logprob(x[s * Bs:(s + 1) * Bs], ts[s:s + 1])
    assert torch.equal(y_u, y_sl[s * Bs:(s + 1) * Bs]) and torch.equal(lp_u, lp_sl[s * Bs:(s + 1) * Bs])
  # ragged: 5 slices of 100 (not a multiple of the tile) -> generic c_block path
  xr = x[:500]
  tr = torch.linspace(0.1, 0.9, 5, device=dev)
  y_r, lp_r = eng.sample_logprob(xr, tr)
  y_r2, lp_r2 = eng.sample_logprob(xr, tr.repeat_interleave(100))
  assert torch.equal(y_r, y_r2) and torch.equal(lp_r, lp_r2)
  # B = 1 and B = 257 (partial tiles)
  for B in (1, 257):
    yb, lpb = eng.sample_logprob(x[:B], ts[:1])
    assert torch.equal(yb, y_sl[:B]) and torch.equal(lpb, lp_sl[:B])


def test_empty_batch_and_errors(dev):
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  from cnf_ot_amd._capi import CnfError
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev)
  with pytest.raises(CnfError):      # params not set yet
    eng.log_prob(torch.zeros(4, 2, device=dev), torch.zeros(1, device=dev))
  eng.load(Params.zeros(cfg, dev))
  y, lp = eng.sample_logprob(torch.zeros(0, 2, device=dev), torch.zeros(1, device=dev))
  assert y.shape == (0, 2) and lp.shape == (0,)
  with pytest.raises(ValueError):
    eng.log_prob(torch.zeros(4, 3, device=dev), torch.zeros(1, device=dev))
  with pytest.raises(ValueError):
    eng.log_prob(torch.zeros(4, 2, device=dev), torch.zeros(3, device=dev))
  with pytest.raises(CnfError):
    FlowEngine(FlowConfig(dim=2, hidden_size=17), dev)


def test_philox_normals_match_oracle_stream(dev):
  import oracle
  from cnf_ot_amd import FlowConfig, FlowEngine
  eng = FlowEngine(FlowConfig(dim=2), dev)
  z = eng.normal(42, 50001).cpu().numpy().reshape(-1)
  ref = oracle.normal(42, 0, z.size)
  assert np.abs(z - ref).max() <= 2e-5
  # element-indexed: a shard that starts at sample 1001 reproduces the same values
  z2 = eng.normal(42, 3000, first_sample=1001).cpu().numpy().reshape(-1)
  assert np.array_equal(z2, z[2002:2002 + 6000])
  z3 = eng.normal((42, 1001), 3000).cpu().numpy().reshape(-1)
  assert np.array_equal(z3, z2)
  # D=3: shards that do not start on a 4-element Philox block
  eng3 = FlowEngine(FlowConfig(dim=3), dev)
  w = eng3.normal(9, 1000).cpu().numpy().reshape(-1)
  assert np.abs(w - oracle.normal(9, 0, 3000)).max() <= 2e-5
  assert np.array_equal(eng3.normal(9, 100, first_sample=333).cpu().numpy().reshape(-1), w[999:1299])


def test_reference_call_surface(dev):
  """The calls cnf_ot/mfc/applications.py makes, verbatim in shape."""
  import oracle
  from cnf_ot_amd import RQSFlow, Params
  model = RQSFlow(event_shape=(2,), num_layers=2, hidden_sizes=[16] * 2, num_bins=5, periodized=False)
  params = model.init(0, torch.zeros(1, 2), torch.zeros(1))
  assert params.flat.is_cuda
  B = 4096
  # applications.py:226-239: same seed => same base noise at two conditions
  cond1 = torch.ones(B, 1, device=dev) * 0.495
  r1 = model.apply.sample(params, seed=7, sample_shape=(B,), cond=cond1)
  r2 = model.apply.sample(params, seed=7, sample_shape=(B,), cond=cond1 + 0.01)
  assert r1.shape == (B, 2) and torch.equal(r1, r2)          # identity flow ignores c
  # applications.py:153-158
  s, lp = model.apply.sample_and_log_prob(params, cond=cond1, seed=7, sample_shape=(B,))
  assert torch.equal(s, r1) and lp.shape == (B,)
  # applications.py:85: log_prob(params, samples, cond=ones(1)*c)
  lp2 = model.apply.log_prob(params, s, cond=torch.ones(1, device=dev) * 0.495)
  ref = (-0.5 * s.double() ** 2 - 0.5 * np.log(2 * np.pi)).sum(1)
  assert (lp2.double() - ref).abs().max().item() <= 1e-5
  assert (lp.double() - ref).abs().max().item() <= 1e-5
  # utils.py:619,627: forward / inverse
  p2 = Params.random(model.cfg, 0.2, seed=1, device=dev)
  y = model.apply.forward(p2, s, torch.ones(1, device=dev) * 0.3)
  xb = model.apply.inverse(p2, y, torch.ones(1, device=dev) * 0.3)
  assert (xb - s).abs().max().item() <= 5e-5
  ocfg = oracle.OracleConfig(D=2)
  y_ref, _ = oracle.forward_logdet(ocfg, p2.flat.cpu().double().numpy(), s.cpu().double().numpy(), [0.3])
  assert _err(y, y_ref).max() <= TOL_Y


@pytest.mark.parametrize("D", [1, 2, 3])
def test_periodized_flow_vs_oracle(dev, D):
  """RQSFlow(periodized=True) (flows.py:58-64,127-131; no reference call site passes it): sin / cos features of
  the conditioner input, splines on [0, 2 pi] with circular boundary slopes.  float32 kernels against the float64
  oracle at the plain-fp32 bars, the float64 kernels at 1e-11, both directions, points inside and outside the
  range; the loss / gradient entry points refuse the configuration."""
  import oracle
  from cnf_ot_amd import FlowConfig, FlowEngine, RQSFlow, Params
  fcfg = FlowConfig.torus(dim=D)
  # (the C ABI carries the range as float32: the oracle gets the same rounded 2 pi, 1.7e-7 above the double)
  ocfg = oracle.OracleConfig(D=D, range_min=0.0, range_max=float(np.float32(2 * np.pi)), periodized=True)
  n = oracle.param_count(ocfg)
  assert n == fcfg.param_count()
  rng = np.random.default_rng(300 + D)
  params = rng.normal(0, 0.3, n).astype(np.float32).astype(np.float64)
  B = 5000
  x = rng.uniform(0.0, 2 * np.pi, size=(B, D)).astype(np.float32)
  x[0] = -0.5; x[1] = 2 * np.pi + 0.25; x[2] = 0.0          # linear tails and the boundary itself
  ts = np.array([0.3, 4.1])                                   # two slices
  c_host = np.repeat(ts, B // 2)
  eng = _engine(fcfg, params, dev)
  y, fldj = eng.forward_logdet(_t(x, dev), _t(ts, dev))
  y_ref, fldj_ref = oracle.forward_logdet(ocfg, params, x.astype(np.float64), c_host)
  print(f"\n[periodized D={D}] forward max|dy|={_err(y, y_ref).max():.2e} max|dlogdet|={_err(fldj, fldj_ref).max():.2e}")
  assert _err(y, y_ref).max() <= TOL_Y and _err(fldj, fldj_ref).max() <= TOL_LD * max(1, D)
  y_in = y_ref.astype(np.float32)
  xb, ildj = eng.inverse_logdet(_t(y_in, dev), _t(ts, dev))
  xb_ref, ildj_ref = oracle.inverse_logdet(ocfg, params, y_in.astype(np.float64), c_host)
  assert _err(xb, xb_ref).max() <= TOL_Y and _err(ildj, ildj_ref).max() <= TOL_LD * max(1, D)
  lp = eng.log_prob(_t(y_in, dev), _t(ts, dev))
  lp_ref = oracle.log_prob(ocfg, params, y_in.astype(np.float64), c_host)
  assert _err(lp, lp_ref).max() <= TOL_LP_FP32_MAX * max(1, D)
  # float64 kernels
  yd, ld = eng.forward_logdet(torch.from_numpy(x.astype(np.float64)).to(dev), torch.from_numpy(ts).to(dev))
  assert yd.dtype == torch.float64
  assert _err(yd, y_ref).max() <= 1e-11 and _err(ld, fldj_ref).max() <= 1e-10
  # the torus conditions: y stays in the range, the conditioner is 2 pi-periodic in c
  inside = (x > 0).all(1) & (x < 2 * np.pi).all(1)
  yi = y[torch.from_numpy(inside).to(dev)]
  assert yi.min().item() >= 0.0 and yi.max().item() <= 2 * np.pi + 1e-6
  if D >= 2:
    y2, _ = eng.forward_logdet(_t(x, dev), _t(ts + 2 * np.pi, dev))
    assert (y2 - y).abs().max().item() <= 5e-5
  # the model object: init is the identity, sampling and log_prob agree with each other
  model = RQSFlow(event_shape=(D,), num_layers=2, hidden_sizes=[16, 16], num_bins=5, periodized=True)
  p0 = model.init(0)
  s, lps = model.apply.sample_and_log_prob(p0, cond=torch.full((64, 1), 0.2, device=dev), seed=3, sample_shape=(64,))
  lpv = model.apply.log_prob(p0, s, cond=torch.tensor([0.2], device=dev))
  assert (lps - lpv).abs().max().item() <= 1e-4
  # losses / gradients: refused, loudly
  from cnf_ot_amd import applications as app
  with pytest.raises((RuntimeError, NotImplementedError)):
    app.kinetic_loss_fn(model, D, 0.01, Params.random(model.cfg, 0.1, seed=1, device=dev), 0.5, 7, 256)


def test_wide_event_dimension(dev):
  """Large D: the LDS tile (2 x D x 256 or 512 floats) needs the > 64 KB opt-in
  and, beyond that, one sample per lane."""
  import oracle
  for D, B in ((24, 700), (40, 300)):
    fcfg, ocfg = _cfg_pair(D=D)
    rng = np.random.default_rng(D)
    params = rng.normal(0, 0.05, oracle.param_count(ocfg)).astype(np.float32).astype(np.float64)
    noise = rng.normal(size=(B, D)).astype(np.float32)
    eng = _engine(fcfg, params, dev)
    for spl in (2, 1):
      eng.set_samples_per_lane(spl)
      y, lp = eng.sample_logprob(_t(noise, dev), torch.tensor([0.4], device=dev))
      y_ref, lp_ref = oracle.sample_logprob(ocfg, params, noise.astype(np.float64), [0.4])
      assert _err(y, y_ref).max() <= TOL_Y and _err(lp, lp_ref).max() <= 5e-5
    xb, _ = eng.inverse_logdet(y, torch.tensor([0.4], device=dev))
    assert (xb.cpu() - torch.from_numpy(noise)).abs().max().item() <= 1e-4


@pytest.mark.parametrize("name", sorted(GOLDEN) + ["flow_d2_wild.npz"])
def test_float64_kernels_match_oracle_to_1e12(golden_dir, dev, name):
  """The float64 instantiation (the reference's dtype, solvers.py:23): every
  golden vector, including the ill-conditioned scale-0.5 `wild` set, to
  float64 round-off."""
  kw = GOLDEN.get(name, dict(D=2))
  fcfg, _ = _cfg_pair(**kw)
  g = np.load(os.path.join(golden_dir, name))
  eng = _engine(fcfg, g["params"], dev)
  d64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dev)
  # the wild set has local slopes up to e^16 per layer: two float64 evaluations that differ by one
  # ulp in an intermediate (ocml vs glibc exp, fma contraction) land 1e-5 apart on its worst samples
  tol = 1e-11 if "wild" not in name else 1e-4
  worst = 0.0
  for tag, c in (("u", g["c_uniform"]), ("p", g["c_per"])):
    y, fldj = eng.forward_logdet(d64(g["noise"]), d64(c))
    assert y.dtype == torch.float64
    _, lp = eng.sample_logprob(d64(g["noise"]), d64(c))
    xb, ildj = eng.inverse_logdet(d64(g[f"y_{tag}"]), d64(c))
    lpd = eng.log_prob(d64(g[f"y_{tag}"]), d64(c))
    for got, want in ((y, g[f"y_{tag}"]), (fldj, g[f"fldj_{tag}"]), (lp, g[f"lp_sample_{tag}"]),
                      (xb, g[f"x_back_{tag}"]), (ildj, g[f"ildj_{tag}"]), (lpd, g[f"lp_{tag}"])):
      e = np.abs(got.cpu().numpy() - want) / np.maximum(1.0, np.abs(want))
      worst = max(worst, e.max())
  print(f"\n[f64 {name}] worst relative-or-absolute error {worst:.2e}")
  assert worst <= tol


def test_threefry_normals_match_oracle(dev):
  """cnf_fill_normal_threefry (the JAX-style draw) == the C restatement, as float64 bit for bit up to erfinv's last
  bits and as float32; sharded calls reproduce the whole draw; model.apply.sample(rng="threefry") uses it."""
  import oracle
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, RQSFlow
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.zeros(cfg, dev))
  n = 50001
  want = oracle.normal_threefry((7, 42), n * 2).reshape(n, 2)
  got64 = eng.normal_threefry(np.array([7, 42], dtype=np.uint32), n, dtype=torch.float64)
  assert np.abs(got64.cpu().numpy() - want).max() <= 1e-11      # two erfinv implementations (ocml, Newton on libm erf)
  got32 = eng.normal_threefry(np.array([7, 42], dtype=np.uint32), n)
  assert np.abs(got32.cpu().numpy().astype(np.float64) - want).max() <= 5e-7
  a = eng.normal_threefry((7 << 32) | 42, 1000, first_sample=123, total_samples=n, dtype=torch.float64)
  assert torch.equal(a, got64[123:1123])
  model = RQSFlow(event_shape=(2,), num_layers=2, hidden_sizes=[16, 16], num_bins=5, rng="threefry")
  y = model.apply.sample(Params.zeros(cfg, dev), cond=torch.tensor([0.5], device=dev),
                         seed=np.array([7, 42], dtype=np.uint32), sample_shape=(n,))
  assert (y - got32).abs().max().item() <= 1e-6      # identity flow: the samples are the base draw
