"""The C ABI across the translation units of libcnf_ot_amd.so (no GPU needed): every entry point the Python side
binds is exported by the built library and declared in the public header, and the build lists only files that exist."""
import os
import re

import numpy as np

from cnf_ot_amd import _capi, build

REPO = os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), "..")


def test_every_bound_symbol_is_exported_and_declared():
  header = open(os.path.join(REPO, "include", "cnf_ot_amd.h")).read()
  lib = _capi.lib()
  assert len(_capi.SYMBOLS) > 0
  for name in _capi.SYMBOLS:
    assert hasattr(lib, name), f"{name}: not exported by {_capi.LIB_PATH}"
    assert re.search(r"\b" + re.escape(name) + r"\s*\(", header), f"{name}: not declared in include/cnf_ot_amd.h"


def test_model_free_step_entry_points_reject_bad_arguments_before_any_device_call():
  """The six entry points of cnf_step.hip check their arguments before they touch a device: every call below must come
  back CNF_ERR_INVALID on a machine without one (the same rejections tests/test_gpu_step_kernels.py asserts on the
  GPU).  The buffers are host memory that no rejected call may read or write: they keep their fill."""
  lib, INV = _capi.lib(), _capi.CNF_ERR_INVALID
  f32, f64, u64 = np.full(64, 7.25, np.float32), np.full(8, 7.25, np.float64), np.full(2, 7, np.uint64)
  p, d, st = f32.ctypes.data, f64.ctypes.data, u64.ctypes.data
  KIN, POT, NLP = _capi.TERM_KINETIC, _capi.TERM_POTENTIAL, _capi.TERM_NEG_LOGPROB
  hyper = (1e-3, 0.9, 0.999, 1e-8)
  bad = {}

  def adam(params=p, grad=p, mu=p, nu=p, n=8, step=1):
    return lib.cnf_adam_step(params, grad, mu, nu, n, *hyper, step, None)

  def adam_dev(params=p, grad=p, mu=p, nu=p, n=8, state=st):
    return lib.cnf_adam_step_dev(params, grad, mu, nu, n, *hyper, state, None)

  for f in (adam, adam_dev):
    for k in ("params", "grad", "mu", "nu"):
      bad[f"{f.__name__} {k}=NULL"] = f(**{k: None})
    bad[f"{f.__name__} n<0"] = f(n=-1)
  bad["adam step<1"] = adam(step=0)
  bad["adam_dev state=NULL"] = adam_dev(state=None)

  def wsum(v=d, w=d, n=4, out=d):
    return lib.cnf_weighted_sum(v, w, n, out, None)

  bad.update({"wsum v=NULL": wsum(v=None), "wsum w=NULL": wsum(w=None), "wsum out=NULL": wsum(out=None), "wsum n<0": wsum(n=-1)})

  def score(r=p, s=p, n=4, count=2, D=2, dt=0.1, drift=_capi.DRIFTS["ou"], sums=d, rb=p, sb=p):
    return lib.cnf_score_residual(r, s, n, count, D, dt, 0.5, drift, 1.0, 0.37, sums, rb, sb, None)

  bad.update({"score r=NULL": score(r=None), "score score=NULL": score(s=None), "score sums=NULL": score(sums=None),
              "score n<0": score(n=-1), "score count<1": score(count=0), "score D<1": score(D=0),
              "score dt=0": score(dt=0.0), "score dt<0": score(dt=-0.1), "score rbar alone": score(sb=None),
              "score sbar alone": score(rb=None), "score drift=7": score(drift=7), "score drift=-2": score(drift=-2),
              "score smile at D=3": score(D=3, drift=_capi.DRIFTS["smile"]),
              "score nongradient at D=3": score(D=3, drift=_capi.DRIFTS["nongradient"]),
              "score lorenz at D=2": score(D=2, drift=_capi.DRIFTS["lorenz"])})

  def term(kind=KIN, r=p, aux=p, n=4, count=2, D=2, subtype=0, p0=0.1, sums=d):
    return lib.cnf_term_residual(kind, r, aux, n, count, D, subtype, p0, 0.37, sums, p, p, None)

  for kind in (KIN, POT, NLP):
    bad.update({f"term {kind} r=NULL": term(kind, r=None), f"term {kind} sums=NULL": term(kind, sums=None),
                f"term {kind} n<0": term(kind, n=-1), f"term {kind} count<1": term(kind, count=0),
                f"term {kind} D<1": term(kind, D=0)})
  bad.update({"term kind=-1": term(-1), "term kind=1": term(_capi.TERM_KINETIC_SCORE), "term kind=4": term(_capi.TERM_REVERSE_KL),
              "term kind=6": term(_capi.TERM_DENSITY_L2), "term kinetic dt=0": term(KIN, p0=0.0),
              "term kinetic dt<0": term(KIN, p0=-0.1), "term potential subtype=-1": term(POT, subtype=-1),
              "term potential subtype=3": term(POT, subtype=3), "term neg_logprob aux=NULL": term(NLP, aux=None)})

  def rkl(y=p, lp=p, n=4, D=2, T=1.0, beta=10.0, out=d, yb=p, lb=p):
    return lib.cnf_rkl_residual(y, lp, n, D, 0.5, T, beta, 0.37, out, yb, lb, None)

  bad.update({"rkl y=NULL": rkl(y=None), "rkl lp=NULL": rkl(lp=None), "rkl sum=NULL": rkl(out=None), "rkl n<0": rkl(n=-1),
              "rkl D<1": rkl(D=0), "rkl T=0": rkl(T=0.0), "rkl beta=0": rkl(beta=0.0), "rkl ybar alone": rkl(lb=None),
              "rkl lpbar alone": rkl(yb=None)})

  assert len(bad) == 64
  wrong = {k: v for k, v in bad.items() if v != INV}
  assert not wrong, wrong
  assert (f32 == 7.25).all() and (f64 == 7.25).all() and (u64 == 7).all()


def test_the_build_lists_existing_files():
  assert len(set(build.SOURCES)) == len(build.SOURCES) and len(set(build.HEADERS)) == len(build.HEADERS)
  for f in build.SOURCES + build.HEADERS:
    assert os.path.isfile(os.path.join(build.SRC_DIR, f)), f
  on_disk = {f for f in os.listdir(build.SRC_DIR) if f.endswith((".hip", ".h"))}
  listed = {f for f in build.SOURCES + build.HEADERS if os.sep not in f}
  assert on_disk == listed, f"csrc/ and build.py disagree: {sorted(on_disk ^ listed)}"
