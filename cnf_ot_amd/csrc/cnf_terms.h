// cnf_terms.h -- the per-sample math of the loss terms (applications.py), one definition each: the forward loss
// kernels (cnf_flow.hip), the fused backward (cnf_grad.hip) and the term epilogues (cnf_step.hip) all call these; and
// of the importance-sampling target (cnf_importance.hip).
//
// Coordinates are read through an accessor `x(d)` (an LDS column, a GROW-strided tile column, a row-major point,
// or a sample pair held in registers); T is the lane type (float, v2f, double).  Formulas that call a transcendental
// take the Math<FAST> policy of their caller: the forward loss kernels pass theirs, the backward passes false.
#pragma once
#include "cnf_device.h"
#include "../../include/cnf_ot_amd.h"

namespace cnf {

constexpr double HALF_LOG_2PI = 0.91893853320467274178;

// accessor of a column of TS-strided rows (lds_get): coordinate d of this lane's sample(s)
template <class T>
__device__ __forceinline__ auto lds_col(const typename Lanes<T>::real* col, int TS) {
  return [=](int d) { return lds_get<T>(col, d, TS); };
}

// log N(x; 0, I) = -|x|^2 / 2 - D log sqrt(2 pi): the base distribution's log-density
template <class T, class X>
__device__ __forceinline__ T base_logprob(X x, int D) {
  typedef typename Lanes<T>::real R;
  T b = splat<T>(0.0f);
  for (int d = 0; d < D; ++d) { const T v = x(d); b = vfma(v * (R)-0.5, v, b); }
  return b - (R)(D * HALF_LOG_2PI);
}

template <class T, class X>
__device__ __forceinline__ T sq_norm(X x, int D) {
  T s = splat<T>(0.0f);
  for (int d = 0; d < D; ++d) { const T v = x(d); s = vfma(v, v, s); }
  return s;
}

// Potential V(r) of potential_loss_fn (applications.py:181-191) and its gradient; `sm`, `sp` are |r - a|^2 and
// |r + a|^2 (double well only).
template <class T>
struct Potential {
  T v, sm, sp;
  int subtype;
  float a;
  // dV / dr_e at the coordinate r = r_e
  template <class C> __device__ __forceinline__ C grad(C r) const {
    if (subtype == CNF_POT_DOUBLE_WELL) return ((r - a) * sp + (r + a) * sm) * 0.5f;
    if (subtype == CNF_POT_OBSTACLE) return r * -v;
    return r;
  }
};

// from the sums |r|^2, |r - a|^2, |r + a|^2
template <bool FAST, class T>
__device__ __forceinline__ Potential<T> potential_of_sums(T s2, T sm, T sp, int subtype, float a) {
  Potential<T> p{splat<T>(0.0f), sm, sp, subtype, a};
  if (subtype == CNF_POT_DOUBLE_WELL) p.v = sm * sp * 0.25f;                  // (|r-a1| |r+a1| / 2)^2, :184-188
  else if (subtype == CNF_POT_OBSTACLE) p.v = Math<FAST>::exp(s2 * -0.5f) * 50.0f;   // :190-191
  else p.v = s2 * 0.5f;                                                       // quadratic, :181-182
  return p;
}

template <bool FAST, class T, class X>
__device__ __forceinline__ Potential<T> potential(X x, int D, int subtype, float a) {
  T s2 = splat<T>(0.0f), sm = splat<T>(0.0f), sp = splat<T>(0.0f);
  for (int d = 0; d < D; ++d) {      // (all three sums: no branch per coordinate)
    const T r = x(d);
    s2 = vfma(r, r, s2);
    sm = vfma(r - a, r - a, sm);
    sp = vfma(r + a, r + a, sp);
  }
  return potential_of_sums<FAST>(s2, sm, sp, subtype, a);
}

// A 2-D point held as one v2f (the dim-2 epilogue): the differences packed, shared with Potential::grad(x)
template <bool FAST>
__device__ __forceinline__ Potential<float> potential(v2f x, int subtype, float a) {
  const v2f xm = x - a, xp = x + a;
  return potential_of_sums<FAST>(fmaf(x.x, x.x, x.y * x.y), fmaf(xm.x, xm.x, xm.y * xm.y), fmaf(xp.x, xp.x, xp.y * xp.y),
                                 subtype, a);
}

// The reverse-KL target log(N(y;0,vs I) ws + N(y;0,vt I) wt) at condition t as a log-sum-exp (applications.py:136-163),
// and g = -(d/dy_e) of it / y_e.  FAST folds -1/(2 v) into one constant; otherwise the exponent divides by v.
// The weights enter the exponents as log |w| and their signs multiply afterwards, so the maximum is over the WEIGHTED
// exponents and the larger term is exp(0): a zero weight (ws at t == T, wt at t == 0) is -inf, and its component drops
// out of the maximum and of the sum however far its exponent lies above the other's.
template <class T> struct RklMix { T logmix, g; };

template <bool FAST, class T, class X>
__device__ __forceinline__ RklMix<T> rkl_mixture(X y, int D, float t, float Tt, float beta) {
  using M = Math<FAST>;
  const T s2 = sq_norm<T>(y, D);
  const float vs = 2.0f / beta * (Tt + 1.0f), vt = 2.0f / beta;
  const float ws = (Tt - t) / Tt, wt = t / Tt;
  const float ss = copysignf(1.0f, ws), st = copysignf(1.0f, wt);
  const float ls = -0.5f * D * logf(6.283185307179586f * vs) + logf(fabsf(ws));
  const float lt = -0.5f * D * logf(6.283185307179586f * vt) + logf(fabsf(wt));
  T as, at;
  if constexpr (FAST) {
    as = vfma(s2, splat<T>(-0.5f / vs), splat<T>(ls));
    at = vfma(s2, splat<T>(-0.5f / vt), splat<T>(lt));
  } else {
    as = s2 * -0.5f / vs + ls;
    at = s2 * -0.5f / vt + lt;
  }
  const T mx = vmax(as, at);
  const T es = M::exp(as - mx) * ss, et = M::exp(at - mx) * st;
  return RklMix<T>{mx + M::log(es + et), (es / vs + et / vt) / (es + et)};
}

// The importance-sampling target (CnfTargetSpec: a Gaussian mixture with a shared covariance shape, Sigma^-1 = W^T W,
// W lower triangular) at the point y, for a slice whose covariance is scale * Sigma:
//   log p(y) = logsumexp_m(log_weight_m - |W (y - mean_m)|^2 / (2 scale)) - D/2 log(2 pi scale) + log|det W|,
// a log-sum-exp with the maximum taken first (a component of weight 0 is -inf and drops out), in float64 whatever the
// type of the point: the log-weights it enters reach thousands, where fp32 holds no more than 1e-4.  A non-finite
// point gives a non-finite result.
template <class X>
__device__ __forceinline__ double target_logprob(const CnfTargetSpec& tg, X y, int D, double scale) {
  const double half_inv = 0.5 / scale;
  double e[CNF_TARGET_MAX_COMP];
  double mx = -__builtin_huge_val();
#pragma unroll
  for (int m = 0; m < CNF_TARGET_MAX_COMP; ++m) {
    e[m] = -__builtin_huge_val();
    if (m < tg.n_comp) {
      double q = 0.0;
      for (int i = 0; i < D; ++i) {
        double r = 0.0;
        for (int j = 0; j <= i; ++j) r = fma(tg.W[i][j], (double)y(j) - tg.mean[m][j], r);
        q = fma(r, r, q);
      }
      e[m] = tg.log_weight[m] - q * half_inv;
      mx = fmax(mx, e[m]);
    }
  }
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < CNF_TARGET_MAX_COMP; ++m)
    if (m < tg.n_comp) s += exp(e[m] - mx);
  return mx + log(s) - D * (HALF_LOG_2PI + 0.5 * log(scale)) + tg.log_det_W;
}

// The density-error target of rmse_mc_loss_fn / rmse_grid_loss_fn (solvers.py:239-305) at condition t:
// p_mix(y; t) = (1 - t) N(y; 0, v0 I) + t N(y; 0, vT I), vT = exp(-2 a T) (v0 - 1/(2a)) + 1/(2a).  Linear space, not a
// log-sum-exp: the weights 1 - t and t are taken literally and may be <= 0 outside [0, 1].  The constants of the two
// Gaussians are made on the host and reach the kernels as arguments: computed in a kernel, the loop-invariant
// logarithms and exponential were hoisted into vector registers held across the flow passes of every term.
struct DensityMix { float e0, l0, eT, lT; };    // exponent factors -1/(2 v) and log-normalisations -D/2 log(2 pi v)

static inline DensityMix density_mix_consts(const CnfLossSpec& s, int D) {
  const double v0 = s.coef, h = 0.5 / s.a, vT = exp(-2.0 * s.a * s.T) * (v0 - h) + h;
  return DensityMix{(float)(-0.5 / v0), (float)(-0.5 * D * log(2.0 * M_PI * v0)), (float)(-0.5 / vT),
                    (float)(-0.5 * D * log(2.0 * M_PI * vT))};
}

template <bool FAST, class T, class X>
__device__ __forceinline__ T density_mixture(X y, int D, float t, const DensityMix& c) {
  using M = Math<FAST>;
  const T s2 = sq_norm<T>(y, D);
  const T p0 = M::exp(vfma(s2, splat<T>(c.e0), splat<T>(c.l0)));
  const T pT = M::exp(vfma(s2, splat<T>(c.eT), splat<T>(c.lT)));
  return p0 * (1.0f - t) + pT * t;
}

// The density-error residual (exp(lp) - p_mix)^2 of one sample, lp the flow's log-density at the point
template <bool FAST, class T>
__device__ __forceinline__ T density_l2_residual(T lp, T pmix) {
  const T d = Math<FAST>::exp(lp) - pmix;
  return d * d;
}

// The OU drift -a r (applications.py:310) is diagonal: coordinate e's drift and adjoint need nothing but coordinate e
template <class T> __device__ __forceinline__ T ou_drift(T r, float a) { return r * -a; }
__device__ __forceinline__ float ou_drift_adjoint(float ub, float a) { return a * ub; }

// Target drift of flow_matching_loss_fn, dimension i, at r; subtype -1: no drift (kinetic_with_score)
template <class T, class X>
__device__ __forceinline__ T drift_field(X r, int i, int subtype, float a) {
  switch (subtype) {
    case CNF_DRIFT_OU: return ou_drift(r(i), a);
    case CNF_DRIFT_SMILE: {                      // :353-357 (2-D)
      const T x = r(0), y = r(1);
      const T q = x * x + y * y - 4.0f;
      return (i == 0 ? -q * x : -q * y - (y - 1.0f) * 2.0f) * a;
    }
    case CNF_DRIFT_NONGRADIENT: {                // :358-363: -a r + 0.5 (r @ J), J=[[0,1],[-1,0]]
      const T x = r(0), y = r(1);
      return i == 0 ? x * -a - y * 0.5f : y * -a + x * 0.5f;
    }
    case CNF_DRIFT_LORENZ: {                     // :364-372, _r = 9
      const T x = r(0), y = r(1), z = r(2);
      if (i == 0) return (y - x) * 10.0f;
      if (i == 1) return x * 9.0f * (splat<T>(28.0f / 9.0f) - z) - y;
      return x * 9.0f * y - z * (8.0f / 3.0f);
    }
    default: return splat<T>(0.0f);
  }
}

// The adjoint of r through u = ... - drift(r): put(e, -sum_d ub_d d drift_d / d r_e) for every e < D (every
// coordinate is read before the first put)
template <class X, class U, class P>
__device__ __forceinline__ void drift_adjoint(X r, U ub, int D, int subtype, float a, P put) {
  switch (subtype) {
    case CNF_DRIFT_OU:
      for (int d = 0; d < D; ++d) put(d, ou_drift_adjoint(ub(d), a));
      break;
    case CNF_DRIFT_SMILE: {
      const float x = r(0), y = r(1), q = x * x + y * y - 4.0f, u0 = ub(0), u1 = ub(1);
      const float b0 = -(u0 * (-a * (q + 2.0f * x * x)) + u1 * (-a * 2.0f * x * y));
      const float b1 = -(u0 * (-a * 2.0f * x * y) + u1 * (-a * (q + 2.0f * y * y + 2.0f)));
      put(0, b0); put(1, b1);
      break;
    }
    case CNF_DRIFT_NONGRADIENT: {
      const float u0 = ub(0), u1 = ub(1);
      put(0, -(u0 * (-a) + u1 * 0.5f));
      put(1, -(u0 * (-0.5f) + u1 * (-a)));
      break;
    }
    case CNF_DRIFT_LORENZ: {
      const float x = r(0), y = r(1), z = r(2), u0 = ub(0), u1 = ub(1), u2 = ub(2);
      const float b0 = -(u0 * -10.0f + u1 * (28.0f - 9.0f * z) + u2 * 9.0f * y);
      const float b1 = -(u0 * 10.0f - u1 + u2 * 9.0f * x);
      const float b2 = -(u1 * (-9.0f * x) + u2 * (-8.0f / 3.0f));
      put(0, b0); put(1, b1); put(2, b2);
      break;
    }
    default:
      for (int d = 0; d < D; ++d) put(d, 0.0f);
  }
}

// The score terms' residual at one dimension, u = vel + coef score - drift (applications.py:245-374, the loss is c u^2),
// and the seed of its adjoints u_bar = 2 c u: vel_bar = u_bar, score_bar = coef u_bar, drift_bar = -u_bar
template <class T>
__device__ __forceinline__ T score_residual(T vel, T score, float coef, T drift) { return vfma(score, coef, vel) - drift; }
__device__ __forceinline__ float score_residual_bar(float u, float c) { return 2.0f * c * u; }

}  // namespace cnf
