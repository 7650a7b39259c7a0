// cnf_interaction_pairs.h -- what the interaction kernels share beyond cnf_pairs.h: their rows per lane, the column
// splits and the shape check in their arguments, the spec checks and the spec as a kernel reads it.  Included by
// cnf_interaction.hip (the energy, the field and the force), cnf_interaction_vjp.hip (the force's vector-Jacobian
// product) and cnf_stein.hip (fits_float and the shape check); host code and constants only, so no unit's kernels
// depend on another's.
#pragma once
#include "cnf_pairs.h"

#include <cmath>

namespace cnf {

// The geometry (cnf_pairs.h) the interaction kernels are written for: IA_THREADS = 256; IA_TILE = 64;
constexpr int IA_THREADS = PAIR_THREADS, IA_TILE = PAIR_TILE;
constexpr int IA_R = 2;                        // rows per lane
constexpr int IA_ROWS = IA_THREADS * IA_R;     // rows per workgroup
static_assert(IA_THREADS == 256 && IA_TILE == 64 && IA_ROWS % IA_TILE == 0, "the interaction kernels' tile geometry");
constexpr int IA_MAX_TERMS = CNF_INTERACTION_MAX_TERMS;

// Term b of a pair at squared distance d2: e_b = exp2(nc_b a), a = d2 (Gaussian, nc_b = -log2 e / (2 bw_b^2)) or
// a = r (exponential, nc_b = -log2 e / bw_b); W += amp_b e_b; the force's weight += ga_b e_b with ga_b = -amp_b / bw_b^2
// (Gaussian: grad W = (x - y) sum_b ga_b e_b) or -amp_b / bw_b (exponential: grad W = (x - y) / r sum_b ga_b e_b).
// The power kind, u = d2 + eps2 and L = log2 u: t_b = exp2(nc_b L) = u^(pw_b / 2 - 1) with nc_b = pw_b / 2 - 1; the
// force's weight += ga_b t_b with ga_b = the spec's amp_b; W = u sum_b amp_b t_b + cl L with amp_b = the spec's
// amp_b / pw_b, or 0 for a term with pw_b = 0, whose amp_b ln 2 / 2 joins IaPower's cl
struct IaCoef {
  float nc[IA_MAX_TERMS], amp[IA_MAX_TERMS], ga[IA_MAX_TERMS];
  int32_t nt;
};
// What the power kind reads beside IaCoef: the LAST kernel argument, so that the other kinds' arguments stay where they
// were and their instruction streams are the ones they had before this kind existed
struct IaPower {
  float eps2;
  float cl;                                    // the log terms' value coefficients, added: W += cl log2 u
};

inline int64_t row_groups(int64_t n) { return pair_row_groups(n, IA_ROWS); }

// Column splits (pair_splits) over the columns' tiles
inline int32_t ia_splits(int32_t S, int64_t rows, int64_t N) {
  return pair_splits((int64_t)S * row_groups(rows), pair_tiles(N));
}

inline bool ia_shape_ok(int32_t S, int64_t N, int64_t Q, int32_t D) {
  return pair_dims_ok(S, D) && N >= 2 && N <= PAIR_MAX_N && Q >= 0 && Q <= PAIR_MAX_N;
}

inline bool finite_nonzero(float v) { return std::isfinite(v) && v != 0.0f; }

inline bool fits_float(double v) { return std::isfinite(v) && std::fabs(v) <= 3.4028234663852886e38; }

// amp eps^e, with eps^0 = 1 also at eps = 0 (std::pow's rule) and +-inf where eps = 0 meets e < 0
inline double power_coef(double amp, double eps, double e) { return amp * std::pow(eps, e); }

// The power kind's spec as the kernel reads it; false for what cnf_interaction refuses in one.  hess: also the pair
// Hessian's coefficient amp (pw - 2) eps^(pw - 4), which cnf_interaction_vjp needs in float32's range (pw = 2 has none)
inline bool ia_coef_power(const CnfInteractionSpec* spec, IaCoef* k, IaPower* pk, bool hess) {
  if (spec->n_terms < 1 || spec->n_terms > IA_MAX_TERMS) return false;
  const double eps = (double)spec->bw[0];
  if (!std::isfinite(eps) || !(eps >= 0.0)) return false;
  k->nt = spec->n_terms;
  double cl = 0.0;
  pk->eps2 = (float)(eps * eps);
  if (!std::isfinite(pk->eps2)) return false;
  for (int b = 0; b < k->nt; ++b) {
    const double amp = (double)spec->amp[b], pw = (double)spec->pw[b];
    if (!finite_nonzero(spec->amp[b]) || !std::isfinite(pw) || !(std::fabs(pw) <= 16.0)) return false;
    if (eps == 0.0 && !(pw >= 2.0)) return false;
    const double value = pw == 0.0 ? amp * std::log(eps) : power_coef(amp / pw, eps, pw);
    if (!fits_float(power_coef(amp, eps, pw - 2.0)) || !fits_float(value)) return false;
    if (pw != 0.0 && !fits_float(power_coef(amp / pw, eps, pw - 2.0))) return false;   // (the value's sum before its factor u)
    if (hess && pw != 2.0 && !fits_float(power_coef(amp * (pw - 2.0), eps, pw - 4.0))) return false;
    k->nc[b] = (float)(0.5 * pw - 1.0);
    k->amp[b] = (float)(pw == 0.0 ? 0.0 : amp / pw);
    k->ga[b] = spec->amp[b];
    if (pw == 0.0) cl += amp * 0.34657359027997264;
    if (!std::isfinite(k->amp[b])) return false;
  }
  pk->cl = (float)cl;
  return true;
}

// The spec as the kernel reads it; false for what cnf_interaction refuses in one
inline bool ia_coef(const CnfInteractionSpec* spec, IaCoef* k, IaPower* pk) {
  *k = IaCoef{};
  *pk = IaPower{};
  if (spec->kind == CNF_INTERACTION_QUADRATIC) return finite_nonzero(spec->amp[0]);
  if (spec->kind == CNF_INTERACTION_POWER) return ia_coef_power(spec, k, pk, false);
  if (spec->kind != CNF_INTERACTION_GAUSSIAN && spec->kind != CNF_INTERACTION_EXPONENTIAL) return false;
  if (spec->n_terms < 1 || spec->n_terms > IA_MAX_TERMS) return false;
  k->nt = spec->n_terms;
  for (int b = 0; b < k->nt; ++b) {
    const double bw = (double)spec->bw[b], amp = (double)spec->amp[b];
    if (!finite_nonzero(spec->amp[b]) || !(bw > 0.0) || !std::isfinite(bw) || !(1.0 / (bw * bw) <= 3.0e38)) return false;
    const double ib = spec->kind == CNF_INTERACTION_GAUSSIAN ? 1.0 / (bw * bw) : 1.0 / bw;
    k->nc[b] = (float)(-1.4426950408889634 * (spec->kind == CNF_INTERACTION_GAUSSIAN ? 0.5 * ib : ib));
    k->amp[b] = spec->amp[b];
    k->ga[b] = (float)(-amp * ib);
    if (!std::isfinite(k->nc[b]) || !std::isfinite(k->ga[b])) return false;
  }
  return true;
}

}  // namespace cnf
