// cnf_interaction_pairs.h -- what the pair passes over a point cloud share: the geometry of a workgroup, the column
// splits, the shape and spec checks and the spec as a kernel reads it.  Included by cnf_interaction.hip (the energy, the
// field and the force) and cnf_interaction_vjp.hip (the force's vector-Jacobian product); host code and constants only,
// so neither unit's kernels depend on the other's.
#pragma once
#include "cnf_common.h"

#include <algorithm>
#include <cmath>

namespace cnf {

constexpr int IA_THREADS = 256;                // lanes per workgroup
constexpr int IA_R = 2;                        // rows per lane
constexpr int IA_ROWS = IA_THREADS * IA_R;     // rows per workgroup
constexpr int IA_TILE = 64;                    // columns per float32 accumulation (divides IA_ROWS)
constexpr int IA_MAX_S = 64;
constexpr int IA_MAX_D = 14;
constexpr int IA_MAX_TERMS = CNF_INTERACTION_MAX_TERMS;
constexpr int IA_MAX_SPLIT = 64;
constexpr int64_t IA_TARGET_WGS = 2048;        // 256 CUs x 8 workgroups of 4 waves: a constant, not a device query
constexpr int64_t IA_MAX_N = int64_t(1) << 20;

// Term b of a pair at squared distance d2: e_b = exp2(nc_b a), a = d2 (Gaussian, nc_b = -log2 e / (2 bw_b^2)) or
// a = r (exponential, nc_b = -log2 e / bw_b); W += amp_b e_b; the force's weight += ga_b e_b with ga_b = -amp_b / bw_b^2
// (Gaussian: grad W = (x - y) sum_b ga_b e_b) or -amp_b / bw_b (exponential: grad W = (x - y) / r sum_b ga_b e_b)
struct IaCoef {
  float nc[IA_MAX_TERMS], amp[IA_MAX_TERMS], ga[IA_MAX_TERMS];
  int32_t nt;
};

inline int64_t row_groups(int64_t n) { return (n + IA_ROWS - 1) / IA_ROWS; }

// Column splits: enough workgroups for the chip, never more splits than the columns have tiles
inline int32_t ia_splits(int32_t S, int64_t rows, int64_t N) {
  const int64_t base = (int64_t)S * row_groups(rows);
  const int64_t want = (IA_TARGET_WGS + base - 1) / base;
  const int64_t tiles = (N + IA_TILE - 1) / IA_TILE;
  const int64_t most = std::max<int64_t>(1, std::min<int64_t>({want, tiles, (int64_t)IA_MAX_SPLIT}));
  const int64_t per = (tiles + most - 1) / most;          // tiles per split; then no split is empty
  return (int32_t)((tiles + per - 1) / per);
}

inline bool ia_shape_ok(int32_t S, int64_t N, int64_t Q, int32_t D) {
  return S >= 1 && S <= IA_MAX_S && N >= 2 && N <= IA_MAX_N && Q >= 0 && Q <= IA_MAX_N && D >= 1 && D <= IA_MAX_D;
}

inline bool finite_nonzero(float v) { return std::isfinite(v) && v != 0.0f; }

// The spec as the kernel reads it; false for what cnf_interaction refuses in one
inline bool ia_coef(const CnfInteractionSpec* spec, IaCoef* k) {
  *k = IaCoef{};
  if (spec->kind == CNF_INTERACTION_QUADRATIC) return finite_nonzero(spec->amp[0]);
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
