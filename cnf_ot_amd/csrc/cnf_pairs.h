// cnf_pairs.h -- what the pair passes share: every row of a point set against every column, in column splits, with a
// fixed-order finish (cnf_mmd, cnf_mmd_perm, cnf_knn, cnf_sinkhorn, cnf_interaction, cnf_interaction_vjp, cnf_stein, cnf_stein_boot, cnf_kde).  The
// geometry of a workgroup, the column splits and a split's tiles, the block tree sum, the dispatch on the dimension and
// the shared part of the shape checks.  Host code, constants and __device__ __forceinline__ helpers only: no kernel, so
// no unit's kernels depend on another's.
#pragma once
#include "cnf_common.h"

#include <algorithm>
#include <type_traits>

namespace cnf {

constexpr int PAIR_THREADS = 256;                // lanes per workgroup
constexpr int PAIR_TILE = 64;                    // columns per float32 accumulation, and the unit a split is counted in
constexpr int PAIR_MAX_S = 64;
constexpr int PAIR_MAX_D = 14;
constexpr int PAIR_MAX_SPLIT = 64;
constexpr int64_t PAIR_TARGET_WGS = 2048;        // 256 CUs x 8 workgroups of 4 waves: a constant, not a device query
constexpr int64_t PAIR_MAX_N = int64_t(1) << 20;

// Workgroups that n rows take at `rows` rows each (PAIR_THREADS times the unit's rows per lane)
inline int64_t pair_row_groups(int64_t n, int rows) { return (n + rows - 1) / rows; }

// Column splits for a pass of base_wgs workgroups per split over `tiles` column tiles: enough workgroups for the chip,
// never more splits than there are tiles
inline int32_t pair_splits(int64_t base_wgs, int64_t tiles) {
  const int64_t want = (PAIR_TARGET_WGS + base_wgs - 1) / base_wgs;
  const int64_t most = std::max<int64_t>(1, std::min<int64_t>({want, tiles, (int64_t)PAIR_MAX_SPLIT}));
  const int64_t per = (tiles + most - 1) / most;          // tiles per split; then no split (of the longer side) is empty
  return (int32_t)((tiles + per - 1) / per);
}
inline int64_t pair_tiles(int64_t n) { return (n + PAIR_TILE - 1) / PAIR_TILE; }

// The set count and the dimension every pair pass takes; a unit's *_shape_ok adds its own bounds on the sizes
inline bool pair_dims_ok(int32_t S, int32_t D) { return S >= 1 && S <= PAIR_MAX_S && D >= 1 && D <= PAIR_MAX_D; }

inline int64_t up8(int64_t bytes) { return (bytes + 7) / 8 * 8; }

// f(std::integral_constant<int, D>) for the run-time dim in 1 .. PAIR_MAX_D; no call for any other
template <int D = 1, typename F> void pair_dispatch_dim(int dim, F&& f) {
  if (dim == D) f(std::integral_constant<int, D>{});
  else if constexpr (D < PAIR_MAX_D) pair_dispatch_dim<D + 1>(dim, f);
}

// The tiles [t0, t1) of split p of P over n_col columns, in the index type I the kernel counts in; a split past the
// shorter side's last tile is empty
template <typename I> struct PairTiles {
  I t0, t1;
};
template <typename I> __device__ __forceinline__ PairTiles<I> pair_tile_range(I n_col, int P, int p) {
  const I tiles = (n_col + PAIR_TILE - 1) / PAIR_TILE, per = (tiles + P - 1) / P;
  const I t0 = p * per < tiles ? p * per : tiles, t1 = t0 + per < tiles ? t0 + per : tiles;
  return {t0, t1};
}

// The threads' totals, already in s_acc[t] (one array or several side by side), meet in a fixed tree: s_acc[0]
template <int THREADS, typename... A> __device__ __forceinline__ void pair_block_tree(int t, A&... s_acc) {
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (t < o) ((s_acc[t] += s_acc[t + o]), ...);
    __syncthreads();
  }
}
template <int THREADS> __device__ __forceinline__ double pair_block_sum(double (&s_acc)[THREADS], int t, double v) {
  s_acc[t] = v;
  pair_block_tree<THREADS>(t, s_acc);
  return s_acc[0];
}

}  // namespace cnf
