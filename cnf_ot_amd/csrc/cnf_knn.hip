// cnf_knn.hip -- the k nearest neighbours of every point of a cloud x, among the other points of x (the SELF block) and
// among the points of a second cloud y (the CROSS block), and the sums the Kozachenko-Leonenko entropy and the
// Leonenko-Pronzato-Savani cross entropy are made of: per block and rank j the sum of log dist_j over the rows whose
// j-th distance is > 0, and the number of rows where it is 0.  Model-free, like cnf_mmd.hip: KL in nats against a
// target that exists only as samples.
//
// ONE launch scans the two blocks of all S sets: the pair loop of cnf_mmd.hip.  A workgroup owns KNN_ROWS rows of one
// block and one of P column splits; a lane holds KNN_R rows in registers.  A column is the same for every lane of the
// wave: its address is built from blockIdx and loop counters only, so it comes through the scalar cache into SGPRs --
// no LDS, no barrier in the pair loop.  A row keeps its CAP best candidates (d2, index) in registers, sorted ascending;
// a column costs D subtractions, D multiply-adds and ONE compare against the list's last entry, and only where that
// compare succeeds the insertion runs, fully unrolled over the compile-time capacity CAP (4 or 16): no dynamic index,
// the list stays in VGPRs.  The diagonal of the self block is skipped by INDEX, and only in the tiles that meet the
// workgroup's own rows.
//
// Order: ascending by (d2 as computed, index).  Columns are scanned in ascending index and inserted on strict <, so of
// two equal d2 the smaller index stays first; the splits are merged in ascending split order with strict < again.  A
// list of capacity CAP >= k holds the k best as its first k entries, whatever CAP: rank j depends neither on k nor on
// the capacity compiled for it.
//
// Each (split, row) writes its first k candidates to the workspace (a slot no column filled: +inf, index -1);
// knn_merge_kernel merges a row's splits, writes dist = (float)sqrt((double)d2) and the indices, and leaves the merged
// d2 in the row's slot of split 0; knn_sum_kernel adds, per (set, block, rank), thread t's rows t, t + 256, ... and the
// threads' totals in a fixed tree: bitwise reproducible, and every workspace word read was written by this call.  P
// depends on (S, N, M) alone.
// What it shares with the other pair passes -- the workgroup's geometry, the split rule, a split's tiles, the finish's
// tree, the dispatch on D -- is cnf_pairs.h's.
#include "cnf_pairs.h"
#include "cnf_terms.h"

#include <math.h>

#include <algorithm>
#include <cmath>

// The distance is mmd_pair's: diff = x - c, d2 = diff_0^2, then one fmaf per further dimension, in dimension order
#pragma clang fp contract(off)

namespace cnf {
namespace {

// The geometry (cnf_pairs.h) this unit's kernels are written for: KNN_THREADS = 256; KNN_TILE = 64;
constexpr int KNN_THREADS = PAIR_THREADS, KNN_TILE = PAIR_TILE;
constexpr int KNN_R = 2;                         // rows per lane
constexpr int KNN_ROWS = KNN_THREADS * KNN_R;    // rows per workgroup
constexpr int KNN_CAP_SMALL = 4;                 // the compiled list capacities: k <= 4, and k <= CNF_KNN_MAX_K
constexpr int KNN_CAP_LARGE = 16;
static_assert(KNN_CAP_LARGE == CNF_KNN_MAX_K, "the large capacity is the largest k");
static_assert(KNN_THREADS == 256 && KNN_TILE == 64, "knn_kernel's tile geometry");
static_assert(KNN_ROWS % KNN_TILE == 0, "a tile lies inside a workgroup's rows or outside");

int64_t row_groups(int64_t n) { return pair_row_groups(n, KNN_ROWS); }
int32_t knn_blocks(int64_t M) { return M > 0 ? 2 : 1; }

// Column splits (pair_splits) over the longer side's tiles
int32_t knn_splits(int32_t S, int64_t N, int64_t M) {
  return pair_splits((int64_t)S * knn_blocks(M) * row_groups(N), pair_tiles(std::max(N, M)));
}

// Workspace: candidates [S][blocks][P][N][k], the d2 as floats, then the indices as int32 in the same layout
int64_t knn_entries(int32_t S, int64_t N, int64_t M, int32_t k) {
  return (int64_t)S * knn_blocks(M) * knn_splits(S, N, M) * N * k;
}

// (d2, idx) into an ascending list on strict <: an entry with an equal d2 that is already there stays in front
template <int CAP>
__device__ __forceinline__ void knn_insert(float (&ld)[CAP], int32_t (&li)[CAP], float d2, int32_t idx) {
#pragma unroll
  for (int j = CAP - 1; j >= 1; --j) {
    const bool up = d2 < ld[j - 1];              // the new entry lands before j - 1, which moves to j
    const bool here = !up && d2 < ld[j];
    ld[j] = up ? ld[j - 1] : here ? d2 : ld[j];
    li[j] = up ? li[j - 1] : here ? idx : li[j];
  }
  if (d2 < ld[0]) {
    ld[0] = d2;
    li[0] = idx;
  }
}

// n <= KNN_TILE columns starting at column c0 of `col` against the lane's rows
template <int D, int CAP, bool DIAG>
__device__ __forceinline__ void knn_tile(const float* __restrict__ col, int64_t c0, int n, int first_local,
                                         const float (&x)[KNN_R][D], float (&ld)[KNN_R][CAP], int32_t (&li)[KNN_R][CAP]) {
  const float* p = col + c0 * D;                 // wave-uniform: scalar loads
  auto column = [&](int j, const float* c) {
#pragma unroll
    for (int r = 0; r < KNN_R; ++r) {
      float diff[D];
#pragma unroll
      for (int d = 0; d < D; ++d) diff[d] = x[r][d] - c[d];
      float d2 = diff[0] * diff[0];
#pragma unroll
      for (int d = 1; d < D; ++d) d2 = fmaf(diff[d], diff[d], d2);
      bool take = d2 < ld[r][CAP - 1];
      if constexpr (DIAG) take = take && first_local + j != r * KNN_THREADS + (int)threadIdx.x;
      if (take) knn_insert<CAP>(ld[r], li[r], d2, (int32_t)c0 + j);
    }
  };
  // U columns are read before the first of them is used -- one wait per group, not one per column: the insertion
  // branches would otherwise keep every load next to its use.  At most 28 SGPRs of coordinates in flight.
  constexpr int U = D <= 2 ? 8 : D <= 4 ? 4 : 2;
  int j = 0;
  for (; j + U <= n; j += U) {
    float c[U * D];
#pragma unroll
    for (int e = 0; e < U * D; ++e) c[e] = p[j * D + e];
#pragma unroll
    for (int u = 0; u < U; ++u) column(j + u, c + u * D);
  }
  for (; j < n; ++j) {
    float c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = p[j * D + d];
    column(j, c);
  }
}

// grid (row groups x P, blocks x S): blockIdx.y = blocks s + block (0 self, 1 cross), blockIdx.x = row group * P + split
template <int D, int CAP>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          int64_t N, int64_t M, int32_t P, int32_t k,
                                                          float* __restrict__ cd, int32_t* __restrict__ ci) {
  const int nb = M > 0 ? 2 : 1;
  const int s = (int)blockIdx.y / nb, b = (int)blockIdx.y % nb;
  const int64_t rg = blockIdx.x / (unsigned)P;
  const int p = (int)(blockIdx.x % (unsigned)P);
  const int64_t row0 = rg * KNN_ROWS;
  const float* rows_p = x + (int64_t)s * N * D;
  const float* col = b == 0 ? rows_p : y + (int64_t)s * M * D;
  const int64_t n_col = b == 0 ? N : M;
  const auto [t0, t1] = pair_tile_range<int64_t>(n_col, P, p);     // (may be empty)

  float xr[KNN_R][D], ld[KNN_R][CAP];
  int32_t li[KNN_R][CAP];
#pragma unroll
  for (int r = 0; r < KNN_R; ++r) {
    const int64_t i = row0 + r * KNN_THREADS + (int64_t)threadIdx.x;
#pragma unroll
    for (int d = 0; d < D; ++d) xr[r][d] = i < N ? rows_p[i * D + d] : 0.0f;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      ld[r][j] = i < N ? INFINITY : -INFINITY;   // (a row past the end takes no candidate)
      li[r][j] = -1;
    }
  }
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t c0 = t * KNN_TILE;
    const int n = (int)(n_col - c0 < KNN_TILE ? n_col - c0 : KNN_TILE);
    if (b == 0 && c0 >= row0 && c0 < row0 + KNN_ROWS)
      knn_tile<D, CAP, true>(col, c0, n, (int)(c0 - row0), xr, ld, li);
    else
      knn_tile<D, CAP, false>(col, c0, n, 0, xr, ld, li);
  }
  // this (set, block, split)'s candidates: [N][k]
  const int64_t base = (((int64_t)blockIdx.y * P + p) * N) * k;
#pragma unroll
  for (int r = 0; r < KNN_R; ++r) {
    const int64_t i = row0 + r * KNN_THREADS + (int64_t)threadIdx.x;
    if (i < N) {
#pragma unroll
      for (int j = 0; j < CAP; ++j) {
        if (j < k) {
          cd[base + i * k + j] = ld[r][j];
          ci[base + i * k + j] = li[r][j];
        }
      }
    }
  }
}

// grid (row groups of KNN_THREADS, blocks x S): a thread merges its row's P candidate lists in ascending split order,
// writes the outputs that were asked for and leaves the merged d2 in the row's slot of split 0
__global__ __launch_bounds__(KNN_THREADS) void knn_merge_kernel(float* __restrict__ cd, const int32_t* __restrict__ ci,
                                                                int64_t N, int32_t P, int32_t k, int32_t nb,
                                                                float* __restrict__ dist_xx, int32_t* __restrict__ idx_xx,
                                                                float* __restrict__ dist_xy, int32_t* __restrict__ idx_xy) {
  const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
  if (i >= N) return;
  const int s = (int)blockIdx.y / nb, b = (int)blockIdx.y % nb;
  const int64_t split = N * k, base = (int64_t)blockIdx.y * P * split + i * k;
  float ld[KNN_CAP_LARGE];
  int32_t li[KNN_CAP_LARGE];
#pragma unroll
  for (int j = 0; j < KNN_CAP_LARGE; ++j) {
    ld[j] = j < k ? cd[base + j] : INFINITY;
    li[j] = j < k ? ci[base + j] : -1;
  }
  for (int p = 1; p < P; ++p) {
    for (int j = 0; j < k; ++j) {
      const float d2 = cd[base + p * split + j];
      if (!(d2 < ld[KNN_CAP_LARGE - 1])) break;  // (a split's list is ascending: nothing after this one enters either)
      knn_insert<KNN_CAP_LARGE>(ld, li, d2, ci[base + p * split + j]);
    }
  }
  float* dist = b == 0 ? dist_xx : dist_xy;
  int32_t* idx = b == 0 ? idx_xx : idx_xy;
  const int64_t o = ((int64_t)s * N + i) * k;
#pragma unroll
  for (int j = 0; j < KNN_CAP_LARGE; ++j) {
    if (j < k) {
      cd[base + j] = ld[j];
      if (dist) dist[o + j] = (float)sqrt((double)ld[j]);
      if (idx) idx[o + j] = li[j];
    }
  }
}

// grid (k, 2 S): sums[s][b][j] = (sum of log sqrt(d2_j) over the rows with d2_j > 0, rows with d2_j == 0), thread t
// taking rows t, t + 256, ... and the threads' totals meeting in a fixed tree.  Without a cross block: zeros there.
__global__ __launch_bounds__(KNN_THREADS) void knn_sum_kernel(const float* __restrict__ cd, int64_t N, int32_t P, int32_t k,
                                                              int32_t nb, double* __restrict__ sums) {
  __shared__ double s_log[KNN_THREADS], s_zero[KNN_THREADS];
  const int t = (int)threadIdx.x, j = (int)blockIdx.x;
  const int s = (int)blockIdx.y / 2, b = (int)blockIdx.y % 2;
  double* out = sums + (((int64_t)s * 2 + b) * k + j) * 2;
  if (b >= nb) {
    if (t < 2) out[t] = 0.0;
    return;
  }
  const float* row = cd + ((int64_t)s * nb + b) * P * N * k + j;
  double acc = 0.0, zeros = 0.0;
  for (int64_t i = t; i < N; i += KNN_THREADS) {
    const float d2 = row[i * k];
    if (d2 > 0.0f) acc += 0.5 * log((double)d2);
    else if (d2 == 0.0f) zeros += 1.0;
  }
  s_log[t] = acc;
  s_zero[t] = zeros;
  pair_block_tree<KNN_THREADS>(t, s_log, s_zero);
  if (t == 0) {
    out[0] = s_log[0];
    out[1] = s_zero[0];
  }
}

struct KnnLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *y;
  int64_t N, M;
  int32_t P, k;
  float* cd;
  int32_t* ci;
};

template <int D> void knn_launch_cap(const KnnLaunch& a) {
  if (a.k <= KNN_CAP_SMALL)
    hipLaunchKernelGGL((knn_kernel<D, KNN_CAP_SMALL>), a.grid, dim3(KNN_THREADS), 0, a.st, a.x, a.y, a.N, a.M, a.P, a.k, a.cd,
                       a.ci);
  else
    hipLaunchKernelGGL((knn_kernel<D, KNN_CAP_LARGE>), a.grid, dim3(KNN_THREADS), 0, a.st, a.x, a.y, a.N, a.M, a.P, a.k, a.cd,
                       a.ci);
}

// (the splits need no k; the call and the workspace query check it beside this)
bool knn_shape_ok(int32_t S, int64_t N, int64_t M, int32_t D) {
  return pair_dims_ok(S, D) && N >= 2 && N <= PAIR_MAX_N && M >= 0 && M <= PAIR_MAX_N;
}
bool knn_sizes_ok(int32_t S, int64_t N, int64_t M, int32_t D, int32_t k) {
  return knn_shape_ok(S, N, M, D) && k >= 1 && k <= CNF_KNN_MAX_K && N >= (int64_t)k + 1 && (M == 0 || M >= k);
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_knn_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t k, int64_t* bytes) {
  if (!bytes || !knn_sizes_ok(S, N, M, D, k)) return CNF_ERR_INVALID;
  *bytes = knn_entries(S, N, M, k) * (int64_t)(sizeof(float) + sizeof(int32_t));
  return CNF_OK;
}

extern "C" int cnf_knn_splits(int32_t S, int64_t N, int64_t M, int32_t D) {
  return knn_shape_ok(S, N, M, D) ? knn_splits(S, N, M) : CNF_ERR_INVALID;
}

extern "C" int cnf_knn(int32_t S, const float* x, int64_t N, const float* y, int64_t M, int32_t D, int32_t k, float* dist_xx,
                       int32_t* idx_xx, float* dist_xy, int32_t* idx_xy, double* sums, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  if (!x || !sums || !workspace || !knn_sizes_ok(S, N, M, D, k)) return CNF_ERR_INVALID;
  if ((y == nullptr) != (M == 0)) return CNF_ERR_INVALID;
  if (M == 0 && (dist_xy || idx_xy)) return CNF_ERR_INVALID;
  const int64_t entries = knn_entries(S, N, M, k);
  if (workspace_bytes < entries * (int64_t)(sizeof(float) + sizeof(int32_t))) return CNF_ERR_INVALID;
  KnnLaunch a{};
  const int32_t nb = knn_blocks(M);
  a.P = knn_splits(S, N, M);
  a.k = k;
  a.grid = dim3((unsigned)(row_groups(N) * a.P), (unsigned)(nb * S));
  a.st = (hipStream_t)stream;
  a.x = x; a.y = y; a.N = N; a.M = M;
  a.cd = (float*)workspace;
  a.ci = (int32_t*)workspace + entries;
  pair_dispatch_dim(D, [&](auto d) { knn_launch_cap<decltype(d)::value>(a); });
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((N + KNN_THREADS - 1) / KNN_THREADS), (unsigned)(nb * S)),
                     dim3(KNN_THREADS), 0, a.st, a.cd, (const int32_t*)a.ci, N, a.P, k, nb, dist_xx, idx_xx, dist_xy, idx_xy);
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  hipLaunchKernelGGL(knn_sum_kernel, dim3((unsigned)k, (unsigned)(2 * S)), dim3(KNN_THREADS), 0, a.st, (const float*)a.cd, N,
                     a.P, k, nb, sums);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
