// cnf_mmd.hip -- the kernel two-sample statistic between two point clouds: the raw sums of the unbiased MMD^2
//   sxx = sum_{i != j} k(x_i, x_j),   syy = sum_{i != j} k(y_i, y_j),   sxy = sum_{i, j} k(x_i, y_j)
// for k(x, y) = sum_b exp(-|x - y|^2 / (2 bw_b^2)) (up to 8 bandwidths) or the energy kernel k = -|x - y|, and the
// gradient of MMD^2 = sxx / (N (N - 1)) + syy / (M (M - 1)) - 2 sxy / (N M) in every x_i.  Model-free, like
// cnf_fp_particles.hip: the samples a flow is compared with need no density.
//
// ONE launch covers the three blocks (xx, yy, xy) of all S sets.  A workgroup owns MMD_ROWS rows of one block and one
// of P column splits; a lane holds MMD_R rows in registers, so a column read serves MMD_R pairs per lane, and a row's
// sum and gradient are that lane's alone: no atomics.  A column is the same for every lane of the wave: its address is
// built from blockIdx and loop counters only, so the compiler reads it through the scalar cache into SGPRs, which the
// VALU subtracts from directly -- no LDS, no barrier in the pair loop.  Distances come from coordinate differences
// (|x|^2 + |y|^2 - 2 x.y cancels in float32 away from the origin).  The Gaussian costs one v_exp_f32 per bandwidth, the
// argument prescaled by -log2 e / (2 bw^2) on the host.  float32 accumulators live for one tile of MMD_TILE = 64
// columns and are then added into doubles.  The diagonal of xx and yy is skipped by INDEX, and only in the tiles that
// meet the workgroup's own rows.
//
// Each (split, row) writes one double (and D doubles of gradient) to the workspace; mmd_finish_kernel adds a row's
// splits in ascending order, then the rows in a fixed strided order and a fixed tree: bitwise reproducible, and every
// workspace word it reads was written by this call.  P depends on (S, N, M) alone.
// What it shares with the other pair passes -- the workgroup's geometry, the split rule, a split's tiles, the finish's
// tree, the dispatch on D -- is cnf_pairs.h's.
#include "cnf_pairs.h"
#include "cnf_terms.h"

#include <math.h>

#include <algorithm>
#include <cmath>

// Every fused multiply-add below is written as one (fmaf): with the compiler free to contract, the instantiations with
// and without the gradient rounded the same value differently
#pragma clang fp contract(off)

namespace cnf {
namespace {

// The geometry (cnf_pairs.h) this unit's kernels are written for: MMD_THREADS = 256; MMD_TILE = 64;
constexpr int MMD_THREADS = PAIR_THREADS, MMD_TILE = PAIR_TILE;
constexpr int MMD_R = 2;                         // rows per lane
constexpr int MMD_ROWS = MMD_THREADS * MMD_R;    // rows per workgroup
static_assert(MMD_THREADS == 256 && MMD_TILE == 64 && MMD_ROWS % MMD_TILE == 0, "mmd_kernel's tile geometry");
constexpr int MMD_MAX_BW = 8;
constexpr int64_t MMD_MAX_N = int64_t(1) << 24;
enum { MMD_XX = 0, MMD_YY = 1, MMD_XY = 2 };

// k_b = exp2(nc_b |x - y|^2), nc_b = -log2 e / (2 bw_b^2); 1 / bw_b^2 = MMD_IB_OVER_NC nc_b, so the gradient's weight
// sum_b k_b / bw_b^2 is accumulated as sum_b k_b nc_b and the constant joins the finish kernel's coefficients
struct MmdCoef {
  float nc[MMD_MAX_BW];
};
constexpr double MMD_IB_OVER_NC = -2.0 * 0.6931471805599453;

int64_t row_groups(int64_t n) { return pair_row_groups(n, MMD_ROWS); }

// Column splits (pair_splits) over the longer side's tiles
int32_t mmd_splits(int32_t S, int64_t N, int64_t M) {
  return pair_splits((int64_t)S * (2 * row_groups(N) + row_groups(M)), pair_tiles(std::max(N, M)));
}

// Workspace, in doubles: row partials [S][P][N | M | N] (xx, yy, xy), then gradient partials [S][2][P][N][D] (xx, xy)
int64_t mmd_row_doubles(int32_t S, int64_t N, int64_t M, int32_t P) { return (int64_t)S * P * (2 * N + M); }
int64_t mmd_workspace_doubles(int32_t S, int64_t N, int64_t M, int32_t D, bool grad) {
  const int32_t P = mmd_splits(S, N, M);
  return mmd_row_doubles(S, N, M, P) + (grad ? (int64_t)S * 2 * P * N * D : 0);
}

// One pair: the kernel value into ks, the gradient's (x - y) w into g.  `same`: the pair is the diagonal (i == j).
template <int D, int NB, bool GRAD, bool DIAG>
__device__ __forceinline__ void mmd_pair(const float (&x)[D], const float (&c)[D], const MmdCoef& k, bool same, float& ks,
                                         float (&g)[D]) {
  float diff[D];
#pragma unroll
  for (int d = 0; d < D; ++d) diff[d] = x[d] - c[d];
  float d2 = diff[0] * diff[0];
#pragma unroll
  for (int d = 1; d < D; ++d) d2 = fmaf(diff[d], diff[d], d2);
  float v, w = 0.0f;
  if constexpr (NB == 0) {                     // energy: k = -|x - y|, d k / d x = -(x - y) / |x - y| (0 at distance 0)
    const float inv = d2 > 1e-30f ? __builtin_amdgcn_rsqf(d2) : 0.0f;
    v = -d2 * inv;
    w = inv;
  } else {
    v = 0.0f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float e = __builtin_amdgcn_exp2f(d2 * k.nc[b]);
      v += e;
      if constexpr (GRAD) w = fmaf(e, k.nc[b], w);
    }
  }
  if constexpr (DIAG) v = same ? 0.0f : v;     // (the gradient's diagonal term is diff = 0 times w: nothing to mask)
  ks += v;
  if constexpr (GRAD) {
#pragma unroll
    for (int d = 0; d < D; ++d) g[d] = fmaf(diff[d], w, g[d]);
  }
}

// n <= MMD_TILE columns starting at column c0 of `col` against the lane's rows; the float32 tile sums into the doubles
template <int D, int NB, bool GRAD, bool DIAG>
__device__ __forceinline__ void mmd_tile(const float* __restrict__ col, int64_t c0, int n, int first_local,
                                         const float (&x)[MMD_R][D], const MmdCoef& k, double (&sum)[MMD_R],
                                         double (&gsum)[MMD_R][D]) {
  float ks[MMD_R], g[MMD_R][D];
#pragma unroll
  for (int r = 0; r < MMD_R; ++r) {
    ks[r] = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) g[r][d] = 0.0f;
  }
  const float* p = col + c0 * D;               // wave-uniform: scalar loads
  // columns in flight: at most 14 SGPRs of coordinates beside the 8 of coefficients (no SGPR spills at any D, NB)
  constexpr int U = D <= 3 ? 4 : D == 4 ? 3 : D <= 6 ? 2 : 1;
#pragma unroll U
  for (int j = 0; j < n; ++j) {
    float c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = p[j * D + d];
#pragma unroll
    for (int r = 0; r < MMD_R; ++r)
      mmd_pair<D, NB, GRAD, DIAG>(x[r], c, k, DIAG && first_local + j == r * MMD_THREADS + (int)threadIdx.x, ks[r], g[r]);
  }
#pragma unroll
  for (int r = 0; r < MMD_R; ++r) {
    sum[r] += (double)ks[r];
    if constexpr (GRAD) {
#pragma unroll
      for (int d = 0; d < D; ++d) gsum[r][d] += (double)g[r][d];
    }
  }
}

// The rows [row0, row0 + MMD_ROWS) of `rows_p` [n_rows, D] against the tiles [t0, t1) of `col` [n_col, D]
template <int D, int NB, bool GRAD>
__device__ __forceinline__ void mmd_block(const float* __restrict__ rows_p, int64_t n_rows, const float* __restrict__ col,
                                          int64_t n_col, int64_t row0, int64_t t0, int64_t t1, bool diag_block,
                                          const MmdCoef& k, double* __restrict__ part, double* __restrict__ gpart) {
  float x[MMD_R][D];
#pragma unroll
  for (int r = 0; r < MMD_R; ++r) {
    const int64_t i = row0 + r * MMD_THREADS + (int64_t)threadIdx.x;
#pragma unroll
    for (int d = 0; d < D; ++d) x[r][d] = i < n_rows ? rows_p[i * D + d] : 0.0f;
  }
  double sum[MMD_R], gsum[MMD_R][D];
#pragma unroll
  for (int r = 0; r < MMD_R; ++r) {
    sum[r] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) gsum[r][d] = 0.0;
  }
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t c0 = t * MMD_TILE;
    const int n = (int)(n_col - c0 < MMD_TILE ? n_col - c0 : MMD_TILE);
    // MMD_TILE divides MMD_ROWS and row0 is a multiple of MMD_ROWS: a tile lies inside the workgroup's rows or outside
    if (diag_block && c0 >= row0 && c0 < row0 + MMD_ROWS)
      mmd_tile<D, NB, GRAD, true>(col, c0, n, (int)(c0 - row0), x, k, sum, gsum);
    else
      mmd_tile<D, NB, GRAD, false>(col, c0, n, 0, x, k, sum, gsum);
  }
#pragma unroll
  for (int r = 0; r < MMD_R; ++r) {
    const int64_t i = row0 + r * MMD_THREADS + (int64_t)threadIdx.x;
    if (i < n_rows) {
      part[i] = sum[r];
      if constexpr (GRAD) {
#pragma unroll
        for (int d = 0; d < D; ++d) gpart[i * D + d] = gsum[r][d];
      }
    }
  }
}

// grid (row groups of the longer side x P, 3 S): blockIdx.y = 3 s + block, blockIdx.x = row group * P + split
template <int D, int NB, bool GRAD>
__global__ __launch_bounds__(MMD_THREADS) void mmd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          int64_t N, int64_t M, int32_t P, const MmdCoef k,
                                                          double* __restrict__ ws, int64_t grad_off) {
  const int s = (int)blockIdx.y / 3, b = (int)blockIdx.y % 3;
  const int64_t rg = blockIdx.x / (unsigned)P;
  const int p = (int)(blockIdx.x % (unsigned)P);
  const int64_t n_rows = b == MMD_YY ? M : N, n_col = b == MMD_XX ? N : M;
  const int64_t row0 = rg * MMD_ROWS;
  if (row0 >= n_rows) return;
  const float* rows_p = (b == MMD_YY ? y + (int64_t)s * M * D : x + (int64_t)s * N * D);
  const float* col = (b == MMD_XX ? x + (int64_t)s * N * D : y + (int64_t)s * M * D);
  const auto [t0, t1] = pair_tile_range<int64_t>(n_col, P, p);     // (may be empty: zeros)
  // this block's partials of set s: [P][n_rows]
  double* part = ws + (int64_t)s * P * (2 * N + M) + (b == MMD_XX ? 0 : b == MMD_YY ? P * N : P * (N + M)) + p * n_rows;
  if (GRAD && b != MMD_YY) {
    double* gpart = ws + grad_off + ((((int64_t)s * 2 + (b == MMD_XY)) * P + p) * N) * D;
    mmd_block<D, NB, GRAD>(rows_p, n_rows, col, n_col, row0, t0, t1, b == MMD_XX, k, part, gpart);
  } else {
    mmd_block<D, NB, false>(rows_p, n_rows, col, n_col, row0, t0, t1, b != MMD_XY, k, part, nullptr);
  }
}

// Workgroups [0, 3 S): sums[s][b] = the rows' totals, a row's splits added first and in ascending order, thread t
// taking rows t, t + 256, ... and the threads' totals meeting in a fixed tree.  The workgroups after them: xgrad.
__global__ __launch_bounds__(MMD_THREADS) void mmd_finish_kernel(const double* __restrict__ ws, int32_t S, int64_t N,
                                                                 int64_t M, int32_t D, int32_t P, int64_t grad_off,
                                                                 double cxx, double cxy, double* __restrict__ sums,
                                                                 float* __restrict__ xgrad) {
  __shared__ double s_acc[MMD_THREADS];
  const int t = (int)threadIdx.x;
  if ((int)blockIdx.x < 3 * S) {
    const int s = (int)blockIdx.x / 3, b = (int)blockIdx.x % 3;
    const int64_t n_rows = b == MMD_YY ? M : N;
    const double* part = ws + (int64_t)s * P * (2 * N + M) + (b == MMD_XX ? 0 : b == MMD_YY ? P * N : P * (N + M));
    double acc = 0.0;
    for (int64_t i = t; i < n_rows; i += MMD_THREADS) {
      double v = part[i];
      for (int p = 1; p < P; ++p) v += part[p * n_rows + i];
      acc += v;
    }
    const double total = pair_block_sum<MMD_THREADS>(s_acc, t, acc);
    if (t == 0) sums[blockIdx.x] = total;
    return;
  }
  if (!xgrad) return;
  const int64_t per_set = N * D;
  const int64_t e = ((int64_t)blockIdx.x - 3 * S) * MMD_THREADS + t;
  if (e >= (int64_t)S * per_set) return;
  const int64_t s = e / per_set, r = e % per_set;
  const double* gxx = ws + grad_off + (s * 2 * P) * per_set + r;
  const double* gxy = gxx + (int64_t)P * per_set;
  double a = gxx[0], c = gxy[0];
  for (int p = 1; p < P; ++p) {
    a += gxx[p * per_set];
    c += gxy[p * per_set];
  }
  xgrad[e] = (float)(cxx * a + cxy * c);
}

struct MmdLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *y;
  int64_t N, M;
  int32_t P;
  MmdCoef k;
  double* ws;
  int64_t grad_off;
  bool grad;
};

template <int D, int NB> void mmd_launch_grad(const MmdLaunch& a) {
  if (a.grad)
    hipLaunchKernelGGL((mmd_kernel<D, NB, true>), a.grid, dim3(MMD_THREADS), 0, a.st, a.x, a.y, a.N, a.M, a.P, a.k, a.ws,
                       a.grad_off);
  else
    hipLaunchKernelGGL((mmd_kernel<D, NB, false>), a.grid, dim3(MMD_THREADS), 0, a.st, a.x, a.y, a.N, a.M, a.P, a.k, a.ws,
                       a.grad_off);
}
// NB = 0: the energy kernel; 1 .. 8: that many bandwidths
template <int D, int NB = 0> void mmd_launch_bw(int nb, const MmdLaunch& a) {
  if (nb == NB) mmd_launch_grad<D, NB>(a);
  else if constexpr (NB < MMD_MAX_BW) mmd_launch_bw<D, NB + 1>(nb, a);
}

bool mmd_shape_ok(int32_t S, int64_t N, int64_t M, int32_t D) {
  return pair_dims_ok(S, D) && N >= 2 && M >= 2 && N <= MMD_MAX_N && M <= MMD_MAX_N;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_mmd_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t want_grad, int64_t* bytes) {
  if (!bytes || !mmd_shape_ok(S, N, M, D)) return CNF_ERR_INVALID;
  *bytes = mmd_workspace_doubles(S, N, M, D, want_grad != 0) * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_mmd_splits(int32_t S, int64_t N, int64_t M, int32_t D) {
  return mmd_shape_ok(S, N, M, D) ? mmd_splits(S, N, M) : CNF_ERR_INVALID;
}

extern "C" int cnf_mmd2(const CnfMmdSpec* spec, int32_t S, const float* x, int64_t N, const float* y, int64_t M, int32_t D,
                        double* sums, float* xgrad, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!spec || !x || !y || !sums || !workspace || !mmd_shape_ok(S, N, M, D)) return CNF_ERR_INVALID;
  if (spec->kind != CNF_MMD_GAUSSIAN && spec->kind != CNF_MMD_ENERGY) return CNF_ERR_INVALID;
  MmdLaunch a{};
  int nb = 0;
  if (spec->kind == CNF_MMD_GAUSSIAN) {
    nb = spec->n_bw;
    if (nb < 1 || nb > MMD_MAX_BW) return CNF_ERR_INVALID;
    for (int b = 0; b < nb; ++b) {
      const double bw = (double)spec->bw[b];
      if (!(bw > 0.0) || !std::isfinite(bw)) return CNF_ERR_INVALID;
      a.k.nc[b] = (float)(-1.4426950408889634 / (2.0 * bw * bw));
      if (!std::isfinite(a.k.nc[b]) || !(1.0 / (bw * bw) <= 3.0e38)) return CNF_ERR_INVALID;   // (1 / bw^2 left float32's range)
    }
  }
  const bool grad = xgrad != nullptr;
  if (workspace_bytes < mmd_workspace_doubles(S, N, M, D, grad) * (int64_t)sizeof(double)) return CNF_ERR_INVALID;
  a.P = mmd_splits(S, N, M);
  a.grid = dim3((unsigned)(row_groups(std::max(N, M)) * a.P), (unsigned)(3 * S));
  a.st = (hipStream_t)stream;
  a.x = x; a.y = y; a.N = N; a.M = M;
  a.ws = (double*)workspace;
  a.grad_off = mmd_row_doubles(S, N, M, a.P);
  a.grad = grad;
  pair_dispatch_dim(D, [&](auto d) { mmd_launch_bw<decltype(d)::value>(nb, a); });
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  const double dN = (double)N, dM = (double)M, gs = nb > 0 ? MMD_IB_OVER_NC : 1.0;
  const int64_t grad_wgs = grad ? ((int64_t)S * N * D + MMD_THREADS - 1) / MMD_THREADS : 0;
  hipLaunchKernelGGL(mmd_finish_kernel, dim3((unsigned)(3 * S + grad_wgs)), dim3(MMD_THREADS), 0, a.st,
                     (const double*)a.ws, S, N, M, D, a.P, a.grad_off, -2.0 * gs / (dN * (dN - 1.0)), 2.0 * gs / (dN * dM), sums,
                     xgrad);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
