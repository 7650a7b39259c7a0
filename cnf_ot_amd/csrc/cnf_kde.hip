// cnf_kde.hip -- a Gaussian kernel density estimate of point sets in the log domain, with its score (include/cnf_ot_amd.h
// has the entry).  For sources x [S, N, D], queries q [S, Q, D] and bandwidths h_b, per (set, b, query i)
//   t_ij = -|q_i - x_j|^2 / (2 h_b^2),  m = max_j t_ij,  s = sum_j exp(t_ij - m),  w_ij = exp(t_ij - m) / s
//   log_rho = m + log s - log n_eff - (D / 2) log(2 pi h_b^2)      score_d = sum_j w_ij (x_jd - q_id) / h_b^2
// Composed in torch this is a Q x N matrix per bandwidth; linear-space sums (cnf_interaction's Gaussian kind) underflow in
// the tails, where the score is wanted most.
//
// Built as sk_block is (cnf_sinkhorn.hip): a workgroup owns KD_THREADS * R query rows of one set and one
// of P column splits; a lane keeps R rows in registers; a source column is the same for every lane of the wave -- its
// address comes from blockIdx and loop counters alone -- and arrives through the scalar cache.  d2 is formed from the
// coordinate differences.  What this shape allows beyond sk_block: every bandwidth shares d2_ij, and every bandwidth's
// maximum sits at the same j, the smallest d2.  So a row carries ONE running minimum dm of d2, and
//   s_b = sum_j exp2(nc_b (d2_ij - dm)),   a_bd = sum_j exp2(nc_b (d2_ij - dm)) (q_id - x_jd),   nc_b = -log2 e / (2 h_b^2)
// are rescaled by exp2(nc_b (dm_old - dm_new)) when the minimum moves, once per chunk of 4 columns (2 from D = 7).  One
// v_sub_f32 per pair serves all bandwidths; a bandwidth costs one v_mul_f32, one v_exp_f32, one v_add_f32 and (score) D
// v_fma_f32.  dm starts at FLT_MAX, not at infinity: a column that does not exist (the tail of a chunk), the pair i == j
// of the leave-one-out mode (skipped by INDEX: a duplicated point elsewhere still counts) and an overflowed distance all
// have d2 = inf, which gives exp2(-inf) = 0 against any finite dm and never a NaN of its own.  A NaN d2 does not move the
// minimum (v_min_f32 keeps the number) but makes its own term, and with it the row's sums, NaN.  The float32 sums live
// for one tile of KD_TILE columns and are then folded, rescaled, into doubles.  Each (split, row) writes (dm, s_b, a_bd);
// kd_merge_kernel brings a row's splits to their common minimum in ascending order and writes log_rho and score;
// kd_finish_kernel adds a (set, bandwidth)'s log_rho in a fixed strided order and a fixed tree.  No atomics, every loop
// counted: two calls give the same bits, and every workspace word read was written by this call.
// What it shares with the other pair passes -- the workgroup's geometry, the split rule, a split's tiles, the finish's
// tree, the dispatch on D -- is cnf_pairs.h's.
#include "cnf_host.h"
#include "cnf_pairs.h"

#include <math.h>

#include <cmath>

// Every fused multiply-add below is written as one (fmaf): with the compiler free to contract, the instantiations with
// and without the score could round the same (dm, s) differently
#pragma clang fp contract(off)

namespace cnf {
namespace {

// The geometry (cnf_pairs.h) this unit's kernels are written for: KD_THREADS = 256; KD_TILE = 64;
constexpr int KD_THREADS = PAIR_THREADS, KD_TILE = PAIR_TILE;
static_assert(KD_THREADS == 256 && KD_TILE == 64, "kd_pair_kernel's tile geometry");
constexpr int KD_MAX_BW = CNF_KDE_MAX_BW;
constexpr float KD_FAR = 3.4028234663852886e38f;          // where a row's minimum of d2 starts

// Rows per lane: a row holds NB (1 + D) float32 sums and as many doubles.  Two rows up to 16 of them: at 18 and 20 the
// compiler's report shows 248 VGPRs and more, into the AGPRs for (D, NB) = (4, 4) and (5, 3), one wave per SIMD
// (profiles/kde/resources_after.txt has every instantiation as built: 0 spills, 0 scratch)
constexpr int kd_rows(int D, int NB) { return NB * (1 + D) <= 16 ? 2 : 1; }
// Columns per chunk: the minimum moves, and the sums are rescaled, once per chunk (D U coordinates in SGPRs at a time)
constexpr int kd_chunk_cols(int D) { return D <= 6 ? 4 : 2; }

int64_t kd_row_groups(int64_t Q, int32_t D, int32_t NB) { return pair_row_groups(Q, KD_THREADS * kd_rows(D, NB)); }

// Column splits (pair_splits) over the sources' tiles.  The row groups are counted for two rows per lane whatever
// (D, n_bw) takes: the count does not depend on the bandwidths.
int32_t kd_splits(int32_t S, int64_t N, int64_t Q) {
  return pair_splits((int64_t)S * pair_row_groups(Q, 2 * KD_THREADS), pair_tiles(N));
}

// Workspace: doubles ps [S][P][NB][Q] (a partial's sums), doubles pa [S][P][NB][Q][D] (score: its weighted differences),
// floats lr [S][NB][Q] (log_rho where the caller asks for sums alone), floats pm [S][P][Q] (a partial's minimum of d2)
struct KdLayout {
  int64_t ps, pa, lr, pm, bytes;               // byte offsets (8-byte aligned) and the total
};
KdLayout kd_layout(int32_t S, int64_t Q, int32_t D, int32_t NB, int32_t P, bool score) {
  KdLayout l;
  l.ps = 0;
  l.pa = (int64_t)S * P * NB * Q * 8;
  l.lr = l.pa + (score ? (int64_t)S * P * NB * Q * D * 8 : 0);
  l.pm = l.lr + up8((int64_t)S * NB * Q * 4);
  l.bytes = l.pm + up8((int64_t)S * P * Q * 4);
  return l;
}

struct KdCoef {
  float nc[KD_MAX_BW];                         // -log2 e / (2 h_b^2)
};

// K <= U columns starting at `p` (column index j0) against the lane's rows.  TAIL: only the first k of the chunk's
// columns exist; the others are read from the last one and count as d2 = inf.  LOO: the column whose index is the
// row's counts as d2 = inf.
template <int D, int NB, bool SCORE, bool LOO, bool TAIL, int R>
__device__ __forceinline__ void kd_chunk_step(const float* __restrict__ p, int j0, int k, const KdCoef& kc,
                                              const int (&row)[R], const float (&x)[R][D], float (&dm)[R],
                                              float (&s)[R][NB], float (&a)[R][NB][SCORE ? D : 1]) {
  constexpr int U = kd_chunk_cols(D);
  float c[U][D];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = TAIL ? (u < k ? u : k - 1) : u;            // wave-uniform: scalar loads
#pragma unroll
    for (int d = 0; d < D; ++d) c[u][d] = p[j * D + d];
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float diff[U][D], d2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      diff[u][0] = x[r][0] - c[u][0];
      float v = diff[u][0] * diff[u][0];
#pragma unroll
      for (int d = 1; d < D; ++d) {
        diff[u][d] = x[r][d] - c[u][d];
        v = fmaf(diff[u][d], diff[u][d], v);
      }
      if (TAIL && u >= k) v = INFINITY;
      if (LOO && j0 + u == row[r]) v = INFINITY;             // the pair i == j, by index
      d2[u] = v;
    }
    float dn = dm[r];
#pragma unroll
    for (int u = 0; u < U; ++u) dn = fminf(dn, d2[u]);       // (a NaN d2 does not move the minimum)
    const float shift = dm[r] - dn;                          // >= 0, and finite: both are
    dm[r] = dn;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float f = __builtin_amdgcn_exp2f(kc.nc[b] * shift);
      s[r][b] *= f;
      if constexpr (SCORE) {
#pragma unroll
        for (int d = 0; d < D; ++d) a[r][b][d] *= f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float t = d2[u] - dn;                            // >= 0; inf for a pair that does not count
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float e = __builtin_amdgcn_exp2f(kc.nc[b] * t);
        s[r][b] += e;
        if constexpr (SCORE) {
#pragma unroll
          for (int d = 0; d < D; ++d) a[r][b][d] = fmaf(e, diff[u][d], a[r][b][d]);
        }
      }
    }
  }
}

// n <= KD_TILE columns starting at column c0
template <int D, int NB, bool SCORE, bool LOO, int R>
__device__ __forceinline__ void kd_tile(const float* __restrict__ col, int c0, int n, const KdCoef& kc, const int (&row)[R],
                                        const float (&x)[R][D], float (&dm)[R], float (&s)[R][NB],
                                        float (&a)[R][NB][SCORE ? D : 1]) {
  constexpr int U = kd_chunk_cols(D);
  const float* p = col + (int64_t)c0 * D;
  int j = 0;
  for (; j + U <= n; j += U) kd_chunk_step<D, NB, SCORE, LOO, false, R>(p + j * D, c0 + j, U, kc, row, x, dm, s, a);
  if (j < n) kd_chunk_step<D, NB, SCORE, LOO, true, R>(p + j * D, c0 + j, n - j, kc, row, x, dm, s, a);
}

struct KdPairArgs {
  float* pm;
  double *ps, *pa;
  int32_t N, Q, P, loo;
  KdCoef kc;
};

// grid (row groups x P, S): blockIdx.y = the set, blockIdx.x = row group * P + split
template <int D, int NB, bool SCORE>
__global__ __launch_bounds__(KD_THREADS) void kd_pair_kernel(const float* __restrict__ x, const float* __restrict__ q,
                                                             const KdPairArgs a) {
  constexpr int R = kd_rows(D, NB);
  constexpr int GD = SCORE ? D : 1;
  const int P = a.P, N = a.N, Q = a.Q;
  const int s = (int)blockIdx.y;
  const int rg = (int)(blockIdx.x / (unsigned)P);
  const int p = (int)(blockIdx.x % (unsigned)P);
  const int row0 = rg * (KD_THREADS * R);
  const float* col = x + (int64_t)s * N * D;
  const float* rows_p = q + (int64_t)s * Q * D;
  const auto [t0, t1] = pair_tile_range<int>(N, P, p);
  float xr[R][D];
  int row[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = row[r] = row0 + r * KD_THREADS + (int)threadIdx.x;
#pragma unroll
    for (int d = 0; d < D; ++d) xr[r][d] = i < Q ? rows_p[(int64_t)i * D + d] : 0.0f;
  }
  float dm[R];
  double sum[R][NB], asum[R][NB][GD];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    dm[r] = KD_FAR;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      sum[r][b] = 0.0;
#pragma unroll
      for (int d = 0; d < GD; ++d) asum[r][b][d] = 0.0;
    }
  }
  for (int t = t0; t < t1; ++t) {
    const int c0 = t * KD_TILE;
    const int n = N - c0 < KD_TILE ? N - c0 : KD_TILE;
    float dm0[R], sv[R][NB], av[R][NB][GD];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      dm0[r] = dm[r];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        sv[r][b] = 0.0f;
#pragma unroll
        for (int d = 0; d < GD; ++d) av[r][b][d] = 0.0f;
      }
    }
    // only the tiles that cross the workgroup's own rows can hold a pair i == j (wave-uniform)
    if (a.loo && c0 < row0 + KD_THREADS * R && c0 + n > row0)
      kd_tile<D, NB, SCORE, true, R>(col, c0, n, a.kc, row, xr, dm, sv, av);
    else
      kd_tile<D, NB, SCORE, false, R>(col, c0, n, a.kc, row, xr, dm, sv, av);
    // the tile's float32 sums into the doubles, which are first brought to the minimum the tile ended with
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float shift = dm0[r] - dm[r];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const double f = (double)__builtin_amdgcn_exp2f(a.kc.nc[b] * shift);
        sum[r][b] = sum[r][b] * f + (double)sv[r][b];
        if constexpr (SCORE) {
#pragma unroll
          for (int d = 0; d < D; ++d) asum[r][b][d] = asum[r][b][d] * f + (double)av[r][b][d];
        }
      }
    }
  }
  const int64_t part = (int64_t)s * P + p;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = row[r];
    if (i < Q) {
      a.pm[part * Q + i] = dm[r];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int64_t o = (part * NB + b) * Q + i;
        a.ps[o] = sum[r][b];
        if constexpr (SCORE) {
#pragma unroll
          for (int d = 0; d < D; ++d) a.pa[o * D + d] = asum[r][b][d];
        }
      }
    }
  }
}

struct KdMergeArgs {
  const float* pm;
  const double *ps, *pa;
  float *log_rho, *score;                      // [S, NB, Q] (the caller's or the workspace's) and [S, NB, Q, D] or null
  int32_t S, Q, D, NB, P;
  float nc[KD_MAX_BW];                         // as the pair kernel read them
  double inv_h2[KD_MAX_BW], cst[KD_MAX_BW];    // 1 / h_b^2 and -log n_eff - (D / 2) log(2 pi h_b^2)
};

// One thread per (set, query): the row's splits brought to their common minimum of d2 in ascending order,
//   sum_j exp2(nc_b d2_ij) = s_b exp2(nc_b dm)
__global__ __launch_bounds__(KD_THREADS) void kd_merge_kernel(const KdMergeArgs a) {
  const int64_t e = (int64_t)blockIdx.x * KD_THREADS + threadIdx.x;
  const int64_t Q = a.Q;
  if (e >= (int64_t)a.S * Q) return;
  const int64_t s = e / Q, i = e % Q;
  const int P = a.P, D = a.D, NB = a.NB;
  const float* pm = a.pm + s * P * Q + i;
  float dmin = pm[0];
  for (int p = 1; p < P; ++p) dmin = fminf(dmin, pm[p * Q]);
  for (int b = 0; b < NB; ++b) {
    const double nc = (double)a.nc[b];
    double sum = 0.0, A[PAIR_MAX_D];
#pragma unroll
    for (int d = 0; d < PAIR_MAX_D; ++d) A[d] = 0.0;
    for (int p = 0; p < P; ++p) {
      const int64_t o = ((s * P + p) * NB + b) * Q + i;
      const double f = exp2(nc * ((double)pm[p * Q] - (double)dmin));
      sum += a.ps[o] * f;
      if (a.score) {
#pragma unroll
        for (int d = 0; d < PAIR_MAX_D; ++d)
          if (d < D) A[d] += a.pa[o * D + d] * f;
      }
    }
    // every t_ij of the row is -inf in float32: no source within reach.  (A NaN sum is not that: it stays NaN.)
    const bool dead = sum == sum && (sum == 0.0 || a.nc[b] * dmin == -INFINITY);
    const int64_t o = (s * NB + b) * Q + i;
    const double lr = (nc * (double)dmin + log2(sum)) * 0.6931471805599453 + a.cst[b];
    a.log_rho[o] = dead ? -INFINITY : (float)lr;
    if (a.score) {
#pragma unroll
      for (int d = 0; d < PAIR_MAX_D; ++d)
        if (d < D) a.score[o * D + d] = dead ? 0.0f : (float)(-(A[d] / sum) * a.inv_h2[b]);   // (a holds q - x)
    }
  }
}

// Workgroup (s, b): sums[s, b] = sum_i log_rho[s, b, i], thread t taking rows t, t + 256, ... and the threads' totals
// meeting in a fixed tree
__global__ __launch_bounds__(KD_THREADS) void kd_finish_kernel(const float* __restrict__ log_rho, int64_t Q,
                                                               double* __restrict__ sums) {
  __shared__ double s_acc[KD_THREADS];
  const int t = (int)threadIdx.x;
  const float* lr = log_rho + (int64_t)blockIdx.x * Q;
  double acc = 0.0;
  for (int64_t i = t; i < Q; i += KD_THREADS) acc += (double)lr[i];
  const double total = pair_block_sum<KD_THREADS>(s_acc, t, acc);
  if (t == 0) sums[blockIdx.x] = total;
}

struct KdLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *q;
  KdPairArgs a;
  bool score;
};

template <int D, int NB> void kd_launch_score(const KdLaunch& l) {
  if (l.score) hipLaunchKernelGGL((kd_pair_kernel<D, NB, true>), l.grid, dim3(KD_THREADS), 0, l.st, l.x, l.q, l.a);
  else hipLaunchKernelGGL((kd_pair_kernel<D, NB, false>), l.grid, dim3(KD_THREADS), 0, l.st, l.x, l.q, l.a);
}
template <int D> void kd_launch_bw(int nb, const KdLaunch& l) {
  switch (nb) {
    case 1: kd_launch_score<D, 1>(l); break;
    case 2: kd_launch_score<D, 2>(l); break;
    case 3: kd_launch_score<D, 3>(l); break;
    default: kd_launch_score<D, 4>(l); break;                // (kd_shape_ok has refused every other count)
  }
}

bool kd_shape_ok(int32_t S, int64_t N, int64_t Q, int32_t D, int32_t n_bw) {
  return pair_dims_ok(S, D) && N >= 1 && N <= PAIR_MAX_N && Q >= 1 && Q <= PAIR_MAX_N && n_bw >= 1 && n_bw <= KD_MAX_BW;
}

// 1 / (2 h^2) as a normal float32, or 0 for a bandwidth cnf_kde refuses
double kd_inv_2h2(float bw) {
  const double h = (double)bw;
  if (!(h > 0.0) || !std::isfinite(h)) return 0.0;
  const double ib = 1.0 / (2.0 * h * h);
  return ib >= 1.1754943508222875e-38 && ib <= 3.4028234663852886e38 ? ib : 0.0;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_kde_workspace(int32_t S, int64_t N, int64_t Q, int32_t D, int32_t n_bw, int32_t want_score,
                                 int64_t* bytes) {
  if (!bytes || !kd_shape_ok(S, N, Q, D, n_bw)) return CNF_ERR_INVALID;
  *bytes = kd_layout(S, Q, D, n_bw, kd_splits(S, N, Q), want_score != 0).bytes;
  return CNF_OK;
}

extern "C" int cnf_kde_splits(int32_t S, int64_t N, int64_t Q, int32_t D) {
  return kd_shape_ok(S, N, Q, D, 1) ? kd_splits(S, N, Q) : CNF_ERR_INVALID;
}

extern "C" int cnf_kde(const CnfKdeSpec* spec, int32_t S, const float* x, int64_t N, const float* q, int64_t Q, int32_t D,
                       float* log_rho, float* score, double* sums, void* workspace, int64_t workspace_bytes,
                       void* stream) {
  if (!spec || !x || !workspace || (!log_rho && !score && !sums)) return CNF_ERR_INVALID;
  if (!kd_shape_ok(S, N, Q, D, spec->n_bw)) return CNF_ERR_INVALID;
  const bool loo = spec->loo != 0;
  if (q ? loo : Q != N) return CNF_ERR_INVALID;              // leave-one-out is self mode's; self mode has Q = N
  if (loo && N < 2) return CNF_ERR_INVALID;
  const int32_t NB = spec->n_bw;
  KdLaunch l{};
  KdMergeArgs ma{};
  const double n_eff = (double)(loo ? N - 1 : N);
  for (int b = 0; b < NB; ++b) {
    const double ib = kd_inv_2h2(spec->bw[b]);
    if (ib == 0.0) return CNF_ERR_INVALID;
    const double h = (double)spec->bw[b];
    l.a.kc.nc[b] = ma.nc[b] = (float)(-1.4426950408889634 * ib);
    if (!std::isfinite(ma.nc[b]) || ma.nc[b] == 0.0f) return CNF_ERR_INVALID;
    ma.inv_h2[b] = 2.0 * ib;
    ma.cst[b] = -std::log(n_eff) - 0.5 * D * std::log(6.283185307179586 * h * h);
  }
  const bool want_score = score != nullptr;
  const int32_t P = kd_splits(S, N, Q);
  const KdLayout lay = kd_layout(S, Q, D, NB, P, want_score);
  if (workspace_bytes < lay.bytes) return CNF_ERR_INVALID;
  char* ws = (char*)workspace;
  l.st = (hipStream_t)stream;
  l.x = x;
  l.q = q ? q : x;
  l.score = want_score;
  l.a.pm = (float*)(ws + lay.pm);
  l.a.ps = (double*)(ws + lay.ps);
  l.a.pa = (double*)(ws + lay.pa);
  l.a.N = (int32_t)N; l.a.Q = (int32_t)Q; l.a.P = P; l.a.loo = loo ? 1 : 0;
  l.grid = dim3((unsigned)(kd_row_groups(Q, D, NB) * P), (unsigned)S);
  pair_dispatch_dim(D, [&](auto d) { kd_launch_bw<decltype(d)::value>(NB, l); });
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  ma.pm = l.a.pm; ma.ps = l.a.ps; ma.pa = l.a.pa;
  ma.log_rho = log_rho ? log_rho : (float*)(ws + lay.lr);
  ma.score = score;
  ma.S = S; ma.Q = (int32_t)Q; ma.D = D; ma.NB = NB; ma.P = P;
  int rc = launch_plain(kd_merge_kernel, ((int64_t)S * Q + KD_THREADS - 1) / KD_THREADS, KD_THREADS, 0, l.st, ma);
  if (rc != CNF_OK || !sums) return rc;
  return launch_plain(kd_finish_kernel, (int64_t)S * NB, KD_THREADS, 0, l.st, (const float*)ma.log_rho, Q, sums);
}
