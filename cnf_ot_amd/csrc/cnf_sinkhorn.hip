// cnf_sinkhorn.hip -- the debiased entropic optimal-transport cost (Sinkhorn divergence) between two point clouds with
// uniform weights, its dual potentials, the barycentric map and the gradient in x, for the cost C(x, y) = |x - y|^2 / 2.
// Model-free, like cnf_mmd.hip: the reference the ot problems are judged against needs no density.
//
// THE RECURSION (the contract; tests/sinkhorn_ref.py restates it in float64).  Inputs x [S, N, D], y [S, M, D] and a
// host array eps[n_iters].  Per set, four potentials, all 0 at the start: f [N] and g [M] of the x-y problem, p [N] of
// x-x, q [M] of y-y.  With the soft minimum over the columns
//   T(h; rows, cols, e)_i = -e log( (1 / n_cols) sum_j exp((h_j - C(row_i, col_j)) / e) )
// iteration k = 0 .. n_iters - 1 updates all four SIMULTANEOUSLY from the old state (averaged Jacobi steps)
//   f <- (f + T(g; x, y, eps_k)) / 2      g <- (g + T(f; y, x, eps_k)) / 2
//   p <- (p + T(p; x, x, eps_k)) / 2      q <- (q + T(q; y, y, eps_k)) / 2
// and one final pass at eps_last = eps[n_iters - 1] takes the soft minima WITHOUT averaging:
//   f* = T(g),  g* = T(f),  p* = T(p),  q* = T(q).
// In that pass the row weights w_ij = exp((g_j - C_ij) / e) / sum_j' exp((g_j' - C_ij') / e) give the barycentric map
// Txy(x_i) = sum_j w_ij y_j (an estimate of the Monge map); the same with p over x gives Txx(x_i), and
//   xgrad_i = (Txx(x_i) - Txy(x_i)) / N
// is the ENVELOPE gradient of S = (sum f* - sum p*) / N + (sum g* - sum q*) / M in x_i: the potentials are held fixed,
// which is exact at the fixed point of the recursion and an approximation before it (the `change` sums say how far).
// The iteration count and every eps are inputs: nothing here decides convergence.
//
// THE KERNELS.  An iteration is ONE pair launch and ONE merge launch.  The pair launch covers the four blocks (f, g, p,
// q) of all S sets.  A workgroup owns SK_ROWS rows of one block and one of P column splits; a lane holds SK_R rows in
// registers.  A column -- its coordinates AND its potential -- is the same for every lane of the wave: the addresses are
// built from blockIdx and loop counters only, so both come through the scalar cache into SGPRs.  The distance is formed
// from coordinate differences, the numerator t = h_j - C_ij in float32, and the argument of v_exp_f32 is t prescaled by
// sc = log2 e / eps with the running maximum taken off in the same fma.  The log-sum-exp is kept online as (m, s): s =
// sum_j 2^(t_j sc - m).  The maximum moves once per chunk of 4 columns (2 from D = 7): one rescale of s per chunk, not
// per pair.  The float32 s lives for one tile of SK_TILE columns and is then added, rescaled, into a double.  Each (split, row)
// writes its (m, s); the merge kernel brings a row's splits to their common maximum in ascending order, applies
// -(1 / sc) (m + log2 s - log2 n_cols) -- 1 / sc = eps ln 2 for the eps the pair kernel actually used -- and the
// averaging, and writes the OTHER half of the double-buffered potentials.  The final pass (MAP) also carries
// sum_j 2^(t_j sc - m) col_j (D accumulators) in the x-row blocks under the same rescaling; it is a template argument,
// so the iterations do not pay for it, and a call that wants neither map nor gradient runs the plain kernel there too
// (the same operations on (m, s): the value does not depend on what else is asked for).  A last kernel adds the final
// potentials in a fixed strided order and a fixed tree.  No atomics, no waiting between workgroups, every loop counted:
// two calls give the same bits, a NaN input ends as NaN, and every workspace word read was written by this call.
// What it shares with the other pair passes -- the workgroup's geometry, the split rule, the dispatch on D -- is
// cnf_pairs.h's.
#include "cnf_host.h"
#include "cnf_pairs.h"

#include <math.h>

#include <algorithm>
#include <cmath>

// Every fused multiply-add below is written as one (fmaf): with the compiler free to contract, the instantiations with
// and without the map could round the same (m, s) differently
#pragma clang fp contract(off)

namespace cnf {
namespace {

// The geometry (cnf_pairs.h) this unit's kernels are written for: SK_THREADS = 256; SK_TILE = 64;
constexpr int SK_THREADS = PAIR_THREADS, SK_TILE = PAIR_TILE;
constexpr int SK_R = 2;                        // rows per lane
constexpr int SK_ROWS = SK_THREADS * SK_R;     // rows per workgroup
static_assert(SK_THREADS == 256 && SK_TILE == 64, "sinkhorn_pair_kernel's tile geometry");
constexpr int SK_MAX_ITERS = 512;
enum { SK_F = 0, SK_G = 1, SK_P = 2, SK_Q = 3 };

int64_t row_groups(int64_t n) { return pair_row_groups(n, SK_ROWS); }

// Column splits (pair_splits) over the longer side's tiles
int32_t sk_splits(int32_t S, int64_t N, int64_t M) {
  return pair_splits((int64_t)S * 2 * (row_groups(N) + row_groups(M)), pair_tiles(std::max(N, M)));
}

// A set's potentials, and a split's row partials, are laid out [f: N | g: M | p: N | q: M]
__host__ __device__ inline int64_t sk_width(int64_t N, int64_t M) { return 2 * (N + M); }
__host__ __device__ inline int64_t sk_offset(int b, int64_t N, int64_t M) {
  return b == SK_F ? 0 : b == SK_G ? N : b == SK_P ? N + M : 2 * N + M;
}

// Workspace: floats pot [3][S][W] (the two halves of the double buffer, then the final potentials), floats pm [S][P][W]
// (a partial's maximum), doubles ps [S][P][W] (its sum), doubles pa [S][P][2][N][D] (the map's sums, blocks f and p)
struct SkLayout {
  int64_t pot, pm, ps, pa, bytes;              // byte offsets (8-byte aligned) and the total
};
SkLayout sk_layout(int32_t S, int64_t N, int64_t M, int32_t D, int32_t P) {
  const int64_t W = sk_width(N, M);
  SkLayout l;
  l.pot = 0;
  l.pm = up8(3 * (int64_t)S * W * 4);
  l.ps = l.pm + up8((int64_t)S * P * W * 4);
  l.pa = l.ps + (int64_t)S * P * W * 8;
  l.bytes = l.pa + (int64_t)S * P * 2 * N * D * 8;
  return l;
}

// Columns per chunk: the running maximum moves, and the sum is rescaled, once per chunk (D U coordinates and U
// potentials in SGPRs at a time)
template <int D> constexpr int sk_chunk() { return D <= 6 ? 4 : 2; }

// K <= U columns starting at `p` / `hp` against the lane's rows: (m, s) and, with MAP, the D weighted column sums.
// TAIL: only the first k of the chunk's columns exist; the others are read from the last one and count as t = -inf.
template <int D, bool MAP, bool TAIL>
__device__ __forceinline__ void sk_chunk_step(const float* __restrict__ p, const float* __restrict__ hp, int k, float sc,
                                              const float (&x)[SK_R][D], float (&m)[SK_R], float (&s)[SK_R],
                                              float (&a)[SK_R][D]) {
  constexpr int U = sk_chunk<D>();
  float c[U][D], h[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = TAIL ? (u < k ? u : k - 1) : u;          // wave-uniform: scalar loads
#pragma unroll
    for (int d = 0; d < D; ++d) c[u][d] = p[j * D + d];
    h[u] = hp[j];
  }
#pragma unroll
  for (int r = 0; r < SK_R; ++r) {
    float t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float diff = x[r][0] - c[u][0];
      float d2 = diff * diff;
#pragma unroll
      for (int d = 1; d < D; ++d) {
        diff = x[r][d] - c[u][d];
        d2 = fmaf(diff, diff, d2);
      }
      t[u] = fmaf(d2, -0.5f, h[u]);                        // the numerator h_j - C_ij
      if (TAIL && u >= k) t[u] = -INFINITY;
    }
    float tm = t[0];
#pragma unroll
    for (int u = 1; u < U; ++u) tm = fmaxf(tm, t[u]);
    const float mn = fmaxf(m[r], tm * sc);                 // (rounding is monotone: the maximum of the scaled numerators)
    const float f = __builtin_amdgcn_exp2f(m[r] - mn);     // (-inf - finite at the very first chunk: 0)
    float sum = s[r] * f;
    m[r] = mn;
    if constexpr (MAP) {
#pragma unroll
      for (int d = 0; d < D; ++d) a[r][d] *= f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float e = __builtin_amdgcn_exp2f(fmaf(t[u], sc, -mn));
      sum += e;
      if constexpr (MAP) {
#pragma unroll
        for (int d = 0; d < D; ++d) a[r][d] = fmaf(e, c[u][d], a[r][d]);
      }
    }
    s[r] = sum;
  }
}

// The rows [row0, row0 + SK_ROWS) of `rows_p` [n_rows, D] against the tiles [t0, t1) of `col` [n_col, D] with the
// column potentials h [n_col]: a row's (maximum, sum) to pm / ps and, with MAP, its D sums to pa
template <int D, bool MAP>
__device__ __forceinline__ void sk_block(const float* __restrict__ rows_p, int64_t n_rows, const float* __restrict__ col,
                                         const float* __restrict__ h, int64_t n_col, int64_t row0, int64_t t0, int64_t t1,
                                         float sc, float* __restrict__ pm, double* __restrict__ ps,
                                         double* __restrict__ pa) {
  constexpr int U = sk_chunk<D>();
  float x[SK_R][D];
#pragma unroll
  for (int r = 0; r < SK_R; ++r) {
    const int64_t i = row0 + r * SK_THREADS + (int64_t)threadIdx.x;
#pragma unroll
    for (int d = 0; d < D; ++d) x[r][d] = i < n_rows ? rows_p[i * D + d] : 0.0f;
  }
  float m[SK_R];
  double sum[SK_R], asum[SK_R][D];
#pragma unroll
  for (int r = 0; r < SK_R; ++r) {
    m[r] = -INFINITY;
    sum[r] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) asum[r][d] = 0.0;
  }
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t c0 = t * SK_TILE;
    const int n = (int)(n_col - c0 < SK_TILE ? n_col - c0 : SK_TILE);
    const float* p = col + c0 * D;               // wave-uniform: scalar loads
    const float* hp = h + c0;
    float m0[SK_R], s[SK_R], a[SK_R][D];
#pragma unroll
    for (int r = 0; r < SK_R; ++r) {
      m0[r] = m[r];
      s[r] = 0.0f;
#pragma unroll
      for (int d = 0; d < D; ++d) a[r][d] = 0.0f;
    }
    int j = 0;
    for (; j + U <= n; j += U) sk_chunk_step<D, MAP, false>(p + j * D, hp + j, U, sc, x, m, s, a);
    if (j < n) sk_chunk_step<D, MAP, true>(p + j * D, hp + j, n - j, sc, x, m, s, a);
    // the tile's float32 sums into the doubles, which are first brought to the maximum the tile ended with
#pragma unroll
    for (int r = 0; r < SK_R; ++r) {
      const double f = (double)__builtin_amdgcn_exp2f(m0[r] - m[r]);
      sum[r] = sum[r] * f + (double)s[r];
      if constexpr (MAP) {
#pragma unroll
        for (int d = 0; d < D; ++d) asum[r][d] = asum[r][d] * f + (double)a[r][d];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < SK_R; ++r) {
    const int64_t i = row0 + r * SK_THREADS + (int64_t)threadIdx.x;
    if (i < n_rows) {
      pm[i] = m[r];                              // (an empty split: -inf and 0)
      ps[i] = sum[r];
      if constexpr (MAP) {
#pragma unroll
        for (int d = 0; d < D; ++d) pa[i * D + d] = asum[r][d];
      }
    }
  }
}

struct SkPairArgs {
  float* pm;
  double *ps, *pa;
  int64_t N, M;
  int32_t P, rgN, rgM;                           // splits, row groups of x and of y
  float sc;                                      // log2 e / eps
};

// One workgroup per (set, block, row group, split): blockIdx.x = ((s groups + u) P + split), u running over the row
// groups of f, g, p, q in turn
template <int D, bool MAP>
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_pair_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                   const float* __restrict__ pot, const SkPairArgs a) {
  const int P = a.P;
  const int p = (int)(blockIdx.x % (unsigned)P);
  const int64_t q = blockIdx.x / (unsigned)P;
  const int groups = 2 * (a.rgN + a.rgM);
  const int s = (int)(q / groups);
  int u = (int)(q % groups), b = SK_F;
  if (u >= a.rgN) { u -= a.rgN; b = SK_G; }
  if (b == SK_G && u >= a.rgM) { u -= a.rgM; b = SK_P; }
  if (b == SK_P && u >= a.rgN) { u -= a.rgN; b = SK_Q; }
  const int64_t N = a.N, M = a.M, W = sk_width(N, M);
  const bool x_rows = b == SK_F || b == SK_P, x_cols = b == SK_G || b == SK_P;
  const int64_t n_rows = x_rows ? N : M, n_col = x_cols ? N : M;
  const float* rows_p = x_rows ? x + (int64_t)s * N * D : y + (int64_t)s * M * D;
  const float* col = x_cols ? x + (int64_t)s * N * D : y + (int64_t)s * M * D;
  // the potential that lives on the columns: g for f's block, f for g's, p and q for their own
  const float* h = pot + (int64_t)s * W + sk_offset(b == SK_F ? SK_G : b == SK_G ? SK_F : b, N, M);
  // (pair_tile_range's two lines, written out: through the helper this kernel's instructions came out in another order)
  const int64_t tiles = (n_col + SK_TILE - 1) / SK_TILE, per = (tiles + P - 1) / P;
  const int64_t t0 = p * per < tiles ? p * per : tiles, t1 = t0 + per < tiles ? t0 + per : tiles;   // (may be empty)
  const int64_t part = ((int64_t)s * P + p) * W + sk_offset(b, N, M);
  const int64_t row0 = (int64_t)u * SK_ROWS;
  if (MAP && x_rows) {
    double* pa = a.pa + ((((int64_t)s * P + p) * 2 + (b == SK_P)) * N) * D;
    sk_block<D, MAP>(rows_p, n_rows, col, h, n_col, row0, t0, t1, a.sc, a.pm + part, a.ps + part, pa);
  } else {
    sk_block<D, false>(rows_p, n_rows, col, h, n_col, row0, t0, t1, a.sc, a.pm + part, a.ps + part, nullptr);
  }
}

__global__ __launch_bounds__(SK_THREADS) void sinkhorn_zero_kernel(float* __restrict__ h, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  if (e < n) h[e] = 0.0f;
}

struct SkMergeArgs {
  const float* pm;
  const double *ps, *pa;
  const float* h_in;                             // the potentials the pair kernel read: [S][W]
  float* h_out;                                  // [S][W]
  float *xmap, *xgrad;                           // [S, N, D] or null (last pass only)
  int64_t N, M;
  int32_t S, D, P, last;
  double inv_sc;                                 // 1 / sc = eps ln 2, for the eps the pair kernel used
};

// A row's splits brought to their common maximum in ascending order: sum_j 2^(t_j sc) = s 2^m
struct SkRow {
  float m;
  double s;
};
__device__ __forceinline__ SkRow sk_merge_row(const float* __restrict__ pm, const double* __restrict__ ps, int64_t stride,
                                              int P) {
  SkRow r{pm[0], ps[0]};                         // (split 0 is never empty: its maximum is finite on finite input)
  for (int p = 1; p < P; ++p) {
    const float mp = pm[p * stride];
    const double sp = ps[p * stride];
    if (mp == -INFINITY) continue;               // an empty split of the shorter side
    const float mx = fmaxf(r.m, mp);
    r.s = r.s * exp2((double)(r.m - mx)) + sp * exp2((double)(mp - mx));
    r.m = mx;
  }
  return r;
}

// One thread per (set, row of x or of y): the two potentials of that row (f and p, or g and q) and, in the last pass,
// the map and the gradient of an x row
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_merge_kernel(const SkMergeArgs a) {
  const int64_t N = a.N, M = a.M, W = sk_width(N, M), per_set = N + M;
  const int64_t e = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  if (e >= (int64_t)a.S * per_set) return;
  const int64_t s = e / per_set, r = e % per_set;
  const bool x_row = r < N;
  const int64_t i = x_row ? r : r - N;
  const int P = a.P, D = a.D;
  const int64_t stride = W;                      // from one split's partials to the next
  SkRow row[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {                  // k = 0: the x-y problem, 1: the self problem
    const int b = x_row ? (k ? SK_P : SK_F) : (k ? SK_Q : SK_G);
    const int64_t off = sk_offset(b, N, M) + i;
    const int64_t part = (int64_t)s * P * W + off;
    row[k] = sk_merge_row(a.pm + part, a.ps + part, stride, P);
    const double n_col = (double)((b == SK_G || b == SK_P) ? N : M);
    const double T = -a.inv_sc * ((double)row[k].m + log2(row[k].s) - log2(n_col));
    const double old = (double)a.h_in[s * W + off];
    a.h_out[s * W + off] = (float)(a.last ? T : 0.5 * (old + T));
  }
  if (!a.last || !x_row || (!a.xmap && !a.xgrad)) return;
  for (int d = 0; d < D; ++d) {
    double t[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {                // the same rescaling, split by split, as the sums
      double acc = 0.0;
      for (int p = 0; p < P; ++p) {
        const int64_t part = (int64_t)s * P + p;
        const float mp = a.pm[part * W + sk_offset(k ? SK_P : SK_F, N, M) + i];
        if (p > 0 && mp == -INFINITY) continue;
        acc += a.pa[((part * 2 + k) * N + i) * D + d] * exp2((double)(mp - row[k].m));
      }
      t[k] = acc / row[k].s;
    }
    const int64_t o = (s * N + i) * D + d;
    if (a.xmap) a.xmap[o] = (float)t[0];
    if (a.xgrad) a.xgrad[o] = (float)((t[1] - t[0]) / (double)N);
  }
}

// The larger of two changes; a NaN stays
__device__ __forceinline__ double sk_max_nan(double a, double b) { return (a != a || b <= a) ? a : b; }

// Workgroup 2 s + k (k = 0: f and g, 1: p and q): the sums of the two final potentials and the largest change of the
// final pass, thread t taking rows t, t + 256, ... and the threads' totals meeting in a fixed tree
__global__ __launch_bounds__(SK_THREADS) void sinkhorn_finish_kernel(const float* __restrict__ fin,
                                                                     const float* __restrict__ prev, int64_t N, int64_t M,
                                                                     double* __restrict__ sums) {
  __shared__ double s_a[SK_THREADS], s_b[SK_THREADS], s_c[SK_THREADS];
  const int t = (int)threadIdx.x;
  const int s = (int)blockIdx.x / 2, k = (int)blockIdx.x % 2;
  const int64_t W = sk_width(N, M);
  const float* f1 = fin + s * W + sk_offset(k ? SK_P : SK_F, N, M);
  const float* f0 = prev + s * W + sk_offset(k ? SK_P : SK_F, N, M);
  const float* g1 = fin + s * W + sk_offset(k ? SK_Q : SK_G, N, M);
  const float* g0 = prev + s * W + sk_offset(k ? SK_Q : SK_G, N, M);
  double sa = 0.0, sb = 0.0, ch = 0.0;
  for (int64_t i = t; i < N; i += SK_THREADS) {
    sa += (double)f1[i];
    ch = sk_max_nan(ch, fabs((double)f1[i] - (double)f0[i]));
  }
  for (int64_t i = t; i < M; i += SK_THREADS) {
    sb += (double)g1[i];
    ch = sk_max_nan(ch, fabs((double)g1[i] - (double)g0[i]));
  }
  s_a[t] = sa;
  s_b[t] = sb;
  s_c[t] = ch;
  __syncthreads();
  for (int o = SK_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) {
      s_a[t] += s_a[t + o];
      s_b[t] += s_b[t + o];
      s_c[t] = sk_max_nan(s_c[t], s_c[t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    sums[s * 6 + 2 * k] = s_a[0];
    sums[s * 6 + 2 * k + 1] = s_b[0];
    sums[s * 6 + 4 + k] = s_c[0];
  }
}

// x [S, N, D], y [S, M, D] and the potentials read, pot [S][W], are arguments of their own: __restrict__ pointers, whose
// wave-uniform loads the compiler may send through the scalar cache
int sk_launch_pair(int dim, bool map, int64_t grid, hipStream_t st, const float* x, const float* y, const float* pot,
                   const SkPairArgs& a) {
  int rc = CNF_ERR_INVALID;
  pair_dispatch_dim(dim, [&](auto d) {
    constexpr int D = decltype(d)::value;
    rc = map ? launch_plain(sinkhorn_pair_kernel<D, true>, grid, SK_THREADS, 0, st, x, y, pot, a)
             : launch_plain(sinkhorn_pair_kernel<D, false>, grid, SK_THREADS, 0, st, x, y, pot, a);
  });
  return rc;
}

bool sk_shape_ok(int32_t S, int64_t N, int64_t M, int32_t D) {
  return pair_dims_ok(S, D) && N >= 2 && M >= 2 && N <= PAIR_MAX_N && M <= PAIR_MAX_N;
}

// log2 e / eps as the kernels receive it, or 0 for an eps they refuse
float sk_scale(double eps) {
  if (!(eps > 0.0) || !std::isfinite(eps)) return 0.0f;
  const float sc = (float)(1.4426950408889634 / eps), inv = (float)(1.0 / eps);
  return std::isfinite(sc) && std::isfinite(inv) && inv >= 1.17549435e-38f ? sc : 0.0f;      // (1 / eps a normal float32)
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_sinkhorn_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int64_t* bytes) {
  if (!bytes || !sk_shape_ok(S, N, M, D)) return CNF_ERR_INVALID;
  *bytes = sk_layout(S, N, M, D, sk_splits(S, N, M)).bytes;
  return CNF_OK;
}

extern "C" int cnf_sinkhorn_splits(int32_t S, int64_t N, int64_t M, int32_t D) {
  return sk_shape_ok(S, N, M, D) ? sk_splits(S, N, M) : CNF_ERR_INVALID;
}

extern "C" int cnf_sinkhorn(int32_t S, const float* x, int64_t N, const float* y, int64_t M, int32_t D, const double* eps,
                            int32_t n_iters, double* sums, float* potentials, float* xgrad, float* xmap, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  if (!x || !y || !eps || !sums || !workspace || !sk_shape_ok(S, N, M, D)) return CNF_ERR_INVALID;
  if (n_iters < 1 || n_iters > SK_MAX_ITERS) return CNF_ERR_INVALID;
  for (int k = 0; k < n_iters; ++k)
    if (sk_scale(eps[k]) == 0.0f) return CNF_ERR_INVALID;
  const int32_t P = sk_splits(S, N, M);
  const SkLayout l = sk_layout(S, N, M, D, P);
  if (workspace_bytes < l.bytes) return CNF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int64_t W = sk_width(N, M), SW = (int64_t)S * W;
  float* pot = (float*)(ws + l.pot);             // halves 0 and 1 of the double buffer, then the final potentials
  float* fin = potentials ? potentials : pot + 2 * SW;
  const int64_t merge_wgs = ((int64_t)S * (N + M) + SK_THREADS - 1) / SK_THREADS;

  SkPairArgs pa{};
  pa.N = N; pa.M = M; pa.P = P;
  pa.rgN = (int32_t)row_groups(N);
  pa.rgM = (int32_t)row_groups(M);
  pa.pm = (float*)(ws + l.pm);
  pa.ps = (double*)(ws + l.ps);
  pa.pa = (double*)(ws + l.pa);
  const int64_t pair_wgs = (int64_t)S * 2 * (pa.rgN + pa.rgM) * P;
  SkMergeArgs ma{};
  ma.pm = pa.pm; ma.ps = pa.ps; ma.pa = pa.pa;
  ma.N = N; ma.M = M; ma.S = S; ma.D = D; ma.P = P;

  int rc = launch_plain(sinkhorn_zero_kernel, (SW + SK_THREADS - 1) / SK_THREADS, SK_THREADS, 0, st, pot, SW);
  // pass k < n_iters: an averaged step from half k % 2 into the other; pass n_iters: the soft minima themselves
  for (int k = 0; k <= n_iters && rc == CNF_OK; ++k) {
    const bool last = k == n_iters;
    const float sc = sk_scale(eps[last ? n_iters - 1 : k]);
    const float* h = pot + (k % 2) * SW;
    pa.sc = sc;
    rc = sk_launch_pair(D, last && (xmap || xgrad), pair_wgs, st, x, y, h, pa);
    if (rc != CNF_OK) break;
    ma.h_in = h;
    ma.h_out = last ? fin : pot + ((k + 1) % 2) * SW;
    ma.last = last;
    ma.xmap = last ? xmap : nullptr;
    ma.xgrad = last ? xgrad : nullptr;
    ma.inv_sc = 1.0 / (double)sc;
    rc = launch_plain(sinkhorn_merge_kernel, merge_wgs, SK_THREADS, 0, st, ma);
  }
  if (rc != CNF_OK) return rc;
  return launch_plain(sinkhorn_finish_kernel, 2 * (int64_t)S, SK_THREADS, 0, st, (const float*)fin,
                      (const float*)(pot + (n_iters % 2) * SW), N, M, sums);
}
