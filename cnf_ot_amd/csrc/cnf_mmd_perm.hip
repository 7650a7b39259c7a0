// cnf_mmd_perm.hip -- the permutation test of the kernel two-sample statistic: the unbiased MMD^2 (or energy distance)
// of the pooled sample z = (x, y), n = N + M points, under P relabellings at once.  With K the zero-diagonal kernel
// matrix of z and a label vector s in {+1, -1}^n (+1: "first sample"), every block sum follows from three numbers,
//   q = s' K s,   r = 1' K s,   t = 1' K 1:   sum_xx = (t + 2 r + q) / 4,  sum_yy = (t - 2 r + q) / 4,  sum_xy = (t - q) / 4,
// so the P statistics are the matrix product C = K S' ([n, n] by [n, P]) and a fold: each kernel value is formed ONCE
// and used P times.  K is never stored: it is the pair pass of cnf_mmd.hip -- the same float32
// operations in the same order -- feeding the matrix cores as the A operand of the exact-fp32 v_mfma_f32_16x16x4_f32;
// the B operand is the sign of a column under 16 label vectors, built from the label bit with an OR into the sign bit
// of 1.0f.  The signs are exact, and the instruction is a k-ordered fmaf chain.
//
// A wave owns 16 pooled rows, a workgroup PERM_ROWS = 64 and one of the column splits.  Lane l (g = l >> 4, s = l & 15)
// forms K[row s][column 4 step + g] of a tile of 64 columns (its row's coordinates in registers, the tile's coordinates
// and label words in LDS), and that one value feeds PERM_CHUNK / 16 MFMAs, one per block of 16 label vectors.  After
// the tile's 16 steps an accumulator register holds 64 pair terms (the project's rule) and is folded into per-lane
// doubles: q_p += s_ip C[i, p], r_p += C[i, p] for the lane's rows i = 4 g + (0..3) and vector p = 16 block + s (r
// needs no second product: K is symmetric).  t is the sum of the same K values, kept beside them.  More than
// PERM_CHUNK label vectors run as further passes over the pairs (blockIdx.y); a pass costs a full chunk.
//
// perm_counts_kernel counts each vector's set bits; perm_finish_kernel adds the (row group, split) partials in
// ascending order and forms the statistic in double.  No atomics; every workspace word read was written by this call.
// A label vector's q and r do not depend on P, on its position or on the other vectors: its chain is its own.
#include "cnf_pairs.h"

#include <math.h>

#include <algorithm>
#include <cmath>

// Every fused multiply-add below is written as one (fmaf), as in cnf_mmd.hip: the pair value is that unit's
#pragma clang fp contract(off)

namespace cnf {
namespace {

constexpr int PERM_THREADS = PAIR_THREADS, PERM_TILE = PAIR_TILE;
constexpr int PERM_WAVES = PERM_THREADS / 64;
constexpr int PERM_ROWS = 16 * PERM_WAVES;       // rows per workgroup: a wave's MFMA block of 16, four waves
// Label vectors per pass: 8 blocks x 4 accumulator registers.  By register count: at 128 the instantiations take 140 ..
// 165 VGPRs (3 waves per SIMD) with no spill; at 256 every one fills the 256 of two waves per SIMD and D = 14 spills
constexpr int PERM_CHUNK = 128;
constexpr int PERM_BLOCKS = PERM_CHUNK / 16, PERM_WORDS = PERM_CHUNK / 32;
constexpr int PERM_MIN_P = 32, PERM_MAX_P = 1024;
constexpr int PERM_MAX_BW = CNF_MMD_MAX_BW;
constexpr int PERM_COUNT_POINTS = 2048, PERM_COUNT_MAX_WGS = 64;     // the popcount pass: points per workgroup, at least
static_assert(PERM_THREADS == 256 && PERM_TILE == 64 && PERM_ROWS == 64, "perm_kernel's tile geometry");
static_assert(PERM_CHUNK == 128 || PERM_CHUNK == 256, "the chunk: 128 or 256 label vectors");
static_assert(PERM_TILE * PERM_WORDS % PERM_THREADS == 0, "perm_kernel stages the tile's label words in whole rounds");

typedef float perm_f4 __attribute__((ext_vector_type(4)));

struct PermCoef {
  float nc[PERM_MAX_BW];                         // -log2 e / (2 bw_b^2), as cnf_mmd.hip's MmdCoef
};

int64_t perm_row_groups(int64_t n) { return pair_row_groups(n, PERM_ROWS); }
int32_t perm_passes(int32_t P) { return (P + PERM_CHUNK - 1) / PERM_CHUNK; }

// Column splits over the pooled sample's tiles: a function of the sizes alone (not of P)
int32_t perm_splits(int32_t S, int64_t n) { return pair_splits((int64_t)S * perm_row_groups(n), pair_tiles(n)); }

int64_t perm_count_wgs(int64_t n) {
  return std::min<int64_t>(PERM_COUNT_MAX_WGS, (n + PERM_COUNT_POINTS - 1) / PERM_COUNT_POINTS);
}

// Workspace: doubles [S][row groups x splits][2 P + 1] = (q [P], r [P], t), then the counts' partials, int32 [wgs][P]
int64_t perm_partials(int32_t S, int64_t n) { return (int64_t)S * perm_row_groups(n) * perm_splits(S, n); }
int64_t perm_part_doubles(int32_t S, int64_t n, int32_t P) { return perm_partials(S, n) * (2 * (int64_t)P + 1); }
int64_t perm_workspace_bytes(int32_t S, int64_t n, int32_t P) {
  return perm_part_doubles(S, n, P) * (int64_t)sizeof(double) + up8(perm_count_wgs(n) * P * (int64_t)sizeof(int32_t));
}

// The kernel value of cnf_mmd.hip's mmd_pair, restated: differences first, d2 by fmaf in ascending d, the Gaussians
// summed in ascending b, the energy value -d2 rsq(d2)
template <int D, int NB>
__device__ __forceinline__ float perm_pair(const float (&x)[D], const float (&c)[D], const PermCoef& k) {
  float diff[D];
#pragma unroll
  for (int d = 0; d < D; ++d) diff[d] = x[d] - c[d];
  float d2 = diff[0] * diff[0];
#pragma unroll
  for (int d = 1; d < D; ++d) d2 = fmaf(diff[d], diff[d], d2);
  float v;
  if constexpr (NB == 0) {
    const float inv = d2 > 1e-30f ? __builtin_amdgcn_rsqf(d2) : 0.0f;
    v = -d2 * inv;
  } else {
    v = 0.0f;
#pragma unroll
    for (int b = 0; b < NB; ++b) v += __builtin_amdgcn_exp2f(d2 * k.nc[b]);
  }
  return v;
}

// What a thread stages of one column tile: its share of the 64 x D coordinates and of the 64 x PERM_WORDS label words
template <int D> struct PermStage {
  static constexpr int NC = (PERM_TILE * D + PERM_THREADS - 1) / PERM_THREADS, NL = PERM_TILE * PERM_WORDS / PERM_THREADS;
  float c[NC];
  uint32_t w[NL];
};

// The pooled sample is x's rows followed by y's: flat element f of [n, D]
template <int D>
__device__ __forceinline__ void perm_load(PermStage<D>& st, const float* __restrict__ xs, const float* __restrict__ ys,
                                          int64_t N, int64_t n, const uint32_t* __restrict__ labels, int PW, int word0,
                                          int64_t c0) {
  const int t = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < PermStage<D>::NC; ++k) {
    const int e = t + k * PERM_THREADS;
    const int64_t f = c0 * D + e;
    st.c[k] = (e < PERM_TILE * D && f < n * D) ? (f < N * D ? xs[f] : ys[f - N * D]) : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < PermStage<D>::NL; ++k) {
    const int e = t + k * PERM_THREADS, w = word0 + e % PERM_WORDS;
    const int64_t j = c0 + e / PERM_WORDS;
    // stored inverted: a set bit (first sample, +1) is a clear sign bit
    st.w[k] = ~((j < n && w < PW) ? labels[j * PW + w] : 0u);
  }
}

template <int D>
__device__ __forceinline__ void perm_store(const PermStage<D>& st, float* s_col, uint32_t* s_lab) {
  const int t = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < PermStage<D>::NC; ++k) {
    const int e = t + k * PERM_THREADS;
    if (e < PERM_TILE * D) s_col[e] = st.c[k];
  }
#pragma unroll
  for (int k = 0; k < PermStage<D>::NL; ++k) s_lab[t + k * PERM_THREADS] = st.w[k];
}

// grid (row groups x SPL, S x passes): blockIdx.x = row group * SPL + split, blockIdx.y = s * passes + pass
template <int D, int NB>
__global__ __launch_bounds__(PERM_THREADS, 2) void perm_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               int64_t N, int64_t M, const uint32_t* __restrict__ labels,
                                                               int32_t P, int32_t SPL, int32_t passes, const PermCoef k,
                                                               double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float s_col[2][PERM_TILE * D];
  __shared__ __attribute__((aligned(16))) uint32_t s_lab[2][PERM_TILE * PERM_WORDS];
  __shared__ double s_red[PERM_WAVES][2][PERM_CHUNK];
  __shared__ double s_t[PERM_WAVES];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, s15 = lane & 15;
  const int s = (int)blockIdx.y / passes, pass = (int)blockIdx.y % passes;
  const int64_t rg = blockIdx.x / (unsigned)SPL;
  const int sp = (int)(blockIdx.x % (unsigned)SPL);
  const int64_t n = N + M;
  const int PW = P / 32, word0 = pass * PERM_WORDS;
  const float* xs = x + (int64_t)s * N * D;
  const float* ys = y + (int64_t)s * M * D;

  // the lane's row as the A operand sees it: row s15 of the wave's 16
  const int64_t i = rg * PERM_ROWS + wave * 16 + s15;
  float xr[D];
#pragma unroll
  for (int d = 0; d < D; ++d) xr[d] = i < n ? (i < N ? xs[i * D + d] : ys[(i - N) * D + d]) : 0.0f;
  // ... and the rows it folds, 4 g + r: bit 4 b + r of neg is set where row 4 g + r is NOT of the first sample under
  // vector 16 b + s15 of this pass
  uint32_t neg[PERM_BLOCKS / 8];
#pragma unroll
  for (int h = 0; h < PERM_BLOCKS / 8; ++h) neg[h] = 0u;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t ir = rg * PERM_ROWS + wave * 16 + 4 * g + r;
#pragma unroll
    for (int w = 0; w < PERM_WORDS; ++w) {
      const uint32_t word = ~((ir < n && word0 + w < PW) ? labels[ir * PW + word0 + w] : 0u);
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const int b = 2 * w + o;
        neg[b / 8] |= ((word >> (16 * o + s15)) & 1u) << (4 * (b % 8) + r);
      }
    }
  }

  perm_f4 acc[PERM_BLOCKS];
  double qd[PERM_BLOCKS], rd[PERM_BLOCKS], td = 0.0;
#pragma unroll
  for (int b = 0; b < PERM_BLOCKS; ++b) {
    acc[b] = perm_f4{0.0f, 0.0f, 0.0f, 0.0f};
    qd[b] = 0.0;
    rd[b] = 0.0;
  }

  const auto [t0, t1] = pair_tile_range<int64_t>(n, SPL, sp);      // (may be empty: zeros)
  PermStage<D> st;
  if (t0 < t1) {
    perm_load<D>(st, xs, ys, N, n, labels, PW, word0, t0 * PERM_TILE);
    perm_store<D>(st, s_col[0], s_lab[0]);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t c0 = tile * PERM_TILE;
    if (tile + 1 < t1) perm_load<D>(st, xs, ys, N, n, labels, PW, word0, c0 + PERM_TILE);
    const float* col = s_col[cur];
    const uint32_t* lab = s_lab[cur];
    float tsum = 0.0f;
#pragma unroll 2
    for (int step = 0; step < PERM_TILE / 4; ++step) {
      const int jl = 4 * step + g;
      float c[D];
#pragma unroll
      for (int d = 0; d < D; ++d) c[d] = col[jl * D + d];
      float v = perm_pair<D, NB>(xr, c, k);
      const int64_t j = c0 + jl;
      v = (j == i || j >= n || i >= n) ? 0.0f : v;           // the diagonal and the padding, by index
      tsum += v;
      uint32_t w[PERM_WORDS];
#pragma unroll
      for (int q4 = 0; q4 < PERM_WORDS / 4; ++q4) {
        const uint4 u = *reinterpret_cast<const uint4*>(lab + jl * PERM_WORDS + 4 * q4);
        w[4 * q4] = u.x; w[4 * q4 + 1] = u.y; w[4 * q4 + 2] = u.z; w[4 * q4 + 3] = u.w;
      }
#pragma unroll
      for (int b = 0; b < PERM_BLOCKS; ++b) {
        // bit 16 (b & 1) + s15 of the (inverted) word into the sign bit of 1.0f
        const uint32_t sign = (w[b / 2] << (31 - 16 * (b & 1) - s15)) & 0x80000000u;
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, __uint_as_float(sign | 0x3f800000u), acc[b], 0, 0, 0);
      }
    }
    // 64 pair terms per accumulator register: fold.  Register r is C[row 4 g + r][vector 16 b + s15]
    td += (double)tsum;
#pragma unroll
    for (int b = 0; b < PERM_BLOCKS; ++b) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float cv = acc[b][r];
        const uint32_t flip = ((neg[b / 8] >> (4 * (b % 8) + r)) & 1u) << 31;
        qd[b] += (double)__uint_as_float(__float_as_uint(cv) ^ flip);
        rd[b] += (double)cv;
      }
      acc[b] = perm_f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    if (tile + 1 < t1) perm_store<D>(st, s_col[cur ^ 1], s_lab[cur ^ 1]);
    __syncthreads();                               // (the other buffer was last read before the previous barrier)
    cur ^= 1;
  }

  // the lane groups g of a wave (the rows), then the waves in ascending order
#pragma unroll
  for (int b = 0; b < PERM_BLOCKS; ++b) {
    double qv = qd[b], rv = rd[b];
    qv += __shfl_xor(qv, 16);
    rv += __shfl_xor(rv, 16);
    qv += __shfl_xor(qv, 32);
    rv += __shfl_xor(rv, 32);
    if (g == 0) {
      s_red[wave][0][16 * b + s15] = qv;
      s_red[wave][1][16 * b + s15] = rv;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) td += __shfl_xor(td, o);
  if (lane == 0) s_t[wave] = td;
  __syncthreads();
  double* part = ws + (((int64_t)s * gridDim.x) + blockIdx.x) * (2 * (int64_t)P + 1);
  for (int e = t; e < 2 * PERM_CHUNK; e += PERM_THREADS) {
    const int kind = e / PERM_CHUNK, p = e % PERM_CHUNK;
    double v = s_red[0][kind][p];
#pragma unroll
    for (int w = 1; w < PERM_WAVES; ++w) v += s_red[w][kind][p];
    if (pass * PERM_CHUNK + p < P) part[kind * P + pass * PERM_CHUNK + p] = v;
  }
  if (t == 0 && pass == 0) {
    double v = s_t[0];
#pragma unroll
    for (int w = 1; w < PERM_WAVES; ++w) v += s_t[w];
    part[2 * P] = v;
  }
}

// grid (P / 32, count workgroups): thread t counts bit t & 31 of word blockIdx.x over every 8th point of its range
__global__ __launch_bounds__(PERM_THREADS) void perm_counts_kernel(const uint32_t* __restrict__ labels, int64_t n, int32_t P,
                                                                   int32_t* __restrict__ counts) {
  __shared__ int32_t s_cnt[PERM_THREADS];
  const int t = (int)threadIdx.x, bit = t & 31, grp = t >> 5, PW = P / 32;
  const int64_t per = (n + gridDim.y - 1) / gridDim.y, lo = blockIdx.y * per, hi = lo + per < n ? lo + per : n;
  int32_t c = 0;
  for (int64_t j = lo + grp; j < hi; j += PERM_THREADS / 32) c += (int32_t)((labels[j * PW + blockIdx.x] >> bit) & 1u);
  s_cnt[t] = c;
  __syncthreads();
  if (t < 32) {
    for (int o = 1; o < PERM_THREADS / 32; ++o) c += s_cnt[t + 32 * o];
    counts[(int64_t)blockIdx.y * P + blockIdx.x * 32 + t] = c;
  }
}

// thread (s, p): the partials in ascending (row group, split) order, then the statistic in double
__global__ __launch_bounds__(PERM_THREADS) void perm_finish_kernel(const double* __restrict__ ws, const int32_t* __restrict__ counts,
                                                                   int32_t S, int64_t n, int32_t P, int64_t groups,
                                                                   int32_t count_wgs, double* __restrict__ stats,
                                                                   double* __restrict__ raw) {
  const int64_t e = (int64_t)blockIdx.x * PERM_THREADS + threadIdx.x;
  if (e >= (int64_t)S * P) return;
  const int64_t s = e / P, p = e % P, stride = 2 * (int64_t)P + 1;
  const double* part = ws + s * groups * stride;
  double q = 0.0, r = 0.0, tt = 0.0;
  for (int64_t gi = 0; gi < groups; ++gi) {
    q += part[gi * stride + p];
    r += part[gi * stride + P + p];
    tt += part[gi * stride + 2 * P];
  }
  int64_t np = 0;
  for (int c = 0; c < count_wgs; ++c) np += counts[(int64_t)c * P + p];
  const double dn = (double)np, dm = (double)(n - np);
  const double sxx = (tt + 2.0 * r + q) * 0.25, syy = (tt - 2.0 * r + q) * 0.25, sxy = (tt - q) * 0.25;
  stats[e] = (np >= 2 && n - np >= 2) ? sxx / (dn * (dn - 1.0)) + syy / (dm * (dm - 1.0)) - 2.0 * sxy / (dn * dm)
                                      : __builtin_nan("");
  if (raw) {
    raw[2 * e] = q;
    raw[2 * e + 1] = r;
    if (p == 0) raw[2 * (int64_t)S * P + s] = tt;
  }
}

struct PermLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *y;
  int64_t N, M;
  const uint32_t* labels;
  int32_t P, SPL, passes;
  PermCoef k;
  double* ws;
};

// NB = 0: the energy kernel; 1 .. 8: that many bandwidths
template <int D, int NB = 0> void perm_launch_bw(int nb, const PermLaunch& a) {
  if (nb == NB)
    hipLaunchKernelGGL((perm_kernel<D, NB>), a.grid, dim3(PERM_THREADS), 0, a.st, a.x, a.y, a.N, a.M, a.labels, a.P, a.SPL,
                       a.passes, a.k, a.ws);
  else if constexpr (NB < PERM_MAX_BW) perm_launch_bw<D, NB + 1>(nb, a);
}

bool perm_shape_ok(int32_t S, int64_t N, int64_t M, int32_t D) {
  return pair_dims_ok(S, D) && N >= 2 && M >= 2 && N <= PAIR_MAX_N && M <= PAIR_MAX_N && N + M <= PAIR_MAX_N;
}
bool perm_vectors_ok(int32_t P) { return P >= PERM_MIN_P && P <= PERM_MAX_P && P % 32 == 0; }

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_mmd_perm_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t P, int64_t* bytes) {
  if (!bytes || !perm_shape_ok(S, N, M, D) || !perm_vectors_ok(P)) return CNF_ERR_INVALID;
  *bytes = perm_workspace_bytes(S, N + M, P);
  return CNF_OK;
}

extern "C" int cnf_mmd_perm_splits(int32_t S, int64_t N, int64_t M, int32_t D) {
  return perm_shape_ok(S, N, M, D) ? perm_splits(S, N + M) : CNF_ERR_INVALID;
}

extern "C" int cnf_mmd_perm(const CnfMmdSpec* spec, int32_t S, const float* x, int64_t N, const float* y, int64_t M, int32_t D,
                            const uint32_t* labels, int32_t P, double* stats, double* raw, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  if (!spec || !x || !y || !labels || !stats || !workspace || !perm_shape_ok(S, N, M, D) || !perm_vectors_ok(P))
    return CNF_ERR_INVALID;
  if (spec->kind != CNF_MMD_GAUSSIAN && spec->kind != CNF_MMD_ENERGY) return CNF_ERR_INVALID;
  PermLaunch a{};
  int nb = 0;
  if (spec->kind == CNF_MMD_GAUSSIAN) {            // (cnf_mmd2's checks and coefficients)
    nb = spec->n_bw;
    if (nb < 1 || nb > PERM_MAX_BW) return CNF_ERR_INVALID;
    for (int b = 0; b < nb; ++b) {
      const double bw = (double)spec->bw[b];
      if (!(bw > 0.0) || !std::isfinite(bw)) return CNF_ERR_INVALID;
      a.k.nc[b] = (float)(-1.4426950408889634 / (2.0 * bw * bw));
      if (!std::isfinite(a.k.nc[b]) || !(1.0 / (bw * bw) <= 3.0e38)) return CNF_ERR_INVALID;
    }
  }
  const int64_t n = N + M;
  if (workspace_bytes < perm_workspace_bytes(S, n, P)) return CNF_ERR_INVALID;
  a.SPL = perm_splits(S, n);
  a.passes = perm_passes(P);
  a.grid = dim3((unsigned)(perm_row_groups(n) * a.SPL), (unsigned)(S * a.passes));
  a.st = (hipStream_t)stream;
  a.x = x; a.y = y; a.N = N; a.M = M;
  a.labels = labels;
  a.P = P;
  a.ws = (double*)workspace;
  int32_t* counts = (int32_t*)(a.ws + perm_part_doubles(S, n, P));
  const int32_t count_wgs = (int32_t)perm_count_wgs(n);
  hipLaunchKernelGGL(perm_counts_kernel, dim3((unsigned)(P / 32), (unsigned)count_wgs), dim3(PERM_THREADS), 0, a.st, labels, n,
                     P, counts);
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  pair_dispatch_dim(D, [&](auto d) { perm_launch_bw<decltype(d)::value>(nb, a); });
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  hipLaunchKernelGGL(perm_finish_kernel, dim3((unsigned)(((int64_t)S * P + PERM_THREADS - 1) / PERM_THREADS)),
                     dim3(PERM_THREADS), 0, a.st, (const double*)a.ws, (const int32_t*)counts, S, n, P,
                     perm_row_groups(n) * a.SPL, count_wgs, stats, raw);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
