// cnf_stein_boot.hip -- the wild bootstrap of the kernel Stein discrepancy: KSD^2_U of a point set against a score under P
// Rademacher sign vectors at once.  With H the Stein kernel matrix of the set with its diagonal zeroed (cnf_stein's
// k_p) and e in {+1, -1}^N, the bootstrap of the degenerate U-statistic is
//   B(e) = e' H e / (N (N - 1)),   KSD^2_U = B(1),
// so the P values are the matrix product C = H E' ([N, N] by [N, P]) and a fold: each Stein kernel value is formed ONCE
// and used P times.  H is never stored: it is the pair value of cnf_stein.hip's st_tile -- the same
// float32 operations in the same order, without the gradient's p3 -- feeding the matrix cores as the A operand of the
// exact-fp32 v_mfma_f32_16x16x4_f32; the B operand is the sign of a column under 16 vectors, built from the sign bit with
// an OR into the sign bit of 1.0f.  The signs are exact, and the instruction is a k-ordered fmaf chain.
//
// The skeleton is cnf_mmd_perm.hip's perm_kernel, restated (DESIGN.md 8 names the duplication).  A wave owns 16 rows, a
// workgroup BOOT_ROWS = 64 and one of the column splits.  Lane l (g = l >> 4, s = l & 15) forms H[row s][column 4 step +
// g] of a tile of 64 columns (its row's x_i and s_i in registers, the tile's x_j, s_j and sign words in LDS), and that
// one value feeds BOOT_CHUNK / 16 MFMAs, one per block of 16 sign vectors.  After the tile's 16 steps an accumulator
// register holds 64 pair terms (the project's rule) and is folded into a per-lane double: q_p += e_ip C[i, p] for the
// lane's rows i = 4 g + (0..3) and vector p = 16 block + s.  There is no second sum: this statistic needs none.
// t = 1' H 1 is one more MFMA per step in pass 0, against 1.0f: the chains, the fold and the reduction of an all +1
// vector, so that such a vector's q is t bit for bit (the lanes' own float32 sums of their 16 values round otherwise,
// 1e-8 of the sum apart).  The diagonal sum_i k_p(x_i, x_i) is added once per row by the workgroups of split 0, pass 0.
// More than BOOT_CHUNK sign vectors run as further passes over the pairs (blockIdx.y); a pass costs a full chunk.
//
// boot_finish_kernel adds the (row group, split) partials in ascending order.  No atomics; every workspace word read was
// written by this call.  A sign vector's q does not depend on P, on its position or on the other vectors: its chain is
// its own; and q is the same bits under the complemented vector (every signed term is).
#include "cnf_interaction_pairs.h"

#include <math.h>

#include <algorithm>
#include <cmath>

// Every fused multiply-add below is written as one (fmaf), as in cnf_stein.hip: the pair value is that unit's
#pragma clang fp contract(off)

namespace cnf {
namespace {

constexpr int BOOT_THREADS = PAIR_THREADS, BOOT_TILE = PAIR_TILE;
constexpr int BOOT_WAVES = BOOT_THREADS / 64;
constexpr int BOOT_ROWS = 16 * BOOT_WAVES;       // rows per workgroup: a wave's MFMA block of 16, four waves
// Sign vectors per pass: 8 blocks x 4 accumulator registers.  By register count (DESIGN.md 5.3u has the table): at 128
// every instantiation stays under the 256 VGPRs of two waves per SIMD with no spill, D = 14 with four terms included
constexpr int BOOT_CHUNK = 128;
constexpr int BOOT_BLOCKS = BOOT_CHUNK / 16, BOOT_WORDS = BOOT_CHUNK / 32;
constexpr int BOOT_MIN_P = 32, BOOT_MAX_P = 1024;
constexpr int BOOT_MAX_TERMS = CNF_STEIN_MAX_TERMS;
static_assert(BOOT_THREADS == 256 && BOOT_TILE == 64 && BOOT_ROWS == 64, "boot_kernel's tile geometry");
static_assert(BOOT_CHUNK == 128, "the chunk: 32 row-sign bits in one word, four sign words in one LDS read");
static_assert(BOOT_TILE * BOOT_WORDS % BOOT_THREADS == 0, "boot_kernel stages the tile's sign words in whole rounds");

typedef float boot_f4 __attribute__((ext_vector_type(4)));

// cnf_stein.hip's StCoef without the gradient's k3: a_b = c_b^2 (IMQ: u_b = q + a_b) or -log2 e / (2 h_b^2) (Gaussian:
// e_b = exp2(a_b q)); p_m += k_m[b] times the term's m-th factor
struct BootCoef {
  float a[BOOT_MAX_TERMS], k0[BOOT_MAX_TERMS], k1[BOOT_MAX_TERMS], k2[BOOT_MAX_TERMS];
  float beta;
};

int64_t boot_row_groups(int64_t N) { return pair_row_groups(N, BOOT_ROWS); }
int32_t boot_passes(int32_t P) { return (P + BOOT_CHUNK - 1) / BOOT_CHUNK; }

// Column splits over the set's tiles: a function of the sizes alone (not of P)
int32_t boot_splits(int32_t S, int64_t N) { return pair_splits((int64_t)S * boot_row_groups(N), pair_tiles(N)); }

// Workspace: doubles [S][row groups x splits][P + 2] = (q [P], t, the diagonal sum)
int64_t boot_partials(int32_t S, int64_t N) { return (int64_t)S * boot_row_groups(N) * boot_splits(S, N); }
int64_t boot_workspace_bytes(int32_t S, int64_t N, int32_t P) {
  return boot_partials(S, N) * ((int64_t)P + 2) * (int64_t)sizeof(double);
}

// The Stein kernel value of cnf_stein.hip's st_tile, restated: differences first, then q, ss, dds by fmaf in ascending
// d, the terms in ascending b, the value without the gradient's p3.  (The pair i == j is zeroed by the caller, by index.)
template <int D, int KIND, int NT>
__device__ __forceinline__ float boot_pair(const float (&x)[D], const float (&s)[D], const float (&c)[D], const float (&h)[D],
                                           const BootCoef& k) {
  float diff[D], ds[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    diff[d] = x[d] - c[d];
    ds[d] = h[d] - s[d];
  }
  float q = diff[0] * diff[0], ss = s[0] * h[0], dds = diff[0] * ds[0];
#pragma unroll
  for (int d = 1; d < D; ++d) {
    q = fmaf(diff[d], diff[d], q);
    ss = fmaf(s[d], h[d], ss);
    dds = fmaf(diff[d], ds[d], dds);
  }
  float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    if constexpr (KIND == CNF_STEIN_IMQ) {
      const float u = q + k.a[b];
      const float inv = __builtin_amdgcn_rcpf(u);
      const float t0 = __builtin_amdgcn_exp2f(k.beta * __builtin_amdgcn_logf(u));
      const float t1 = t0 * inv, t2 = t1 * inv;
      p0 = fmaf(t0, k.k0[b], p0);
      p1 = fmaf(t1, k.k1[b], p1);
      p2 = fmaf(t2, k.k2[b], p2);
    } else {
      const float e = __builtin_amdgcn_exp2f(q * k.a[b]);
      p0 = fmaf(e, k.k0[b], p0);
      p1 = fmaf(e, k.k1[b], p1);
      p2 = fmaf(e, k.k2[b], p2);
    }
  }
  const float p2q = p2 * q;
  return fmaf(p0, ss, fmaf(p1, fmaf(2.0f, dds, -2.0f * D), -4.0f * p2q));
}

// What a thread stages of one column tile: its share of the 64 x D coordinates, of the 64 x D score components behind
// them and of the 64 x BOOT_WORDS sign words
template <int D> struct BootStage {
  static constexpr int NC = (2 * BOOT_TILE * D + BOOT_THREADS - 1) / BOOT_THREADS, NL = BOOT_TILE * BOOT_WORDS / BOOT_THREADS;
  float c[NC];
  uint32_t w[NL];
};

template <int D>
__device__ __forceinline__ void boot_load(BootStage<D>& st, const float* __restrict__ xs, const float* __restrict__ ss,
                                          int64_t N, const uint32_t* __restrict__ signs, int PW, int word0, int64_t c0) {
  const int t = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < BootStage<D>::NC; ++k) {
    const int e = t + k * BOOT_THREADS;
    const bool second = e >= BOOT_TILE * D;          // the score follows the points, in LDS as in the arguments
    const int64_t f = c0 * D + (second ? e - BOOT_TILE * D : e);
    st.c[k] = (e < 2 * BOOT_TILE * D && f < N * D) ? (second ? ss[f] : xs[f]) : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < BootStage<D>::NL; ++k) {
    const int e = t + k * BOOT_THREADS, w = word0 + e % BOOT_WORDS;
    const int64_t j = c0 + e / BOOT_WORDS;
    // stored inverted: a set bit (+1) is a clear sign bit
    st.w[k] = ~((j < N && w < PW) ? signs[j * PW + w] : 0u);
  }
}

template <int D>
__device__ __forceinline__ void boot_store(const BootStage<D>& st, float* s_col, uint32_t* s_sgn) {
  const int t = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < BootStage<D>::NC; ++k) {
    const int e = t + k * BOOT_THREADS;
    if (e < 2 * BOOT_TILE * D) s_col[e] = st.c[k];
  }
#pragma unroll
  for (int k = 0; k < BootStage<D>::NL; ++k) s_sgn[t + k * BOOT_THREADS] = st.w[k];
}

// grid (row groups x SPL, S x passes): blockIdx.x = row group * SPL + split, blockIdx.y = s * passes + pass
template <int D, int KIND, int NT>
__global__ __launch_bounds__(BOOT_THREADS, 2) void boot_kernel(const float* __restrict__ x, const float* __restrict__ score,
                                                               int64_t N, const uint32_t* __restrict__ signs, int32_t P,
                                                               int32_t SPL, int32_t passes, const BootCoef k, double phi0,
                                                               double dphi0, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float s_col[2][2 * BOOT_TILE * D];
  __shared__ __attribute__((aligned(16))) uint32_t s_sgn[2][BOOT_TILE * BOOT_WORDS];
  __shared__ double s_red[BOOT_WAVES][BOOT_CHUNK];
  __shared__ double s_t[BOOT_WAVES][2];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, s15 = lane & 15;
  const int s = (int)blockIdx.y / passes, pass = (int)blockIdx.y % passes;
  const int64_t rg = blockIdx.x / (unsigned)SPL;
  const int sp = (int)(blockIdx.x % (unsigned)SPL);
  const int PW = P / 32, word0 = pass * BOOT_WORDS;
  const float* xs = x + (int64_t)s * N * D;
  const float* ss = score + (int64_t)s * N * D;

  // the lane's row as the A operand sees it: row s15 of the wave's 16
  const int64_t i = rg * BOOT_ROWS + wave * 16 + s15;
  float xr[D], sr[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    xr[d] = i < N ? xs[i * D + d] : 0.0f;
    sr[d] = i < N ? ss[i * D + d] : 0.0f;
  }
  // ... and the rows it folds, 4 g + r: bit 4 b + r of neg is set where row 4 g + r has the sign -1 under vector
  // 16 b + s15 of this pass
  uint32_t neg = 0u;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t ir = rg * BOOT_ROWS + wave * 16 + 4 * g + r;
#pragma unroll
    for (int w = 0; w < BOOT_WORDS; ++w) {
      const uint32_t word = ~((ir < N && word0 + w < PW) ? signs[ir * PW + word0 + w] : 0u);
#pragma unroll
      for (int o = 0; o < 2; ++o) neg |= ((word >> (16 * o + s15)) & 1u) << (4 * (2 * w + o) + r);
    }
  }

  boot_f4 acc[BOOT_BLOCKS], acct = boot_f4{0.0f, 0.0f, 0.0f, 0.0f};
  double qd[BOOT_BLOCKS], td = 0.0;
#pragma unroll
  for (int b = 0; b < BOOT_BLOCKS; ++b) {
    acc[b] = boot_f4{0.0f, 0.0f, 0.0f, 0.0f};
    qd[b] = 0.0;
  }

  const auto [t0, t1] = pair_tile_range<int64_t>(N, SPL, sp);        // (may be empty: zeros)
  BootStage<D> st;
  if (t0 < t1) {
    boot_load<D>(st, xs, ss, N, signs, PW, word0, t0 * BOOT_TILE);
    boot_store<D>(st, s_col[0], s_sgn[0]);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t c0 = tile * BOOT_TILE;
    if (tile + 1 < t1) boot_load<D>(st, xs, ss, N, signs, PW, word0, c0 + BOOT_TILE);
    const float* col = s_col[cur];
    const uint32_t* sgn = s_sgn[cur];
#pragma unroll 2
    for (int step = 0; step < BOOT_TILE / 4; ++step) {
      const int jl = 4 * step + g;
      float c[D], h[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        c[d] = col[jl * D + d];
        h[d] = col[BOOT_TILE * D + jl * D + d];
      }
      float v = boot_pair<D, KIND, NT>(xr, sr, c, h, k);
      const int64_t j = c0 + jl;
      v = (j == i || j >= N || i >= N) ? 0.0f : v;           // the diagonal and the padding, by index
      // t = 1' H 1 in the chains of an all +1 vector (pass 0 alone; wave-uniform)
      if (pass == 0) acct = __builtin_amdgcn_mfma_f32_16x16x4f32(v, 1.0f, acct, 0, 0, 0);
      const uint4 u = *reinterpret_cast<const uint4*>(sgn + jl * BOOT_WORDS);
      const uint32_t w[BOOT_WORDS] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int b = 0; b < BOOT_BLOCKS; ++b) {
        // bit 16 (b & 1) + s15 of the (inverted) word into the sign bit of 1.0f
        const uint32_t sign = (w[b / 2] << (31 - 16 * (b & 1) - s15)) & 0x80000000u;
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, __uint_as_float(sign | 0x3f800000u), acc[b], 0, 0, 0);
      }
    }
    // 64 pair terms per accumulator register: fold.  Register r is C[row 4 g + r][vector 16 b + s15]
#pragma unroll
    for (int r = 0; r < 4; ++r) td += (double)acct[r];
    acct = boot_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int b = 0; b < BOOT_BLOCKS; ++b) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t flip = ((neg >> (4 * b + r)) & 1u) << 31;
        qd[b] += (double)__uint_as_float(__float_as_uint(acc[b][r]) ^ flip);
      }
      acc[b] = boot_f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    if (tile + 1 < t1) boot_store<D>(st, s_col[cur ^ 1], s_sgn[cur ^ 1]);
    __syncthreads();                               // (the other buffer was last read before the previous barrier)
    cur ^= 1;
  }

  // the diagonal k_p(x_i, x_i) = phi(0) |s_i|^2 - 2 D phi'(0), once per row: lane group 0 of split 0, pass 0
  double dd = 0.0;
  if (sp == 0 && pass == 0 && g == 0 && i < N) {
    double n2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) n2 += (double)sr[d] * (double)sr[d];
    dd = phi0 * n2 - 2.0 * D * dphi0;
  }

  // the lane groups g of a wave (the rows), then the waves in ascending order
#pragma unroll
  for (int b = 0; b < BOOT_BLOCKS; ++b) {
    double qv = qd[b];
    qv += __shfl_xor(qv, 16);
    qv += __shfl_xor(qv, 32);
    if (g == 0) s_red[wave][16 * b + s15] = qv;
  }
  // t as an all +1 vector's q is reduced (every column of its MFMA block holds the same sums: column 0's are taken)
  td += __shfl_xor(td, 16);
  td += __shfl_xor(td, 32);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) dd += __shfl_xor(dd, o);
  if (lane == 0) {
    s_t[wave][0] = td;
    s_t[wave][1] = dd;
  }
  __syncthreads();
  double* part = ws + (((int64_t)s * gridDim.x) + blockIdx.x) * ((int64_t)P + 2);
  if (t < BOOT_CHUNK) {
    double v = s_red[0][t];
#pragma unroll
    for (int w = 1; w < BOOT_WAVES; ++w) v += s_red[w][t];
    if (pass * BOOT_CHUNK + t < P) part[pass * BOOT_CHUNK + t] = v;
  }
  if (t >= BOOT_CHUNK && t < BOOT_CHUNK + 2 && pass == 0) {
    const int e = t - BOOT_CHUNK;                    // 0: t, 1: the diagonal sum (0 from every split but the first)
    double v = s_t[0][e];
#pragma unroll
    for (int w = 1; w < BOOT_WAVES; ++w) v += s_t[w][e];
    part[P + e] = v;
  }
}

// thread (s, p): the partials in ascending (row group, split) order, then the statistic in double
__global__ __launch_bounds__(BOOT_THREADS) void boot_finish_kernel(const double* __restrict__ ws, int32_t S, int64_t N, int32_t P,
                                                                   int64_t groups, double* __restrict__ stats,
                                                                   double* __restrict__ raw) {
  const int64_t e = (int64_t)blockIdx.x * BOOT_THREADS + threadIdx.x;
  if (e >= (int64_t)S * P) return;
  const int64_t s = e / P, p = e % P, stride = (int64_t)P + 2;
  const double* part = ws + s * groups * stride;
  double q = 0.0;
  for (int64_t gi = 0; gi < groups; ++gi) q += part[gi * stride + p];
  stats[e] = q / ((double)N * (double)(N - 1));
  if (raw) {
    raw[e] = q;
    if (p == 0) {
      double tt = 0.0, dd = 0.0;
      for (int64_t gi = 0; gi < groups; ++gi) {
        tt += part[gi * stride + P];
        dd += part[gi * stride + P + 1];
      }
      raw[(int64_t)S * P + s] = tt;
      raw[(int64_t)S * P + S + s] = dd;
    }
  }
}

struct BootLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *score;
  int64_t N;
  const uint32_t* signs;
  int32_t P, SPL, passes;
  BootCoef k;
  double phi0, dphi0;
  double* ws;
};

template <int D, int KIND, int NT = 1> void boot_launch_terms(int nt, const BootLaunch& a) {
  if (nt == NT)
    hipLaunchKernelGGL((boot_kernel<D, KIND, NT>), a.grid, dim3(BOOT_THREADS), 0, a.st, a.x, a.score, a.N, a.signs, a.P, a.SPL,
                       a.passes, a.k, a.phi0, a.dphi0, a.ws);
  else if constexpr (NT < BOOT_MAX_TERMS) boot_launch_terms<D, KIND, NT + 1>(nt, a);
}
template <int D> void boot_launch_kind(int kind, int nt, const BootLaunch& a) {
  if (kind == CNF_STEIN_IMQ) boot_launch_terms<D, CNF_STEIN_IMQ>(nt, a);
  else boot_launch_terms<D, CNF_STEIN_GAUSSIAN>(nt, a);      // (boot_coef has refused every other kind)
}

bool boot_shape_ok(int32_t S, int64_t N, int32_t D) { return ia_shape_ok(S, N, 0, D); }
bool boot_vectors_ok(int32_t P) { return P >= BOOT_MIN_P && P <= BOOT_MAX_P && P % 32 == 0; }

// cnf_stein.hip's st_coef, restated: the spec as boot_kernel reads it and phi(0), phi'(0) for the diagonal; false for
// what cnf_stein refuses in one (the third derivative's coefficient included: the same specs are legal in both)
bool boot_coef(const CnfSteinSpec* spec, BootCoef* k, int* nt, double* phi0, double* dphi0) {
  *k = BootCoef{};
  *phi0 = *dphi0 = 0.0;
  if (spec->kind != CNF_STEIN_IMQ && spec->kind != CNF_STEIN_GAUSSIAN) return false;
  if (spec->n_terms < 1 || spec->n_terms > BOOT_MAX_TERMS) return false;
  const double beta = (double)spec->beta;
  if (spec->kind == CNF_STEIN_IMQ && !(beta > -1.0 && beta < 0.0)) return false;
  *nt = spec->n_terms;
  k->beta = spec->kind == CNF_STEIN_IMQ ? spec->beta : 0.0f;
  for (int b = 0; b < *nt; ++b) {
    const double w = (double)spec->w[b], bw = (double)spec->bw[b];
    if (!(w > 0.0) || !std::isfinite(w) || !(bw > 0.0) || !std::isfinite(bw)) return false;
    double c[4];
    if (spec->kind == CNF_STEIN_IMQ) {
      const double c2 = bw * bw;
      if (!fits_float(c2) || !(c2 >= 1.1754943508222875e-38) || !fits_float(1.0 / c2)) return false;
      c[0] = w; c[1] = w * beta; c[2] = c[1] * (beta - 1.0); c[3] = c[2] * (beta - 2.0);
      if (!fits_float(c[3] * std::pow(c2, beta - 3.0)) || !fits_float(w * std::pow(c2, beta))) return false;
      k->a[b] = (float)c2;
      *phi0 += w * std::pow(c2, beta);
      *dphi0 += c[1] * std::pow(c2, beta - 1.0);
    } else {
      const double ib = 1.0 / (2.0 * bw * bw);
      c[0] = w; c[1] = -w * ib; c[2] = w * ib * ib; c[3] = -w * ib * ib * ib;
      if (!fits_float(ib) || !fits_float(c[3])) return false;
      k->a[b] = (float)(-1.4426950408889634 * ib);
      if (!std::isfinite(k->a[b])) return false;
      *phi0 += w;
      *dphi0 += c[1];
    }
    k->k0[b] = (float)c[0]; k->k1[b] = (float)c[1]; k->k2[b] = (float)c[2];
  }
  return true;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_stein_boot_workspace(int32_t S, int64_t N, int32_t D, int32_t P, int64_t* bytes) {
  if (!bytes || !boot_shape_ok(S, N, D) || !boot_vectors_ok(P)) return CNF_ERR_INVALID;
  *bytes = boot_workspace_bytes(S, N, P);
  return CNF_OK;
}

extern "C" int cnf_stein_boot_splits(int32_t S, int64_t N, int32_t D) {
  return boot_shape_ok(S, N, D) ? boot_splits(S, N) : CNF_ERR_INVALID;
}

extern "C" int cnf_stein_boot(const CnfSteinSpec* spec, int32_t S, const float* x, const float* score, int64_t N, int32_t D,
                              const uint32_t* signs, int32_t P, double* stats, double* raw, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  if (!spec || !x || !score || !signs || !stats || !workspace || !boot_shape_ok(S, N, D) || !boot_vectors_ok(P))
    return CNF_ERR_INVALID;
  BootLaunch a{};
  int nt = 0;
  if (!boot_coef(spec, &a.k, &nt, &a.phi0, &a.dphi0)) return CNF_ERR_INVALID;
  if (workspace_bytes < boot_workspace_bytes(S, N, P)) return CNF_ERR_INVALID;
  a.SPL = boot_splits(S, N);
  a.passes = boot_passes(P);
  a.grid = dim3((unsigned)(boot_row_groups(N) * a.SPL), (unsigned)(S * a.passes));
  a.st = (hipStream_t)stream;
  a.x = x; a.score = score; a.N = N;
  a.signs = signs;
  a.P = P;
  a.ws = (double*)workspace;
  pair_dispatch_dim(D, [&](auto d) { boot_launch_kind<decltype(d)::value>(spec->kind, nt, a); });
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  hipLaunchKernelGGL(boot_finish_kernel, dim3((unsigned)(((int64_t)S * P + BOOT_THREADS - 1) / BOOT_THREADS)),
                     dim3(BOOT_THREADS), 0, a.st, (const double*)a.ws, S, N, P, boot_row_groups(N) * a.SPL, stats, raw);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
