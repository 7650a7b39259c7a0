// cnf_sliced.hip -- the sliced Wasserstein distance between two point clouds with uniform weights, for directions the
// caller supplies, with the per-projection values, their maximum and the envelope gradient in x.  Model-free, like
// cnf_mmd.hip and cnf_sinkhorn.hip, but N log N per projection where those walk all N x M pairs.
//
// THE DEFINITION (the contract; tests/sliced_ref.py restates it in float64).  Inputs x [S, N, D], y [S, M, D] and
// theta [P, D].  Per set s and projection p:
//   key      k_i = x[i, 0] theta[p, 0], then k_i = fmaf(x[i, d], theta[p, d], k_i) for d = 1 .. D - 1 in ascending d,
//            in float32; then k_i = fmaf(k_i, 0, k_i), which leaves a finite key as it is and turns an infinite one into
//            NaN (so that a non-finite coordinate ends as NaN and not as inf).  l_j the same for y.
//   order    both key arrays ascending, ties broken by the sample's index.  A NaN sorts by its bit pattern: above +inf
//            with a clear sign bit, below -inf with a set one.
//   value    w[s, p] = 1/2 sum_i sum_j o_ij (k_(i) - l_(j))^2,
//            o_ij = max(0, min((i + 1) M, (j + 1) N) - max(i M, j N)) / (N M): the length on which the quantile
//            functions of the two empirical measures sit at ranks i and j, formed in 64-bit integers up to the one
//            division.  Rank i of x meets the ranks floor(i M / N) .. floor(((i + 1) M - 1) / N) of y.
//   SW[s] = (1 / P) sum_p w[s, p], the cost |.|^2 / 2 of utils.sinkhorn;  max-sliced = max_p w[s, p].
//   gradient grad[s, i, :] = (1 / P) sum_p a[s, p, i] theta[p, :] + 0 SW[s],  a = sum_j o_ij (k_i - l_j) at the rank
//            sample i took (the permutation held fixed: exact wherever the keys are distinct).  The last term is 0 for a
//            finite SW and makes every gradient row of a set NaN whose value is NaN.
//
// THE KERNELS.  A key is 64 bits: the order-preserving unsigned image of the float above the sample's index, so that
// one integer sort is stable and carries the permutation.  Projections are processed in groups of G; a row is one
// (set, projection of the group) and holds the N keys of x and then the M keys of y.
//   sliced_sort_kernel<D>  one workgroup per (row, cloud, tile of SL_TILE keys): forms the keys (coalesced), pads the
//       tile with the all-ones key (above every real key), sorts it in LDS by a bitonic network -- a lane owns SL_E = 16
//       consecutive keys, and the stages of distance < 16 run in its registers -- and writes a sorted run.
//   sliced_merge_kernel    one pass doubles the run length; it runs only for a cloud of more than one tile.  A
//       workgroup owns SL_TILE consecutive outputs of one pair of runs: two lanes find its two input ranges by binary
//       search on the merge path, the ranges are staged in LDS, every lane finds its own 16 outputs' start the same way
//       and merges them serially.  Keys are distinct (the index), so no tie rule is needed here.
//   sliced_w2_kernel       one lane per rank of x: the short loop over the ranks of y it meets, in double; a stored to
//       the slot of the sample's own index (each index occurs once per row: plain stores); the workgroup's value in a
//       fixed tree to one partial.
//   sliced_value_kernel    a row's partials in a fixed strided order and a fixed tree -> sums[s, p].
//   sliced_grad_kernel     one lane per (set, sample, coordinate): the running gradient is a DOUBLE in the workspace,
//       overwritten by the first group, added to in ascending p by every group, and rounded once to float32 by the last:
//       the same operations on the same doubles for every G, so the result does not depend on G.
//   sliced_mean_kernel     after the last group: the mean in ascending p and the maximum (a NaN stays).
// The value and gradient finishes are three kernels and not the one the sort and merge kernels feed because the
// gradient's last step reads SW[s], which exists only after every projection's value does.
// No atomics, no waiting between workgroups, every loop counted; every workspace word read was written by this call.
#include "cnf_host.h"

#include <math.h>

#include <algorithm>
#include <cmath>

// Every fused multiply-add below is written as one (fmaf / fma): the key's operation order is part of the contract
#pragma clang fp contract(off)

namespace cnf {
namespace {

#ifndef SL_TILE
#define SL_TILE 4096                             // keys per sorted tile (an experiment may set another power of two)
#endif
constexpr int SL_E = 16;                         // consecutive keys a lane owns
constexpr int SL_T = SL_TILE;
constexpr int SL_THREADS = SL_T / SL_E;          // lanes per workgroup of the sort and merge kernels
constexpr int SL_LDS = SL_T + SL_T / SL_E;       // keys of LDS: one pad per 16 keeps a lane's 16 off its neighbours' banks
constexpr int SL_ROWS = 256;                     // ranks per workgroup of sliced_w2_kernel (and lanes of the finishes)
constexpr int SL_MAX_S = 64;
constexpr int SL_MAX_D = 14;
constexpr int SL_MAX_P = 1024;
constexpr int64_t SL_MAX_N = int64_t(1) << 20;
constexpr uint64_t SL_PAD = ~uint64_t(0);
static_assert((SL_T & (SL_T - 1)) == 0 && SL_THREADS >= 128 && SL_THREADS <= 1024, "SL_TILE: a power of two, 2048 .. 16384");

__host__ __device__ inline int64_t sl_tiles(int64_t n) { return (n + SL_T - 1) / SL_T; }
__host__ __device__ inline int64_t sl_blocks(int64_t n) { return (n + SL_ROWS - 1) / SL_ROWS; }
// merge passes a cloud of n keys needs: run lengths SL_T, 2 SL_T, ... until one run holds it
inline int sl_passes(int64_t n) {
  int k = 0;
  for (int64_t run = SL_T; run < n; run *= 2) ++k;
  return k;
}

// Workspace, all 8-byte words: keys [2][S G (N + M)] (ping and pong), partial [S G blocks(N)] doubles, and with the
// gradient coef [S G N] doubles and gacc [S N D] doubles (the running gradient)
struct SlLayout {
  int64_t keys, partial, coef, gacc, bytes;      // byte offsets and the total
};
SlLayout sl_layout(int32_t S, int64_t N, int64_t M, int32_t D, int32_t G, bool want_grad) {
  const int64_t R = (int64_t)S * G;
  SlLayout l;
  l.keys = 0;
  l.partial = 2 * R * (N + M) * 8;
  l.coef = l.partial + R * sl_blocks(N) * 8;
  l.gacc = l.coef + (want_grad ? R * N * 8 : 0);
  l.bytes = l.gacc + (want_grad ? (int64_t)S * N * D * 8 : 0);
  return l;
}

// float -> unsigned, order-preserving, and back
__device__ __forceinline__ uint32_t sl_image(float k) {
  const uint32_t b = __float_as_uint(k);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sl_float(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

__device__ __forceinline__ int sl_phys(int e) { return e + (e >> 4); }

// ascending (asc) or descending order of the pair
__device__ __forceinline__ void sl_cmpx(uint64_t& a, uint64_t& b, bool asc) {
  const bool sw = (a > b) == asc;
  const uint64_t lo = sw ? b : a, hi = sw ? a : b;
  a = lo;
  b = hi;
}

// the stages of distance 8, 4, 2, 1 of one merge step inside a lane's 16 keys, all in the direction asc
__device__ __forceinline__ void sl_reg_merge(uint64_t (&v)[SL_E], bool asc) {
#pragma unroll
  for (int j = SL_E / 2; j >= 1; j >>= 1) {
#pragma unroll
    for (int e = 0; e < SL_E; ++e)
      if ((e & j) == 0) sl_cmpx(v[e], v[e | j], asc);
  }
}

// a lane's 16 keys sorted by the network's steps k = 2 .. 16; asc16: the direction of step 16 (bit 16 of the lane's base)
__device__ __forceinline__ void sl_reg_sort(uint64_t (&v)[SL_E], bool asc16) {
#pragma unroll
  for (int k = 2; k <= SL_E; k <<= 1) {
#pragma unroll
    for (int j = k / 2; j >= 1; j >>= 1) {
#pragma unroll
      for (int e = 0; e < SL_E; ++e)
        if ((e & j) == 0) sl_cmpx(v[e], v[e | j], k == SL_E ? asc16 : (e & k) == 0);
    }
  }
}

struct SlArgs {
  int64_t N, M;
  int32_t G, p0;                                 // projections in this group, and the first of them
  int32_t tN, tM;                                // tiles of x and of y
};

// One workgroup per (row, cloud, tile): blockIdx.x = row (tN + tM) + u, u running over the tiles of x and then of y
template <int D>
__global__ __launch_bounds__(SL_THREADS) void sliced_sort_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 const float* __restrict__ theta,
                                                                 uint64_t* __restrict__ keys, const SlArgs a) {
  __shared__ uint64_t lds[SL_LDS];
  const int t = (int)threadIdx.x;
  const int tiles = a.tN + a.tM;
  const int64_t row = blockIdx.x / (unsigned)tiles;
  int u = (int)(blockIdx.x % (unsigned)tiles);
  const bool is_y = u >= a.tN;
  if (is_y) u -= a.tN;
  const int64_t s = row / a.G;
  const int p = a.p0 + (int)(row % a.G);
  const int64_t n = is_y ? a.M : a.N;
  const float* pts = is_y ? y + s * a.M * D : x + s * a.N * D;
  const float* th = theta + (int64_t)p * D;      // wave-uniform: scalar loads
  const int64_t first = (int64_t)u * SL_T;
  const int cnt = (int)(n - first < SL_T ? n - first : SL_T);
  float dir[D];
#pragma unroll
  for (int d = 0; d < D; ++d) dir[d] = th[d];
#pragma unroll
  for (int q = 0; q < SL_E; ++q) {
    const int e = t + q * SL_THREADS;
    uint64_t key = SL_PAD;
    if (e < cnt) {
      const float* pt = pts + (first + e) * D;
      float k = pt[0] * dir[0];
#pragma unroll
      for (int d = 1; d < D; ++d) k = fmaf(pt[d], dir[d], k);
      k = fmaf(k, 0.0f, k);                      // finite: unchanged; infinite: NaN
      key = ((uint64_t)sl_image(k) << 32) | (uint32_t)(first + e);
    }
    lds[sl_phys(e)] = key;
  }
  __syncthreads();
  uint64_t v[SL_E];
  const int base = t * SL_E;
#pragma unroll
  for (int e = 0; e < SL_E; ++e) v[e] = lds[t * (SL_E + 1) + e];
  sl_reg_sort(v, (base & SL_E) == 0);
  for (int k = 2 * SL_E; k <= SL_T; k <<= 1) {
#pragma unroll
    for (int e = 0; e < SL_E; ++e) lds[t * (SL_E + 1) + e] = v[e];
    __syncthreads();
    for (int j = k / 2; j >= SL_E; j >>= 1) {
#pragma unroll
      for (int q = 0; q < SL_E / 2; ++q) {
        const int pr = t + q * SL_THREADS;
        const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1));
        uint64_t lo = lds[sl_phys(i)], hi = lds[sl_phys(i + j)];
        sl_cmpx(lo, hi, (i & k) == 0);
        lds[sl_phys(i)] = lo;
        lds[sl_phys(i + j)] = hi;
      }
      __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < SL_E; ++e) v[e] = lds[t * (SL_E + 1) + e];
    sl_reg_merge(v, (base & k) == 0);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < SL_E; ++e) lds[t * (SL_E + 1) + e] = v[e];
  __syncthreads();
  uint64_t* out = keys + row * (a.N + a.M) + (is_y ? a.N : 0) + first;
#pragma unroll
  for (int q = 0; q < SL_E; ++q) {
    const int e = t + q * SL_THREADS;
    if (e < cnt) out[e] = lds[sl_phys(e)];       // (the pads are the last SL_T - cnt keys)
  }
}

// The number of keys of A [0, la) among the first d of the merge of A and B [0, lb); keys are distinct
template <class PA, class PB>
__device__ __forceinline__ int64_t sl_corank(int64_t d, PA A, int64_t la, PB B, int64_t lb) {
  int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (A[mid] < B[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct SlMergeArgs {
  int64_t N, M, run;                             // run: the length of the sorted runs that come in
  int32_t segN, segM;                            // output segments of x and of y in this pass (0: the cloud is done)
};

// One workgroup per (row, cloud, segment of SL_T outputs): blockIdx.x = row (segN + segM) + u
__global__ __launch_bounds__(SL_THREADS) void sliced_merge_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                                  const SlMergeArgs a) {
  __shared__ uint64_t lds[SL_LDS];
  __shared__ int64_t cut[2];
  const int t = (int)threadIdx.x;
  const int segs = a.segN + a.segM;
  const int64_t row = blockIdx.x / (unsigned)segs;
  int u = (int)(blockIdx.x % (unsigned)segs);
  const bool is_y = u >= a.segN;
  if (is_y) u -= a.segN;
  const int64_t n = is_y ? a.M : a.N;
  const int64_t cloud = row * (a.N + a.M) + (is_y ? a.N : 0);
  const int64_t o0 = (int64_t)u * SL_T, o1 = o0 + SL_T < n ? o0 + SL_T : n;
  const int64_t ps = o0 / (2 * a.run) * (2 * a.run);                        // the pair of runs this segment lies in
  const int64_t a_end = ps + a.run < n ? ps + a.run : n, b_end = ps + 2 * a.run < n ? ps + 2 * a.run : n;
  const uint64_t* A = in + cloud + ps;
  const uint64_t* B = in + cloud + a_end;
  const int64_t lenA = a_end - ps, lenB = b_end - a_end;
  if (t == 0) cut[0] = sl_corank(o0 - ps, A, lenA, B, lenB);
  if (t == 64) cut[1] = sl_corank(o1 - ps, A, lenA, B, lenB);
  __syncthreads();
  const int64_t a0 = cut[0], a1 = cut[1], b0 = o0 - ps - a0;
  const int la = (int)(a1 - a0), cnt = (int)(o1 - o0), lb = cnt - la;
#pragma unroll
  for (int q = 0; q < SL_E; ++q) {
    const int e = t + q * SL_THREADS;
    if (e < cnt) lds[e] = e < la ? A[a0 + e] : B[b0 + (e - la)];
  }
  __syncthreads();
  const int d0 = t * SL_E < cnt ? t * SL_E : cnt;
  const uint64_t* LA = lds;
  const uint64_t* LB = lds + la;
  int ia = (int)sl_corank(d0, LA, la, LB, lb), ib = d0 - ia;
  uint64_t v[SL_E];
#pragma unroll
  for (int e = 0; e < SL_E; ++e) {
    const uint64_t ka = ia < la ? LA[ia] : SL_PAD, kb = ib < lb ? LB[ib] : SL_PAD;     // (a real key is below the pad)
    const bool take_a = ka < kb;
    v[e] = take_a ? ka : kb;
    ia += take_a;
    ib += !take_a;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < SL_E; ++e) lds[t * (SL_E + 1) + e] = v[e];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < SL_E; ++q) {
    const int e = t + q * SL_THREADS;
    if (e < cnt) out[cloud + o0 + e] = lds[sl_phys(e)];
  }
}

// One lane per (row, rank of x): blockIdx.x = row blocks(N) + block
__global__ __launch_bounds__(SL_ROWS) void sliced_w2_kernel(const uint64_t* __restrict__ kx, const uint64_t* __restrict__ ky,
                                                            double* __restrict__ coef, double* __restrict__ partial,
                                                            int64_t N, int64_t M) {
  __shared__ double red[SL_ROWS];
  const int t = (int)threadIdx.x;
  const int64_t nb = sl_blocks(N);
  const int64_t row = blockIdx.x / (uint64_t)nb, i = (blockIdx.x % (uint64_t)nb) * SL_ROWS + t;
  double val = 0.0;
  if (i < N) {
    const uint64_t key = kx[row * (N + M) + i];
    const double k = (double)sl_float((uint32_t)(key >> 32));
    const uint64_t* l = ky + row * (N + M) + N;
    const double nm = (double)(N * M);
    const int64_t x0 = i * M, x1 = x0 + M;
    const int64_t j0 = x0 / N, j1 = (x1 - 1) / N;
    double acc = 0.0;
    for (int64_t j = j0; j <= j1; ++j) {
      const int64_t y0 = j * N, y1 = y0 + N;
      const int64_t len = (x1 < y1 ? x1 : y1) - (x0 > y0 ? x0 : y0);
      const double o = (double)len / nm;
      const double diff = k - (double)sl_float((uint32_t)(l[j] >> 32));
      acc = fma(o, diff, acc);
      val = fma(o * diff, diff, val);
    }
    if (coef && (int64_t)(uint32_t)key < N) coef[row * N + (uint32_t)key] = acc;      // (always: a key carries its sample)
  }
  red[t] = val;
  __syncthreads();
  for (int o = SL_ROWS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) partial[blockIdx.x] = 0.5 * red[0];
}

// Workgroup = row (s, g): its partials, lane t taking t, t + 256, ..., the lanes' totals meeting in a fixed tree
__global__ __launch_bounds__(SL_ROWS) void sliced_value_kernel(const double* __restrict__ partial, int64_t nb, int32_t G,
                                                               int32_t p0, int32_t P, double* __restrict__ sums) {
  __shared__ double red[SL_ROWS];
  const int t = (int)threadIdx.x;
  const double* p = partial + (int64_t)blockIdx.x * nb;
  double acc = 0.0;
  for (int64_t b = t; b < nb; b += SL_ROWS) acc += p[b];
  red[t] = acc;
  __syncthreads();
  for (int o = SL_ROWS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) sums[(int64_t)(blockIdx.x / (unsigned)G) * (P + 2) + p0 + (int)(blockIdx.x % (unsigned)G)] = red[0];
}

// Workgroup = set: the mean of its P values in ascending p and their maximum (a NaN stays)
__global__ __launch_bounds__(64) void sliced_mean_kernel(double* __restrict__ sums, int32_t P) {
  if (threadIdx.x != 0) return;
  double* w = sums + (int64_t)blockIdx.x * (P + 2);
  double sum = 0.0, mx = w[0];
  for (int p = 0; p < P; ++p) {
    sum += w[p];
    mx = (mx != mx || w[p] <= mx) ? mx : w[p];
  }
  w[P] = sum / (double)P;
  w[P + 1] = mx;
}

struct SlGradArgs {
  const double* coef;                            // [S, G, N]
  const float* theta;                            // [P, D]
  const double* sums;                            // [S, P + 2], complete in the last group
  double* gacc;                                  // [S, N, D]
  float* grad;                                   // [S, N, D]
  int64_t N, total;                              // total = S N D
  int32_t D, G, p0, P, first, last;
};

// One lane per (set, sample, coordinate)
__global__ __launch_bounds__(SL_ROWS) void sliced_grad_kernel(const SlGradArgs a) {
  const int64_t e = (int64_t)blockIdx.x * SL_ROWS + threadIdx.x;
  if (e >= a.total) return;
  const int d = (int)(e % a.D);
  const int64_t si = e / a.D, s = si / a.N, i = si % a.N;
  double acc = a.first ? 0.0 : a.gacc[e];
  const double* c = a.coef + s * a.G * a.N + i;
  for (int g = 0; g < a.G; ++g) acc = fma(c[(int64_t)g * a.N], (double)a.theta[(int64_t)(a.p0 + g) * a.D + d], acc);
  if (a.last) a.grad[e] = (float)(acc / (double)a.P + 0.0 * a.sums[s * (a.P + 2) + a.P]);
  else a.gacc[e] = acc;
}

template <int D = 1>
int sl_launch_sort(int dim, int64_t grid, hipStream_t st, const float* x, const float* y, const float* theta, uint64_t* keys,
                   const SlArgs& a) {
  if (dim == D) return launch_plain(sliced_sort_kernel<D>, grid, SL_THREADS, 0, st, x, y, theta, keys, a);
  if constexpr (D < SL_MAX_D) return sl_launch_sort<D + 1>(dim, grid, st, x, y, theta, keys, a);
  return CNF_ERR_INVALID;
}

bool sl_shape_ok(int32_t S, int64_t N, int64_t M, int32_t D) {
  return S >= 1 && S <= SL_MAX_S && N >= 1 && M >= 1 && N <= SL_MAX_N && M <= SL_MAX_N && D >= 1 && D <= SL_MAX_D;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_sliced_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t G, int32_t want_grad, int64_t* bytes) {
  if (!bytes || !sl_shape_ok(S, N, M, D) || G < 1 || G > SL_MAX_P) return CNF_ERR_INVALID;
  *bytes = sl_layout(S, N, M, D, G, want_grad != 0).bytes;
  return CNF_OK;
}

extern "C" int cnf_sliced_tile(void) { return SL_T; }

extern "C" int cnf_sliced_w2(int32_t S, const float* x, int64_t N, const float* y, int64_t M, int32_t D, const float* theta,
                             int32_t P, int32_t G, double* sums, float* grad, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  if (!x || !y || !theta || !sums || !workspace || !sl_shape_ok(S, N, M, D)) return CNF_ERR_INVALID;
  if (P < 1 || P > SL_MAX_P || G < 1 || G > P) return CNF_ERR_INVALID;
  const SlLayout l = sl_layout(S, N, M, D, G, grad != nullptr);
  if (workspace_bytes < l.bytes) return CNF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int64_t W = N + M, nb = sl_blocks(N);
  uint64_t* buf[2] = {(uint64_t*)(ws + l.keys), (uint64_t*)(ws + l.keys) + (int64_t)S * G * W};
  double* partial = (double*)(ws + l.partial);
  double* coef = grad ? (double*)(ws + l.coef) : nullptr;
  double* gacc = grad ? (double*)(ws + l.gacc) : nullptr;
  const int passN = sl_passes(N), passM = sl_passes(M);

  int rc = CNF_OK;
  for (int32_t p0 = 0; p0 < P && rc == CNF_OK; p0 += G) {
    const int32_t g = std::min(G, P - p0);
    const int64_t R = (int64_t)S * g;
    SlArgs a{};
    a.N = N; a.M = M; a.G = g; a.p0 = p0;
    a.tN = (int32_t)sl_tiles(N);
    a.tM = (int32_t)sl_tiles(M);
    rc = sl_launch_sort(D, R * (a.tN + a.tM), st, x, y, theta, buf[0], a);
    // pass k merges runs of SL_T 2^k keys from buf[k % 2] into the other; a cloud that is one run already stays where it is
    int64_t run = SL_T;
    for (int k = 0; k < std::max(passN, passM) && rc == CNF_OK; ++k, run *= 2) {
      SlMergeArgs m{};
      m.N = N; m.M = M; m.run = run;
      m.segN = k < passN ? a.tN : 0;
      m.segM = k < passM ? a.tM : 0;
      rc = launch_plain(sliced_merge_kernel, R * (m.segN + m.segM), SL_THREADS, 0, st, (const uint64_t*)buf[k % 2],
                        buf[(k + 1) % 2], m);
    }
    if (rc != CNF_OK) break;
    rc = launch_plain(sliced_w2_kernel, R * nb, SL_ROWS, 0, st, (const uint64_t*)buf[passN % 2],
                      (const uint64_t*)buf[passM % 2], coef, partial, N, M);
    if (rc != CNF_OK) break;
    rc = launch_plain(sliced_value_kernel, R, SL_ROWS, 0, st, (const double*)partial, nb, g, p0, P, sums);
    if (rc != CNF_OK) break;
    const bool last = p0 + g >= P;
    if (last) rc = launch_plain(sliced_mean_kernel, (int64_t)S, 64, 0, st, sums, P);
    if (rc != CNF_OK || !grad) continue;
    SlGradArgs ga{};
    ga.coef = coef; ga.theta = theta; ga.sums = sums; ga.gacc = gacc; ga.grad = grad;
    ga.N = N; ga.total = (int64_t)S * N * D;
    ga.D = D; ga.G = g; ga.p0 = p0; ga.P = P; ga.first = p0 == 0; ga.last = last;
    rc = launch_plain(sliced_grad_kernel, (ga.total + SL_ROWS - 1) / SL_ROWS, SL_ROWS, 0, st, ga);
  }
  return rc;
}
