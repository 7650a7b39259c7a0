// cnf_pwl_build.h -- the BUILDER of the dim-2 conditioner tables (pwl_build_kernel and its helpers): included by the
// one translation unit that launches it (cnf_flow.hip).  The table layout and the readers are in cnf_pwl.h.
#pragma once

#include "cnf_pwl.h"

namespace cnf {

__global__ __launch_bounds__(512) void pwl_build_kernel(const float* __restrict__ weights /* prep + hdr */,
                                                        int64_t per_layer, const float* __restrict__ cvals,
                                                        float c_offset, int L, double sp_offset,
                                                        float* __restrict__ tables) {
  __shared__ double a1[PWL_H], b1v[PWL_H], W1[PWL_H * PWL_H], bb1[PWL_H], Wo[PWL_H * PWL_P], bo[PWL_P];
  __shared__ double bpu[PWL_H], sbp[PWL_H];
  __shared__ double candu[PWL_NPIECE - 1], cand[PWL_NPIECE - 1];
  __shared__ double PQ[PWL_CHUNK * PWL_H * 2];
  __shared__ double RAW[PWL_CHUNK * PWL_P * 2];     // (S, T about u_ref) of every output of the chunk's pieces
  __shared__ int bad[PWL_NPIECE];                  // piece needs the general spline evaluation
  __shared__ double urefs[PWL_CHUNK];
  __shared__ int icnt[17], ioff[17];               // finite roots per first-layer interval, and their prefix sums
  // Second-layer pre-activations P u + Q of every (first-layer interval, unit): inside an interval the first layer's
  // activity pattern is fixed, so every piece of the interval has these coefficients -- stage 1 below looks them up
  // instead of redoing the 16-term sums per (piece, unit).  biv[q]: the interval of the piece to the LEFT of
  // breakpoint q.
  __shared__ double IPQ[17 * PWL_H * 2];
  __shared__ int biv[PWL_NPIECE];
  const int tid = threadIdx.x;
  const int slice = blockIdx.x / L, l = blockIdx.x % L;
  const float* w = weights + l * per_layer;         // D = 2: the layer's only conditioner (d = 1)
  const double c = (double)cvals[slice] + (double)c_offset;
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  // flat layout: W0[2][16] | b0[16] | W1[16][16] | b1[16] | Wout[16][16] | bout[16]
  if (tid < PWL_H) {
    const double a = (double)w[PWL_H + tid], b = (double)w[tid] * c + (double)w[2 * PWL_H + tid];
    a1[tid] = a;
    b1v[tid] = b;
    bpu[tid] = a != 0.0 ? -b / a : INF;
    bb1[tid] = (double)w[3 * PWL_H + 256 + tid];
    // spline-side pre-scaling of the output layer (see above)
    bo[tid] = (double)w[3 * PWL_H + 256 + PWL_H + 256 + tid];
  }
  for (int i = tid; i < 256; i += blockDim.x) {
    W1[i] = (double)w[3 * PWL_H + i];
    Wo[i] = (double)w[3 * PWL_H + 256 + PWL_H + i];
  }
  __syncthreads();
  if (tid < PWL_H) {         // rank sort of the 16 first-layer breakpoints
    const double v = bpu[tid];
    int r = 0;
    for (int j = 0; j < PWL_H; ++j) r += (bpu[j] < v || (bpu[j] == v && j < tid)) ? 1 : 0;
    sbp[r] = v;
  }
  __syncthreads();
  auto test_point = [&](double lo, double hi) -> double {
    const bool fl = lo > -INF, fh = hi < INF;
    return fl && fh ? 0.5 * (lo + hi) : (fl ? lo + 1.0 : (fh ? hi - 1.0 : 0.0));
  };
  // second-layer zero crossings inside each of the 17 first-layer intervals
  double root = INF;
  const int iv = tid / PWL_H, kk = tid % PWL_H;        // interval, second-layer unit (tid < 17 * 16)
  if (tid < 17 * PWL_H) {
    const double lo = iv == 0 ? -INF : sbp[iv - 1], hi = iv == PWL_H ? INF : sbp[iv];
    if (lo < INF) {             // (an interval between tied breakpoints is empty but still owns a zero-width piece)
      const double u = test_point(lo, hi);
      double P = 0.0, Q = bb1[kk];
      for (int j = 0; j < PWL_H; ++j) {
        const double on = a1[j] * u + b1v[j] > 0.0 ? W1[j * PWL_H + kk] : 0.0;
        P += on * a1[j];
        Q += on * b1v[j];
      }
      IPQ[2 * tid] = P; IPQ[2 * tid + 1] = Q;
      if (lo < hi && P != 0.0) { const double r = -Q / P; if (r > lo && r < hi) root = r; }
    }
    candu[PWL_H + tid] = root;
  }
  for (int p = tid; p < PWL_NPIECE - 1; p += blockDim.x) cand[p] = INF;
  for (int p = tid; p < PWL_NPIECE; p += blockDim.x) bad[p] = 0;
  __syncthreads();
  // Sorted order without a 288 x 288 rank sort: the roots of interval i lie strictly between the sorted
  // first-layer breakpoints sbp[i-1] and sbp[i], so the sorted sequence is, interval by interval, the interval's
  // roots (ranked among the <= 16 of them: 16 comparisons, ties by unit) followed by sbp[i].
  int rank_in = 0;
  if (tid < 17 * PWL_H) {
    int cnt = 0;
    for (int j = 0; j < PWL_H; ++j) {
      const double o = candu[PWL_H + iv * PWL_H + j];
      rank_in += (o < root || (o == root && j < kk)) ? 1 : 0;
      cnt += o < INF ? 1 : 0;
    }
    if (kk == 0) icnt[iv] = cnt;
  }
  __syncthreads();
  if (tid < 17) {                                   // roots before interval tid
    int sum = 0;
    for (int i = 0; i < tid; ++i) sum += icnt[i];
    ioff[tid] = sum;
  }
  __syncthreads();
  if (tid < 17 * PWL_H && root < INF) {          // iv first-layer breakpoints precede it
    cand[iv + ioff[iv] + rank_in] = root;
    biv[iv + ioff[iv] + rank_in] = iv;
  }
  if (tid < PWL_H && sbp[tid] < INF) {
    cand[tid + ioff[tid] + icnt[tid]] = sbp[tid];
    biv[tid + ioff[tid] + icnt[tid]] = tid;       // the piece that ends at the t-th sorted first-layer breakpoint
  }
  int n1 = 0;
  for (int j = 0; j < PWL_H; ++j) n1 += sbp[j] < INF ? 1 : 0;
  const int n = n1 + ioff[16] + icnt[16];             // finite breakpoints; pieces 0 .. n
  __syncthreads();
  float* T = tables + (int64_t)blockIdx.x * PWL_TBL;
  for (int p = tid; p < PWL_NBP; p += blockDim.x)
    // padding: NaN -- `bp <= u` is false for every u, +inf included, so the searches stop there unaided
    T[p] = p == PWL_N_SLOT ? __int_as_float(n) : (p < n ? (float)cand[p] : __int_as_float(0x7fc00000));
  // affine map of every piece, PWL_CHUNK pieces per pass:
  //   stage 1, task (p, k): second-layer pre-activation P u + Q on the piece (zeroed if its ReLU is off)
  //   stage 2, task (p, m): theta_m = S u + T
  const double LOG2E_D = 1.4426950408889634;
  for (int base = 0; base <= n; base += PWL_CHUNK) {
    const int np = n + 1 - base < PWL_CHUNK ? n + 1 - base : PWL_CHUNK;
    for (int t = tid; t < np * PWL_H; t += blockDim.x) {
      const int p = base + (t >> 4), k = t & 15;
      const double lo = p == 0 ? -INF : cand[p - 1], hi = p < n ? cand[p] : INF;
      const double u = test_point(lo, hi);
      const int ivp = p < n ? biv[p] : n1;          // the last piece lies beyond every finite first-layer breakpoint
      const double P = IPQ[2 * (ivp * PWL_H + k)], Q = IPQ[2 * (ivp * PWL_H + k) + 1];
      const bool act = P * u + Q > 0.0;
      PQ[2 * t] = act ? P : 0.0;
      PQ[2 * t + 1] = act ? Q : 0.0;
    }
    __syncthreads();
    for (int t = tid; t < np * PWL_P; t += blockDim.x) {
      const int pl = t >> 4, m = t & 15, p = base + pl;
      double S = 0.0, Tt = bo[m];
      for (int k = 0; k < PWL_H; ++k) {
        const double wo = Wo[k * PWL_P + m];
        S += wo * PQ[2 * (pl * PWL_H + k)];
        Tt += wo * PQ[2 * (pl * PWL_H + k) + 1];
      }
      // Refer the map to the point of the piece nearest to 0, kept inside the search grid: samples live
      // there, and a piece can be thousands wide (a midpoint reference at u ~ 1000 makes S (u - u_ref) and
      // T cancel catastrophically for u ~ 10).  The reference need not lie inside the piece -- T is the
      // value of the piece's affine map at u_ref, not of the network.
      const double lo = p == 0 ? -INF : cand[p - 1], hi = p < n ? cand[p] : INF;
      const double nearest = lo > 0.0 ? lo : (hi < 0.0 ? hi : 0.0);
      const float uref = (float)(nearest < (double)PWL_GMIN ? (double)PWL_GMIN : (nearest > -(double)PWL_GMIN ? -(double)PWL_GMIN : nearest));
      Tt += S * (double)uref;
      if (m == 0) {        // also in the row's first padding slot: it then arrives with the row's own LDS reads
        T[PWL_OFF_REF + p] = uref; urefs[pl] = (double)uref;
        T[PWL_OFF_PIECE + p * PWL_ROW + 2 * PWL_P] = uref;
      }
      RAW[2 * t] = S;
      RAW[2 * t + 1] = Tt;
    }
    __syncthreads();
    for (int t = tid; t < np * PWL_P; t += blockDim.x) {
      const int pl = t >> 4, m = t & 15, p = base + pl;
      double S = RAW[2 * t], Tt = RAW[2 * t + 1];
      const double lo = p == 0 ? -INF : cand[p - 1], hi = p < n ? cand[p] : INF;
      const double uref = urefs[pl];
      // the part of the piece a sample can reach through an unmarked grid cell
      const double ulo = fmax(lo, (double)PWL_GMIN - 0.01), uhi = fmin(hi, -(double)PWL_GMIN + 0.01);
      bool out_of_bounds = false;
      if (m < 2 * 5) {
        // shift of the group: its largest logit at the centre of the reachable part of the piece; bounds: the
        // group maximum at both ends of that part (linear logits: the extremes of the maximum are at the ends
        // or at the centre, where it is 0 by construction -- the maximum of linear functions is convex)
        const int r0 = m < 5 ? 0 : 5;
        const double uc = ulo <= uhi ? 0.5 * (ulo + uhi) : uref;
        double Mc = -INF, Mlo = -INF, Mhi = -INF;
        for (int k = r0; k < r0 + 5; ++k) {
          const double Sk = RAW[2 * (pl * PWL_P + k)], Tk = RAW[2 * (pl * PWL_P + k) + 1];
          Mc = fmax(Mc, Tk + Sk * (uc - uref));
          Mlo = fmax(Mlo, Tk + Sk * (ulo - uref));
          Mhi = fmax(Mhi, Tk + Sk * (uhi - uref));
        }
        if (ulo <= uhi)
          out_of_bounds = fmax(fabs(Mlo - Mc), fabs(Mhi - Mc)) * LOG2E_D > PWL_FAST_LOGIT;
        S *= LOG2E_D;
        Tt = (Tt - Mc) * LOG2E_D;
      } else {
        Tt += sp_offset;
        if (ulo <= uhi) {
          const double a = Tt + S * (ulo - uref), b = Tt + S * (uhi - uref);
          out_of_bounds = fmin(a, b) < PWL_FAST_SLOPE_LO || fmax(a, b) > PWL_FAST_SLOPE_HI;
        }
        S *= LOG2E_D; Tt *= LOG2E_D;
      }
      if (out_of_bounds || !(S == S) || !(Tt == Tt)) bad[p] = 1;      // (benign race: everybody writes 1)
      float* row = T + PWL_OFF_PIECE + p * PWL_ROW;
      row[m] = (float)S;
      row[PWL_P + m] = (float)Tt;
    }
    __syncthreads();
  }
  // search grid: number of breakpoints <= the cell's left edge (a lower bound for the search).  The edge is
  // pulled in by 1e-4: pwl_cell() computes the cell in fp32, and u a rounding error below an edge may land
  // in the cell above it.  PWL_G_MANY: more than two breakpoints in (left edge, right edge] -- the kernels compare
  // against two breakpoints unconditionally and loop only in such cells (cell 0 / the last cell also serve every
  // u beyond the grid).  PWL_G_GENERAL: the cell touches a piece that needs the general spline evaluation, or is
  // one of the two outermost cells.
  // lo_ of cell g = the number of breakpoints b <= x_g = GMIN + g / GSCALE - 1e-4 -- counted from the breakpoints'
  // side: breakpoint b is below the left edge of every cell from g_b = ceil((b + 1e-4 - GMIN) GSCALE) on, so each
  // breakpoint adds one at g_b and lo_ is the running sum (a block scan: four consecutive cells per thread, a
  // shuffle scan inside the wave, the eight wave totals through LDS).  Round 2's first version searched every cell
  // through nine dependent LDS reads: the largest phase of the kernel.  A cell index off by one through rounding is
  // covered by the 1e-4 the edge is pulled in by (see above).
  int* delta = reinterpret_cast<int*>(PQ);               // PQ is free again: 2 049 + 8 ints
  static_assert(sizeof(double) * PWL_CHUNK * PWL_H * 2 >= sizeof(int) * (PWL_NG + 16), "scratch for the grid scan");
  constexpr int CPT = 4;
  static_assert(PWL_NG == 512 * CPT, "one thread owns four consecutive cells (512 threads)");
  for (int g = tid; g < PWL_NG + 16; g += blockDim.x) delta[g] = 0;
  __syncthreads();
  for (int p = tid; p < n; p += blockDim.x) {
    const double gb = ceil((cand[p] + 1e-4 - (double)PWL_GMIN) * (double)PWL_GSCALE);
    // (cell 0 serves every u below the grid and searches from piece 0: breakpoints below the grid count from cell 1)
    const int g0 = gb < 1.0 ? 1 : (gb >= (double)PWL_NG ? PWL_NG : (int)gb);
    atomicAdd(&delta[g0], 1);                             // (slot PWL_NG: breakpoints beyond the grid, never summed)
  }
  __syncthreads();
  {
    const int g0 = tid * CPT;
    int c0 = delta[g0], c1 = c0 + delta[g0 + 1], c2 = c1 + delta[g0 + 2], c3 = c2 + delta[g0 + 3];
    int run = c3;                                         // inclusive scan of the threads' totals over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(run, off, 64);
      if ((tid & 63) >= off) run += v;
    }
    int* wtot = delta + PWL_NG + 8;                       // eight wave totals
    __syncthreads();                                      // (everybody has read its delta entries)
    if ((tid & 63) == 63) wtot[tid >> 6] = run;
    __syncthreads();
    int before = run - c3;                                // exclusive within the wave
    for (int w2 = 0; w2 < (tid >> 6); ++w2) before += wtot[w2];
    const int cnt[CPT] = {before + c0, before + c1, before + c2, before + c3};
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int g = g0 + i;
      const int lo_ = g == 0 ? 0 : cnt[i];
      const double xr = g == PWL_NG - 1 ? INF : (double)PWL_GMIN + (double)(g + 1) / (double)PWL_GSCALE + 1e-4;
      int mark = (g == 0 || g == PWL_NG - 1) ? 1 : 0;
      for (int p = lo_; p <= n && !mark; ++p) {          // pieces lo_ .. the one holding the cell's right edge
        mark |= bad[p];
        if (p < n && cand[p] > xr) break;
      }
      const bool many = lo_ + 2 < n && cand[lo_ + 2] <= xr;      // a third breakpoint a sample of the cell can pass
      reinterpret_cast<uint16_t*>(T + PWL_OFF_GRID)[g] =
          (uint16_t)((uint32_t)lo_ | (mark ? PWL_G_GENERAL : 0u) | (many ? PWL_G_MANY : 0u));
    }
  }
}


// ---- the lean builder: the same tables, bit for bit, from one wave per table ---------------------------------------
// pwl_build_kernel above stays as the reference (cnf_model_set_pwl_builder).  Every stored value keeps its operation
// order -- the 16-term sums in j / k order, the same test_point, uref, Mc and LOG2E_D products --; what differs is who
// computes a value and how often:
//   * every phase is a strided loop over its tasks, so a table needs NT threads, not 512.  NT = 64: a table belongs to
//     ONE wave, and there is no block-wide barrier anywhere (LDS operations of a wave complete in order: a compiler fence is all the
//     phases need between them), no wave that walks to a barrier with nothing to do, 10 KB of LDS per table instead of
//     50 and 128 registers x 1 wave instead of 126 x 8 -- a CU holds 16 tables in flight (4 waves per SIMD, 16 x 10 KB of
//     its 160 KB of LDS) instead of 2;
//   * NT is a multiple of 16, so a thread's second-layer unit / output index (tid & 15) is the same in every pass: its
//     column of W1 and of Wout lives in registers, converted once per table, and neither matrix is staged in LDS;
//   * the affine maps go NT / 16 pieces per pass, one (piece, output) task per thread: S and T stay in registers from the
//     sum to the row, the PQ / RAW scratch is 2 x NT doubles;
//   * a softmax group's three maxima (centre, both ends of the reachable part) are computed once per (piece, group) by
//     one thread each and shared through LDS -- the reference computes all three in each of the group's five threads;
//   * n1, n and the prefix sums are computed once (by thread 16) instead of by every thread;
//   * the grid scan packs two 16-bit counts per LDS word (a cell holds at most 288 breakpoints) and a thread writes its
//     NG / NT consecutive cells four at a time.
// (the body is written over NT and a barrier functor; 128 and 256 threads per table with __syncthreads() were measured
// and dropped -- fewer tables in flight, slower at 4 096 tables: profiles/r06_lean_builder)
struct PwlWaveSync {
  __device__ __forceinline__ void operator()() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

constexpr int PWL_NROOT = 17 * PWL_H;     // (first-layer interval, second-layer unit) pairs: candidates for a root

template <int NT>
struct PwlLeanLds {
  static constexpr int CHUNK = NT / 16;                     // pieces per pass of the affine maps
  // bpu (the unsorted first-layer breakpoints) is dead once sbp is sorted, candu (the unsorted roots) once cand is:
  // candu takes bpu's place, PQ and RAW candu's
  static constexpr int WORK = 4 * NT > PWL_NROOT ? 4 * NT : PWL_NROOT;
  double ab[2 * PWL_H];                                     // (a, b) of the first-layer units, interleaved
  double sbp[PWL_H];
  double cand[PWL_NPIECE - 1];
  double IPQ[PWL_NROOT * 2];                                // the grid scan's counts take its place at the end
  double work[WORK];                                        // bpu | candu | PQ[2 NT], RAW[2 NT]
  double urefs[CHUNK];
  double gmax[CHUNK * 6];                                   // (Mc, Mlo, Mhi) of (piece, softmax group)
  int icnt[17], ioff[17], nn[2];
  uint8_t bad[PWL_NPIECE + 3], biv[PWL_NPIECE + 3];
};

template <int NT, class Sync>
__device__ __forceinline__ void pwl_build_lean(const float* __restrict__ w, double c, double sp_offset,
                                               float* __restrict__ T, PwlLeanLds<NT>& s, int tid, Sync sync) {
  static_assert(NT == 64, "one wave per table: the grid scan is a scan over ONE wave");
  static_assert(PWL_NG % (4 * NT) == 0, "a thread owns a multiple of four grid cells");
  constexpr int CHUNK = PwlLeanLds<NT>::CHUNK;
  constexpr int NR = (PWL_NROOT + NT - 1) / NT;            // passes over the root candidates
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  const int kk = tid & 15;
  // flat layout: W0[2][16] | b0[16] | W1[16][16] | b1[16] | Wout[16][16] | bout[16]
  double w1c[PWL_H];
#pragma unroll
  for (int j = 0; j < PWL_H; ++j) w1c[j] = (double)w[3 * PWL_H + j * PWL_H + kk];
  const double bb1k = (double)w[3 * PWL_H + 256 + kk];
  double* bpu = s.work;
  if (tid < PWL_H) {
    const double a = (double)w[PWL_H + tid], b = (double)w[tid] * c + (double)w[2 * PWL_H + tid];
    s.ab[2 * tid] = a;
    s.ab[2 * tid + 1] = b;
    bpu[tid] = a != 0.0 ? -b / a : INF;
  }
  sync();
  if (tid < PWL_H) {         // rank sort of the 16 first-layer breakpoints
    const double v = bpu[tid];
    int r = 0;
    for (int j = 0; j < PWL_H; ++j) r += (bpu[j] < v || (bpu[j] == v && j < tid)) ? 1 : 0;
    s.sbp[r] = v;
  }
  sync();
  auto test_point = [&](double lo, double hi) -> double {
    const bool fl = lo > -INF, fh = hi < INF;
    return fl && fh ? 0.5 * (lo + hi) : (fl ? lo + 1.0 : (fh ? hi - 1.0 : 0.0));
  };
  // second-layer zero crossings inside each of the 17 first-layer intervals
  double* candu = s.work;
#pragma unroll 1
  for (int i = 0; i < NR; ++i) {
    asm volatile("" ::: "memory");                         // (a, b) are read from LDS in every pass, not kept in 64 registers
    const int t = tid + i * NT, iv = t >> 4;               // (t & 15 == kk)
    if (t < PWL_NROOT) {
      double root = INF;
      const double lo = iv == 0 ? -INF : s.sbp[iv - 1], hi = iv == PWL_H ? INF : s.sbp[iv];
      if (lo < INF) {
        const double u = test_point(lo, hi);
        double P = 0.0, Q = bb1k;
#pragma unroll
        for (int j = 0; j < PWL_H; ++j) {
          const double a = s.ab[2 * j], b = s.ab[2 * j + 1];
          const double on = a * u + b > 0.0 ? w1c[j] : 0.0;
          P += on * a;
          Q += on * b;
        }
        s.IPQ[2 * t] = P; s.IPQ[2 * t + 1] = Q;
        if (lo < hi && P != 0.0) { const double r = -Q / P; if (r > lo && r < hi) root = r; }
      }
      candu[t] = root;
    }
  }
  for (int p = tid; p < PWL_NPIECE - 1; p += NT) s.cand[p] = INF;
  for (int p = tid; p < PWL_NPIECE; p += NT) s.bad[p] = 0;
  sync();
  // sorted order: interval by interval, the interval's roots (ranked among themselves, ties by unit), then sbp[i]
  uint32_t rk = 0;                                          // the ranks of the thread's roots, four bits per pass
  static_assert(NR <= 8, "ranks of all passes in one word");
#pragma unroll 1
  for (int i = 0; i < NR; ++i) {
    const int t = tid + i * NT, iv = t >> 4;
    if (t < PWL_NROOT) {
      const double root = candu[t];
      int cnt = 0, rank_in = 0;
      for (int j = 0; j < PWL_H; ++j) {
        const double o = candu[iv * PWL_H + j];
        rank_in += (o < root || (o == root && j < kk)) ? 1 : 0;
        cnt += o < INF ? 1 : 0;
      }
      rk |= (uint32_t)rank_in << (4 * i);
      if (kk == 0) s.icnt[iv] = cnt;
    }
  }
  sync();
  if (tid < 17) {                                   // roots before interval tid
    int sum = 0;
    for (int i = 0; i < tid; ++i) sum += s.icnt[i];
    s.ioff[tid] = sum;
    if (tid == 16) {
      int n1 = 0;
      for (int j = 0; j < PWL_H; ++j) n1 += s.sbp[j] < INF ? 1 : 0;
      s.nn[0] = n1;
      s.nn[1] = n1 + sum + s.icnt[16];              // finite breakpoints; pieces 0 .. n
    }
  }
  sync();
#pragma unroll 1
  for (int i = 0; i < NR; ++i) {
    const int t = tid + i * NT, iv = t >> 4;
    if (t < PWL_NROOT) {
      const double root = candu[t];
      if (root < INF) {                             // iv first-layer breakpoints precede it
        const int q = iv + s.ioff[iv] + (int)((rk >> (4 * i)) & 15u);
        s.cand[q] = root;
        s.biv[q] = (uint8_t)iv;
      }
    }
  }
  if (tid < PWL_H && s.sbp[tid] < INF) {
    const int q = tid + s.ioff[tid] + s.icnt[tid];
    s.cand[q] = s.sbp[tid];
    s.biv[q] = (uint8_t)tid;                        // the piece that ends at the t-th sorted first-layer breakpoint
  }
  sync();
  const int n1 = s.nn[0], n = s.nn[1];
  for (int p = tid; p < PWL_NBP; p += NT)
    T[p] = p == PWL_N_SLOT ? __int_as_float(n) : (p < n ? (float)s.cand[p] : __int_as_float(0x7fc00000));
  // affine map of every piece, CHUNK pieces per pass, thread = (piece pl, unit / output kk)
  const double LOG2E_D = 1.4426950408889634;
  // (loaded here: W1's column is dead, the two never share registers)
  double woc[PWL_H];
#pragma unroll
  for (int k = 0; k < PWL_H; ++k) woc[k] = (double)w[3 * PWL_H + 256 + PWL_H + k * PWL_P + kk];
  const double bok = (double)w[3 * PWL_H + 256 + PWL_H + 256 + kk];
  double* PQ = s.work;
  double* RAW = s.work + 2 * NT;
  const int pl = tid >> 4, m = kk;
  for (int base = 0; base <= n; base += CHUNK) {
    const int np = n + 1 - base < CHUNK ? n + 1 - base : CHUNK;
    const int p = base + pl;
    const bool mine = pl < np;
    const double lo = !mine || p == 0 ? -INF : s.cand[p - 1], hi = mine && p < n ? s.cand[p] : INF;
    if (mine) {
      const double u = test_point(lo, hi);
      const int ivp = p < n ? s.biv[p] : n1;        // the last piece lies beyond every finite first-layer breakpoint
      const double P = s.IPQ[2 * (ivp * PWL_H + kk)], Q = s.IPQ[2 * (ivp * PWL_H + kk) + 1];
      const bool act = P * u + Q > 0.0;
      PQ[2 * tid] = act ? P : 0.0;
      PQ[2 * tid + 1] = act ? Q : 0.0;
    }
    sync();
    double S = 0.0, Tt = bok;
    if (mine) {
      // ONE address, the 16 pairs at immediate offsets from it: left to itself the compiler keeps 16 addresses in
      // registers across the loop, and the kernel no longer fits the 128 registers of four waves per SIMD
      const double* pq = PQ + 2 * pl * PWL_H;
      asm volatile("" : "+v"(pq));
#pragma unroll
      for (int k = 0; k < PWL_H; ++k) {
        const double wo = woc[k];
        S += wo * pq[2 * k];
        Tt += wo * pq[2 * k + 1];
      }
      // the map is referred to the point of the piece nearest to 0, kept inside the search grid (pwl_build_kernel)
      const double nearest = lo > 0.0 ? lo : (hi < 0.0 ? hi : 0.0);
      const float uref = (float)(nearest < (double)PWL_GMIN ? (double)PWL_GMIN : (nearest > -(double)PWL_GMIN ? -(double)PWL_GMIN : nearest));
      Tt += S * (double)uref;
      if (m == 0) {
        T[PWL_OFF_REF + p] = uref; s.urefs[pl] = (double)uref;
        T[PWL_OFF_PIECE + p * PWL_ROW + 2 * PWL_P] = uref;
      }
      RAW[2 * tid] = S;
      RAW[2 * tid + 1] = Tt;
    }
    sync();
    // the part of a piece a sample can reach through an unmarked grid cell; a softmax group's largest logit at its
    // centre (the shift of the group) and at both ends (the bounds): task (piece, group, point)
    if (tid < np * 6) {
      const int ql = tid / 6, r = tid - 6 * ql, r0 = r < 3 ? 0 : 5, which = r < 3 ? r : r - 3, q = base + ql;
      const double qlo = q == 0 ? -INF : s.cand[q - 1], qhi = q < n ? s.cand[q] : INF;
      const double uref = s.urefs[ql];
      const double ulo = fmax(qlo, (double)PWL_GMIN - 0.01), uhi = fmin(qhi, -(double)PWL_GMIN + 0.01);
      const double uc = ulo <= uhi ? 0.5 * (ulo + uhi) : uref;
      const double x = which == 0 ? uc : (which == 1 ? ulo : uhi);
      double M = -INF;
      for (int k = r0; k < r0 + 5; ++k) {
        const double Sk = RAW[2 * (ql * PWL_P + k)], Tk = RAW[2 * (ql * PWL_P + k) + 1];
        M = fmax(M, Tk + Sk * (x - uref));
      }
      s.gmax[tid] = M;
    }
    sync();
    if (mine) {
      const double uref = s.urefs[pl];
      const double ulo = fmax(lo, (double)PWL_GMIN - 0.01), uhi = fmin(hi, -(double)PWL_GMIN + 0.01);
      bool out_of_bounds = false;
      if (m < 2 * 5) {
        const double* g = s.gmax + pl * 6 + (m < 5 ? 0 : 3);
        const double Mc = g[0], Mlo = g[1], Mhi = g[2];
        if (ulo <= uhi)
          out_of_bounds = fmax(fabs(Mlo - Mc), fabs(Mhi - Mc)) * LOG2E_D > PWL_FAST_LOGIT;
        S *= LOG2E_D;
        Tt = (Tt - Mc) * LOG2E_D;
      } else {
        Tt += sp_offset;
        if (ulo <= uhi) {
          const double a = Tt + S * (ulo - uref), b = Tt + S * (uhi - uref);
          out_of_bounds = fmin(a, b) < PWL_FAST_SLOPE_LO || fmax(a, b) > PWL_FAST_SLOPE_HI;
        }
        S *= LOG2E_D; Tt *= LOG2E_D;
      }
      if (out_of_bounds || !(S == S) || !(Tt == Tt)) s.bad[p] = 1;      // (benign race: everybody writes 1)
      float* row = T + PWL_OFF_PIECE + p * PWL_ROW;
      row[m] = (float)S;
      row[PWL_P + m] = (float)Tt;
    }
    sync();
  }
  // search grid (pwl_build_kernel): each breakpoint adds one at the first cell whose left edge it is below, lo_ is the
  // running sum.  Two 16-bit counts per word: cell g in half g & 1 of word g >> 1.
  uint32_t* delta = reinterpret_cast<uint32_t*>(s.IPQ);
  static_assert(sizeof(s.IPQ) >= sizeof(uint32_t) * (PWL_NG / 2 + 1), "scratch for the grid scan");
  constexpr int CPT = PWL_NG / NT;                         // consecutive cells per thread
  for (int g = tid; g < PWL_NG / 2 + 1; g += NT) delta[g] = 0;
  sync();
  for (int p = tid; p < n; p += NT) {
    const double gb = ceil((s.cand[p] + 1e-4 - (double)PWL_GMIN) * (double)PWL_GSCALE);
    // (cell 0 serves every u below the grid and searches from piece 0: breakpoints below the grid count from cell 1)
    const int g0 = gb < 1.0 ? 1 : (gb >= (double)PWL_NG ? PWL_NG : (int)gb);
    atomicAdd(&delta[g0 >> 1], 1u << (16 * (g0 & 1)));   // (cell PWL_NG: breakpoints beyond the grid, never summed)
  }
  sync();
  {
    const int g0 = tid * CPT;
    int tot = 0;
#pragma unroll
    for (int i = 0; i < CPT / 2; ++i) { const uint32_t d = delta[g0 / 2 + i]; tot += (int)(d & 0xffffu) + (int)(d >> 16); }
    int run = tot;                                          // inclusive scan of the threads' totals over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(run, off, 64);
      if ((tid & 63) >= off) run += v;
    }
    const int before = run - tot;                           // exclusive
    uint2* gout = reinterpret_cast<uint2*>(T + PWL_OFF_GRID) + g0 / 4;
    int cnt = before;
    for (int q4 = 0; q4 < CPT / 4; ++q4) {
      const uint32_t d0 = delta[g0 / 2 + 2 * q4], d1 = delta[g0 / 2 + 2 * q4 + 1];
      const int dc[4] = {(int)(d0 & 0xffffu), (int)(d0 >> 16), (int)(d1 & 0xffffu), (int)(d1 >> 16)};
      uint32_t e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int g = g0 + 4 * q4 + i;
        cnt += dc[i];
        const int lo_ = g == 0 ? 0 : cnt;
        const double xr = g == PWL_NG - 1 ? INF : (double)PWL_GMIN + (double)(g + 1) / (double)PWL_GSCALE + 1e-4;
        int mark = (g == 0 || g == PWL_NG - 1) ? 1 : 0;
        for (int p = lo_; p <= n && !mark; ++p) {          // pieces lo_ .. the one holding the cell's right edge
          mark |= s.bad[p];
          if (p < n && s.cand[p] > xr) break;
        }
        const bool many = lo_ + 2 < n && s.cand[lo_ + 2] <= xr;      // a third breakpoint a sample of the cell can pass
        e[i] = (uint32_t)lo_ | (mark ? PWL_G_GENERAL : 0u) | (many ? PWL_G_MANY : 0u);
      }
      gout[q4] = uint2{e[0] | (e[1] << 16), e[2] | (e[3] << 16)};
    }
  }
}

// One workgroup of NT threads per (slice, layer), as pwl_build_kernel
template <int NT>
__global__ __launch_bounds__(NT, 4) void pwl_build_lean_kernel(const float* __restrict__ weights /* prep + hdr */,
                                                            int64_t per_layer, const float* __restrict__ cvals,
                                                            float c_offset, int L, double sp_offset,
                                                            float* __restrict__ tables) {
  __shared__ PwlLeanLds<NT> s;
  const int slice = blockIdx.x / L, l = blockIdx.x % L;
  const double c = (double)cvals[slice] + (double)c_offset;
  float* T = tables + (int64_t)blockIdx.x * PWL_TBL;
  pwl_build_lean<NT>(weights + l * per_layer, c, sp_offset, T, s, (int)threadIdx.x, PwlWaveSync());
}


}  // namespace cnf
