// cnf_grad_pwl.hip -- the table backward: the reverse of ONE flow pass at dim 2 on the conditioner tables
// (cnf_pwl.h), with per-piece statistics in fixed point in place of per-sample weight gradients.  Like the MLP backward
// of cnf_grad.hip it replaces `jax.value_and_grad(loss_fn)` in cnf_ot/mfc/solvers.py:90-97, for the
// terms that are composed from separate flow launches: cnf_pass_vjp's table form, the density fit
// (cnf_neg_logprob_vjp) and the kinetic + potential pair (cnf_kinetic_potential_vjp).
// Built for the reference's network only: hidden 16, 2 hidden layers, 5 bins.
#include "cnf_backward.h"
#include "cnf_host.h"
#include "cnf_pwl.h"

#include <math.h>

namespace cnf {

// ---------------------------------------------------------------------------
// The backward of ONE flow pass at dim 2 on the conditioner tables (cnf_pwl.h), with PER-PIECE SUFFICIENT
// STATISTICS in place of per-sample weight gradients.  On a piece of a slice's table both ReLU activity patterns
// are constant and theta, h2, h1 are affine in the conditioner's scalar input u, so every weight gradient is linear
// in  A = sum theta_bar  and  B = sum (u - u_ref) theta_bar  over the samples that land in the piece
// (oracle/pwl_grad.py restates the algebra; checked against per-sample backprop to 1e-9).  Per sample that leaves:
// the forward through the tables, the spline partials (cond_spline_bwd / table_spline_bwd as in the MLP kernels),
// the input adjoint S . theta_bar from the row already in LDS, and 20 accumulations -- no MLP recompute and no
// per-sample GEMM.  pwl_stats_finish_kernel turns the statistics into gradient slabs, once per piece.
//   vjp_pwl_kernel: two samples per lane (packed arithmetic), 512 threads; LDS = `first` table | L tables (PWL_LROWS-row window) |
//   64-bit fixed-point accumulators [L][64 pieces][33] (A | B per piece).
// ---------------------------------------------------------------------------
constexpr int PWL_STAT = 2 * PWL_P;                 // statistics per piece: A[16] | B[16]
// The statistics are accumulated in 64-bit FIXED POINT: measured on MI355X, ds_add_f32 retires a lane every ~2.6
// cycles whatever the addresses (the accumulation was 0.9 of 1.2 ms per 4.2 M-point pass, and neither bank padding
// nor replicated accumulators changed it), integer LDS atomics are ~15 x faster -- and integer sums do not depend
// on the order of the additions, so the gradient is bitwise reproducible like the slab scheme of the MLP kernels.
// Scale: 2^s with s = 28 - exponent of the largest |ybar|, |ldbar| of the call (adjoint_max_kernel): resolution
// 2^-28 of that magnitude (float32 itself resolves 2^-24), a single term may be 2^23 x it (the 1.5 2^52 rounding trick
// holds below 2^51), a sum 2^35 x it.
// In LDS a piece's 32 accumulators are 33 entries apart (entry m of piece p in bank pair (p + m) mod 32: lanes of
// different pieces do not collide); only the first PWL_ACC_W pieces have LDS accumulators (the rest -- far pieces,
// few samples -- go to global memory).
typedef unsigned long long stat_t;
constexpr int PWL_STAT_LDS = PWL_STAT + 1;
constexpr int PWL_ACC_W = 64;
constexpr int PWL_STAT_SLICES = 128;                // slices per chunk of the table backward (statistics buffer: 2 x 9.5 MB per flow layer)
// Lanes of a wave that land in the same piece add to the same addresses, and the LDS serialises them: the accumulators
// exist up to PWL_ACC_R times (as many as fit in LDS next to the L tables: 3 at L = 2, 1 from L = 3 on), lane t uses
// copy t mod acc_r (summed when a slice's statistics are flushed).  Measured at L = 2, one pass over 4.2 M points:
// 1 copy 0.34-0.39 ms, 3 copies 0.28-0.33 (scripts/exp_vjp_tables_only.py).
constexpr int PWL_ACC_R = 3;
// ... and what remains must not become a bank conflict instead: entry i of a piece sits in the 128-byte line slot
// (p + i) mod 16, so copy r starts PWL_ACC_SKEW r entries late and the B entries are stored rotated by 8 -- the six
// (copy, A | B) combinations of one piece and entry are six different slots.
constexpr int PWL_ACC_SKEW = 5;
__host__ __device__ constexpr int pwl_acc_entry(int e) { return e < PWL_P ? e : PWL_P + ((e - PWL_P + 8) & 15); }

// 2^(28 - e) for the largest adjoint magnitude 2^e <= |x| < 2^(e+1) (bits of |x| as given by adjoint_max_kernel);
// all-zero adjoints: any scale will do
__device__ __forceinline__ double stat_scale(uint32_t amax_bits) {
  int e = (int)(amax_bits >> 23) - 127;
  if (amax_bits == 0) e = 0;
  if (e < -100) e = -100;
  return __longlong_as_double((long long)(1023 + 28 - e) << 52);
}

// the largest |ybar|, |ldbar| of a call (bit pattern of a non-negative float: ordered like the integers)
__global__ __launch_bounds__(256) void adjoint_max_kernel(const float* __restrict__ ybar, int64_t n_y,
                                                         const float* __restrict__ ldbar, int64_t n_l, uint32_t* out) {
  uint32_t m = 0, bad = 0;      // bad: an Inf / NaN adjoint was seen -> out[1] (the table backward then answers NaN, like the MLP backward)
  auto take = [&](float v) { const uint32_t b = __float_as_uint(v) & 0x7fffffffu; bad |= b >= 0x7f800000u ? 1u : 0u; m = (b > m && b < 0x7f800000u) ? b : m; };
  auto scan = [&](const float* __restrict__ p, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {            // 16-byte loads, four in flight per thread
      const f4* q = reinterpret_cast<const f4*>(p);
      const int64_t n4 = n >> 2;
      int64_t i = t;
      for (; i + 3 * stride < n4; i += 4 * stride) {             // (explicitly: the compiler kept one load per iteration)
        const f4 v0 = q[i], v1 = q[i + stride], v2 = q[i + 2 * stride], v3 = q[i + 3 * stride];
#pragma unroll
        for (int e = 0; e < 4; ++e) { take(v0[e]); take(v1[e]); take(v2[e]); take(v3[e]); }
      }
      for (; i < n4; i += stride) { const f4 v = q[i]; take(v[0]); take(v[1]); take(v[2]); take(v[3]); }
      for (int64_t i = (n4 << 2) + t; i < n; i += stride) take(p[i]);
    } else {
      for (int64_t i = t; i < n; i += stride) take(p[i]);
    }
  };
  if (ybar) scan(ybar, n_y);
  if (ldbar) scan(ldbar, n_l);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(m, off, 64); m = o > m ? o : m; }
  __shared__ uint32_t wm[4];                 // one atomic per workgroup: they all land on one address
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t a01 = wm[0] > wm[1] ? wm[0] : wm[1], a23 = wm[2] > wm[3] ? wm[2] : wm[3];
    const uint32_t mm = a01 > a23 ? a01 : a23;
    if (mm) atomicMax(out, mm);
  }
  if (__builtin_amdgcn_ballot_w64(bad != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(out + 1, 1u);
}

struct VjpPwlArgs {
  ModelArgs m;
  const float* pts;      // [B, 2] inputs of the pass
  const float* ybar;     // [B, 2] or null
  const float* ldbar;    // [B] or null
  float* xbar;           // [B, 2] or null
  const float* tables;   // [n_slices][L][PWL_TBL]
  stat_t* stats;         // [n_slices][L][PWL_NPIECE][PWL_STAT] fixed point, zero on entry
  stat_t* coarse;        // the same shape at 2^-32 of the scale: terms too large for `stats` (ill-conditioned flows)
  uint32_t* amax;        // [0] bits of the largest |adjoint| of the call (adjoint_max_kernel), [1] non-finite flag
  float* slabs;          // slab b (this workgroup's): zeroed here, its first GP entries receive the `first` spline's
  int64_t n_params;      // per-bin adjoint sums (one owner per slab: a fixed summation order)
  int64_t B, slice_len;
  int32_t n_slices, tiles_per_slice;
  int32_t acc_r;         // copies of the LDS accumulators (1 .. PWL_ACC_R)
  // SEED (cnf_neg_logprob_vjp): the output adjoints are formed in the kernel -- ybar = seed_coef * base point,
  // ldbar = -seed_coef -- and sums[slice] receives sum -log_prob; amax_bits != 0: the scale's magnitude (no
  // adjoint_max_kernel ran: the seeds are bounded by what the kernel itself produces)
  float seed_coef;
  double* sums;
  uint32_t amax_bits;
  int32_t pts_shared;    // the slices share ONE set of points pts[slice_len, 2] (cnf_kinetic_potential_vjp)
};

constexpr int VJP_PWL_THREADS = 512;      // two samples per lane: tiles of 1 024 samples

// LFIX > 0: the number of flow layers is this constant (the reference's 2): the layer loops are unrolled, the kept
// inputs and outputs of the layers are registers with fixed names instead of arrays indexed by a loop counter
// (which the compiler served from select chains and 16 bytes of scratch)
template <bool TO_BASE, int LFIX = 0, bool SEED = false>
__global__ __launch_bounds__(VJP_PWL_THREADS) void vjp_pwl_kernel(const VjpPwlArgs a) {
  static_assert(!SEED || TO_BASE, "the density-fit term: data -> base");
  constexpr int K = GK, WIN = PWL_LROWS;
  constexpr bool INV = !TO_BASE;
  constexpr int MAXL = LFIX ? LFIX : 4;
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  constexpr int HDR = (hdr_floats(K) + 3) & ~3;
  const int L = LFIX ? LFIX : a.m.L, NT = blockDim.x, tid = threadIdx.x, TS = 2 * NT;
  float* tab = lds_raw;
  float* tbl = lds_raw + HDR;
  stat_t* acc = reinterpret_cast<stat_t*>(tbl + L * pwl_ltbl(WIN));      // [L][PWL_ACC_W][PWL_STAT_LDS] (8-byte aligned: HDR, pwl_ltbl even)
  const int acc_n = L * PWL_ACC_W * PWL_STAT_LDS;                          // one copy
  const int acc_r = a.acc_r;
  float* red = reinterpret_cast<float*>(acc + acc_r * (acc_n + PWL_ACC_SKEW));      // [waves][GP]
  for (int i = tid; i < hdr_floats(K); i += NT) tab[i] = a.m.prep[i];
  for (int i = tid; i < acc_r * (acc_n + PWL_ACC_SKEW); i += NT) acc[i] = 0;
  stat_t* acc_mine = acc + (tid % acc_r) * (acc_n + PWL_ACC_SKEW);
  const SplineConsts sc = sc_scalars(a.m.sc);
  // fixed-point scale 2^(28 - e), e = the exponent of the largest adjoint; x -> round(x scale) by the 1.5 2^52 trick
  const double fx_scale = SliceSum::uniform(stat_scale(a.amax_bits ? a.amax_bits : *a.amax));      // (wave-uniform: a scalar register pair)
  [[maybe_unused]] SliceSum ssum;
  auto to_fixed = [&](double xs) -> stat_t {              // xs = x scale, |xs| < 2^50
    const double d = xs + 6755399441055744.0;
    return (stat_t)(__double_as_longlong(d) - __double_as_longlong(6755399441055744.0));
  };
  // one term into accumulator `e` of (slice, layer l, piece p): LDS for the first PWL_ACC_W pieces; a term beyond the
  // fine scale's reach (|x| >= 2^22 x the largest adjoint: only ill-conditioned flows produce them) goes, 2^32
  // coarser, to the second statistics array in global memory
  auto accumulate = [&](int slice, int l, int p, int e, float x) {
    const double xs = (double)x * fx_scale;
    if (fabs(xs) < 1125899906842624.0) {                     // 2^50
      const stat_t q = to_fixed(xs);
      if (p < PWL_ACC_W) {
        typedef stat_t __attribute__((address_space(3))) * lds_q_ptr;
        lds_q_ptr d3 = (lds_q_ptr)(uintptr_t)(uint32_t)(uintptr_t)(acc_mine + (l * PWL_ACC_W + p) * PWL_STAT_LDS + pwl_acc_entry(e));
        __hip_atomic_fetch_add(d3, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        atomicAdd(a.stats + (((int64_t)slice * L + l) * PWL_NPIECE + p) * PWL_STAT + e, q);
      }
    } else if (fabs(xs) < 4835703278458516698824704.0) {     // 2^82
      atomicAdd(a.coarse + (((int64_t)slice * L + l) * PWL_NPIECE + p) * PWL_STAT + e, to_fixed(xs * 2.3283064365386963e-10));
    }                                                         // (beyond: not representable in float32 sums either)
  };
  // One sample's theta_bar into the statistics of its piece.  The adjoints of a softmax group's logits sum to zero: the
  // last width and the last height entry are not accumulated (pwl_stats_finish_kernel restores them as minus the sum
  // of the other four) -- 20 atomic instructions per sample and layer.  One range test decides between the
  // straight-line form (every term within the fine scale, the piece's accumulators in LDS) and the general one.
  auto add_stats = [&](int slice, int l, int p, float du, const float (&t)[2 * K], int kk, float sb0, float sb1) {
    float big = fmaxf(fabsf(sb0), fabsf(sb1));
#pragma unroll
    for (int m2 = 0; m2 < 2 * K; ++m2) big = fmaxf(big, fabsf(t[m2]));
    big *= fmaxf(1.0f, fabsf(du));
    // (fmaxf drops NaNs: the sum of the terms does not) a non-finite term poisons the call's gradient, like the
    // float accumulation of the MLP backward would -- the fixed-point sums cannot carry it themselves
    float chk = (sb0 + sb1) * du;
#pragma unroll
    for (int m2 = 0; m2 < 2 * K; ++m2) chk += t[m2];
    if (!(fabsf(chk) < INFINITY) || !(big < INFINITY)) {
      atomicOr(a.amax + 1, 1u);
    } else if (p < PWL_ACC_W && (double)big * fx_scale < 1125899906842624.0) {
      typedef stat_t __attribute__((address_space(3))) * lds_q_ptr;
      lds_q_ptr d3 = (lds_q_ptr)(uintptr_t)(uint32_t)(uintptr_t)(acc_mine + (l * PWL_ACC_W + p) * PWL_STAT_LDS);
      auto add = [&](lds_q_ptr d, float x) {
        const double dd = fma((double)x, fx_scale, 6755399441055744.0);
        __hip_atomic_fetch_add(d, (stat_t)(__double_as_longlong(dd) - __double_as_longlong(6755399441055744.0)),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      };
      // odd lanes add their B entry where even lanes add their A entry: lanes of one piece meet on two addresses per
      // instruction instead of one
      const bool sw = tid & 1;
      const float f0 = sw ? du : 1.0f, f1 = sw ? 1.0f : du;
      // (entry e of A at e, of B at pwl_acc_entry(16 + e) = 16 + (e + 8) mod 16: for the lane, B - A is +24 below e = 8, +8 from there)
      static_assert(2 * K + K <= PWL_P && pwl_acc_entry(PWL_P + 8) == PWL_P, "slope entries 10 .. 15 do not wrap");
      const lds_q_ptr qa = d3 + (sw ? PWL_P + 8 : 0), qb = d3 + (sw ? 0 : PWL_P + 8);      // entries 0 .. 7
      const lds_q_ptr ra = d3 + (sw ? PWL_P - 8 : 0), rb = d3 + (sw ? 0 : PWL_P - 8);      // entries 8 .. 15
      // ... and lanes 2, 3 (mod 4) take the entries of each pair (0,1) (2,3) (5,6) (7,8) (slopes) in the other order: twelve
      // slots per piece and instruction pair.  A selected value, and the lane's address moved by one entry.
      const bool sx = tid & 2;
      const int up = sx ? 1 : 0;
      auto add_pair = [&](lds_q_ptr a0, lds_q_ptr b0, int i, float x, float y) {      // x -> entry i, y -> entry i + 1
        const float u0 = sx ? y : x, u1 = sx ? x : y;
        add(a0 + i + up, f0 * u0);     add(b0 + i + up, f1 * u0);
        add(a0 + i + 1 - up, f0 * u1); add(b0 + i + 1 - up, f1 * u1);
      };
      add_pair(qa, qb, 0, t[0], t[1]); add_pair(qa, qb, 2, t[2], t[3]);
      add_pair(qa, qb, 5, t[5], t[6]);
      // (entries 7 | 8 straddle the rotation of the B half)
      {
        const float u0 = sx ? t[8] : t[7], u1 = sx ? t[7] : t[8];
        add((sx ? ra : qa) + 7 + up, f0 * u0);     add((sx ? rb : qb) + 7 + up, f1 * u0);
        add((sx ? qa : ra) + 8 - up, f0 * u1);     add((sx ? qb : rb) + 8 - up, f1 * u1);
      }
      add_pair(ra, rb, 2 * K + kk, sb0, sb1);
    } else {
#pragma unroll
      for (int m2 = 0; m2 < 2 * K; ++m2)
        if (m2 % K != K - 1) { accumulate(slice, l, p, m2, t[m2]); accumulate(slice, l, p, PWL_P + m2, du * t[m2]); }
      accumulate(slice, l, p, 2 * K + kk, sb0);     accumulate(slice, l, p, PWL_P + 2 * K + kk, du * sb0);
      accumulate(slice, l, p, 2 * K + kk + 1, sb1); accumulate(slice, l, p, PWL_P + 2 * K + kk + 1, du * sb1);
    }
  };
  // the `first` spline's per-bin adjoint sums of the lane's samples (pair-wide; folded at the end)
  v2f Wb[K], Hb[K], Db[K + 1];
#pragma unroll
  for (int j = 0; j < K; ++j) { Wb[j] = splat<v2f>(0.0f); Hb[j] = splat<v2f>(0.0f); }
#pragma unroll
  for (int j = 0; j <= K; ++j) Db[j] = splat<v2f>(0.0f);

  auto flush = [&](int slice) {          // LDS accumulators -> the slice's statistics, and clear
    __syncthreads();
    stat_t* g = a.stats + (int64_t)slice * L * PWL_NPIECE * PWL_STAT;
    for (int i = tid; i < L * PWL_ACC_W * PWL_STAT; i += NT) {
      const int lp = i / PWL_STAT, m2 = i - lp * PWL_STAT;            // (layer, piece), entry
      const int l = lp / PWL_ACC_W, p = lp - l * PWL_ACC_W;
      stat_t* e = acc + lp * PWL_STAT_LDS + pwl_acc_entry(m2);
      stat_t v = 0;
      for (int r = 0; r < acc_r; ++r) { v += e[r * (acc_n + PWL_ACC_SKEW)]; e[r * (acc_n + PWL_ACC_SKEW)] = 0; }
      if (v != 0) atomicAdd(g + ((int64_t)l * PWL_NPIECE + p) * PWL_STAT + m2, v);
    }
    __syncthreads();
  };

  const int total = a.n_slices * a.tiles_per_slice;
  const int per_block = (total + gridDim.x - 1) / gridDim.x;
  const int t0 = blockIdx.x * per_block;
  const int t1 = t0 + per_block < total ? t0 + per_block : total;
  int cur = -1;
  // A tile's points and adjoints are requested one tile ahead: issued where they are used, the loads' ~2 us were a
  // third of a wave's time (rocprofv3 counters of round 3: 37 % of the wave cycles in s_waitcnt, 3 % of them on LDS)
  struct TileIn { f4 x, yb; v2f ldb; };
  auto tile_geom = [&](int tile, int& slice, int64_t& g, bool& v0, bool& v1) {
    slice = tile / a.tiles_per_slice;
    const int64_t s0 = (int64_t)slice * a.slice_len;
    const int64_t len = a.B - s0 < a.slice_len ? a.B - s0 : a.slice_len;
    const int64_t j = (int64_t)(tile - slice * a.tiles_per_slice) * TS + 2 * tid;      // the lane's samples: j, j + 1
    g = s0 + j;
    v0 = j < len; v1 = j + 1 < len;
  };
  auto tile_load = [&](int tile) {
    TileIn t;
    t.x = f4{0.f, 0.f, 0.f, 0.f}; t.yb = t.x; t.ldb = v2f{0.f, 0.f};
    int slice; int64_t g; bool v0, v1;
    tile_geom(tile, slice, g, v0, v1);
    const int64_t gp = a.pts_shared ? g - (int64_t)slice * a.slice_len : g;
    if (v1) {
      t.x = *reinterpret_cast<const f4*>(a.pts + 2 * gp);
      if (a.ybar) t.yb = *reinterpret_cast<const f4*>(a.ybar + 2 * g);
      if (a.ldbar) t.ldb = *reinterpret_cast<const v2f*>(a.ldbar + g);
    } else if (v0) {
      t.x[0] = a.pts[2 * gp]; t.x[1] = a.pts[2 * gp + 1];
      if (a.ybar) { t.yb[0] = a.ybar[2 * g]; t.yb[1] = a.ybar[2 * g + 1]; }
      if (a.ldbar) t.ldb.x = a.ldbar[g];
    }
    return t;
  };
  TileIn nxt;
  if (t0 < t1) nxt = tile_load(t0);
  for (int tile = t0; tile < t1; ++tile) {
    int slice; int64_t g; bool v0, v1;
    tile_geom(tile, slice, g, v0, v1);
    if (slice != cur) {
      if (cur >= 0) flush(cur); else __syncthreads();
      pwl_stage<WIN>(tbl, a.tables + (int64_t)slice * L * PWL_TBL, L, tid, NT);
      cur = slice;
      __syncthreads();
    }
    const f4 x = nxt.x, yb = nxt.yb;
    v2f ld_bar = nxt.ldb;
    if (tile + 1 < t1) nxt = tile_load(tile + 1);
    __builtin_amdgcn_sched_barrier(0);
    // a non-finite POINT would pass unnoticed (the table search and the splines' clamps turn it into some finite
    // point): it poisons the call's gradient like a non-finite adjoint does
    if (!(fabsf((x[0] + x[1]) + (x[2] + x[3])) < INFINITY)) atomicOr(a.amax + 1, 1u);
    v2f u0 = {x[0], x[2]}, u1 = {x[1], x[3]};
    v2f ob0 = {yb[0], yb[2]}, ob1 = {yb[1], yb[3]};
    [[maybe_unused]] v2f lacc = splat<v2f>(0.0f);      // SEED: the pass's log|det J|
    const float* gtbl = a.tables + (int64_t)slice * L * PWL_TBL;
    // ---- forward through the tables, keeping every layer's inputs and outputs (flow2_tables' calls)
    v2f in_f[MAXL], in_o[MAXL], out_f[MAXL];
#pragma unroll
    for (int step = 0; step < MAXL; ++step) {
      if (step < L) {
        const int l = TO_BASE ? L - 1 - step : step;
        const bool odd = l & 1;
        const v2f uf = odd ? u1 : u0, uo = odd ? u0 : u1;
        v2f of, oo = splat<v2f>(0.0f), ld;
        table_spline<K, INV, true, v2f>(tab, uf, sc, of, ld);
        if constexpr (SEED) lacc += ld;
        // The backward never reads a layer's conditioned OUTPUT: data -> base takes the spline partials at the layer's
        // input, base -> data at the output, which cond_spline_bwd_rows forms itself in the bin it selects.  So the last
        // layer's table lookup, softmax and spline -- whose result nothing downstream reads -- are skipped here
        if (SEED || step != L - 1) {      // (SEED: the term's value and seeds need the whole pass)
          const float* tl = tbl + l * pwl_ltbl(WIN);
          const float* gl = gtbl + (int64_t)l * PWL_TBL;
          const v2f uc = TO_BASE ? of : uf;
          PwlRows rr;
          bool general;
          v2f qa[K], qb[K];
          pwl_find<WIN>(tl, uc, rr, general);
          rr.dua = pwl_logit_pairs<WIN>(rr.ra, gl, rr.pa, uc.x, qa);
          rr.dub = pwl_logit_pairs<WIN>(rr.rb, gl, rr.pb, uc.y, qb);
          auto slopes = [&](int ka, int kb, v2f& ta, v2f& tb) {
            ta = pwl_slope_pair<WIN>(rr.ra, gl, rr.pa, ka, rr.dua);
            tb = pwl_slope_pair<WIN>(rr.rb, gl, rr.pb, kb, rr.dub);
          };
          cond_spline_rows<K, INV, true, false, false>(qa, qb, slopes, uo, sc, oo, ld);
          if constexpr (SEED) lacc += ld;
        }
        in_f[step] = uf; in_o[step] = uo; out_f[step] = of;
        u0 = odd ? oo : of; u1 = odd ? of : oo;
      }
    }
    if constexpr (SEED) {
      // -log_prob = |x|^2 / 2 + log 2 pi - ildj at the recovered base point x; d(seed_coef * sum) / d(x, ildj)
      const v2f nlp = -base_logprob<v2f>([&](int q) { return q == 0 ? u0 : u1; }, 2) - lacc;
      float part = (v0 ? nlp.x : 0.0f) + (v1 ? nlp.y : 0.0f);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      ssum.add(a.sums, slice, part);
      ob0 = v2f{v0 ? u0.x : 0.0f, v1 ? u0.y : 0.0f} * a.seed_coef;
      ob1 = v2f{v0 ? u1.x : 0.0f, v1 ? u1.y : 0.0f} * a.seed_coef;
      ld_bar = v2f{v0 ? -a.seed_coef : 0.0f, v1 ? -a.seed_coef : 0.0f};
    }
    // ---- backward
#pragma unroll
    for (int step = MAXL - 1; step >= 0; --step) {
      if (step < L) {
        const int l = TO_BASE ? L - 1 - step : step;
        const bool odd = l & 1;
        v2f ob_f = odd ? ob1 : ob0;
        const v2f ob_o = odd ? ob0 : ob1;
        const float* tl = tbl + l * pwl_ltbl(WIN);
        const float* gl = gtbl + (int64_t)l * PWL_TBL;
        const v2f uc = TO_BASE ? out_f[step] : in_f[step];
        PwlRows rr;
        bool general;
        v2f qa[K], qb[K];
        pwl_find<WIN>(tl, uc, rr, general);
        rr.dua = pwl_logit_pairs<WIN>(rr.ra, gl, rr.pa, uc.x, qa);
        rr.dub = pwl_logit_pairs<WIN>(rr.rb, gl, rr.pb, uc.y, qb);
        auto slopes = [&](int ka, int kb, v2f& ta, v2f& tb) {
          ta = pwl_slope_pair<WIN>(rr.ra, gl, rr.pa, ka, rr.dua);
          tb = pwl_slope_pair<WIN>(rr.rb, gl, rr.pb, kb, rr.dub);
        };
        // theta_bar: the 2K softmax entries in tb, the two non-zero slope entries (knots kk, kk + 1 of the selected
        // bin) apart -- their accumulators and their rows' slopes are addressed with kk
        v2f tb[2 * K], kkf, sb0, sb1;
        const v2f ub_o = cond_spline_bwd_rows<K, INV, true>(qa, qb, slopes, in_o[step], ob_o, ld_bar, sc, tb, kkf, sb0, sb1,
                                                            __builtin_amdgcn_ballot_w64(general) == 0);
        const int kka = (int)kkf.x, kkb = (int)kkf.y;
        float ta[2 * K], tc[2 * K];
#pragma unroll
        for (int m2 = 0; m2 < 2 * K; ++m2) { ta[m2] = tb[m2].x; tc[m2] = tb[m2].y; }
        const v2f ucond_bar = v2f{pwl_row_dot<WIN>(rr.ra, gl, rr.pa, kka, ta, sb0.x, sb1.x),
                                  pwl_row_dot<WIN>(rr.rb, gl, rr.pb, kkb, tc, sb0.y, sb1.y)};
        v2f ub_f = splat<v2f>(0.0f);
        if (TO_BASE) ob_f += ucond_bar; else ub_f = ucond_bar;
        ub_f += table_spline_bwd<K, INV, true>(tab, in_f[step], ob_f, ld_bar, sc, Wb, Hb, Db);
        // (last: LDS operations complete in order, a read issued behind the 40 accumulations would wait for all of them)
        if (v0) add_stats(slice, l, rr.pa, rr.dua, ta, kka, sb0.x, sb1.x);
        if (v1) add_stats(slice, l, rr.pb, rr.dub, tc, kkb, sb0.y, sb1.y);
        ob0 = odd ? ub_o : ub_f; ob1 = odd ? ub_f : ub_o;
      }
    }
    if (a.xbar) {
      if (v1) *reinterpret_cast<f4*>(a.xbar + 2 * g) = f4{ob0.x, ob1.x, ob0.y, ob1.y};
      else if (v0) { a.xbar[2 * g] = ob0.x; a.xbar[2 * g + 1] = ob1.x; }
    }
  }
  if (cur >= 0) flush(cur);
  if constexpr (SEED) ssum.flush();
  // the `first` spline's per-bin adjoint sums: wave shuffle, block reduce, one slab entry per block
  {
    float r[GP];
#pragma unroll
    for (int j = 0; j < GK; ++j) { r[j] = Wb[j].x + Wb[j].y; r[GK + j] = Hb[j].x + Hb[j].y; }
#pragma unroll
    for (int j = 0; j <= GK; ++j) r[2 * GK + j] = Db[j].x + Db[j].y;
#pragma unroll
    for (int j = 0; j < GP; ++j) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) r[j] += __shfl_xor(r[j], off, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int j = 0; j < GP; ++j) red[(tid >> 6) * GP + j] = r[j];
    }
    __syncthreads();
    float* slab = a.slabs + (int64_t)blockIdx.x * a.n_params;
    for (int64_t i = GP + tid; i < a.n_params; i += NT) slab[i] = 0.0f;
    if (tid < GP) {
      float s = 0.0f;
      for (int w2 = 0; w2 < (NT >> 6); ++w2) s += red[w2 * GP + tid];
      slab[tid] = s;
    }
  }
}

// One block per (slice, layer): the slice's per-piece statistics -> that layer's 592 conditioner gradients, written
// (with zeros elsewhere) into slab first_slab + block; the statistics are cleared for the next call.
struct StatsFinishArgs {
  const float* weights;  // prep + hdr: the conditioner weights snapshot
  int64_t per_layer;
  const float* cvals;    // [n_slices]
  const float* tables;
  stat_t* stats;
  stat_t* coarse;
  const uint32_t* amax;  // [0] largest adjoint, [1] non-finite flag
  uint32_t amax_bits;    // != 0: in place of amax[0] (VjpPwlArgs)
  float* slabs;          // [first_slab + n_slices * L][n_params]
  int64_t n_params;
  int32_t L, first_slab;
  int32_t split;         // blocks per (slice, layer): block g of them takes the pieces of every split-th group of four
};

__global__ __launch_bounds__(256) void pwl_stats_finish_kernel(const StatsFinishArgs a) {
  constexpr int H = PWL_H, P = PWL_P, NW = 2 * H + H + H * H + H + H * P + P;      // 592 floats of one conditioner
  constexpr int NWV = 4;                                   // waves: one piece per wave at a time
  constexpr int PER_LANE = (NW + 63) / 64;                 // 10 outputs per lane
  __shared__ float av[H], bv[H], W1[H * H], b1[H], Wo[H * P];
  __shared__ float stat[PWL_NPIECE * PWL_STAT];            // the slice-layer's statistics, read once (37 KB)
  __shared__ float scr[NWV][9 * H];                        // per wave: Bu | m1a | m1b | Pk | Qk | G2 | G2u | G1 | G1u
  __shared__ float part[NWV][NW];                          // the waves' partial results
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // (few slices -- the density-fit term has one -- would leave the chip to ns x L workgroups walking 289 pieces each)
  const int sl = blockIdx.x / a.split, gsub = blockIdx.x - sl * a.split;
  const int slice = sl / a.L, l = sl % a.L;
  const float* w = a.weights + l * a.per_layer;
  const float c = a.cvals[slice];
  if (tid < H) {
    av[tid] = w[H + tid];
    bv[tid] = fmaf(w[tid], c, w[2 * H + tid]);
    b1[tid] = w[3 * H + H * H + tid];
  }
  for (int i = tid; i < H * H; i += blockDim.x) { W1[i] = w[3 * H + i]; Wo[i] = w[3 * H + H * H + H + i]; }
  const float* T = a.tables + (int64_t)sl * PWL_TBL;
  stat_t* st = a.stats + (int64_t)sl * PWL_NPIECE * PWL_STAT;
  const int n = __float_as_int(T[PWL_N_SLOT]);
  const double inv_scale = 1.0 / stat_scale(a.amax_bits ? a.amax_bits : *a.amax);
  stat_t* sc2 = a.coarse + (int64_t)sl * PWL_NPIECE * PWL_STAT;
  auto mine = [&](int p) { return (p / NWV) % a.split == gsub; };
  for (int i = tid; i < (n + 1) * PWL_STAT; i += blockDim.x) {
    if (!mine(i / PWL_STAT)) continue;
    const stat_t q = st[i], qc = sc2[i];
    stat[i] = (float)(((double)(long long)q + (double)(long long)qc * 4294967296.0) * inv_scale);
    if (q != 0) st[i] = 0;                                 // cleared for the next call
    if (qc != 0) sc2[i] = 0;
  }
  __syncthreads();
  // vjp_pwl_kernel leaves out the last logit of each softmax group (widths, heights): the group's adjoints sum to zero
  for (int i = tid; i < (n + 1) * 4; i += blockDim.x) {
    if (!mine(i >> 2)) continue;
    float* g = stat + (i >> 2) * PWL_STAT + (i & 2 ? P : 0) + (i & 1 ? GK : 0);
    g[GK - 1] = -((g[0] + g[1]) + (g[2] + g[3]));
  }
  __syncthreads();
  float out[PER_LANE];
#pragma unroll
  for (int q = 0; q < PER_LANE; ++q) out[q] = 0.0f;
  float* Bu = scr[wv], *m1a = Bu + H, *m1b = m1a + H, *Pk = m1b + H, *Qk = Pk + H, *G2 = Qk + H, *G2u = G2 + H,
        *G1 = G2u + H, *G1u = G1 + H;
  for (int p = wv + NWV * gsub; p <= n; p += NWV * a.split) {      // wave-uniform loop: no block barrier inside
    const float* A = stat + p * PWL_STAT;
    const float sv = lane < PWL_STAT ? A[lane] : 0.0f;
    if (__builtin_amdgcn_ballot_w64(sv != 0.0f) == 0) continue;
    const float lo = p == 0 ? -INFINITY : T[p - 1], hi = p < n ? T[p] : INFINITY;
    const bool fl = lo > -INFINITY, fh = hi < INFINITY;
    const float ut = fl && fh ? 0.5f * (lo + hi) : (fl ? lo + 1.0f : (fh ? hi - 1.0f : 0.0f));
    const float uref = T[PWL_OFF_REF + p];
    float on1 = 0.0f;
    if (lane < H) {
      Bu[lane] = fmaf(uref, A[lane], A[P + lane]);          // sum (u - u_ref) g  ->  sum u g
      on1 = fmaf(av[lane], ut, bv[lane]) > 0.0f ? 1.0f : 0.0f;
      m1a[lane] = on1 * av[lane]; m1b[lane] = on1 * bv[lane];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
    if (lane < H) {
      const int k = lane;
      float Ps = 0.0f, Qs = b1[k], ha = 0.0f, hb = 0.0f;
      for (int j = 0; j < H; ++j) { Ps = fmaf(W1[j * H + k], m1a[j], Ps); Qs = fmaf(W1[j * H + k], m1b[j], Qs); }
      for (int m = 0; m < P; ++m) { ha = fmaf(Wo[k * P + m], A[m], ha); hb = fmaf(Wo[k * P + m], Bu[m], hb); }
      const float on2 = fmaf(Ps, ut, Qs) > 0.0f ? 1.0f : 0.0f;
      Pk[k] = on2 * Ps; Qk[k] = on2 * Qs; G2[k] = on2 * ha; G2u[k] = on2 * hb;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
    if (lane < H) {
      float ga = 0.0f, gb = 0.0f;
      for (int k = 0; k < H; ++k) { ga = fmaf(W1[lane * H + k], G2[k], ga); gb = fmaf(W1[lane * H + k], G2u[k], gb); }
      G1[lane] = on1 * ga; G1u[lane] = on1 * gb;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
      const int o = lane + q * 64;
      if (o < NW) {
        float v;
        if (o < H) v = c * G1[o];                                            // W0[c row]
        else if (o < 2 * H) v = G1u[o - H];                                  // W0[u row]
        else if (o < 3 * H) v = G1[o - 2 * H];                               // b0
        else if (o < 3 * H + H * H) { const int e = o - 3 * H, j = e / H, k = e % H; v = fmaf(m1a[j], G2u[k], m1b[j] * G2[k]); }
        else if (o < 4 * H + H * H) v = G2[o - 3 * H - H * H];               // b1
        else if (o < 4 * H + H * H + H * P) { const int e = o - 4 * H - H * H, k = e / P, m = e % P; v = fmaf(Pk[k], Bu[m], Qk[k] * A[m]); }
        else v = A[o - 4 * H - H * H - H * P];                               // bo
        out[q] += v;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();      // scr is reused by the next piece
  }
#pragma unroll
  for (int q = 0; q < PER_LANE; ++q) { const int o = lane + q * 64; if (o < NW) part[wv][o] = out[q]; }
  __syncthreads();
  // slab 1 + block: zeros except this layer's conditioner
  float* slab = a.slabs + (int64_t)(a.first_slab + blockIdx.x) * a.n_params;
  const int64_t base = GP + (int64_t)l * a.per_layer;
  for (int64_t i = tid; i < a.n_params; i += blockDim.x) {
    const int64_t o = i - base;
    slab[i] = (o >= 0 && o < NW) ? (part[0][o] + part[1][o]) + (part[2][o] + part[3][o]) : 0.0f;
  }
  if (a.amax[1] != 0) {      // a non-finite adjoint or term somewhere in the call: the gradient says so
    for (int64_t i = tid; i < a.n_params; i += blockDim.x) slab[i] = __int_as_float(0x7fc00000);
  }
}

}  // namespace cnf

using namespace cnf;

// [64 bytes: the call's largest adjoint][statistics][coarse statistics] of PWL_STAT_SLICES slices
size_t pwl_stats_bytes(int L) { return 64 + 2 * sizeof(stat_t) * (size_t)PWL_STAT_SLICES * L * PWL_NPIECE * PWL_STAT; }

// The vjp_pwl_kernel instantiation of a pass (L = 2, every configuration of the reference, has its own with the layer
// loop unrolled; seeded: the density-fit form, data -> base)
typedef void (*VjpPwlKernel)(const VjpPwlArgs);
static VjpPwlKernel vjp_pwl_kernel_of(bool seeded, int to_base, int L) {
  if (seeded) return L == 2 ? vjp_pwl_kernel<true, 2, true> : vjp_pwl_kernel<true, 0, true>;
  if (to_base) return L == 2 ? vjp_pwl_kernel<true, 2> : vjp_pwl_kernel<true>;
  return L == 2 ? vjp_pwl_kernel<false, 2> : vjp_pwl_kernel<false>;
}

// (cnf_host.h)  vjp_pwl_kernel + pwl_stats_finish_kernel + grad_finish_kernel: dim 2, the reference's network, a
// condition uniform over slices, tables reserved on the stream (cnf_model_reserve) for at least min(n_slices,
// PWL_STAT_SLICES) slices.  seed_sums != null (cnf_neg_logprob_vjp): no adjoints come in, the kernel seeds itself with
// seed_coef and writes the slices' sums of -log_prob.  built != null: the slices' tables are built (one chunk), the
// adjoint maximum is in place (term_residual_launch left it), and `pts` is ONE slice of points that every slice reads.
int pass_vjp_pwl(CnfModel* m, int to_base, const float* pts, const float* c, int64_t c_block, const float* ybar,
                 const float* ldbar, float* xbar, float* grad, const float* params, int64_t B, hipStream_t stream,
                 float seed_coef, double* seed_sums, const float* built) {
  static_assert(PWL_H == 16 && GK == 5, "pwl_network (cnf_common.h) states the tables' network");
  const int L = m->cfg.num_layers;
  const int64_t slice_len = c_block < B ? c_block : B;
  const int64_t n_slices = (B + slice_len - 1) / slice_len;
  if (!pwl_term_on_tables(m, slice_len, B, true)) return CNF_ERR_UNSUPPORTED;
  // (a lane's two samples are one 16-byte access of the points and adjoints, one 8-byte access of ldbar)
  if ((reinterpret_cast<uintptr_t>(pts) & 15) || (reinterpret_cast<uintptr_t>(ybar) & 15) ||
      (reinterpret_cast<uintptr_t>(xbar) & 15) || (reinterpret_cast<uintptr_t>(ldbar) & 7) || (n_slices > 1 && (slice_len & 1)))
    return CNF_ERR_UNSUPPORTED;
  const int threads = VJP_PWL_THREADS, tile = 2 * threads;
  auto lds_bytes = [&](int acc_r) {
    return sizeof(float) * (size_t)(((hdr_floats(GK) + 3) & ~3) + L * pwl_ltbl(PWL_LROWS) +
                                    2 * acc_r * (L * PWL_ACC_W * PWL_STAT_LDS + PWL_ACC_SKEW) + (threads / 64) * GP);
  };
  int acc_r = PWL_ACC_R;
  while (acc_r > 1 && lds_bytes(acc_r) > 160 * 1024) --acc_r;
  const size_t lds = lds_bytes(acc_r);
  if (lds > 160 * 1024) return CNF_ERR_UNSUPPORTED;
  const bool seeded = seed_sums != nullptr;
  const VjpPwlKernel kernel = vjp_pwl_kernel_of(seeded, to_base, L);
  if (!ensure_lds(kernel, lds)) return CNF_ERR_UNSUPPORTED;
  // The seeds are seed_coef x (a base point | 1): the scale is set for adjoints up to 32 |seed_coef| -- base points
  // lie within the splines' range of +-10 unless the data does not -- with the 2^22 of head room every term has
  uint32_t amax_bits = 0;
  if (seeded) {
    const float bound = 32.0f * fabsf(seed_coef);
    union { float f; uint32_t u; } bits; bits.f = bound; amax_bits = bits.u;
    if (!(bound < INFINITY)) return CNF_ERR_INVALID;
    if (zero_sums(seed_sums, n_slices, B, stream) < 0) return CNF_ERR_HIP;
  }
  const int64_t tps = (slice_len + tile - 1) / tile;
  if (built && n_slices > PWL_STAT_SLICES) return CNF_ERR_UNSUPPORTED;
  for (int64_t s0 = 0; s0 < n_slices; s0 += PWL_STAT_SLICES) {
    const int64_t ns = n_slices - s0 < PWL_STAT_SLICES ? n_slices - s0 : PWL_STAT_SLICES;
    float* tables = const_cast<float*>(built);
    const int r = built ? CNF_OK : cnf_internal_build_tables(m, stream, c + s0, ns, &tables);
    if (r != CNF_OK) return s0 == 0 ? r : CNF_ERR_HIP;          // (a later chunk cannot fail on its own)
    m->last_path = CNF_PATH_TABLES;
    const int64_t first = s0 * slice_len;
    VjpPwlArgs a;
    a.m = model_args(m);
    a.pts = pts + (built ? 0 : 2 * first); a.pts_shared = built ? 1 : 0; a.ybar = ybar ? ybar + 2 * first : nullptr; a.ldbar = ldbar ? ldbar + first : nullptr;
    a.xbar = xbar ? xbar + 2 * first : nullptr;
    uint32_t* amax = reinterpret_cast<uint32_t*>(m->pwl_stats);
    stat_t* stats = reinterpret_cast<stat_t*>(reinterpret_cast<char*>(m->pwl_stats) + 64);
    stat_t* coarse = stats + (size_t)PWL_STAT_SLICES * L * PWL_NPIECE * PWL_STAT;
    a.tables = tables; a.stats = stats; a.coarse = coarse; a.amax = amax; a.slabs = m->grad_slabs; a.n_params = m->n_params;
    a.B = (B - first) < ns * slice_len ? (B - first) : ns * slice_len;
    a.slice_len = slice_len; a.n_slices = (int32_t)ns; a.tiles_per_slice = (int32_t)tps; a.acc_r = acc_r;
    a.seed_coef = seed_coef; a.sums = seeded ? seed_sums + s0 : nullptr; a.amax_bits = amax_bits;
    // (amax is zero on entry: cleared at allocation and by the grad_finish_kernel launch of the previous chunk or call)
    if (!seeded && !built &&
        launch_plain(adjoint_max_kernel, m->num_cus * 4, 256, 0, stream, a.ybar, a.ybar ? 2 * a.B : 0, a.ldbar,
                     a.ldbar ? a.B : 0, amax) != CNF_OK)
      return CNF_ERR_HIP;
    const int64_t tiles = ns * tps;
    const int64_t grid = tiles < m->num_cus ? tiles : m->num_cus;
    const int split = ns * L <= 32 ? 8 : 1;
    if (grid + ns * L * split > m->grad_max_blocks * 4) return s0 == 0 ? CNF_ERR_UNSUPPORTED : CNF_ERR_HIP;      // (slabs: cnf_grad_enable)
    StatsFinishArgs f;
    f.weights = m->prep + hdr_floats(GK); f.per_layer = m->per_layer; f.cvals = c + s0; f.tables = tables;
    f.stats = stats; f.coarse = coarse; f.amax = amax; f.amax_bits = amax_bits; f.slabs = m->grad_slabs; f.n_params = m->n_params; f.L = L;
    f.first_slab = (int32_t)grid; f.split = split;
    if (launch_plain(kernel, grid, threads, lds, stream, a) != CNF_OK ||
        launch_plain(pwl_stats_finish_kernel, ns * L * split, 256, 0, stream, f) != CNF_OK ||
        grad_finish(m, grid + ns * L * split, params, grad, amax, stream) != CNF_OK)
      return CNF_ERR_HIP;
  }
  return CNF_OK;
}

extern "C" int cnf_kinetic_potential_vjp(CnfModel* m, const float* z, int64_t count, const float* c, int32_t S, float dt,
                                         float c_kin, int32_t subtype, float pot_a, float c_pot, double* kin,
                                         double* pot, float* grad, const float* params, float* work, void* stream_) {
  if (!m || !z || !c || !kin || (grad && !params) || !work || count < 1 || S < 1 || !(dt > 0.f)) return CNF_ERR_INVALID;
  if ((subtype >= 0) != (pot != nullptr) || (subtype >= 0 && !potential_ok(subtype))) return CNF_ERR_INVALID;
  // (local, not backward_check: slab room is asked before the config here, and the config only where gradients are)
  if (!m->params_set || (grad && !m->grad_slabs)) return CNF_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t sets = pot ? 3 : 2, ns = sets * S, B = ns * count, n = (int64_t)S * count;
  // (what pass_vjp_pwl will ask, before anything is launched; grad == NULL: the terms' values alone)
  if (!pwl_term_on_tables(m, count, B, grad != nullptr) || (grad && !cnf_grad_supported(&m->cfg))) return CNF_ERR_UNSUPPORTED;
  if (ns > PWL_STAT_SLICES || (count & 1) || (reinterpret_cast<uintptr_t>(work) & 15)) return CNF_ERR_UNSUPPORTED;
  if (const int rc = backward_check(m, CHECK_WAIT, stream); rc != CNF_OK) return rc;
  float* r = work;
  float* rbar = grad ? work + 2 * B : nullptr;
  float* tables = nullptr;
  int rc = cnf_internal_build_tables(m, stream, c, ns, &tables);
  if (rc != CNF_OK) return rc;
  rc = cnf_internal_flow_shared(m, stream, z, c, count, ns, tables, r);
  if (rc != CNF_OK) return rc;                                   // (UNSUPPORTED: nothing but the tables was touched)
  uint32_t* amax = grad ? reinterpret_cast<uint32_t*>(m->pwl_stats) : nullptr;    // zero on entry (pass_vjp_pwl)
  if (zero_sums(kin, S, n, stream) < 0 || (pot && zero_sums(pot, S, n, stream) < 0)) return CNF_ERR_HIP;
  rc = term_residual_launch(CNF_TERM_KINETIC, r, nullptr, n, count, 2, 0, dt, c_kin, kin, rbar, nullptr, amax, stream);
  if (rc == CNF_OK && pot)
    rc = term_residual_launch(CNF_TERM_POTENTIAL, r + 4 * n, nullptr, n, count, 2, subtype, pot_a, c_pot, pot,
                              rbar ? rbar + 4 * n : nullptr, nullptr, amax, stream);
  if (rc != CNF_OK || !grad) return rc;
  rc = pass_vjp_pwl(m, 0, z, c, count, rbar, nullptr, nullptr, grad, params, B, stream, 0.0f, nullptr, tables);
  if (rc != CNF_OK) {      // the adjoint maximum was left behind for a backward that did not run
    (void)hipMemsetAsync(amax, 0, 8, stream);
    return rc == CNF_ERR_UNSUPPORTED ? CNF_ERR_HIP : rc;
  }
  return CNF_OK;
}

extern "C" int cnf_neg_logprob_vjp(CnfModel* m, const float* pts, const float* c, int64_t c_block, float loss_coef,
                                   double* sums, float* grad, const float* params, int64_t B, void* stream) {
  if (!m || !pts || !c || !sums || !grad || !params || B < 0 || c_block < 1) return CNF_ERR_INVALID;
  if (!m->grad_slabs) return CNF_ERR_INVALID;      // (local: this entry asks for slab room before the config)
  if (const int rc = backward_check(m, CHECK_MODEL, nullptr); rc != CNF_OK) return rc;
  if (B == 0) return CNF_OK;
  if (const int rc = backward_check(m, CHECK_WAIT, (hipStream_t)stream); rc != CNF_OK) return rc;
  return pass_vjp_pwl(m, 1, pts, c, c_block, nullptr, nullptr, nullptr, grad, params, B, (hipStream_t)stream, loss_coef, sums);
}
