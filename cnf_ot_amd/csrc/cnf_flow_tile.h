// cnf_flow_tile.h -- device code shared by the kernel families that run the flow on an LDS tile or on a sample pair
// held in registers (flow_kernel, flow_dpar_kernel, flow_pwl_kernel, loss_kernel, loss_pwl_kernel, fields_kernel: all
// in cnf_flow.hip): the flow kernels' argument struct, the tile load / store / noise helpers, flow_pass, and the table
// path's flow2_tables.  Templates and __forceinline__ functions only: no kernel is defined here.
#pragma once
#include "cnf_common.h"
#include "cnf_pwl.h"
#include "cnf_first_table.h"

namespace cnf {

enum CMode { C_SINGLE = 0, C_PER_SAMPLE = 1, C_TILE_UNIFORM = 2, C_GENERIC = 3 };
enum AuxMode { AUX_LOGDET = 0, AUX_LOGPROB = 1 };


template <class R> struct FlowArgsT {
  ModelArgs m;
  const R* in;           // [B, D]
  const R* c;            // conditions
  R* out;                // [B, D] or null
  R* aux;                // [B] logdet / logprob, or null
  int64_t B;
  int64_t c_block;
  int32_t c_mode, aux_mode;
  int32_t div_magic;     // ceil(2^32 / D): e / D == umulhi(e, magic) for e < 2^16
  // device-side choice between two kernels enqueued for the same call (uniform-condition detection,
  // cond_uniform_kernel): this kernel runs only if (*gate == gate_epoch) == gate_want; null: always
  const uint32_t* gate;
  uint32_t gate_epoch;
  int32_t gate_want;
  // finite-difference mode (cnf_logprob_fd; data -> base only): `in` holds B / fd2 points r_i and evaluation
  // point j = i * fd2 + 2 d + s is r_i + (s ? -fd_h : +fd_h) e_d (fd2 = 2 D); aux[i * D + d] receives
  // (log_prob(j) - log_prob(j + 1)) * fd_inv_dx.  fd2 = 0: off.
  int32_t fd2;
  R fd_h, fd_inv_dx;
  // in == null (float32, base -> data only; cnf_sample_logprob_seeded): the points are base noise drawn in the kernel,
  // sample i = stream sample first_sample + (i / c_block) * slice_stride + i % c_block of the cnf_fill_normal stream
  uint64_t seed;
  int64_t first_sample, slice_stride;
};
typedef FlowArgsT<float> FlowArgs;
typedef FlowArgsT<double> FlowArgsD;

template <class A> __device__ __forceinline__ bool gate_closed(const A& a) {
  return a.gate && ((*a.gate == a.gate_epoch) ? 1 : 0) != a.gate_want;
}

// ---------------------------------------------------------------------------
// LDS tile: [hdr table][U: D x TS][O: D x TS], TS = 256 * SPL samples per
// workgroup.  Lane t owns samples SPL*t .. SPL*t+SPL-1 of the tile: its column
// is U[d*TS + SPL*t] (one ds_read_b32 / ds_read_b64 per dimension,
// conflict-free).
// ---------------------------------------------------------------------------
// e / D for e < 2^16 (a tile has at most 512 * 64 elements): one v_mul_hi_u32
// instead of the ~20-instruction 32-bit division sequence.
template <class R>
__device__ __forceinline__ void tile_load(const R* __restrict__ g, R* U, int D, uint32_t magic, int TS,
                                          int64_t tile_start, int64_t B) {
  const int64_t base = tile_start * D;
  const int n_el = (int)(B - tile_start < TS ? B - tile_start : TS) * D;
  for (int e = threadIdx.x; e < TS * D; e += TILE) {
    const int s = magic ? (int)__umulhi((uint32_t)e, magic) : e, d = e - s * D;   // magic 0: D = 1
    U[d * TS + s] = e < n_el ? g[base + e] : (R)0;
  }
}

// One tile of base noise straight into LDS: the tile's TS*D stream elements are
// contiguous; a thread draws whole Philox blocks (4 normals) and scatters them.
__device__ __forceinline__ void tile_noise(uint64_t seed, uint64_t first_element, float* U, int D, uint32_t magic,
                                           int TS, int64_t n_valid_samples, int nthreads = TILE) {
  const int n_el = (int)(n_valid_samples < TS ? n_valid_samples : TS) * D;
  const uint64_t blk0 = first_element >> 2;
  const int n_blk = (int)(((first_element + (uint64_t)(TS * D) - 1) >> 2) - blk0) + 1;
  for (int q = threadIdx.x; q < n_blk; q += nthreads) {
    const uint64_t blk = blk0 + (uint64_t)q;
    float z[4];
    philox_normals4(seed, blk, z);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t e = (int64_t)((blk << 2) + r) - (int64_t)first_element;
      if (e >= 0 && e < TS * D) {
        const int s = magic ? (int)__umulhi((uint32_t)e, magic) : (int)e, d = (int)e - s * D;
        U[d * TS + s] = e < n_el ? z[r] : 0.0f;
      }
    }
  }
}

__device__ __forceinline__ float normal_at(uint64_t seed, uint64_t e) {     // element e of the cnf_fill_normal stream
  float z[4];
  philox_normals4(seed, e >> 2, z);
  return z[e & 3];
}

// The tile of a seeded flow call (FlowArgsT::in == null): one contiguous run of the stream where the tile lies in
// one slice (or the slices follow each other in the stream), element by element otherwise.
__device__ __forceinline__ void tile_noise_flow(const FlowArgsT<float>& a, float* U, int D, uint32_t magic, int TS,
                                                int64_t tile_start, int nthreads) {
  const int64_t left = a.B - tile_start;
  const int64_t last = tile_start + (left < TS ? left : TS) - 1;
  const bool one = a.c_block >= a.B;
  const int64_t s0 = one ? 0 : tile_start / a.c_block, s1 = one ? 0 : last / a.c_block;
  if (s0 == s1 || a.slice_stride == a.c_block) {
    const int64_t st = a.first_sample + s0 * a.slice_stride + (tile_start - s0 * a.c_block);
    tile_noise(a.seed, (uint64_t)st * (uint64_t)D, U, D, magic, TS, left, nthreads);
    return;
  }
  const int n_el = (int)(left < TS ? left : TS) * D;
  for (int e = threadIdx.x; e < TS * D; e += nthreads) {
    const int s = magic ? (int)__umulhi((uint32_t)e, magic) : e, d = e - s * D;
    float v = 0.0f;
    if (e < n_el) {
      const int64_t i = tile_start + s, sl = i / a.c_block;
      const int64_t st = a.first_sample + sl * a.slice_stride + (i - sl * a.c_block);
      v = normal_at(a.seed, (uint64_t)st * (uint64_t)D + (uint64_t)d);
    }
    U[d * TS + s] = v;
  }
}
__device__ __forceinline__ void tile_noise_flow(const FlowArgsT<double>&, double*, int, uint32_t, int, int64_t, int) {}

template <class R>
__device__ __forceinline__ void tile_store(R* __restrict__ g, const R* U, int D, uint32_t magic, int TS,
                                           int64_t tile_start, int64_t B) {
  const int64_t base = tile_start * D;
  const int n_el = (int)(B - tile_start < TS ? B - tile_start : TS) * D;
  for (int e = threadIdx.x; e < TS * D; e += TILE) {
    const int s = magic ? (int)__umulhi((uint32_t)e, magic) : e, d = e - s * D;
    if (e < n_el) g[base + e] = U[d * TS + s];
  }
}

template <class R>
__device__ __forceinline__ R load_cond1(const FlowArgsT<R>& a, int64_t tile_start, int64_t i) {
  if (a.fd2) {                                   // evaluation point -> its base point's condition
    if (a.c_mode == C_SINGLE) return a.c[0];
    return i < a.B ? a.c[(i / a.fd2) / a.c_block] : (R)0;
  }
  switch (a.c_mode) {
    case C_SINGLE: return a.c[0];
    case C_PER_SAMPLE: return i < a.B ? a.c[i] : (R)0;
    case C_TILE_UNIFORM: return a.c[tile_start / a.c_block];
    default: return i < a.B ? a.c[i / a.c_block] : (R)0;
  }
}
template <class T> __device__ __forceinline__ T load_cond(const FlowArgsT<typename Lanes<T>::real>& a, int64_t tile_start, int64_t i);
template <> __device__ __forceinline__ float load_cond<float>(const FlowArgs& a, int64_t ts, int64_t i) {
  return load_cond1(a, ts, i);
}
template <> __device__ __forceinline__ double load_cond<double>(const FlowArgsD& a, int64_t ts, int64_t i) {
  return load_cond1(a, ts, i);
}
template <> __device__ __forceinline__ v2f load_cond<v2f>(const FlowArgs& a, int64_t ts, int64_t i) {
  if (a.c_mode == C_SINGLE || a.c_mode == C_TILE_UNIFORM) return splat<v2f>(load_cond1(a, ts, i));
  return v2f{load_cond1(a, ts, i), load_cond1(a, ts, i + 1)};
}

// finite-difference mode: the tile's evaluation points are built from the base points on the fly
template <class R>
__device__ __forceinline__ void tile_load_fd(const FlowArgsT<R>& a, R* U, int D, uint32_t magic, int TS, int64_t tile_start) {
  const int n_el = (int)(a.B - tile_start < TS ? a.B - tile_start : TS) * D;
  for (int e = threadIdx.x; e < TS * D; e += TILE) {
    const int s = magic ? (int)__umulhi((uint32_t)e, magic) : e, d = e - s * D;
    R v = (R)0;
    if (e < n_el) {
      const int64_t j = tile_start + s, i = j / a.fd2;
      const int k = (int)(j - i * a.fd2);
      v = a.in[i * D + d];
      if ((k >> 1) == d) v += (k & 1) ? -a.fd_h : a.fd_h;
    }
    U[d * TS + s] = v;
  }
}
// (log_prob(+) - log_prob(-)) / dx of the pair (j, j + 1), j even
__device__ __forceinline__ void store_fd(const FlowArgs& a, int64_t j, v2f lp) {
  if (j + 1 < a.B) a.aux[j >> 1] = (lp.x - lp.y) * a.fd_inv_dx;
}
__device__ __forceinline__ void store_fd(const FlowArgs& a, int64_t j, float lp) {
  const float other = __shfl_xor(lp, 1, 64);
  if (!(j & 1) && j + 1 < a.B) a.aux[j >> 1] = (lp - other) * a.fd_inv_dx;
}
__device__ __forceinline__ void store_fd(const FlowArgsD&, int64_t, double) {}

__device__ __forceinline__ float hsum(float v) { return v; }
__device__ __forceinline__ v2f hsum(v2f v) { return v; }

// One pass of the whole flow over the thread's own sample(s), in place in LDS.
// TO_BASE=false: base -> data (chain.inverse, spline inverse, conditions on the
// layer input: conditional.py:169-177, autoregressive.py:109-136).
// TO_BASE=true : data -> base (chain.forward, spline forward, conditions on
// already-produced outputs: conditional.py:159-167, autoregressive.py:76-107).
// Returns the accumulated log|det J|; the result is left in `U` (swapped).
// PRECISE (TO_BASE only): the precise position path of cnf_device.h; `e2tab` is its 2^(-i/32) table in LDS and
// `bacc` receives sum_d x_d^2 of the recovered base point in float64.
// DFIX > 0: the event dimension is this compile-time constant (the single-batch kernel at dim 2: the dimension
// loop, the conditioner offsets and the tile transposes lose their runtime arithmetic)
template <int H, int K, bool TO_BASE, bool FAST, class T, bool MFMA = false, bool PRECISE = false, bool PERIODIC = false, int DFIX = 0>
__device__ __forceinline__ T flow_pass(const ModelArgs& a, const typename Lanes<T>::real* tab,
                                       typename Lanes<T>::real*& U, typename Lanes<T>::real*& O, T c,
                                       const double* e2tab = nullptr, const double* tabd = nullptr,
                                       typename Lanes<T>::real* LO = nullptr, BaseAcc<T>* bacc = nullptr) {
  typedef typename Lanes<T>::real R;
  static_assert(!PRECISE || (TO_BASE && !std::is_same<T, double>::value), "precise path: data -> base, fp32 kernels");
  const SplineConstsT<R>& sc = sc_of<R>(a);
  static_assert(!MFMA || (H == 16 && K == 5), "the MFMA conditioner is built for H = 16, P = 16");
  static_assert(!PERIODIC || (!MFMA && !PRECISE), "periodized: the scalar-weight conditioner, plain positions");
  constexpr int P = 3 * K + 1;
  constexpr bool INV = !TO_BASE;
  constexpr int SPL = Lanes<T>::N;
  constexpr int TS = TILE * SPL;
  uniform_ptr weights = as_uniform(a.prep + hdr_floats(K));
  const int D = DFIX ? DFIX : a.D;
  T acc = splat<T>(0.0f);
  for (int step = 0; step < a.L; ++step) {
    const int l = TO_BASE ? a.L - 1 - step : step;
    const bool odd = l & 1;                       // flows.py:141-143 perms
    const int first_idx = odd ? D - 1 : 0, idx_step = odd ? -1 : 1;
    R* cu = U + SPL * threadIdx.x;
    R* co = O + SPL * threadIdx.x;
    T o, ld, olo;
    const bool last = step == a.L - 1;
    [[maybe_unused]] R* clo = nullptr;
    if constexpr (PRECISE) {
      // LO[d]: what rounding dimension d's value to fp32 dropped (this thread's column; in place: read as the
      // layer's input, overwritten with its output).  The data themselves are exact fp32: zero before layer 1.
      clo = LO + SPL * threadIdx.x;
      const T vlo = step == 0 ? splat<T>(0.0f) : lds_get<T>(clo, first_idx, TS);
      table_spline_precise<K, FAST>(tab, tabd, lds_get<T>(cu, first_idx, TS), vlo, sc, o, ld, olo);
      lds_put(clo, first_idx, TS, olo);
      if (last) bacc->add(o, olo);
    } else {
      table_spline<K, INV, FAST, T>(tab, lds_get<T>(cu, first_idx, TS), sc, o, ld);
    }
    lds_put(co, first_idx, TS, o);
    acc += ld;
    uniform_ptr w = weights + l * a.per_layer;
    const float* wq = a.wq + l * a.per_layer_q;
    for (int d = 1; d < D; ++d) {
      const int i = first_idx + d * idx_step;
      T th[P];
      if constexpr (MFMA && !std::is_same<T, double>::value) {
        // (at dim 2 the MFMA-layout first layer is three back-to-back vector loads: faster than scalar loads +
        // a transpose for a lone wave -- 6.1 vs 6.4 us per 65 536-sample call; from dim 3 the row loop dominates)
        conditioner_mfma<T>(reinterpret_cast<const f4*>(wq), d, a.M, c, TO_BASE ? co : cu, first_idx, idx_step, TS, th,
                            D >= 3 ? w : nullptr);
        wq += cond_floats_mfma(d, a.M);
        w += cond_floats(d, H, a.M, P);
      } else {
        conditioner<H, P, T, PERIODIC>(w, d, a.M, c, TO_BASE ? co : cu, first_idx, idx_step, TS, th);
        w += cond_floats_p(d, H, a.M, P, PERIODIC);
      }
      if constexpr (PRECISE) {
        const T vlo = step == 0 ? splat<T>(0.0f) : lds_get<T>(clo, i, TS);
        cond_spline_precise<K, FAST, false>(th, lds_get<T>(cu, i, TS), vlo, sc, a.scd, e2tab, o, ld, olo);
        lds_put(clo, i, TS, olo);
        if (last) bacc->add(o, olo);
      } else {
        cond_spline<K, INV, FAST, T>(th, lds_get<T>(cu, i, TS), sc, o, ld);
      }
      lds_put(co, i, TS, o);
      acc += ld;
    }
    R* t = U; U = O; O = t;
  }
  return acc;
}

__device__ __forceinline__ void store_aux(float* aux, int64_t i, int64_t B, float r) {
  if (i < B) aux[i] = r;
}
__device__ __forceinline__ void store_aux(double* aux, int64_t i, int64_t B, double r) {
  if (i < B) aux[i] = r;
}
__device__ __forceinline__ void store_aux(float* aux, int64_t i, int64_t B, v2f r) {
  if (i + 1 < B && ((reinterpret_cast<uintptr_t>(aux + i) & 7) == 0)) *reinterpret_cast<v2f*>(aux + i) = r;
  else { if (i < B) aux[i] = r.x; if (i + 1 < B) aux[i + 1] = r.y; }
}

template <class R>
__device__ __forceinline__ void tile_load_n(const R* __restrict__ g, R* U, int D, uint32_t magic, int TS,
                                            int64_t tile_start, int64_t B, int nthreads) {
  const int64_t base = tile_start * D;
  const int n_el = (int)(B - tile_start < TS ? B - tile_start : TS) * D;
  for (int e = threadIdx.x; e < TS * D; e += nthreads) {
    const int s = magic ? (int)__umulhi((uint32_t)e, magic) : e, d = e - s * D;
    U[d * TS + s] = e < n_el ? g[base + e] : (R)0;
  }
}
template <class R>
__device__ __forceinline__ void tile_store_n(R* __restrict__ g, const R* U, int D, uint32_t magic, int TS,
                                             int64_t tile_start, int64_t B, int nthreads) {
  const int64_t base = tile_start * D;
  const int n_el = (int)(B - tile_start < TS ? B - tile_start : TS) * D;
  for (int e = threadIdx.x; e < n_el; e += nthreads) {
    const int s = magic ? (int)__umulhi((uint32_t)e, magic) : e, d = e - s * D;
    g[base + e] = U[d * TS + s];
  }
}

constexpr int PWL_MAX_THREADS = 1024;

// flow_pwl_kernel's dynamic LDS in floats: [header][L tables of `lrows` rows][the `first` spline's inverse table]; the
// precise path's float64 tables (data -> base) follow the L tables and are counted by the launch site.
constexpr int pwl_flow_lds_floats(int K, int L, int lrows, bool first_table) {
  return ((hdr_floats(K) + 3) & ~3) + L * pwl_ltbl(lrows) + (first_table ? FT_LDS_FLOATS : 0);
}
static_assert(pwl_flow_lds_floats(FT_K, 2, PWL_NPIECE, true) * sizeof(float) <= 160 * 1024,
              "the L = 2 kernel holds both conditioner tables and the inverse table");

// The dim-2 flow on one sample pair held in registers, conditioner from the tables (`tbl`: the L
// tables in LDS, `gtbl`: the same in global memory for rows past the LDS window).  In place;
// returns the accumulated log|det J| of the direction.
// SHIFT_FREE_OK: use the shift-free spline evaluation where the sample's grid cell allows it (the flow kernels;
// the loss kernel, at its register limit with three table sets, always evaluates the general form).
// LFIX > 0: the number of flow layers is this compile-time constant -- the layer loop is unrolled, the layer's
// parity (which coordinate is conditioned on which) and its table's LDS offset are literals instead of per-layer
// selects and address arithmetic.
// LEAN_OK (flow_pwl_kernel): the sampling direction takes the shorter instruction stream of DESIGN 5.1d -- the
// quadratic's root without a Newton step (the `first` spline everywhere, the conditioned one in shift-free waves),
// one logarithm per layer, one tail test per layer.  The loss kernel keeps its arithmetic.
// FTAB (LEAN only): the `first` spline from its certified inverse table `ft` (cnf_first_table.h) instead of the closed
// form: (out, ld) by lookup, ld added to the sum directly, and the layer's logarithm takes the conditioned spline's
// argument alone.  The caller chooses between the two instantiations with one wave-uniform branch.
template <int K, bool TO_BASE, bool FAST, bool PRECISE = false, bool SHIFT_FREE_OK = false, int LROWS = PWL_LROWS, int LFIX = 0,
          bool LEAN_OK = false, bool FTAB = false>
__device__ __forceinline__ v2f flow2_tables(const float* tab, const float* tbl, const float* __restrict__ gtbl,
                                            int L, const SplineConsts sc, v2f& u0, v2f& u1,
                                            const PreciseConsts* pc = nullptr, const double* e2tab = nullptr,
                                            const double* tabd = nullptr, BaseAcc<v2f>* bacc = nullptr,
                                            const FtConsts ft = FtConsts{}) {
  constexpr bool INV = !TO_BASE;
  constexpr bool LEAN = LEAN_OK && INV && FAST;
  static_assert(!FTAB || LEAN, "the inverse table: the lean sampling direction");
  static_assert(!PRECISE || TO_BASE, "precise path: data -> base");
  v2f acc = splat<v2f>(0.0f);
  [[maybe_unused]] v2f lo0 = splat<v2f>(0.0f), lo1 = lo0;      // precise path: what rounding u0 / u1 to fp32 dropped
  if (LFIX) L = LFIX;
#pragma unroll
  for (int step = 0; step < (LFIX ? LFIX : L); ++step) {
    const int l = TO_BASE ? L - 1 - step : step;
    const bool odd = l & 1;                     // flows.py:141-143 perms
    const v2f uf = odd ? u1 : u0, uo = odd ? u0 : u1;
    v2f of, oo, ld, olo_f, olo_o;
    bool general;
    const float* tl = tbl + l * pwl_ltbl(LROWS);
    const float* gl = gtbl + (int64_t)l * PWL_TBL;
    if constexpr (PRECISE) {
      table_spline_precise<K, FAST>(tab, tabd, uf, odd ? lo1 : lo0, sc, of, ld, olo_f);
      if (step == L - 1) bacc->add(of, olo_f);
      acc += ld;
      v2f th[PWL_P];
      pwl_eval<LROWS>(tl, gl, of, th, general);
      cond_spline_precise<K, FAST, true>(th, uo, odd ? lo0 : lo1, sc, *pc, e2tab, oo, ld, olo_o);
      if (step == L - 1) bacc->add(oo, olo_o);
      lo0 = odd ? olo_o : olo_f;
      lo1 = odd ? olo_f : olo_o;
    } else {
      // base -> data: the conditioner sees the layer's INPUT, so its table search and row reads (a chain of three
      // dependent LDS round trips) are issued first and complete under the arithmetic of the `first` spline
      PwlRows rr;
      v2f qa[K], qb[K];
      // (the inverse table's lookup goes first: its two LDS round trips and ten packed FMAs leave little for the
      // conditioner's reads to hide under, and a row of each in flight at once costs registers the kernel does not have)
      if constexpr (FTAB) ft_eval(ft, uf, of, ld);
      if (!TO_BASE) {
        pwl_find<LROWS>(tl, uf, rr, general);
        rr.dua = pwl_logit_pairs<LROWS>(rr.ra, gl, rr.pa, uf.x, qa);
        rr.dub = pwl_logit_pairs<LROWS>(rr.rb, gl, rr.pb, uf.y, qb);
      }
      // One logarithm per layer where every lane takes the shift-free form: both splines return the argument of
      // their log|f'| (the derivative itself) and the product goes through one v_log_f32.  The conditioned
      // factor is bounded there (slope logits in [-3, 40]: knot slopes d in [0.049, 40]; bins >= 1e-4 of a range of
      // 20: s in [5e-6, 2e5]).  With t = z (1 - z) <= 1/4, f' = s^2 num2 / den^2 has num2 >= min(d0, d1) / 2 and
      // s / 2 <= den <= max(s, (d0 + d1 + 2 s) / 4), hence 2 s^2 d_lo / (d_hi + s)^2 ~ 1.5e-15 <= f' <= 4 max(d, s)
      // ~ 8e5.  The product of the two factors of a layer stays a normal fp32 number for a `first` spline with
      // derivatives within 1e-22 .. 1e32.
      constexpr bool LOGPROD = LEAN;
      // Both splines read the layer's inputs (uf, uo): one wave-level test guards both linear-tail fix-ups.
      bool tails = true;
      if constexpr (LEAN) tails = __builtin_amdgcn_ballot_w64(maybe_outside(uf, uo, sc.lo, sc.hi)) != 0;
      v2f larg = splat<v2f>(1.0f);
      if constexpr (FTAB) {
        if (tails) table_spline_tails<K, INV, false, v2f>(tab, uf, sc, of, ld);
        acc += ld;
      } else if constexpr (LOGPROD) {
        table_spline<K, INV, FAST, v2f, true, LEAN>(tab, uf, sc, of, larg, tails);
      } else {
        table_spline<K, INV, FAST, v2f, false, LEAN>(tab, uf, sc, of, ld, tails);
        acc += ld;
      }
      if (TO_BASE) {
        pwl_find<LROWS>(tl, of, rr, general);
        rr.dua = pwl_logit_pairs<LROWS>(rr.ra, gl, rr.pa, of.x, qa);
        rr.dub = pwl_logit_pairs<LROWS>(rr.rb, gl, rr.pb, of.y, qb);
      }
      auto slopes = [&](int ka, int kb, v2f& ta, v2f& tb) {
        ta = pwl_slope_pair<LROWS>(rr.ra, gl, rr.pa, ka, rr.dua);
        tb = pwl_slope_pair<LROWS>(rr.rb, gl, rr.pb, kb, rr.dub);
      };
      if (!SHIFT_FREE_OK || __builtin_amdgcn_ballot_w64(general) != 0)      // wave-uniform: a lane's cell is marked
      {       // marked cells (ill-conditioned pieces, far-out inputs): the general form, and its own logarithm
        cond_spline_rows<K, INV, FAST, false, false, LEAN>(qa, qb, slopes, uo, sc, oo, ld, tails);
        if constexpr (LOGPROD && !FTAB) { const v2f lg = Math<FAST>::log(larg); ld += INV ? -lg : lg; }
      } else {
        cond_spline_rows<K, INV, FAST, true, LOGPROD, LEAN>(qa, qb, slopes, uo, sc, oo, ld, tails);
        if constexpr (LOGPROD) { const v2f lg = Math<FAST>::log(FTAB ? ld : larg * ld); ld = INV ? -lg : lg; }
      }
    }
    acc += ld;
    u0 = odd ? oo : of;
    u1 = odd ? of : oo;
  }
  return acc;
}

}  // namespace cnf
