// cnf_grad.hip -- the MLP backward of the fused Monte-Carlo loss terms and of single flow passes: the MI355X
// replacement of `jax.value_and_grad(loss_fn)` in cnf_ot/mfc/solvers.py:90-97.  (The table backward
// at dim 2: cnf_grad_pwl.hip.  `optax.adam` and the terms' residual kernels: cnf_step.hip.)
//
// One launch = one loss term over (time-slice, sample tile), like loss_kernel,
// but it also back-propagates the term through every flow pass it made:
//   * each pass is re-run with its layer inputs stashed in LDS (recompute
//     instead of storing activations), then differentiated layer by layer in
//     reverse: spline partials (cnf_backward.h) -> conditioner backward;
//   * data backprop through the 16x16 layers uses scalar (SGPR) weights;
//   * weight gradients are batch GEMMs on the matrix cores
//     (v_mfma_f32_16x16x4_f32), accumulated straight into a per-wave gradient
//     slab in global memory (plain read-modify-write: a slab has one owner, so
//     the result is deterministic); grad_finish_kernel sums the slabs.
// Built for the reference's network only: hidden 16, 2 hidden layers, 5 bins.
#include "cnf_backward.h"
#include "cnf_host.h"

#include <math.h>

namespace cnf {

// One sample per lane; a tile = one workgroup's samples = blockDim.x (64, 128 or 256: the host picks the size that
// puts the most waves on a CU -- a tile's LDS working set is (L + 3 .. L + 9) x D floats per sample plus 8.7 KB of
// MFMA staging per wave, and at 1 wave per SIMD a wave issues at half rate with every latency exposed).
#define GTS ((int)blockDim.x)
constexpr int GTS_MAX = TILE;
// LDS geometry of a tile.  Every [D][samples] buffer (noise, stashes, adjoints ...) has rows of GROW = GTS + 4 floats:
// a wave's 64 samples of one input dimension are contiguous, and rows read 16 bytes per lane along the samples (the
// A operand of the first layer's weight-gradient GEMM, cnf_backward.h) fall into different banks.  In front of them:
// the `first` spline's table, 64 ones (the bias row of the first layer's MFMA operands) and the tile's condition column.
#define GROW (GTS + 4)
constexpr int HDRG = hdr_floats(GK);
constexpr int ONES_OFF = HDRG, C_OFF = HDRG + 64;
#define PRE_FLOATS (HDRG + 64 + GROW)

__device__ __forceinline__ void tile_consts(float* lds) {
  for (int i = threadIdx.x; i < 64; i += GTS) lds[ONES_OFF + i] = 1.0f;
}

// One launch evaluates up to GRAD_MAX_JOBS loss terms ("jobs": the terms of one composite loss, each with its own
// points, slices and coefficient): their tiles share the grid, so small terms run side by side instead of one
// under-filled launch after the other (a default-config training step is three launches of 8 tiles each).
constexpr int GRAD_MAX_JOBS = 4;
struct GradJob {
  CnfLossSpec spec;
  const float* pts;
  const float* t;
  double* sums;          // [n_slices] loss-term sums (value of value_and_grad)
  int64_t B, n_slices, pts_slice_stride;
  int64_t first_tile;    // of this job, in the launch's tile numbering
  float scale;           // d(total loss) / d(this term's sum)
};
struct GradArgs {
  ModelArgs m;
  GradJob job[GRAD_MAX_JOBS];
  int32_t n_jobs;
  float* slabs;          // [gridDim.x * 4][n_params]
  int64_t n_params;
  int64_t n_tiles;       // of all jobs
  uint32_t div_magic;
};

// A wave zeroes its own gradient slab before its first tile (the host used to clear all slabs with one memset
// per term: a 10 MB fill kernel and its launch in front of every backward launch).  Same wave, same addresses
// later: the read-modify-writes that follow are ordered behind these stores.
__device__ __forceinline__ void slab_clear(float* gslab, int64_t n_params, int lane) {
  for (int64_t j = lane; j < n_params; j += 64) gslab[j] = 0.0f;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
}

struct FirstAcc { float Wb[GK], Hb[GK], Db[GK + 1]; };

__device__ __forceinline__ void tile_load1(const float* __restrict__ g, float* U, int D, uint32_t magic,
                                           int64_t tile_start, int64_t B) {
  const int64_t base = tile_start * D;
  const int n_el = (int)(B - tile_start < GTS ? B - tile_start : GTS) * D;
  for (int e = threadIdx.x; e < GTS * D; e += GTS) {
    const int s = magic ? (int)__umulhi((uint32_t)e, magic) : e, d = e - s * D;
    U[d * GROW + s] = e < n_el ? g[base + e] : 0.0f;
  }
}

// Offsets inside a flow layer's conditioners in 32-bit closed form (H = 16, M = 2, P = 16): conditioner d has
// cond_floats(d) = 16 d + 576 flat weights and cond_floats_mfma(d, 2) = 256 (d + 6) MFMA-layout floats (64-bit loops
// over d here cost ~130 scalar instructions per layer and a dozen scalar registers spilled to vector lanes)
__device__ __forceinline__ int cond_size(int d) { return 16 * d + 576; }
__device__ __forceinline__ int cond_size_q(int d) { return 256 * (d + 6); }
__device__ __forceinline__ int cond_prefix(int d) { return (d - 1) * (8 * d + 576); }          // conditioners 1 .. d-1
__device__ __forceinline__ int cond_prefix_q(int d) { return (d - 1) * (128 * d + 1536); }
static_assert(cond_floats(3, 16, 2, 16) == 16 * 3 + 576 && cond_floats_mfma(3, 2) == 256 * (3 + 6), "conditioner sizes");

// forward of one pass with every layer input kept: St[s] is the input of step s
// (St[0] filled by the caller), St[L] the result.  Returns the log-det sum.
// The direction is a RUNTIME (wave-uniform) flag and every pass of the kernel
// goes through the single call site of this function and of pass_bwd: the
// conditioner code (the bulk) exists once, so the kernel fits the instruction
// cache (the first version inlined 10 forward + 6 backward copies: 34 k
// instructions, 4x the cache).
template <bool FAST, int DFIX = 0>
__device__ __forceinline__ float pass_fwd_stash(const ModelArgs& a, float* lds, float* St, float c, bool to_base) {
  const int D = DFIX ? DFIX : a.D;
  const float* tab = lds;
  const int wbase = threadIdx.x & ~63;
  lds[C_OFF + threadIdx.x] = c;
  uniform_ptr weights = as_uniform(a.prep + hdr_floats(GK));
  float acc = 0.0f;
  for (int s = 0; s < a.L; ++s) {
    const int l = to_base ? a.L - 1 - s : s;
    const bool odd = l & 1;
    const int first_idx = odd ? D - 1 : 0, idx_step = odd ? -1 : 1;
    const float* cu = St + s * D * GROW + threadIdx.x;
    float* co = St + (s + 1) * D * GROW + threadIdx.x;
    uniform_ptr w = weights + l * (int)a.per_layer;
    [[maybe_unused]] const float* wflat = a.prep + hdr_floats(GK) + l * (int)a.per_layer;
    [[maybe_unused]] const float* wq = a.wq + l * (int)a.per_layer_q;
    [[maybe_unused]] int qo = 0;       // this conditioner's offset in the layer's MFMA-layout weights
    [[maybe_unused]] CondW cw;         // the NEXT conditioner's weights: one conditioner ahead (cnf_backward.h)
    if constexpr (FAST) { if (D > 1) cw = cond_weights(wq, 0, wflat, 1); __builtin_amdgcn_sched_barrier(0); }
    float o, ld;
    if (to_base) table_spline<GK, false, FAST, float>(tab, cu[first_idx * GROW], a.sc, o, ld);
    else table_spline<GK, true, FAST, float>(tab, cu[first_idx * GROW], a.sc, o, ld);
    co[first_idx * GROW] = o;
    acc += ld;
    for (int d = 1; d < D; ++d) {
      const int i = first_idx + d * idx_step;
      float th[GP];
      if constexpr (FAST) {        // matrix cores (cnf_backward.h); `wq` walks the MFMA-layout weights
        const CondGeom G{(int)((to_base ? co : cu) - lds) - (int)threadIdx.x + wbase, C_OFF + wbase, ONES_OFF, first_idx,
                         idx_step, GROW, d};
        const CondW cur = cw;
        qo += cond_size_q(d);
        wflat += cond_size(d);
        if (d + 1 < D) cw = cond_weights(wq, qo, wflat, d + 1);
        __builtin_amdgcn_sched_barrier(0);
        float h1m[4][4], h2m[4][4];
        cond_fwd_mfma(lds, G, wq, cur, h1m, h2m, th);
      } else {
        conditioner<16, GP, float>(w, d, 2, c, to_base ? co : cu, first_idx, idx_step, GROW, th);
        w += cond_size(d);
      }
      if (to_base) cond_spline<GK, false, FAST, float>(th, cu[i * GROW], a.sc, o, ld);
      else cond_spline<GK, true, FAST, float>(th, cu[i * GROW], a.sc, o, ld);
      co[i * GROW] = o;
      acc += ld;
    }
  }
  return acc;
}

// backward of the pass whose stash is in St.  Aa holds the adjoint of the final
// output on entry; the function ping-pongs between Aa and Ab and returns the
// buffer that holds the adjoint of the pass input.
// fa_lds (optional): the `first` spline's per-bin adjoint sums live in 16 LDS rows instead of `fa` -- sixteen registers
// that are then free during the conditioner loop (the generic-dimension loss kernel has none to spare)
// AHEAD: the recomputation weights of the next conditioner are fetched during the current one's backward (twelve
// registers held across it; the generic-dimension loss kernel, whose tile state is larger, fetches them at use)
template <bool FAST, bool WGRAD = true, int DFIX = 0, bool AHEAD = true>
__device__ __forceinline__ float* pass_bwd(const ModelArgs& a, float* lds, const float* St, float* Aa,
                                           float* Ab, float ld_bar, float c, bool to_base, float* gslab,
                                           float* stage, FirstAcc& fa, float* fa_lds = nullptr) {
  const int D = DFIX ? DFIX : a.D;
  const float* tab = lds;
  const int wbase = threadIdx.x & ~63;
  lds[C_OFF + threadIdx.x] = c;
  uniform_ptr weights = as_uniform(a.prep + hdr_floats(GK));
  float* Aout = Aa;
  float* Ain = Ab;
  for (int s = a.L - 1; s >= 0; --s) {
    const int l = to_base ? a.L - 1 - s : s;
    const bool odd = l & 1;
    const int first_idx = odd ? D - 1 : 0, idx_step = odd ? -1 : 1;
    const float* cu = St + s * D * GROW + threadIdx.x;
    const float* co = St + (s + 1) * D * GROW + threadIdx.x;
    float* ao = Aout + threadIdx.x;
    float* au = Ain + threadIdx.x;
    for (int d = 0; d < D; ++d) au[d * GROW] = 0.0f;
    const int lay = l * (int)a.per_layer, layq = l * (int)a.per_layer_q;
    int off = cond_prefix(D);                          // end of this layer's conditioners
    [[maybe_unused]] int offq = cond_prefix_q(D);      // the same in the MFMA-layout weights
    [[maybe_unused]] CondW cw;                         // the NEXT conditioner's recomputation weights, one conditioner ahead
    if constexpr (FAST && AHEAD) {
      if (D > 1) {
        cw = cond_weights(a.wq + layq, offq - cond_size_q(D - 1), a.prep + hdr_floats(GK) + lay + off - cond_size(D - 1), D - 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    for (int d = D - 1; d >= 1; --d) {
      off -= cond_size(d);
      const int i = first_idx + d * idx_step;
      float* gw = WGRAD ? gslab + GP + lay + off : nullptr;
      WgradPre pre;
      float th[GP], tb[GP];
      if constexpr (FAST) {      // recompute, data backprop and weight gradients on the matrix cores (cnf_backward.h)
        offq -= cond_size_q(d);
        const float* wflat = a.prep + hdr_floats(GK) + lay + off;
        const CondGeom G{(int)((to_base ? co : cu) - lds) - (int)threadIdx.x + wbase, C_OFF + wbase, ONES_OFF, first_idx,
                         idx_step, GROW, d};
        float h1m[4][4], h2m[4][4];
        if constexpr (!AHEAD) cw = cond_weights(a.wq + layq, offq, wflat, d);
        cond_fwd_mfma(lds, G, a.wq + layq, cw, h1m, h2m, th);
        // fetched here, the spline backward ahead of their first use: the first data-backprop operand and the first
        // accumulator tile of the weight gradient (the others at the start of cond_bwd_mfma)
        const int o_wo = (1 + d) * 16 + 16 + 256 + 16;
        const f4 Ao = cond_weight_T(wflat + o_wo);
        WgradAcc pre_o;
        if constexpr (WGRAD) pre_o = wgrad_fetch(gw + o_wo, 16, gw + o_wo + 256);
        __builtin_amdgcn_sched_barrier(0);
        float vb;
        if (to_base) vb = cond_spline_bwd<GK, false, FAST>(th, cu[i * GROW], co[i * GROW], ao[i * GROW], ld_bar, a.sc, tb);
        // (base -> data: the output is formed again inside, in the bin the backward selects -- next to a knot the stashed
        // one can lie a rounding outside that bin, and 1 / f' of a clipped position is garbage: soak_vjp_case_1_16.log)
        else vb = cond_spline_bwd<GK, true, FAST>(th, cu[i * GROW], co[i * GROW], ao[i * GROW], ld_bar, a.sc, tb, nullptr, nullptr,
                                                  nullptr, true);
        au[i * GROW] += vb;
        // the next conditioner's recomputation weights: covered by this one's backward
        if constexpr (AHEAD) { if (d > 1) cw = cond_weights(a.wq + layq, offq - cond_size_q(d - 1), wflat - cond_size(d - 1), d - 1); }
        cond_bwd_mfma<WGRAD>(lds, G, (int)((to_base ? Aout : Ain) - lds) + wbase, wflat, Ao, h1m, h2m, tb, gw, stage, pre_o);
      } else {
        uniform_ptr w = weights + lay + off;
        if constexpr (WGRAD) pre = wgrad_prefetch(gw, d);
        float h1[16], h2[16];
        conditioner_keep(w, d, c, to_base ? co : cu, first_idx, idx_step, GROW, h1, h2, th);
        float vb;
        if (to_base) vb = cond_spline_bwd<GK, false, FAST>(th, cu[i * GROW], co[i * GROW], ao[i * GROW], ld_bar, a.sc, tb);
        else vb = cond_spline_bwd<GK, true, FAST>(th, cu[i * GROW], co[i * GROW], ao[i * GROW], ld_bar, a.sc, tb, nullptr, nullptr,
                                                  nullptr, true);
        au[i * GROW] += vb;
        conditioner_bwd<WGRAD>(w, d, c, to_base ? co : cu, first_idx, idx_step, GROW, h1, h2, tb, to_base ? ao : au,
                               gw, stage, pre);
      }
    }
    float vb0;
    if (fa_lds) {
      FirstAcc t0;
#pragma unroll
      for (int j = 0; j < GK; ++j) { t0.Wb[j] = 0.0f; t0.Hb[j] = 0.0f; }
#pragma unroll
      for (int j = 0; j <= GK; ++j) t0.Db[j] = 0.0f;
      if (to_base) vb0 = table_spline_bwd<GK, false, FAST>(tab, cu[first_idx * GROW], co[first_idx * GROW], ao[first_idx * GROW],
                                                           ld_bar, a.sc, t0.Wb, t0.Hb, t0.Db);
      else vb0 = table_spline_bwd<GK, true, FAST>(tab, cu[first_idx * GROW], co[first_idx * GROW], ao[first_idx * GROW],
                                                  ld_bar, a.sc, t0.Wb, t0.Hb, t0.Db);
      float* f = fa_lds + threadIdx.x;
#pragma unroll
      for (int j = 0; j < GK; ++j) { f[j * GROW] += t0.Wb[j]; f[(GK + j) * GROW] += t0.Hb[j]; }
#pragma unroll
      for (int j = 0; j <= GK; ++j) f[(2 * GK + j) * GROW] += t0.Db[j];
    } else if (to_base) {
      vb0 = table_spline_bwd<GK, false, FAST>(tab, cu[first_idx * GROW], co[first_idx * GROW], ao[first_idx * GROW],
                                              ld_bar, a.sc, fa.Wb, fa.Hb, fa.Db);
    } else {
      vb0 = table_spline_bwd<GK, true, FAST>(tab, cu[first_idx * GROW], co[first_idx * GROW], ao[first_idx * GROW],
                                             ld_bar, a.sc, fa.Wb, fa.Hb, fa.Db);
    }
    au[first_idx * GROW] += vb0;
    float* t = Aout; Aout = Ain; Ain = t;
  }
  return Aout;
}

// Roles of the steps of a tile's pass program.  Every step is: build the pass
// input, run the forward with stash, act on its result, optionally seed and run
// the backward, act on the input adjoint.
enum Role {
  R_NEG,          // -log_prob of the points (data -> base)
  R_POT, R_RKL,   // potential / reverse KL (base -> data)
  R_R1, R_R2,     // finite-difference velocity: r1 kept, then velocity formed
  R_R3,           // sample at t for the score terms
  R_LPP, R_LPM,   // log_prob at r3 +- dx/2 e_d (forward only / forward + backward of the minus pass)
  R_LPPB,         // the plus pass again, with backward
  R_R3B, R_R2B, R_R1B   // backward of r3 / r2 / r1 (forward recomputed)
};

// DFIX > 0: the event dimension as a compile-time constant (dim 2: the reference's main configurations)
template <bool FAST, int DFIX = 0>
__global__ __launch_bounds__(GTS_MAX, 2) void grad_kernel(const GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int HDR = hdr_floats(GK);
  const int D = DFIX ? DFIX : a.m.D, L = a.m.L;
  const int DT = D * GROW;
  float* Nn = lds + PRE_FLOATS;
  float* St = Nn + DT;                  // (L+1) stashes
  float* Aa = St + (L + 1) * DT;
  float* Ab = Aa + DT;
  float* V = Ab + DT;
  float* R3 = V + DT;
  float* R3b = R3 + DT;
  float* Ub = R3b + DT;
  float* stage = Ub + DT + (threadIdx.x >> 6) * STAGE_FLOATS;
  // generic dimension: the `first` spline's 16 accumulators per lane in LDS (pass_bwd), not in registers
  float* fa_lds = DFIX ? nullptr : Ub + DT + (GTS >> 6) * STAGE_FLOATS;
  for (int i = threadIdx.x; i < HDR; i += GTS) lds[i] = a.m.prep[i];
  tile_consts(lds);
  if (!DFIX) { for (int j = 0; j < GP; ++j) fa_lds[j * GROW + threadIdx.x] = 0.0f; }
  const int tid = threadIdx.x;
  // (wave-uniform: a scalar register pair, not two vector registers)
  float* gslab = a.slabs + (int64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (GTS >> 6) + (tid >> 6))) * a.n_params;
  slab_clear(gslab, a.n_params, tid & 63);
  FirstAcc fa;
#pragma unroll
  for (int j = 0; j < GK; ++j) { fa.Wb[j] = 0.0f; fa.Hb[j] = 0.0f; }
#pragma unroll
  for (int j = 0; j <= GK; ++j) fa.Db[j] = 0.0f;

  SliceSum ssum;
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    int jb = 0;
#pragma unroll
    for (int q = 1; q < GRAD_MAX_JOBS; ++q) jb += (q < a.n_jobs && tile >= a.job[q].first_tile) ? 1 : 0;
    const GradJob& J = a.job[jb];
    const int kind = J.spec.kind;
    const float dt = J.spec.dt, dx = J.spec.dx, coef = J.spec.coef;
    const bool score = kind == CNF_TERM_KINETIC_SCORE || kind == CNF_TERM_FLOW_MATCHING;
    // number of steps of the pass program
    const int n_steps = kind == CNF_TERM_KINETIC ? 3 : (score ? 3 + 3 * D + 3 : 1);
    const int64_t tiles_per_slice = (J.B + GTS - 1) / GTS;
    const int64_t lt = tile - J.first_tile;
    const int64_t slice = lt / tiles_per_slice;
    const int64_t tile_start = (lt - slice * tiles_per_slice) * GTS;
    const bool valid = tile_start + tid < J.B;
    const float sc = valid ? J.scale : 0.0f;
    __syncthreads();
    tile_load1(J.pts + slice * J.pts_slice_stride * D, Nn, D, a.div_magic, tile_start, J.B);
    const float t = J.t[slice];
    __syncthreads();
    float* n_ = Nn + tid;
    float* s0 = St + tid;               // stash 0 column
    float* sL = St + L * DT + tid;      // final output column
    float* aa = Aa + tid;
    float* v_ = V + tid;
    float* r3 = R3 + tid;
    float* r3b = R3b + tid;
    float* ub = Ub + tid;
    const auto out = lds_col<float>(sL, GROW);      // the pass's output point
    float lossv = 0.0f, lp_plus = 0.0f, ubar = 0.0f;

    for (int st = 0; st < n_steps; ++st) {
      // ---- decode the step
      int role, dd = 0;
      if (kind == CNF_TERM_NEG_LOGPROB) role = R_NEG;
      else if (kind == CNF_TERM_POTENTIAL) role = R_POT;
      else if (kind == CNF_TERM_REVERSE_KL) role = R_RKL;
      else if (kind == CNF_TERM_KINETIC) role = st == 0 ? R_R1 : (st == 1 ? R_R2 : R_R1B);
      else {
        if (st < 3) role = st == 0 ? R_R1 : (st == 1 ? R_R2 : R_R3);
        else if (st < 3 + 3 * D) { dd = (st - 3) / 3; const int q = (st - 3) - 3 * dd; role = q == 0 ? R_LPP : (q == 1 ? R_LPM : R_LPPB); }
        else { const int q = st - (3 + 3 * D); role = q == 0 ? R_R3B : (q == 1 ? R_R2B : R_R1B); }
      }
      const bool to_base = role == R_NEG || role == R_LPP || role == R_LPM || role == R_LPPB;
      const float c = (role == R_R1 || role == R_R1B) ? t - 0.5f * dt
                    : ((role == R_R2 || role == R_R2B) ? t + 0.5f * dt : t);
      // ---- pass input
      if (role == R_LPP || role == R_LPM || role == R_LPPB) {
        for (int e = 0; e < D; ++e) s0[e * GROW] = r3[e * GROW];
        s0[dd * GROW] += role == R_LPM ? -0.5f * dx : 0.5f * dx;
      } else {
        for (int e = 0; e < D; ++e) s0[e * GROW] = n_[e * GROW];
      }
      const float ldsum = pass_fwd_stash<FAST, DFIX>(a.m, lds, St, c, to_base);
      // ---- act on the result, prepare the seeds
      bool do_bwd = false;
      float ld_bar = 0.0f;
      switch (role) {
        case R_NEG: {
          lossv = -(base_logprob<float>(out, D) + ldsum);
          for (int e = 0; e < D; ++e) aa[e * GROW] = sc * sL[e * GROW];      // d(-lp)/dx_e = x_e
          ld_bar = -sc; do_bwd = true;
          break;
        }
        case R_POT: {
          const Potential<float> p = potential<false, float>(out, D, J.spec.subtype, J.spec.a);
          lossv = p.v;
          for (int e = 0; e < D; ++e) aa[e * GROW] = sc * p.grad(sL[e * GROW]);
          do_bwd = true;
          break;
        }
        case R_RKL: {
          const RklMix<float> mix = rkl_mixture<false, float>(out, D, t, J.spec.T, J.spec.beta);
          lossv = base_logprob<float>(lds_col<float>(n_, GROW), D) - ldsum - mix.logmix;
          for (int e = 0; e < D; ++e) aa[e * GROW] = sc * mix.g * sL[e * GROW];
          ld_bar = -sc; do_bwd = true;
          break;
        }
        case R_R1:
          for (int e = 0; e < D; ++e) v_[e * GROW] = sL[e * GROW];
          break;
        case R_R2: {
          const float inv_dt = 1.0f / dt;
          for (int e = 0; e < D; ++e) v_[e * GROW] = (sL[e * GROW] - v_[e * GROW]) * inv_dt;      // velocity
          if (kind == CNF_TERM_KINETIC) {
            for (int e = 0; e < D; ++e) {
              const float v = v_[e * GROW];
              lossv = fmaf(v, v, lossv);
              ub[e * GROW] = 2.0f * sc * v;
              aa[e * GROW] = ub[e * GROW] * inv_dt;
            }
            do_bwd = true;                          // the r2 stash is live
          }
          break;
        }
        case R_R3:
          for (int e = 0; e < D; ++e) { r3[e * GROW] = sL[e * GROW]; r3b[e * GROW] = 0.0f; }
          break;
        case R_LPP:
          lp_plus = base_logprob<float>(out, D) + ldsum;
          break;
        case R_LPM: {
          const float lp_minus = base_logprob<float>(out, D) + ldsum;
          const float dr = drift_field<float>(lds_col<float>(r3, GROW), dd, kind == CNF_TERM_FLOW_MATCHING ? J.spec.subtype : -1, J.spec.a);
          const float u = score_residual(v_[dd * GROW], (lp_plus - lp_minus) / dx, coef, dr);
          lossv = fmaf(u, u, lossv);
          ubar = score_residual_bar(u, sc);
          ub[dd * GROW] = ubar;
          ld_bar = -ubar * coef / dx;                // d u / d lp_minus
          for (int e = 0; e < D; ++e) aa[e * GROW] = -ld_bar * sL[e * GROW];     // d base / d x_e = -x_e
          do_bwd = true;
          break;
        }
        case R_LPPB:
          ld_bar = ubar * coef / dx;
          for (int e = 0; e < D; ++e) aa[e * GROW] = -ld_bar * sL[e * GROW];
          do_bwd = true;
          break;
        case R_R3B:
          if (kind == CNF_TERM_FLOW_MATCHING)
            drift_adjoint(lds_col<float>(r3, GROW), lds_col<float>(ub, GROW), D, J.spec.subtype, J.spec.a,
                          [&](int e, float b) { r3b[e * GROW] += b; });
          for (int e = 0; e < D; ++e) aa[e * GROW] = r3b[e * GROW];
          do_bwd = true;
          break;
        case R_R2B:
          for (int e = 0; e < D; ++e) aa[e * GROW] = ub[e * GROW] / dt;
          do_bwd = true;
          break;
        default:   // R_R1B
          for (int e = 0; e < D; ++e) aa[e * GROW] = -ub[e * GROW] / dt;
          do_bwd = true;
          break;
      }
      if (do_bwd) {
        const float* ain = pass_bwd<FAST, true, DFIX, DFIX != 0>(a.m, lds, St, Aa, Ab, ld_bar, c, to_base, gslab, stage, fa, fa_lds) + tid;
        if (role == R_LPM || role == R_LPPB)
          for (int e = 0; e < D; ++e) r3b[e * GROW] += ain[e * GROW];
      }
    }
    float part = valid ? lossv : 0.0f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    ssum.add(J.sums, slice, part);
  }
  ssum.flush();
  // per-bin adjoint sums of the shared `first` spline: wave reduce, one owner write
  float red[GP];
  if (!DFIX) {
#pragma unroll
    for (int j = 0; j < GP; ++j) red[j] = fa_lds[j * GROW + tid];
  } else {
#pragma unroll
    for (int j = 0; j < GK; ++j) { red[j] = fa.Wb[j]; red[GK + j] = fa.Hb[j]; }
#pragma unroll
    for (int j = 0; j <= GK; ++j) red[2 * GK + j] = fa.Db[j];
  }
#pragma unroll
  for (int j = 0; j < GP; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) red[j] += __shfl_xor(red[j], off, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < GP; ++j) gslab[j] += red[j];
  }
}

// ---------------------------------------------------------------------------
// vjp_kernel: vector-Jacobian product of ONE flow pass with respect to its
// input points -- the building block of the reference's autodiff helpers
// forward_jac / inverse_jac / gauge_potential (flows.py:203-211):
//   xbar[b,:] = ybar[b,:] . dF/dx(b)  +  ldbar[b] * d logdet/dx(b)
// Same forward-with-stash + backward as grad_kernel, without weight gradients.
// ---------------------------------------------------------------------------
struct VjpArgs {
  ModelArgs m;
  const float* pts;      // [B, D]
  const float* c;
  const float* ybar;     // [B, D] or null (= 0)
  const float* ldbar;    // [B] or null (= 0)
  float* xbar;           // [B, D] or null
  float* slabs;          // WGRAD: per-wave gradient slabs
  int64_t n_params;
  int64_t B, c_block;
  int32_t to_base;
  uint32_t div_magic;
  // finite-difference mode (cnf_logprob_fd_vjp): pts holds B / fd2 base points r_i; the pass differentiated is
  // log_prob at the evaluation point j = i * fd2 + 2 d + s (r_i -+ fd_h e_d) with seed +-gbar[i, d] * fd_inv_dx;
  // xbar[i, :] receives the SUM of the adjoints of r_i's fd2 evaluation points.  fd2 = 0: off.
  int32_t fd2;
  float fd_h, fd_inv_dx;
  const float* gbar;     // [B / fd2, D]
  // fused score term (cnf_score_fd_vjp): r1 != null.  pts = r3 (the samples at t), r1 / r2 the samples at t -+ dt/2; the
  // kernel forms the score from ITS forward passes, the residual u = (r2 - r1)/dt + coef score - drift(r3), the per-slice
  // sums of u^2 (sums), the adjoints of r1 / r2 (rbar1 / rbar2; xbar = the adjoint of r3) and seeds its own backward:
  // no gbar, and no separate forward launch over the 2 D evaluation points
  const float* r1; const float* r2;
  float* rbar1; float* rbar2;
  double* sums;
  float inv_dt, coef, drift_a, loss_coef;
  int32_t drift;         // CnfDrift or -1
};

// WGRAD=true additionally accumulates the parameter gradient of the pass (the
// backward of a differentiable flow op: cnf_pass_vjp).
template <bool FAST, bool WGRAD, int DFIX = 0>
__global__ __launch_bounds__(GTS_MAX, 2) void vjp_kernel(const VjpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int HDR = hdr_floats(GK);
  const int D = DFIX ? DFIX : a.m.D, L = a.m.L, DT = D * GROW;
  float* St = lds + PRE_FLOATS;
  float* Aa = St + (L + 1) * DT;
  float* Ab = Aa + DT;
  float* stage = Ab + DT + (threadIdx.x >> 6) * STAGE_FLOATS;       // (WGRAD = false: nothing is staged)
  float* gslab = WGRAD ? a.slabs + (int64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (GTS >> 6) + (threadIdx.x >> 6))) * a.n_params : nullptr;
  if (WGRAD) slab_clear(gslab, a.n_params, threadIdx.x & 63);
  for (int i = threadIdx.x; i < HDR; i += GTS) lds[i] = a.m.prep[i];
  tile_consts(lds);
  const int tid = threadIdx.x;
  FirstAcc fa;      // WGRAD=false: written, never read: removed by the compiler
#pragma unroll
  for (int j = 0; j < GK; ++j) { fa.Wb[j] = 0.0f; fa.Hb[j] = 0.0f; }
#pragma unroll
  for (int j = 0; j <= GK; ++j) fa.Db[j] = 0.0f;
  // finite-difference mode: a tile holds whole groups of fd2 evaluation points (tp <= GTS of them)
  const int tp = a.fd2 ? (GTS / a.fd2) * a.fd2 : GTS;
  const int64_t n_tiles = (a.B + tp - 1) / tp;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t tile_start = tile * tp;
    const int64_t i = tile_start + tid;
    __syncthreads();
    float c, ld_bar;
    if (a.fd2) {
      const bool valid = tid < tp && i < a.B;
      const int64_t ib = valid ? i / a.fd2 : 0;
      const int k = (int)(i - ib * a.fd2), dd = k >> 1;
      for (int e = 0; e < D; ++e) {
        float v = valid ? a.pts[ib * D + e] : 0.0f;
        if (e == dd) v += (k & 1) ? -a.fd_h : a.fd_h;
        St[e * GROW + tid] = v;
        Aa[e * GROW + tid] = 0.0f;
      }
      const int64_t n_base = a.B / a.fd2;
      c = valid ? a.c[a.c_block >= n_base ? 0 : ib / a.c_block] : 0.0f;
      ld_bar = (valid && a.gbar) ? ((k & 1) ? -a.gbar[ib * D + dd] : a.gbar[ib * D + dd]) * a.fd_inv_dx : 0.0f;
    } else {
      tile_load1(a.pts, St, D, a.div_magic, tile_start, a.B);
      if (a.ybar) tile_load1(a.ybar, Aa, D, a.div_magic, tile_start, a.B);
      else for (int e = tid; e < DT; e += GTS) Aa[e] = 0.0f;
      c = i < a.B ? a.c[a.c_block >= a.B ? 0 : i / a.c_block] : 0.0f;
      ld_bar = (a.ldbar && i < a.B) ? a.ldbar[i] : 0.0f;
    }
    __syncthreads();
    const float ldsum = pass_fwd_stash<FAST, DFIX>(a.m, lds, St, c, a.to_base != 0);
    float ub_drift = 0.0f;      // fused score term: a * u_bar of this lane's (point, dimension) -- the OU drift's share of r3_bar
    if (a.fd2) {       // log_prob = sum -x^2/2 + ildj: the adjoint of the recovered base point is -ld_bar x
      const float* sL = St + L * DT + tid;
      if (a.r1) {      // the residual of this lane's (point, dimension) from the pair's two log_prob values
        const bool valid = tid < tp && i < a.B;
        const int64_t ib = valid ? i / a.fd2 : 0;
        const int k = (int)(i - ib * a.fd2), dd = k >> 1;
        const float lp = base_logprob<float>(lds_col<float>(sL, GROW), D) + ldsum;
        const float other = __shfl_xor(lp, 1, 64);             // (groups start at even lanes: the partner is lane ^ 1)
        const float score = ((k & 1) ? other - lp : lp - other) * a.fd_inv_dx;
        const int64_t o = ib * D + dd;
        const float r3d = valid ? a.pts[o] : 0.0f;
        const float vel = valid ? (a.r2[o] - a.r1[o]) * a.inv_dt : 0.0f;
        const bool ou = a.drift == CNF_DRIFT_OU;                // (a lane per dimension: the diagonal field or none)
        const float u = valid ? score_residual(vel, score, a.coef, ou ? ou_drift(r3d, a.drift_a) : 0.0f) : 0.0f;
        const float ub = score_residual_bar(u, a.loss_coef);
        ld_bar = ((k & 1) ? -a.coef : a.coef) * ub * a.fd_inv_dx;
        ub_drift = ou ? ou_drift_adjoint(ub, a.drift_a) : 0.0f;
        const bool owner = valid && !(k & 1);                  // one lane of the pair writes / counts
        if (owner) { a.rbar1[o] = -ub * a.inv_dt; a.rbar2[o] = ub * a.inv_dt; }
        // per-slice sums of u^2: lanes are ordered by point, so a wave's slices are those of its first and last valid lane
        const int64_t n_base = a.B / a.fd2;
        const long long slice = !valid ? -1 : (a.c_block >= n_base ? 0 : (long long)(ib / a.c_block));
        const int nv = (int)(a.B - tile_start < tp ? a.B - tile_start : tp) - (tid & ~63);      // valid lanes of this wave
        if (nv > 0) {
          const long long s_lo = __shfl(slice, 0, 64), s_hi = __shfl(slice, nv < 64 ? nv - 1 : 63, 64);
          float part = owner ? u * u : 0.0f;
          if (s_lo == s_hi) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
            if ((tid & 63) == 0) unsafeAtomicAdd(a.sums + s_lo, (double)part);
          } else if (owner) {
            unsafeAtomicAdd(a.sums + slice, (double)part);
          }
        }
      }
      for (int e = 0; e < D; ++e) Aa[e * GROW + tid] = -ld_bar * sL[e * GROW];
    }
    float* ain = pass_bwd<FAST, WGRAD, DFIX>(a.m, lds, St, Aa, Ab, ld_bar, c, a.to_base != 0, gslab, stage, fa);
    float* spare = ain == Aa ? Ab : Aa;            // the adjoint buffer the pass finished NOT in: scratch now
    if (a.fd2 && a.r1) spare[tid] = ub_drift;
    __syncthreads();
    if (a.fd2) {       // xbar[i, e] = sum over the fd2 evaluation points of base point i (fixed order: deterministic)
      if (a.xbar) {
        const int groups = tp / a.fd2;
        const int64_t first_base = tile_start / a.fd2, n_base = a.B / a.fd2;
        for (int idx = tid; idx < groups * D; idx += GTS) {
          const int il = idx / D, e = idx - il * D;
          if (first_base + il < n_base) {
            float sum = a.r1 ? spare[il * a.fd2 + 2 * e] : 0.0f;      // (+ the OU drift's -J^T u_bar = a u_bar, diagonal)
            for (int k = 0; k < a.fd2; ++k) sum += ain[e * GROW + il * a.fd2 + k];
            a.xbar[(first_base + il) * D + e] = sum;
          }
        }
      }
    } else if (a.xbar) {      // coalesced store of the input adjoints
      const int64_t base = tile_start * D;
      const int n_el = (int)(a.B - tile_start < GTS ? a.B - tile_start : GTS) * D;
      for (int e = tid; e < GTS * D; e += GTS) {
        const int s = a.div_magic ? (int)__umulhi((uint32_t)e, a.div_magic) : e, d = e - s * D;
        if (e < n_el) a.xbar[base + e] = ain[d * GROW + s];
      }
    }
  }
  if constexpr (WGRAD) {
    float red[GP];
#pragma unroll
    for (int j = 0; j < GK; ++j) { red[j] = fa.Wb[j]; red[GK + j] = fa.Hb[j]; }
#pragma unroll
    for (int j = 0; j <= GK; ++j) red[2 * GK + j] = fa.Db[j];
#pragma unroll
    for (int j = 0; j < GP; ++j) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) red[j] += __shfl_xor(red[j], off, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int j = 0; j < GP; ++j) gslab[j] += red[j];
    }
  }
}

// ---------------------------------------------------------------------------
// score_kernel: the exact score of the flow's density (cnf_score),
//   log rho(x, c) = -|z|^2 / 2 - D/2 log 2 pi + ildj(x, c),  z = F^-1(x, c)
//   grad_x log rho = (dz/dx)^T (-z) + grad_x ildj
// = the input adjoint of ONE data -> base pass seeded, from its own stash, with ybar = -z and ldbar = 1.  A kernel of
// its own and not a mode of vjp_kernel: no ybar / ldbar loads, no gradient slabs, no staging, and nothing added to the
// instruction stream of the training step.  A tile = GTS points of ONE slice (condition c[slice], wave-uniform).
// ---------------------------------------------------------------------------
struct ScoreArgs {
  ModelArgs m;
  const float* pts;      // [n_slices * count, D]; pts_slice_stride = 0: [count, D], the same points for every slice
  const float* c;        // [n_slices]
  float* score;          // [n_slices * count, D]
  float* log_prob;       // [n_slices * count] or null
  int64_t count, n_slices, pts_slice_stride;
  uint32_t div_magic;
};

template <bool FAST, int DFIX = 0>
__global__ __launch_bounds__(GTS_MAX, 2) void score_kernel(const ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int HDR = hdr_floats(GK);
  const int D = DFIX ? DFIX : a.m.D, L = a.m.L, DT = D * GROW;
  float* St = lds + PRE_FLOATS;
  float* Aa = St + (L + 1) * DT;
  float* Ab = Aa + DT;
  for (int i = threadIdx.x; i < HDR; i += GTS) lds[i] = a.m.prep[i];
  tile_consts(lds);
  const int tid = threadIdx.x;
  FirstAcc fa;      // (WGRAD = false: written, never read: removed by the compiler)
#pragma unroll
  for (int j = 0; j < GK; ++j) { fa.Wb[j] = 0.0f; fa.Hb[j] = 0.0f; }
#pragma unroll
  for (int j = 0; j <= GK; ++j) fa.Db[j] = 0.0f;
  const int64_t tiles_per_slice = (a.count + GTS - 1) / GTS, n_tiles = tiles_per_slice * a.n_slices;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t slice = tile / tiles_per_slice;
    const int64_t tile_start = (tile - slice * tiles_per_slice) * GTS;
    __syncthreads();
    tile_load1(a.pts + slice * a.pts_slice_stride * D, St, D, a.div_magic, tile_start, a.count);
    const float c = a.c[slice];
    __syncthreads();
    // the splines' clamps and bin searches turn a NaN / Inf coordinate into a finite point (flow_kernel): v - v is 0
    // for a finite v and NaN otherwise
    float poison = 0.0f;
    for (int e = 0; e < D; ++e) { const float v = St[e * GROW + tid]; poison += v - v; }
    const float ldsum = pass_fwd_stash<FAST, DFIX>(a.m, lds, St, c, true);
    const float* sL = St + L * DT + tid;
    // log_prob = -|z|^2 / 2 - D/2 log 2 pi + ildj: z and ildj are the fp32 pass's, only this sum is float64 (D FMAs
    // per point) -- at dim 10 it reaches -70, where each of D fp32 additions would round by 4e-6
    double base = -(D * HALF_LOG_2PI);
    for (int e = 0; e < D; ++e) { const double z = sL[e * GROW]; base = fma(-0.5 * z, z, base); }
    const float lp = (float)(base + (double)ldsum) + poison;
    for (int e = 0; e < D; ++e) Aa[e * GROW + tid] = -sL[e * GROW];      // d(-|z|^2 / 2) / dz_e
    float* ain = pass_bwd<FAST, false, DFIX>(a.m, lds, St, Aa, Ab, 1.0f, c, true, nullptr, nullptr, fa);
    for (int e = 0; e < D; ++e) ain[e * GROW + tid] += poison;
    const int64_t row0 = slice * a.count + tile_start;
    if (a.log_prob && tile_start + tid < a.count) a.log_prob[row0 + tid] = lp;
    __syncthreads();
    const int n_el = (int)(a.count - tile_start < GTS ? a.count - tile_start : GTS) * D;      // coalesced store of the rows
    for (int e = tid; e < GTS * D; e += GTS) {
      const int s = a.div_magic ? (int)__umulhi((uint32_t)e, a.div_magic) : e, d = e - s * D;
      if (e < n_el) a.score[row0 * D + e] = ain[d * GROW + s];
    }
  }
}

// grad[p] += sum over slabs; the first 16 entries are per-bin adjoint sums of
// the `first` spline and go through the softmax / softplus Jacobians (float64).
// Block = 32 parameters x 32 slab stripes (a thread that walks all slabs alone
// pays one dependent L2 round trip per slab: 1-2 ms for 2 048 slabs).
__global__ __launch_bounds__(1024) void grad_finish_kernel(const float* __restrict__ slabs, int64_t n_slabs,
                                                           int64_t n_params, const float* __restrict__ params,
                                                           float* __restrict__ grad, double span_eff,
                                                           double sp_offset, uint32_t* clear2) {
  // clear2: two words this launch leaves zero for the next call (the table backward's adjoint maximum and non-finite
  // flag: every reader ran before this kernel on the same stream)
  if (clear2 && blockIdx.x == 0 && threadIdx.x < 2) clear2[threadIdx.x] = 0;
  __shared__ float part[32][33];
  __shared__ double raw[GP];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t p = (int64_t)blockIdx.x * 32 + tx;
  float acc = 0.0f;
  if (p < n_params) {
    int64_t b = ty;
    for (; b + 96 < n_slabs; b += 128) {       // four independent loads in flight
      const float v0 = slabs[b * n_params + p], v1 = slabs[(b + 32) * n_params + p];
      const float v2 = slabs[(b + 64) * n_params + p], v3 = slabs[(b + 96) * n_params + p];
      acc += (v0 + v1) + (v2 + v3);
    }
    for (; b < n_slabs; b += 32) acc += slabs[b * n_params + p];
  }
  part[ty][tx] = acc;
  __syncthreads();
  if (ty == 0) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 32; ++k) s += part[k][tx];
    if (blockIdx.x == 0 && tx < GP) raw[tx] = (double)s;
    else if (p < n_params) grad[p] += s;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < GP) {
    const int j = threadIdx.x;
    double g;
    if (j < 2 * GK) {
      const int pt = j / GK, jj = j % GK;
      double mx = params[pt * GK];
      for (int k = 1; k < GK; ++k) mx = fmax(mx, (double)params[pt * GK + k]);
      double pr[GK], sum = 0.0, dot = 0.0;
      for (int k = 0; k < GK; ++k) { pr[k] = exp((double)params[pt * GK + k] - mx); sum += pr[k]; }
      for (int k = 0; k < GK; ++k) { pr[k] /= sum; dot += raw[pt * GK + k] * pr[k]; }
      g = span_eff * pr[jj] * (raw[j] - dot);
    } else {
      g = raw[j] / (1.0 + exp(-((double)params[j] + sp_offset)));
    }
    grad[j] += (float)g;
  }
}

}  // namespace cnf

using namespace cnf;

#undef GTS
// The backward kernel families by the LDS a tile of theirs needs: grad_kernel (its dim-2 instantiation keeps the
// `first` spline's accumulators in registers), vjp_kernel and score_kernel without and vjp_kernel with weight gradients
enum BwdFamily { BWD_GRAD, BWD_GRAD_D2, BWD_VJP, BWD_VJP_WGRAD };
static size_t backward_lds_bytes(BwdFamily f, int D, int L, int ts) {
  // table, ones / zeros, condition column + rows of ts + 4 floats: (L+1) stashes + 2 adjoint buffers (grad_kernel: + noise,
  // velocity, r3, r3_bar, u_bar; its generic form: + the `first` spline's accumulators) + one MFMA staging area per wave
  const bool grad = f == BWD_GRAD || f == BWD_GRAD_D2, first_acc = f == BWD_GRAD, staged = f != BWD_VJP;
  const int rows = D * ((L + 1) + (grad ? 7 : 2)) + (first_acc ? GP : 0);
  return (size_t)(hdr_floats(GK) + 64 + (ts + 4) + rows * (ts + 4) + (staged ? (ts / 64) * STAGE_FLOATS : 0)) * sizeof(float);
}
// The tile size (threads per workgroup) that puts the most waves on a CU, and its LDS: LDS allows 160 KB / lds(ts)
// workgroups of ts / 64 waves; the backward kernels' ~230 VGPRs allow 8 waves (2 per SIMD).  Ties go to the larger tile.
struct TileLds { int ts; size_t lds; };
static TileLds backward_tile(const CnfModel* m, BwdFamily f) {
  const int D = m->cfg.dim, L = m->cfg.num_layers;
  int best = 64, best_waves = 0;
  for (int ts = GTS_MAX; ts >= 64; ts >>= 1) {
    const size_t b = backward_lds_bytes(f, D, L, ts);
    if (b > 160 * 1024) continue;
    int waves = (int)((160 * 1024) / b) * (ts / 64);
    if (waves > 8) waves = 8;
    if (waves > best_waves) { best_waves = waves; best = ts; }
  }
  return {best, backward_lds_bytes(f, D, L, best)};
}

extern "C" int cnf_grad_supported(const CnfConfig* c) {
  // hidden 16 / 2 hidden layers / 5 bins (the MFMA weight-gradient tiles are 16x16), dim <= 14 (the
  // first layer's inputs + bias row fit 16 MFMA rows), and the tile's LDS working set within one CU
  return c && !c->periodized && c->hidden_size == 16 && c->mlp_num_layers == 2 && c->num_bins == 5 && c->dim >= 1 && c->dim <= 14 &&
         c->num_layers >= 1 && backward_lds_bytes(BWD_GRAD, c->dim, c->num_layers, 64) <= 160 * 1024;
}

// (cnf_host.h)
int grad_finish(const CnfModel* m, int64_t n_slabs, const float* params, float* grad, uint32_t* amax, hipStream_t stream) {
  return launch_plain(grad_finish_kernel, (m->n_params + 31) / 32, 1024, 0, stream, m->grad_slabs, n_slabs, m->n_params,
                      params, grad, (double)m->sc.span_eff, (double)m->sc.sp_offset, amax);
}

// Launches a backward kernel over n_tiles tiles: as many workgroups as are resident at once.  grad != null: its waves
// write gradient slabs (one each: no more workgroups than cnf_grad_enable made room for), which grad_finish then adds
// to grad.  CNF_ERR_UNSUPPORTED when the kernel cannot have the tile's LDS (nothing launched).
template <class K, class A>
static int launch_backward(const CnfModel* m, K kernel, const A& a, int64_t n_tiles, TileLds tl, float* grad,
                           const float* params, hipStream_t stream) {
  if (!ensure_lds(kernel, tl.lds)) return CNF_ERR_UNSUPPORTED;
  const int64_t max_grid = grad ? m->grad_max_blocks * 4 / (tl.ts / 64) : (int64_t)1 << 30;
  int64_t cap = (int64_t)resident_blocks_per_cu(kernel, tl.ts, tl.lds) * m->num_cus;
  if (cap > max_grid) cap = max_grid;
  const int64_t grid = balanced_grid(n_tiles, cap);
  const int rc = launch_plain(kernel, grid, tl.ts, tl.lds, stream, a);
  return rc != CNF_OK || !grad ? rc : grad_finish(m, grid * (tl.ts / 64), params, grad, nullptr, stream);
}

// The kernel instantiations of a model (dim 2 with fast math has its own; without weight gradients nothing is staged)
static auto grad_kernel_of(const CnfModel* m, BwdFamily f) -> void (*)(const GradArgs) {
  if (f == BWD_GRAD_D2) return grad_kernel<true, 2>;
  return m->fast_math ? grad_kernel<true> : grad_kernel<false>;
}
typedef void (*VjpKernel)(const VjpArgs);
static VjpKernel vjp_kernel_of(const CnfModel* m, bool wgrad) {
  if (!wgrad) return m->fast_math ? vjp_kernel<true, false> : vjp_kernel<false, false>;
  if (!m->fast_math) return vjp_kernel<false, true>;
  return m->cfg.dim == 2 ? vjp_kernel<true, true, 2> : vjp_kernel<true, true>;
}
static auto score_kernel_of(const CnfModel* m) -> void (*)(const ScoreArgs) {
  if (!m->fast_math) return score_kernel<false>;
  return m->cfg.dim == 2 ? score_kernel<true, 2> : score_kernel<true>;
}

extern "C" int cnf_loss_terms_grad_multi(CnfModel* m, int32_t n_terms, const CnfLossSpec* specs, const float* const* pts,
                                         const int32_t* pts_shared, const float* const* t, const int64_t* n_slices,
                                         const int64_t* B, const float* scale, double* const* sums, float* grad,
                                         const float* params, void* stream_) {
  if (!m || n_terms < 1 || n_terms > GRAD_MAX_JOBS || !specs || !pts || !pts_shared || !t || !n_slices || !B || !scale ||
      !sums || !grad || !params)
    return CNF_ERR_INVALID;
  if (const int rc = backward_check(m, CHECK_MODEL, nullptr); rc != CNF_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const BwdFamily family = m->fast_math && m->cfg.dim == 2 ? BWD_GRAD_D2 : BWD_GRAD;
  const TileLds tl = backward_tile(m, family);
  if (tl.lds > 160 * 1024) return CNF_ERR_UNSUPPORTED;
  GradArgs a;
  a.m = model_args(m); a.slabs = m->grad_slabs; a.n_params = m->n_params; a.div_magic = m->div_magic;
  a.n_jobs = 0; a.n_tiles = 0;
  for (int i = 0; i < n_terms; ++i)      // (every term is checked before anything is enqueued)
    if (term_grad_spec_check(specs + i, m->cfg.dim) != CNF_OK || !pts[i] || !t[i] || !sums[i] || n_slices[i] < 0 || B[i] < 0)
      return CNF_ERR_INVALID;
  for (int i = 0; i < n_terms; ++i) {
    const int todo = zero_sums(sums[i], n_slices[i], B[i], stream);
    if (todo < 0) return todo;
    if (!todo) continue;
    GradJob& J = a.job[a.n_jobs++];
    J.spec = specs[i]; J.pts = pts[i]; J.t = t[i]; J.sums = sums[i];
    J.B = B[i]; J.n_slices = n_slices[i]; J.pts_slice_stride = pts_shared[i] ? 0 : B[i];
    J.scale = scale[i]; J.first_tile = a.n_tiles;
    a.n_tiles += ((B[i] + tl.ts - 1) / tl.ts) * n_slices[i];
  }
  if (a.n_jobs == 0) return CNF_OK;
  for (int i = a.n_jobs; i < GRAD_MAX_JOBS; ++i) { a.job[i] = a.job[0]; a.job[i].first_tile = a.n_tiles; }
  // (the slab room is asked here, after the terms' checks and sums, not with the model's: an empty call needs none)
  if (const int rc = backward_check(m, CHECK_SLABS | CHECK_WAIT, stream); rc != CNF_OK) return rc;
  const int rc = launch_backward(m, grad_kernel_of(m, family), a, a.n_tiles, tl, grad, params, stream);
  return rc == CNF_ERR_UNSUPPORTED ? CNF_ERR_HIP : rc;
}

extern "C" int cnf_loss_terms_grad(CnfModel* m, const CnfLossSpec* spec, const float* pts, int pts_shared,
                                   const float* t, int64_t n_slices, int64_t B, float scale, double* sums,
                                   float* grad, const float* params, void* stream_) {
  if (!spec || !pts || !t || !sums) return CNF_ERR_INVALID;
  const int32_t shared = pts_shared ? 1 : 0;
  return cnf_loss_terms_grad_multi(m, 1, spec, &pts, &shared, &t, &n_slices, &B, &scale, &sums, grad, params, stream_);
}

extern "C" int cnf_grad_enable(CnfModel* m, int64_t max_blocks) {
  if (!m) return CNF_ERR_INVALID;
  if (!cnf_grad_supported(&m->cfg)) return CNF_ERR_UNSUPPORTED;
  if (max_blocks <= 0) max_blocks = (int64_t)m->num_cus * 2;
  if (m->grad_slabs && m->grad_max_blocks >= max_blocks) return CNF_OK;
  if (m->grad_slabs) { (void)hipFree(m->grad_slabs); m->grad_slabs = nullptr; }
  if (hipMalloc((void**)&m->grad_slabs, sizeof(float) * (size_t)(max_blocks * 4 * m->n_params)) != hipSuccess) return CNF_ERR_NOMEM;
  m->grad_max_blocks = max_blocks;
  // the table backward of dim-2 passes (cnf_grad_pwl.hip): per-piece statistics, kept zero between calls
  // (pwl_stats_finish_kernel clears what it reads)
  if (!m->pwl_stats && pwl_backward_network(m->cfg)) {
    const size_t bytes = pwl_stats_bytes(m->cfg.num_layers);
    if (hipMalloc((void**)&m->pwl_stats, bytes) != hipSuccess) m->pwl_stats = nullptr;          // (the MLP backward remains)
    else if (hipMemset(m->pwl_stats, 0, bytes) != hipSuccess) { (void)hipFree(m->pwl_stats); m->pwl_stats = nullptr; }
  }
  return CNF_OK;
}

// The arguments of a plain pass: the finite-difference mode and the fused score term are off
static VjpArgs vjp_args(const CnfModel* m, int to_base, const float* pts, const float* c, int64_t c_block,
                        const float* ybar, const float* ldbar, float* xbar, int64_t B) {
  VjpArgs a;
  a.m = model_args(m); a.pts = pts; a.c = c; a.ybar = ybar; a.ldbar = ldbar; a.xbar = xbar;
  a.slabs = m->grad_slabs; a.n_params = m->n_params;
  a.B = B; a.c_block = c_block; a.to_base = to_base ? 1 : 0; a.div_magic = m->div_magic;
  a.fd2 = 0; a.fd_h = 0.f; a.fd_inv_dx = 0.f; a.gbar = nullptr;
  a.r1 = a.r2 = nullptr; a.rbar1 = a.rbar2 = nullptr; a.sums = nullptr; a.inv_dt = a.coef = a.drift_a = a.loss_coef = 0.f; a.drift = -1;
  return a;
}

extern "C" int cnf_pass_vjp(CnfModel* m, int to_base, const float* pts, const float* c, int64_t c_block,
                            const float* ybar, const float* ldbar, float* xbar, float* grad, const float* params,
                            int64_t B, void* stream_) {
  if (!m || !pts || !c || B < 0 || c_block < 1 || (!ybar && !ldbar) || (!xbar && !grad)) return CNF_ERR_INVALID;
  if (grad && !params) return CNF_ERR_INVALID;
  if (const int rc = backward_check(m, CHECK_MODEL, nullptr); rc != CNF_OK) return rc;
  if (B == 0) return CNF_OK;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = backward_check(m, (grad ? CHECK_SLABS : 0) | CHECK_WAIT, stream); rc != CNF_OK) return rc;
  if (grad) {
    const int r = pass_vjp_pwl(m, to_base, pts, c, c_block, ybar, ldbar, xbar, grad, params, B, stream);
    if (r != CNF_ERR_UNSUPPORTED) return r;
  }
  const VjpArgs a = vjp_args(m, to_base, pts, c, c_block, ybar, ldbar, xbar, B);
  const TileLds tl = backward_tile(m, grad ? BWD_VJP_WGRAD : BWD_VJP);
  return launch_backward(m, vjp_kernel_of(m, grad != nullptr), a, (B + tl.ts - 1) / tl.ts, tl, grad, params, stream);
}

extern "C" int cnf_input_vjp(CnfModel* m, int to_base, const float* pts, const float* c, int64_t c_block,
                             const float* ybar, const float* ldbar, float* xbar, int64_t B, void* stream) {
  if (!xbar) return CNF_ERR_INVALID;
  return cnf_pass_vjp(m, to_base, pts, c, c_block, ybar, ldbar, xbar, nullptr, nullptr, B, stream);
}

extern "C" int cnf_score(CnfModel* m, const float* pts, int32_t pts_shared, const float* c, int64_t n_slices,
                         int64_t count, float* score, float* log_prob, void* stream_) {
  if (!m || !pts || !c || !score || n_slices < 0 || count < 0) return CNF_ERR_INVALID;
  if (const int rc = backward_check(m, CHECK_MODEL, nullptr); rc != CNF_OK) return rc;
  if (n_slices == 0 || count == 0) return CNF_OK;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = backward_check(m, CHECK_WAIT, stream); rc != CNF_OK) return rc;
  ScoreArgs a;
  a.m = model_args(m); a.pts = pts; a.c = c; a.score = score; a.log_prob = log_prob;
  a.count = count; a.n_slices = n_slices; a.pts_slice_stride = pts_shared ? 0 : count; a.div_magic = m->div_magic;
  const TileLds tl = backward_tile(m, BWD_VJP);      // (cnf_grad_supported: the larger grad_kernel tile fits a CU)
  const int rc = launch_backward(m, score_kernel_of(m), a, ((count + tl.ts - 1) / tl.ts) * n_slices, tl, nullptr, nullptr, stream);
  if (rc != CNF_ERR_UNSUPPORTED) m->last_path = CNF_PATH_SCORE;      // (only a call that launched reports its path)
  return rc;
}

// The finite-difference launches (cnf_logprob_fd_vjp, cnf_score_fd_vjp): a.pts holds n base points, the kernel
// differentiates log_prob at their 2 D evaluation points r_i -+ dx/2 e_d (generated in the kernel), a.B of them.
static int fd_vjp_launch(CnfModel* m, VjpArgs& a, float dx, float* grad, const float* params, hipStream_t stream) {
  const int D = m->cfg.dim;
  a.fd2 = 2 * D; a.fd_h = 0.5f * dx; a.fd_inv_dx = 1.0f / dx;
  // a tile holds at least one group of 2 D evaluation points (every tile does: 64 samples, dim <= 14)
  const TileLds tl = backward_tile(m, BWD_VJP_WGRAD);
  if (tl.ts < 2 * D || tl.lds > 160 * 1024) return CNF_ERR_UNSUPPORTED;
  const int64_t tp = (tl.ts / (2 * D)) * (2 * D);
  return launch_backward(m, vjp_kernel_of(m, true), a, (a.B + tp - 1) / tp, tl, grad, params, stream);
}

extern "C" int cnf_logprob_fd_vjp(CnfModel* m, const float* pts, const float* c, int64_t c_block, float dx,
                                  const float* gbar, float* pts_bar, float* grad, const float* params, int64_t B,
                                  void* stream_) {
  if (!m || !pts || !c || !gbar || B < 0 || c_block < 1 || !(dx > 0.f) || (!pts_bar && !grad)) return CNF_ERR_INVALID;
  if (!grad || !params) return CNF_ERR_INVALID;       // the parameter gradient is what this entry point is for
  if (const int rc = backward_check(m, CHECK_MODEL, nullptr); rc != CNF_OK) return rc;
  if (B == 0) return CNF_OK;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = backward_check(m, CHECK_SLABS | CHECK_WAIT, stream); rc != CNF_OK) return rc;
  VjpArgs a = vjp_args(m, 1, pts, c, c_block, nullptr, nullptr, pts_bar, B * 2 * m->cfg.dim);
  a.gbar = gbar;
  return fd_vjp_launch(m, a, dx, grad, params, stream);
}

extern "C" int cnf_score_fd_vjp(CnfModel* m, const float* r, const float* c, int64_t count, float dt, float dx, float coef,
                                int32_t drift, float a_, float loss_coef, double* sums, float* rbar, float* grad,
                                const float* params, int64_t n, void* stream_) {
  if (!m || !r || !c || !sums || !rbar || !grad || !params || n < 0 || count < 1 || !(dt > 0.f) || !(dx > 0.f))
    return CNF_ERR_INVALID;
  if (drift != -1 && drift != CNF_DRIFT_OU) return CNF_ERR_UNSUPPORTED;      // (the coupled 2-D / 3-D fields: cnf_loss_terms_grad)
  if (const int rc = backward_check(m, CHECK_MODEL, nullptr); rc != CNF_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  // (the sums are zeroed before the slab room is asked)
  if (const int todo = zero_sums(sums, (n + count - 1) / count, n, stream); todo <= 0) return todo;
  if (const int rc = backward_check(m, CHECK_SLABS | CHECK_WAIT, stream); rc != CNF_OK) return rc;
  const int64_t nD = n * m->cfg.dim;
  VjpArgs a = vjp_args(m, 1, r + 2 * nD, c, count, nullptr, nullptr, rbar + 2 * nD, 2 * nD);
  a.r1 = r; a.r2 = r + nD; a.rbar1 = rbar; a.rbar2 = rbar + nD; a.sums = sums;
  a.inv_dt = 1.0f / dt; a.coef = coef; a.drift_a = a_; a.loss_coef = loss_coef; a.drift = drift;
  return fd_vjp_launch(m, a, dx, grad, params, stream);
}
