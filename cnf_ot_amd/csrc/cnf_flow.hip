// cnf_flow.hip -- the kernels that run the flow, and their host layer: the parameter snapshot (prepare_kernel,
// circular_slopes_kernel, cnf_model_set_params), the flow (flow_kernel, flow_dpar_kernel, flow_pwl_kernel, the table
// route), the fused loss terms (loss_kernel, loss_pwl_kernel) and the fields (fields_kernel).  They share one unit
// because their generated code depends on it (profiles/split_units/README.md).  The model object: cnf_model.hip;
// the noise fills: cnf_rng.hip; shared device code: cnf_flow_tile.h; what crosses units: cnf_host.h.
// Declarations and the reference interfaces they replace: include/cnf_ot_amd.h.
//
// Kernel design (DESIGN.md has the numbers):
//  * one sample per lane, a 256-sample tile per workgroup, grid-stride over
//    tiles; the tile's [256, D] rows are one contiguous HBM range, so loads and
//    stores are fully coalesced and transposed through LDS into per-thread
//    columns u[d][tid] (conflict-free per-lane access);
//  * all L layers, all D dimensions, conditioner MLP + spline + log|det J|
//    accumulate are fused: HBM sees only the input row, the output row and one
//    float of log-det / log-prob per sample;
//  * conditioner weights are wave-uniform: they reach the per-lane FMAs as
//    scalar (SGPR) operands through the scalar cache, not through LDS/VGPRs;
//  * the shared `first` spline is pre-normalised (float64, once per parameter
//    set) into a 12-float-per-bin table that is staged in LDS and gathered by
//    per-lane bin index.
#include "cnf_flow_tile.h"
#include "cnf_host.h"
#include "cnf_pwl_build.h"

#include <math.h>
#include <new>
#include <stdlib.h>
#include <string.h>

namespace cnf {

// boundary_slopes='circular' (RQSFlow(periodized=True), flows.py:131): the last knot's unnormalized slope IS the
// first knot's.  Run after prepare_kernel on the same stream: in the weight snapshot, column 3K of every output
// layer becomes a copy of column 2K, so the kernels produce theta[3K] == theta[2K] bit for bit with no code of
// their own (the caller's parameters are not touched).  One block per conditioner.
__global__ void circular_slopes_kernel(const float* __restrict__ params, float* __restrict__ prep, int K, int H,
                                       int D, int L, int M, int64_t per_layer) {
  const int P = 3 * K + 1;
  const int hdr = hdr_floats(K);
  const int l = blockIdx.x / (D - 1), d = 1 + blockIdx.x % (D - 1);
  int64_t o = (int64_t)l * per_layer;
  for (int dd = 1; dd < d; ++dd) o += cond_floats_p(dd, H, M, P, true);
  o += cond_floats_p(d, H, M, P, true) - ((int64_t)H * P + P);       // this conditioner's output layer
  for (int r = threadIdx.x; r <= H; r += blockDim.x)                  // H weight rows + the bias row
    prep[hdr + o + (int64_t)r * P + 3 * K] = params[P + o + (int64_t)r * P + 2 * K];
}

// ---------------------------------------------------------------------------
// prepare_kernel: params (flat, caller-owned) -> prepared model buffer.
// Thread 0 normalises the `first` spline in float64; all threads snapshot the
// conditioner weights.
// ---------------------------------------------------------------------------
__global__ void prepare_kernel(const float* __restrict__ params, float* __restrict__ prep,
                               int K, int64_t n_params, double lo, double hi, double min_bin,
                               double min_slope, int D, int L, int M, int64_t per_layer,
                               int64_t per_layer_q, int64_t mfma_off, int64_t tabd_off, int H, int periodic,
                               int64_t ft_off) {
  const int P = 3 * K + 1;
  const int hdr = hdr_floats(K);
  constexpr int MAXK = 64;
  // The LAST block normalises the `first` spline (float64); the others snapshot the weights.  The ~40 float64
  // exp / log calls of the normalisation used to run one after the other on thread 0 of block 0, behind its share of
  // the copies: 20 us for a kernel every loss evaluation starts with -- now one call per lane, and only the sums
  // (whose order fixes the result's bits) stay serial.
  if (blockIdx.x != gridDim.x - 1) {
    const int nb = gridDim.x - 1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_params - P; i += (int64_t)nb * blockDim.x)
      prep[hdr + i] = params[P + i];
    if (mfma_off > 0) {
      // MFMA-layout copy of every conditioner (H = P = 16): see conditioner_mfma.
      const int nc = L * (D - 1);
      for (int ci = blockIdx.x; ci < nc; ci += nb) {
        const int l = ci / (D - 1), d = 1 + ci % (D - 1);
        int64_t so = P + l * per_layer, qo = mfma_off + l * per_layer_q;
        for (int dd = 1; dd < d; ++dd) { so += cond_floats(dd, 16, M, 16); qo += cond_floats_mfma(dd, M); }
        const float* src = params + so;
        float* dst = prep + qo;
        const int nf = (1 + d) + 1 + 2 * M;
        for (int idx = threadIdx.x; idx < nf * 64; idx += blockDim.x) {
          const int f = idx >> 6, lane = idx & 63, g = lane >> 4, i = lane & 15;
          float o[4];
          if (f <= d) {                         // W0 row f (f = 0: the c row)
            for (int t = 0; t < 4; ++t) o[t] = src[f * 16 + 4 * g + t];
          } else if (f == d + 1) {              // b0
            for (int t = 0; t < 4; ++t) o[t] = src[(1 + d) * 16 + 4 * g + t];
          } else {
            const int m = (f - (d + 2)) >> 1;
            const float* Wm = src + (1 + d) * 16 + 16 + m * (256 + 16);
            if (((f - (d + 2)) & 1) == 0) { for (int t = 0; t < 4; ++t) o[t] = Wm[(4 * g + t) * 16 + i]; }   // A step t
            else { for (int t = 0; t < 4; ++t) o[t] = Wm[256 + 4 * g + t]; }                               // bias rows 4g+r
          }
          for (int t = 0; t < 4; ++t) dst[(f * 64 + lane) * 4 + t] = o[t];
        }
      }
    }
    return;
  }

  __shared__ double ex[2][MAXK], dl[MAXK + 1], mxs[2];
  // new parameters: the `first` spline's inverse table (cnf_first_table.h) is stale until its builder has certified it
  if (ft_off > 0 && threadIdx.x < FT_WORDS) reinterpret_cast<uint32_t*>(prep + ft_off)[threadIdx.x] = 0u;
  if (threadIdx.x < 2) {
    const float* u = params + threadIdx.x * K;
    double mx = u[0];
    for (int k = 1; k < K; ++k) mx = fmax(mx, (double)u[k]);
    mxs[threadIdx.x] = mx;
  }
  __syncthreads();
  const double offset = log(exp(1.0 - min_slope) - 1.0);
  for (int idx = threadIdx.x; idx < 3 * K + 1; idx += blockDim.x) {
    if (idx < 2 * K) {
      const int part = idx / K, k = idx - part * K;
      ex[part][k] = exp((double)params[part * K + k] - mxs[part]);
    } else {
      const int k = idx - 2 * K;
      const double v = (double)params[2 * K + (periodic && k == K ? 0 : k)] + offset;      // circular: slope K := slope 0
      dl[k] = fmax(v, 0.0) + log1p(exp(-fabs(v))) + min_slope;
    }
  }
  __syncthreads();
  __shared__ double xk[MAXK + 1], yk[MAXK + 1];
  double* td = reinterpret_cast<double*>(prep + tabd_off);     // the same table in float64
  for (int i = threadIdx.x; i < hdr; i += blockDim.x) { prep[i] = 0.0f; td[i] = 0.0; }
  const double total = (hi - lo) - K * min_bin;
  if (threadIdx.x < 2) {       // the knot positions: running sums, in the one order that fixes their bits
    const int part = threadIdx.x;
    double* pos = part == 0 ? xk : yk;
    double sum = 0;
    for (int k = 0; k < K; ++k) sum += ex[part][k];
    double run = 0;
    pos[0] = lo;
    for (int k = 0; k < K - 1; ++k) {
      run += ex[part][k] / sum * total + min_bin;
      pos[k + 1] = lo + run;
    }
    pos[K] = hi;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += blockDim.x) {      // one bin per thread
    const double bw = xk[k + 1] - xk[k], bh = yk[k + 1] - yk[k], s = bh / bw;
    td[tab_off(F_X0, K) + k] = xk[k];            td[tab_off(F_Y0, K) + k] = yk[k];
    td[tab_off(F_BW, K) + k] = bw;               td[tab_off(F_BH, K) + k] = bh;
    td[tab_off(F_IBW, K) + k] = 1.0 / bw;        td[tab_off(F_IBH, K) + k] = 1.0 / bh;
    td[tab_off(F_S, K) + k] = s;                 td[tab_off(F_ST, K) + k] = dl[k + 1] + dl[k] - 2.0 * s;
    td[tab_off(F_D0, K) + k] = dl[k];            td[tab_off(F_D1, K) + k] = dl[k + 1];
    td[tab_off(F_L2S, K) + k] = 2.0 * log(s);
    prep[tab_off(F_X0, K) + k] = (float)xk[k];
    prep[tab_off(F_Y0, K) + k] = (float)yk[k];
    prep[tab_off(F_BW, K) + k] = (float)bw;
    prep[tab_off(F_BH, K) + k] = (float)bh;
    prep[tab_off(F_IBW, K) + k] = (float)(1.0 / bw);
    prep[tab_off(F_IBH, K) + k] = (float)(1.0 / bh);
    prep[tab_off(F_S, K) + k] = (float)s;
    prep[tab_off(F_ST, K) + k] = (float)(dl[k + 1] + dl[k] - 2.0 * s);
    prep[tab_off(F_D0, K) + k] = (float)dl[k];
    prep[tab_off(F_D1, K) + k] = (float)dl[k + 1];
    prep[tab_off(F_L2S, K) + k] = (float)(2.0 * log(s));
    // the per-bin products of the sampling direction's quadratic (rqs_bin_eval PRE)
    td[tab_off(F_D0BH, K) + k] = dl[k] * bh;     td[tab_off(F_2S, K) + k] = 2.0 * s;
    prep[tab_off(F_D0BH, K) + k] = (float)(dl[k] * bh);
    prep[tab_off(F_2S, K) + k] = 2.0f * (float)s;      // exactly twice F_S, which the derivative's denominator reads
  }
  for (int k = threadIdx.x; k <= K; k += blockDim.x) {
    const float big = 1.152921504606846976e18f;      // 2^60
    if (2 * k + 1 < 2 * tab_stride(K)) {
      prep[tab_off(F_XKB, K) + 2 * k] = prep[tab_off(F_XKB, K) + 2 * k + 1] = -(float)xk[k] * big;
      prep[tab_off(F_YKB, K) + 2 * k] = prep[tab_off(F_YKB, K) + 2 * k + 1] = -(float)yk[k] * big;
    }
    prep[tab_off(F_XK, K) + k] = (float)xk[k];
    prep[tab_off(F_YK, K) + k] = (float)yk[k];
    td[tab_off(F_XK, K) + k] = xk[k];
    td[tab_off(F_YK, K) + k] = yk[k];
  }
  if (threadIdx.x != 64) return;       // the linear tails (a lane of another wave than the bins')
  double* tld = td + tab_off(F_TAIL, K);
  tld[T_DLO] = dl[0];            tld[T_DHI] = dl[K];
  tld[T_LOG_DLO] = log(dl[0]);   tld[T_LOG_DHI] = log(dl[K]);
  tld[T_INV_DLO] = 1.0 / dl[0];  tld[T_INV_DHI] = 1.0 / dl[K];
  float* tl = prep + tab_off(F_TAIL, K);
  tl[T_DLO] = (float)dl[0];             tl[T_DHI] = (float)dl[K];
  tl[T_LOG_DLO] = (float)log(dl[0]);    tl[T_LOG_DHI] = (float)log(dl[K]);
  tl[T_INV_DLO] = (float)(1.0 / dl[0]); tl[T_INV_DHI] = (float)(1.0 / dl[K]);
}

template <int H, int K, bool TO_BASE, bool FAST, class T, bool MFMA = false, bool PRECISE = false, bool PERIODIC = false, int DFIX = 0>
__global__ __launch_bounds__(TILE, 2) void flow_kernel(const FlowArgsT<typename Lanes<T>::real> a) {
  typedef typename Lanes<T>::real R;
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);
  constexpr int HDR = hdr_floats(K);
  constexpr int SPL = Lanes<T>::N;
  constexpr int TS = TILE * SPL;
  const int DD = DFIX ? DFIX : a.m.D;
  const uint32_t dmagic = DFIX == 2 ? 0x80000000u : (uint32_t)a.div_magic;
  R* tab = lds;
  R* U = lds + HDR;
  R* O = U + DD * TS;
  if (gate_closed(a)) return;
  for (int i = threadIdx.x; i < HDR; i += TILE) tab[i] = table_of<R>(a.m)[i];
  [[maybe_unused]] double* e2tab = nullptr;
  [[maybe_unused]] double* tabd = nullptr;
  [[maybe_unused]] R* LO = nullptr;
  if constexpr (PRECISE) {      // [.. U O][LO][2^(-i/32) table][float64 `first` table]; HDR, D * TS even: 8-byte aligned
    LO = O + DD * TS;
    e2tab = reinterpret_cast<double*>(LO + DD * TS);
    tabd = e2tab + EXP2_N;
    for (int i = threadIdx.x; i < EXP2_N; i += TILE) e2tab[i] = a.m.e2tab[i];
    for (int i = threadIdx.x; i < HDR; i += TILE) tabd[i] = a.m.tabd[i];
  }

  const int64_t n_tiles = (a.B + TS - 1) / TS;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t tile_start = tile * TS;
    const int64_t i = tile_start + SPL * threadIdx.x;
    __syncthreads();                       // previous tile's stores are done with U/O
    if (TO_BASE && !PRECISE && a.fd2) tile_load_fd<R>(a, U, DD, dmagic, TS, tile_start);
    else if (a.in) tile_load<R>(a.in, U, DD, dmagic, TS, tile_start, a.B);
    else tile_noise_flow(a, U, DD, dmagic, TS, tile_start, TILE);
    const T c = load_cond<T>(a, tile_start, i);
    __syncthreads();

    T base = splat<T>(0.0f);
    if (!TO_BASE && a.aux_mode == AUX_LOGPROB && a.aux) base = base_logprob<T>(lds_col<T>(U + SPL * threadIdx.x, TS), DD);
    BaseAcc<T> bacc;
    // data -> base: the splines' clamps and bin searches turn a NaN coordinate into a finite point (log_prob(NaN) came
    // out as -58.9); the reference's arithmetic propagates it.  v - v is 0 for a finite v and NaN otherwise.
    [[maybe_unused]] T poison = splat<T>(0.0f);
    if constexpr (TO_BASE) {
      for (int d = 0; d < DD; ++d) { const T v = lds_get<T>(U + SPL * threadIdx.x, d, TS); poison += v - v; }
    }
    const T acc = flow_pass<H, K, TO_BASE, FAST, T, MFMA, PRECISE, PERIODIC, DFIX>(a.m, tab, U, O, c, e2tab, tabd, LO, &bacc);
    if (a.aux) {
      T r = acc;
      if (a.aux_mode == AUX_LOGPROB) {
        // log_prob = base(x) + ildj (conditional.py:316-321); lp_y = lp_x - fldj (:399-401)
        if constexpr (PRECISE) r = bacc.log_prob(acc, DD);
        else r = TO_BASE ? base_logprob<T>(lds_col<T>(U + SPL * threadIdx.x, TS), DD) + acc : base - acc;
      }
      if constexpr (TO_BASE) r += poison;
      if (TO_BASE && !PRECISE && a.fd2) store_fd(a, i, r);
      else store_aux(a.aux, i, a.B, r);
    }
    if (a.out) {
      if constexpr (TO_BASE) {
        for (int d = 0; d < DD; ++d) lds_put(U + SPL * threadIdx.x, d, TS, lds_get<T>(U + SPL * threadIdx.x, d, TS) + poison);
      }
      __syncthreads();
      tile_store<R>(a.out, U, DD, dmagic, TS, tile_start, a.B);
    }
  }
}


// ---------------------------------------------------------------------------
// flow_dpar_kernel: base -> data (sample / sample_and_log_prob / forward) for D >= 3 with the D - 1 conditioners
// of a layer on different WAVES.  In this direction every conditioner of a layer sees the layer's INPUTS
// (autoregressive.py:109-136: `y[perm[:d]]` of the incoming event), so they are independent of each other; the
// one-sample-per-lane kernel above runs them back to back on one lane and needs ~2 M samples to fill the chip
// (config 4's per-GPU shard is 32 768: 512 waves on 1 024 SIMDs, each with a chain of 2 x 9 conditioners).
// Here a workgroup owns a tile of 64 * SPL samples and has one wave per conditioned dimension (d = 1 + wave,
// strided if D - 1 exceeds the wave count): the weights stay wave-uniform (scalar operands), a layer costs one
// conditioner + one spline per wave and a barrier, and the shard becomes 256-512 workgroups of D - 1 waves.  The
// waves' log-det shares are summed in a fixed order (deterministic).
// ---------------------------------------------------------------------------
template <int H, int K, bool FAST, class T>
__global__ __launch_bounds__(1024) void flow_dpar_kernel(const FlowArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int HDR = hdr_floats(K), P = 3 * K + 1, SPL = Lanes<T>::N, TS = 64 * SPL;
  const int D = a.m.D, L = a.m.L, NT = blockDim.x, NW = NT >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float* tab = lds;
  float* U = lds + HDR;
  float* O = U + D * TS;
  float* LD = O + D * TS;                                  // [NW][TS] log-det shares
  if (gate_closed(a)) return;
  for (int i = threadIdx.x; i < HDR; i += NT) tab[i] = a.m.prep[i];
  const SplineConsts& sc = a.m.sc;
  uniform_ptr weights = as_uniform(a.m.prep + HDR);
  // floats of the conditioners 1 .. d-1 of a layer: sum_{q<d} ((1 + q) H + C), C = the d-independent part
  const int64_t cpart = cond_floats(0, H, a.m.M, P) - H;

  const int64_t n_tiles = (a.B + TS - 1) / TS;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t tile_start = tile * TS;
    const int64_t i = tile_start + SPL * lane;
    __syncthreads();
    if (a.in) tile_load_n<float>(a.in, U, D, a.div_magic, TS, tile_start, a.B, NT);
    else tile_noise_flow(a, U, D, a.div_magic, TS, tile_start, NT);
    const T c = load_cond<T>(a, tile_start, i);
    __syncthreads();
    T base = splat<T>(0.0f);
    if (wave == 0 && a.aux_mode == AUX_LOGPROB && a.aux) base = base_logprob<T>(lds_col<T>(U + SPL * lane, TS), D);
    T acc = splat<T>(0.0f);
    for (int l = 0; l < L; ++l) {
      const bool odd = l & 1;                              // flows.py:141-143 perms
      const int first_idx = odd ? D - 1 : 0, idx_step = odd ? -1 : 1;
      const float* cu = U + SPL * lane;
      float* co = O + SPL * lane;
      T o, ld;
      if (wave == 0) {
        table_spline<K, true, FAST, T>(tab, lds_get<T>(cu, first_idx, TS), sc, o, ld);
        lds_put(co, first_idx, TS, o);
        acc += ld;
      }
      for (int d = 1 + wave; d < D; d += NW) {
        const int64_t off = l * a.m.per_layer + (int64_t)H * ((d - 1) + (int64_t)d * (d - 1) / 2) + (d - 1) * cpart;
        T th[P];
        conditioner<H, P, T>(weights + off, d, a.m.M, c, cu, first_idx, idx_step, TS, th);
        const int idx = first_idx + d * idx_step;
        cond_spline<K, true, FAST, T>(th, lds_get<T>(cu, idx, TS), sc, o, ld);
        lds_put(co, idx, TS, o);
        acc += ld;
      }
      __syncthreads();
      float* t = U; U = O; O = t;
    }
    if (a.aux) lds_put(LD + wave * TS + SPL * lane, 0, TS, acc);
    __syncthreads();
    if (a.aux && wave == 0) {
      T tot = splat<T>(0.0f);
      for (int w = 0; w < NW; ++w) tot += lds_get<T>(LD + w * TS + SPL * lane, 0, TS);
      store_aux(a.aux, i, a.B, a.aux_mode == AUX_LOGPROB ? base - tot : tot);
    }
    if (a.out) tile_store_n<float>(a.out, U, D, a.div_magic, TS, tile_start, a.B, NT);
  }
}

// ---------------------------------------------------------------------------
// flow_pwl_kernel: the dim-2 flow with the conditioner read from the exact
// piecewise-linear tables of cnf_pwl.h (condition uniform per slice).  One
// 1024-thread workgroup per CU keeps the L tables of its current slice in LDS
// (every row when L <= 3: L x 48 KB; else L x 22 KB: header arrays + the first PWL_LROWS rows); each lane owns
// two consecutive samples, whose 4 input floats are one 16-byte load and whose
// outputs are one 16-byte + one 8-byte store -- no LDS staging of the points.
// ---------------------------------------------------------------------------
struct PwlArgs {
  ModelArgs m;
  const float* in;
  float* out;
  float* aux;
  const float* tables;
  int64_t B, slice_len;
  int32_t n_slices, tiles_per_slice, aux_mode;
  const uint32_t* gate;      // see FlowArgsT
  uint32_t gate_epoch;
  int32_t gate_want;
  // in == null: base noise drawn in the kernel -- sample j of slice s (of this launch) is stream sample
  // first_sample + s * slice_stride + j of the cnf_fill_normal stream of `seed`
  uint64_t seed;
  int64_t first_sample, slice_stride;
  int32_t in_shared;         // the slices share ONE set of input points in[slice_len, 2] (the same base draw pushed to
                             // several times: cnf_kinetic_potential_vjp)
  const float* ft;           // the `first` spline's inverse table (cnf_first_table.h) with its status words, or null:
};                           // the closed form.  Read only by the instantiations that have the table path (FTAB).

// Every reference call site hands the flow one time broadcast to cond[B,1] (applications.py:153,226,231):
// per-sample in form, uniform in content.  For launches large enough for the table path this kernel checks it on
// the device: a block that finds c[i] != c[0] stamps the call's epoch into *flag.  The table kernels and the MLP
// kernel of the call are both enqueued and read the stamp: exactly one of them does the work (no host round trip).
__global__ void cond_uniform_kernel(const float* __restrict__ c, int64_t B, uint32_t* flag, uint32_t epoch) {
  const uint32_t c0 = __float_as_uint(c[0]);
  bool diff = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x)
    diff |= __float_as_uint(c[i]) != c0;
  if (__syncthreads_or(diff) && threadIdx.x == 0) *flag = epoch;
}

// s_waitcnt vmcnt(0) as the builtin's immediate (gfx9: vmcnt in bits 3:0 and 15:14), the export and LDS / scalar
// counters at their maxima, i.e. not waited for
constexpr int PWL_WAIT_VM0 = 0x0F70;

template <int K, bool TO_BASE, bool FAST, bool PRECISE = false, int LROWS = PWL_LROWS, int LFIX = 0, bool SEEDED = false>
__global__ __launch_bounds__(PWL_MAX_THREADS) void flow_pwl_kernel(const PwlArgs a) {
  const int PWL_THREADS = blockDim.x, PWL_TS = 2 * PWL_THREADS;
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  constexpr int HDR = (hdr_floats(K) + 3) & ~3;
  float* tab = lds_raw;
  float* tbl = lds_raw + HDR;
  const int tid = threadIdx.x;
  const int L = LFIX ? LFIX : a.m.L;
  if (gate_closed(a)) return;
  for (int i = tid; i < hdr_floats(K); i += PWL_THREADS) tab[i] = table_of<float>(a.m)[i];
  const SplineConsts sc = sc_scalars(sc_of<float>(a.m));
  [[maybe_unused]] double* e2tab = nullptr;
  [[maybe_unused]] double* tabd = nullptr;
  if constexpr (PRECISE) {                 // after the L tables (HDR and PWL_LTBL are even: 8-byte aligned)
    e2tab = reinterpret_cast<double*>(tbl + L * pwl_ltbl(LROWS));
    tabd = e2tab + EXP2_N;
    for (int i = tid; i < EXP2_N; i += PWL_THREADS) e2tab[i] = a.m.e2tab[i];
    for (int i = tid; i < hdr_floats(K); i += PWL_THREADS) tabd[i] = a.m.tabd[i];
  }
  // The sampling direction at L = 2: the `first` spline from its inverse table where the builder has certified it.
  // The model-wide word is read once, as a scalar; the table is staged once per workgroup (it does not depend on the
  // slice; the first tile's barrier covers it).  Not certified, or switched off by the host: the closed form.
  constexpr bool FTAB = !TO_BASE && FAST && !PRECISE && LFIX == 2 && LROWS >= PWL_NPIECE && K == FT_K;
  [[maybe_unused]] bool use_ft = false;
  [[maybe_unused]] FtConsts fc{};
  if constexpr (FTAB) {
    if (a.ft)
      use_ft = __builtin_amdgcn_readfirstlane((int)reinterpret_cast<const uint32_t*>(a.ft)[FT_W_CERT]) == (int)FT_CERTIFIED;
    if (use_ft) {
      float* ftl = lds_raw + pwl_flow_lds_floats(K, LFIX, LROWS, false);
      ft_stage(ftl, a.ft, tid, PWL_THREADS);
      fc = ft_consts(ftl, sc);
    }
  }

  const int total = a.n_slices * a.tiles_per_slice;
  const int per_block = (total + gridDim.x - 1) / gridDim.x;
  const int t0 = blockIdx.x * per_block;
  const int t1 = t0 + per_block < total ? t0 + per_block : total;
  int cur = -1;
  // Tile geometry is wave-uniform (scalar registers): the slice, the tile's first sample and how many of its
  // PWL_TS samples exist.  A lane's share is then a 32-bit offset from a scalar base address, and a full tile
  // -- every tile but the last of a slice of odd size -- takes the unmasked path.
  // A block's tiles are contiguous: only its first tile's slice takes a division, each next tile steps (slice, ti).
  // `left`: the slice's samples from the tile's first one on, in 32 bits where the launch's slice length is below
  // 2^30 (`big` otherwise, a launch constant: every slice of such a launch, a short last one included, keeps tile_at
  // per tile): within a slice the next tile is then a handful of 32-bit scalar steps, and the 64-bit arithmetic of
  // tile_at runs once per slice.  No slice is longer than slice_len and a slice has fewer than slice_len / PWL_TS + 1
  // tiles, so `left` stays within (-2^30 - PWL_TS, 2^30) however far the steps go; it is clamped before it is
  // narrowed all the same.
  const bool big = a.slice_len >= ((int64_t)1 << 30);
  struct Tile { int slice; int ti; int valid; int left; int64_t g0; int64_t st0; int64_t gin; };
  auto tile_at = [&](int slice, int ti) {
    Tile t;
    t.slice = slice;
    t.ti = ti;
    const int64_t s0 = (int64_t)t.slice * a.slice_len;
    const int64_t len = a.B - s0 < a.slice_len ? a.B - s0 : a.slice_len;
    const int64_t jt = (int64_t)ti * PWL_TS;
    const int64_t left = len - jt;
    t.valid = left >= PWL_TS ? PWL_TS : (left > 0 ? (int)left : 0);
    t.left = big ? 0 : (int)(left < -(int64_t)PWL_TS ? -(int64_t)PWL_TS : left);
    t.g0 = s0 + jt;
    t.gin = a.in_shared ? jt : t.g0;
    t.st0 = a.first_sample + (int64_t)t.slice * a.slice_stride + jt;      // (seeded calls: the tile's first stream sample)
    return t;
  };
  auto tile_of = [&](int tile) { const int sl = tile / a.tiles_per_slice; return tile_at(sl, tile - sl * a.tiles_per_slice); };
  auto tile_next = [&](const Tile& t) {
    if (t.ti + 1 >= a.tiles_per_slice) return tile_at(t.slice + 1, 0);
    if (big) return tile_at(t.slice, t.ti + 1);
    Tile n = t;
    n.ti = t.ti + 1;
    n.left = t.left - PWL_TS;
    n.valid = n.left >= PWL_TS ? PWL_TS : (n.left > 0 ? n.left : 0);
    n.g0 = t.g0 + PWL_TS; n.gin = t.gin + PWL_TS; n.st0 = t.st0 + PWL_TS;
    return n;
  };
  const uint32_t lane2 = 2u * (uint32_t)tid;             // the lane's first sample within the tile
  // What the launch asks for is the same in every tile: bit 0 aux, bit 1 out, bit 2 aux is log_prob.
  const bool lp = a.aux_mode == AUX_LOGPROB;
  const int omode = (a.aux ? 1 : 0) | (a.out ? 2 : 0) | (lp ? 4 : 0);
  auto tile_points = [&](const Tile& t) {
    f4 x = {0.f, 0.f, 0.f, 0.f};
    if (SEEDED && !a.in) {   // the pair's four normals (one Philox block when the pair starts on an even sample)
      const uint64_t e0 = (uint64_t)(t.st0 + lane2) * 2u;
      if ((int)lane2 < t.valid) {
        if ((e0 & 3) == 0) {
          float z[4];
          philox_normals4(a.seed, e0 >> 2, z);
#pragma unroll
          for (int q = 0; q < 4; ++q) x[q] = z[q];
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) x[q] = normal_at(a.seed, e0 + q);
        }
        if ((int)lane2 + 1 >= t.valid) { x[2] = 0.f; x[3] = 0.f; }
      }
      return x;
    }
    const float* p = a.in + 2 * t.gin;
    if (t.valid == PWL_TS) return *reinterpret_cast<const f4*>(p + 2u * lane2);
    if ((int)lane2 + 1 < t.valid) x = *reinterpret_cast<const f4*>(p + 2u * lane2);
    else if ((int)lane2 < t.valid) { x[0] = p[2u * lane2]; x[1] = p[2u * lane2 + 1]; }
    // A partial tile's masked loads (a slice's last tile, once per slice at most) are waited for where they are
    // issued.  Left pending they reach the block where they merge with the full-tile load, and the compiler's
    // wait-count bookkeeping then guards the full tile's address computation with an s_waitcnt vmcnt(0) in front of
    // the prefetch: every wave waited there, once per tile, for the two stores it had issued a moment before.
    __builtin_amdgcn_s_waitcnt(PWL_WAIT_VM0);
    return x;
  };
  // The points of tile i + 1 are requested before tile i is computed: measured (r02e PMC) a wave spent half its
  // time in s_waitcnt, much of it on this one load issued right in front of its first use.
  [[maybe_unused]] f4 xn = {0.f, 0.f, 0.f, 0.f};
  Tile tn{};
  if (t0 < t1) { tn = tile_of(t0); xn = tile_points(tn); }
  f4 x = xn;
  // (the first tile's points, taken here: with the wait in tile_points alone the compiler puts a vmcnt(0) at the top
  // of the tile body, directly behind the prefetch -- worse than what it replaces; with both, the full-tile path has
  // one vmcnt wait per tile, the one in front of the stores below.  Read the assembly after any edit around here.)
  __builtin_amdgcn_s_waitcnt(PWL_WAIT_VM0);
  for (int tile = t0; tile < t1; ++tile) {
    const Tile tl = tn;
    const int slice = tl.slice;
    if (slice != cur) {
      __syncthreads();
      // (FTAB: the staging addresses are formed here, once per slice, from a lane index the compiler cannot see
      // through: hoisted out of the tile loop they are two registers the seeded instantiation has to spill)
      int stid = tid;
      if constexpr (FTAB) asm volatile("" : "+v"(stid));
      pwl_stage<LROWS>(tbl, a.tables + (int64_t)slice * L * PWL_TBL, L, stid, PWL_THREADS);
      cur = slice;
      __syncthreads();
    }
    const bool full = tl.valid == PWL_TS;
    if (tile + 1 < t1) { tn = tile_next(tl); xn = tile_points(tn); }
    __builtin_amdgcn_sched_barrier(0);
    v2f u0 = {x[0], x[2]}, u1 = {x[1], x[3]};
    [[maybe_unused]] v2f poison = splat<v2f>(0.0f);      // (flow_kernel: a NaN coordinate must come out as NaN)
    if constexpr (TO_BASE) poison = (u0 - u0) + (u1 - u1);

    // (pinned here: left to the compiler the base term is sunk to the end of the tile, which keeps the four input
    // registers live across the whole flow and costs four moves to re-pair them)
    v2f base = splat<v2f>(0.0f);
    if (!TO_BASE && lp && a.aux) base = (u0 * u0 + u1 * u1) * -0.5f - (float)(2 * HALF_LOG_2PI);
    if (!TO_BASE) asm volatile("" : "+v"(base));
    BaseAcc<v2f> bacc;
    v2f acc;
    if (FTAB && use_ft)      // wave-uniform (a scalar branch): the whole launch takes one side
      acc = flow2_tables<K, TO_BASE, FAST, PRECISE, true, LROWS, LFIX, true, FTAB>(tab, tbl, a.tables + (int64_t)slice * L * PWL_TBL, L, sc,
                                                              u0, u1, &a.m.scd, e2tab, tabd, &bacc, fc);
    else
      acc = flow2_tables<K, TO_BASE, FAST, PRECISE, true, LROWS, LFIX, true>(tab, tbl, a.tables + (int64_t)slice * L * PWL_TBL, L, sc,
                                                              u0, u1, &a.m.scd, e2tab, tabd, &bacc);
    // The next tile's points are taken BEFORE this tile's stores are issued: stores count in vmcnt, and a wait for
    // the points behind them is a wait for the stores' acknowledgement -- once per tile, with nothing to overlap it.
    // In front of them only the load and the previous tile's stores are outstanding; these stores drain under the
    // next tile's arithmetic.
    asm volatile("" : "+v"(xn));
    __builtin_amdgcn_sched_barrier(0);
    // has_aux / is_lp / has_out / whole: constants in the branch of a full tile of a call for both outputs (every
    // tile but a slice's last in the sampling calls), where the stores are then unconditional and lane validity
    // is not even formed; the launch's own values otherwise.
    auto emit = [&](bool has_aux, bool is_lp, bool has_out, bool whole) {
      const bool v0 = (int)lane2 < tl.valid, v1 = (int)lane2 + 1 < tl.valid;
      if (has_aux) {
        v2f r = acc;
        if constexpr (PRECISE) { if (is_lp) r = bacc.log_prob(acc, 2); }
        else if (is_lp)
          r = TO_BASE ? (u0 * u0 + u1 * u1) * -0.5f - (float)(2 * HALF_LOG_2PI) + acc : base - acc;
        if constexpr (TO_BASE) r += poison;
        float* q = a.aux + tl.g0;
        if (whole || v1) *reinterpret_cast<v2f*>(q + lane2) = r;
        else if (v0) q[lane2] = r.x;
      }
      if (has_out) {
        float* q = a.out + 2 * tl.g0;
        if constexpr (TO_BASE) { u0 += poison; u1 += poison; }
        if (whole || v1) *reinterpret_cast<f4*>(q + 2u * lane2) = f4{u0.x, u1.x, u0.y, u1.y};
        else if (v0) { q[2u * lane2] = u0.x; q[2u * lane2 + 1] = u1.x; }
      }
    };
    if (full && omode == 7) emit(true, true, true, true);
    else emit(a.aux != nullptr, lp, a.out != nullptr, full);
    x = xn;
  }
}

// ---------------------------------------------------------------------------
// loss_kernel: fused Monte-Carlo loss terms (cnf_ot/mfc/applications.py
// :129-374, cnf_ot/utils.py:311-389).  One tile of samples of one time-slice
// per workgroup iteration; several flow passes share the tile's base noise in
// LDS (the reference reuses one rng for them: applications.py:233-239); only
// one double per tile leaves the chip (atomicAdd into sums[slice]).
// LDS: [hdr][N noise][U][O][V velocity][R r3], each D x TS.
// ---------------------------------------------------------------------------
struct LossArgs {
  ModelArgs m;
  CnfLossSpec spec;
  const float* pts;     // base noise (or data points for NEG_LOGPROB, DENSITY_L2_DATA)
  const float* t;       // [n_slices]
  double* sums;         // [n_slices]
  int64_t B;            // samples per slice
  int64_t n_slices;
  int64_t pts_slice_stride;   // samples between slices in pts (0: shared draw)
  uint32_t div_magic;
  // pts == nullptr: base noise is generated in the kernel (Philox stream of
  // fill_normal_kernel): sample i of slice s is stream sample first_sample + s * pts_slice_stride + i
  uint64_t seed;
  int64_t first_sample;
  DensityMix mix;       // the density-error terms' mixture (density_mix_consts)
};

template <class T>
__device__ __forceinline__ void copy_cols(float* dst, const float* src, int D, int TS) {
  for (int d = 0; d < D; ++d) lds_put(dst, d, TS, lds_get<T>(src, d, TS));
}

__device__ __forceinline__ float mask_tail(float v, int64_t i, int64_t B) { return i < B ? v : 0.0f; }
__device__ __forceinline__ float mask_tail(v2f v, int64_t i, int64_t B) {
  return (i < B ? v.x : 0.0f) + (i + 1 < B ? v.y : 0.0f);
}

template <int H, int K, bool FAST, class T>
__global__ __launch_bounds__(TILE, 2) void loss_kernel(const LossArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int HDR = hdr_floats(K);
  constexpr int SPL = Lanes<T>::N;
  constexpr int TS = TILE * SPL;
  using M = Math<FAST>;
  const int D = a.m.D;
  float* tab = lds;
  float* Nn = lds + HDR;
  float* U = Nn + D * TS;
  float* O = U + D * TS;
  float* V = O + D * TS;
  float* R = V + D * TS;
  for (int i = threadIdx.x; i < HDR; i += TILE) tab[i] = a.m.prep[i];
  const int col = SPL * threadIdx.x;
  const int kind = a.spec.kind;

  const int64_t tiles_per_slice = (a.B + TS - 1) / TS;
  const int64_t n_tiles = tiles_per_slice * a.n_slices;
  SliceSum ssum;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t slice = tile / tiles_per_slice;
    const int64_t tile_start = (tile - slice * tiles_per_slice) * TS;
    const int64_t i = tile_start + col;
    __syncthreads();
    if (a.pts)
      tile_load<float>(a.pts + slice * a.pts_slice_stride * D, Nn, D, a.div_magic, TS, tile_start, a.B);
    else
      tile_noise(a.seed, (uint64_t)(a.first_sample + slice * a.pts_slice_stride + tile_start) * (uint64_t)D, Nn, D,
                 a.div_magic, TS, a.B - tile_start);
    const float t = a.t[slice];
    __syncthreads();

    // Each flow direction is instantiated ONCE (a pass is ~2.5k instructions;
    // one inlined copy per use would overflow the 64 KB instruction cache):
    // the base->data passes run in a loop over (condition, destination), the
    // data->base passes in a loop over (dimension, sign).
    T acc = splat<T>(0.0f);
    const float dt = a.spec.dt;
    const bool kin = kind <= CNF_TERM_FLOW_MATCHING;
    const bool data = kind == CNF_TERM_NEG_LOGPROB || kind == CNF_TERM_DENSITY_L2_DATA;    // points are data
    const int n_fwd = data ? 0 : (kind == CNF_TERM_KINETIC ? 2 : (kin ? 3 : 1));
    T fldj = splat<T>(0.0f);
    for (int p = 0; p < n_fwd; ++p) {
      const float c = !kin ? t : (p == 0 ? t - 0.5f * dt : (p == 1 ? t + 0.5f * dt : t));
      copy_cols<T>(U + col, Nn + col, D, TS);
      fldj = flow_pass<H, K, false, FAST, T>(a.m, tab, U, O, splat<T>(c));
      if (kin) {
        if (p == 0) copy_cols<T>(V + col, U + col, D, TS);                       // r1
        else if (p == 1) {                                                      // velocity = (r2 - r1)/dt
          const float inv_dt = 1.0f / dt;
          for (int d = 0; d < D; ++d)
            lds_put(V + col, d, TS, (lds_get<T>(U + col, d, TS) - lds_get<T>(V + col, d, TS)) * inv_dt);
        } else copy_cols<T>(R + col, U + col, D, TS);                            // r3
      }
    }
    if (kind == CNF_TERM_KINETIC) {
      acc = sq_norm<T>(lds_col<T>(V + col, TS), D);
    } else if (kind == CNF_TERM_POTENTIAL) {
      acc = potential<FAST, T>(lds_col<T>(U + col, TS), D, a.spec.subtype, a.spec.a).v;
    } else if (kind == CNF_TERM_REVERSE_KL) {
      const T lp = base_logprob<T>(lds_col<T>(Nn + col, TS), D) - fldj;
      acc = lp - rkl_mixture<FAST, T>(lds_col<T>(U + col, TS), D, t, a.spec.T, a.spec.beta).logmix;
    } else if (kind == CNF_TERM_DENSITY_L2) {
      const T lp = base_logprob<T>(lds_col<T>(Nn + col, TS), D) - fldj;
      acc = density_l2_residual<FAST, T>(lp, density_mixture<FAST, T>(lds_col<T>(U + col, TS), D, t, a.mix));
    }
    // data->base passes: NEG_LOGPROB / DENSITY_L2_DATA (one, on the points themselves) or the
    // central differences of log_prob at r3 +- dx/2 e_d (applications.py:264-273)
    const bool neg = data;
    const int n_tb = neg ? 1 : ((kind == CNF_TERM_KINETIC_SCORE || kind == CNF_TERM_FLOW_MATCHING) ? 2 * D : 0);
    const float dx = a.spec.dx;
    T lp0 = splat<T>(0.0f);
    for (int e = 0; e < n_tb; ++e) {
      const int d = e >> 1, sgn = e & 1;
      copy_cols<T>(U + col, (neg ? Nn : R) + col, D, TS);
      if (!neg) lds_put(U + col, d, TS, lds_get<T>(R + col, d, TS) + (sgn == 0 ? 0.5f * dx : -0.5f * dx));
      // (the mixture at the data point waits in the unused velocity column: nothing more is live across the pass)
      if (kind == CNF_TERM_DENSITY_L2_DATA)
        lds_put(V + col, 0, TS, density_mixture<FAST, T>(lds_col<T>(Nn + col, TS), D, t, a.mix));
      const T ildj = flow_pass<H, K, true, FAST, T>(a.m, tab, U, O, splat<T>(t));
      const T lp = base_logprob<T>(lds_col<T>(U + col, TS), D) + ildj;
      if (kind == CNF_TERM_DENSITY_L2_DATA) acc = density_l2_residual<FAST, T>(lp, lds_get<T>(V + col, 0, TS));
      else if (neg) acc = -lp;
      else if (sgn == 0) lp0 = lp;
      else {
        const T dr = drift_field<T>(lds_col<T>(R + col, TS), d, kind == CNF_TERM_FLOW_MATCHING ? a.spec.subtype : -1, a.spec.a);
        const T u = score_residual(lds_get<T>(V + col, d, TS), (lp0 - lp) * (1.0f / dx), a.spec.coef, dr);
        acc = vfma(u, u, acc);
      }
    }
    // tile reduction: lanes -> wave (shuffles) -> the wave's running sum of the slice
    float part = mask_tail(acc, i, a.B);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    ssum.add(a.sums, slice, part);
  }
  ssum.flush(a.sums);
}


// ---------------------------------------------------------------------------
// fields_kernel: the arrays under the reference's figures (cnf_ot/utils.py:598-798, solvers.py:309-493) -- density,
// log-density, velocity and score at fixed points of data space, and the characteristics through given start points
// with the velocity along them -- for S times in one launch.  One tile of 256 points of one time per workgroup
// iteration, one point per lane.  Per (time, point): one data -> base pass (at the slice's own time, or at t0 for
// trajectories) leaves the base point xi in LDS; the base -> data passes at t (trajectory) and t -+ dt/2 (velocity)
// start from that copy; the score takes 2 D plain-fp32 data -> base passes at r +- dx/2 e_d (as cnf_logprob_fd: the
// precise position path would only be cancelled by the difference).  The points of a regular 2-D grid are generated
// here from (lo, step, nx): index i nx + j is (x_j, y_i), the reference's meshgrid + hstack; several sections along a
// third axis are averaged in a fixed order inside the thread (plot_proj_density's prob / len(section)).  Each flow
// direction is instantiated once per use (loops over the passes), as in loss_kernel.
// LDS: [hdr][P points][U][O][X xi][V result], each D x TILE; float32: + [LO][2^(-i/32) table][float64 `first` table].
// ---------------------------------------------------------------------------
template <class R> struct FieldArgsT {
  ModelArgs m;
  const R* pts;          // [N, D] explicit points, or null: the grid below
  const R* t;            // [S]
  const R* fixed;        // grid: [D] values of the coordinates the grid does not span
  const R* sec;          // grid: [n_sec] values of coordinate sec_axis, or null
  R* rho;                // [S, N]     mean over sections of exp(log_prob), or null
  R* logp;               // [S, N]     or null
  R* vel;                // [S, N, D]  or null
  R* score;              // [S, N, D]  or null
  R* traj;               // [S, N, D]  or null
  double lo_x, lo_y, step_x, step_y;
  int64_t N, S;
  int32_t nx, axis_x, axis_y, sec_axis, n_sec;
  int32_t fixed_base;    // trajectories: the data -> base pass runs at t0, not at the slice's time
  int32_t slice_chunk;   // slices one workgroup iteration walks (fixed_base: they share the data -> base pass)
  R t0, dt, dx;
  uint32_t div_magic;
};

template <class T>
__device__ __forceinline__ void field_copy(typename Lanes<T>::real* dst, const typename Lanes<T>::real* src, int D) {
  for (int d = 0; d < D; ++d) lds_put(dst, d, TILE, lds_get<T>(src, d, TILE));
}
// v - v summed over the coordinates: 0 for a finite point, NaN otherwise (see flow_kernel)
template <class T>
__device__ __forceinline__ T field_poison(const typename Lanes<T>::real* col, int D) {
  T p = (T)0;
  for (int d = 0; d < D; ++d) { const T v = lds_get<T>(col, d, TILE); p += v - v; }
  return p;
}

template <int H, int K, bool FAST, class T>
__global__ __launch_bounds__(TILE, 2) void fields_kernel(const FieldArgsT<T> a) {
  static_assert(Lanes<T>::N == 1, "one point per lane");
  typedef T R;
  constexpr bool PR = std::is_same<T, float>::value;      // the density pass of the float32 kernel: precise positions
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);
  constexpr int HDR = hdr_floats(K);
  constexpr int TS = TILE;
  const int D = a.m.D;
  R* tab = lds;
  R* P = lds + HDR;
  R* U = P + D * TS;
  R* O = U + D * TS;
  R* X = O + D * TS;
  R* V = X + D * TS;
  for (int i = threadIdx.x; i < HDR; i += TILE) tab[i] = table_of<R>(a.m)[i];
  [[maybe_unused]] double* e2tab = nullptr;
  [[maybe_unused]] double* tabd = nullptr;
  [[maybe_unused]] R* LO = nullptr;
  if constexpr (PR) {                                      // HDR, D * TS are multiples of 4 floats: 8-byte aligned
    LO = V + D * TS;
    e2tab = reinterpret_cast<double*>(LO + D * TS);
    tabd = e2tab + EXP2_N;
    for (int i = threadIdx.x; i < EXP2_N; i += TILE) e2tab[i] = a.m.e2tab[i];
    for (int i = threadIdx.x; i < HDR; i += TILE) tabd[i] = a.m.tabd[i];
  }
  const int col = threadIdx.x;
  const bool want_xi = a.vel || a.traj;
  const bool want_base = want_xi || a.rho || a.logp;
  const R half_dt = (R)0.5 * a.dt, inv_dt = (R)1 / a.dt, half_dx = (R)0.5 * a.dx, inv_dx = (R)1 / a.dx;

  const int64_t tiles = (a.N + TS - 1) / TS;
  const int64_t chunks = (a.S + a.slice_chunk - 1) / a.slice_chunk;
  for (int64_t item = blockIdx.x; item < tiles * chunks; item += gridDim.x) {
    const int64_t chunk = item / tiles;
    const int64_t tile_start = (item - chunk * tiles) * TS;
    const int64_t i = tile_start + col;
    const int64_t s0 = chunk * a.slice_chunk, s1 = s0 + a.slice_chunk < a.S ? s0 + a.slice_chunk : a.S;
    __syncthreads();                                       // the previous item's stores are done with U / V
    if (a.pts) {
      tile_load<R>(a.pts, P, D, a.div_magic, TS, tile_start, a.N);
    } else {
      const int64_t n = i < a.N ? i : 0;
      const int64_t iy = n / a.nx, ix = n - iy * a.nx;
      for (int d = 0; d < D; ++d) lds_put(P + col, d, TS, a.fixed[d]);
      if (a.sec) lds_put(P + col, a.sec_axis, TS, a.sec[0]);
      // numpy.linspace's own arithmetic: a product and a sum, each rounded (no fused multiply-add)
      lds_put(P + col, a.axis_x, TS, (R)__dadd_rn(__dmul_rn((double)ix, a.step_x), a.lo_x));
      lds_put(P + col, a.axis_y, TS, (R)__dadd_rn(__dmul_rn((double)iy, a.step_y), a.lo_y));
    }
    __syncthreads();

    T poison = (T)0;
    for (int64_t s = s0; s < s1; ++s) {
      const R ts = a.t[s];
      if (want_base && (s == s0 || !a.fixed_base)) {
        double rho_acc = 0.0;
        T lp = (T)0;
        for (int k = 0; k < a.n_sec; ++k) {
          field_copy<T>(U + col, P + col, D);
          if (a.sec) lds_put(U + col, a.sec_axis, TS, a.sec[k]);
          poison = field_poison<T>(U + col, D);
          BaseAcc<T> bacc;
          const T ildj = flow_pass<H, K, true, FAST, T, false, PR>(a.m, tab, U, O, a.fixed_base ? a.t0 : ts, e2tab, tabd,
                                                                   LO, &bacc);
          if constexpr (PR) lp = bacc.log_prob(ildj, D) + poison;
          else lp = base_logprob<T>(lds_col<T>(U + col, TS), D) + ildj + poison;
          rho_acc += exp((double)lp);
        }
        if (want_xi) field_copy<T>(X + col, U + col, D);
        if (a.logp && i < a.N) a.logp[s * a.N + i] = lp;
        if (a.rho && i < a.N) a.rho[s * a.N + i] = (R)(rho_acc / (double)a.n_sec);
      }
      // base -> data from xi: at t (the trajectory), then at t - dt/2 and t + dt/2 (the velocity)
      const int n_fwd = (a.traj ? 1 : 0) + (a.vel ? 2 : 0);
      for (int p = 0; p < n_fwd; ++p) {
        const int q = p - (a.traj ? 1 : 0);               // -1: trajectory, 0 / 1: the velocity's two ends
        const R c = q < 0 ? ts : (q == 0 ? ts - half_dt : ts + half_dt);
        field_copy<T>(U + col, X + col, D);
        (void)flow_pass<H, K, false, FAST, T>(a.m, tab, U, O, c);
        if (q == 0) { field_copy<T>(V + col, U + col, D); continue; }
        for (int d = 0; d < D; ++d) {
          const T r = lds_get<T>(U + col, d, TS);
          lds_put(V + col, d, TS, q < 0 ? r + poison : (r - lds_get<T>(V + col, d, TS)) * inv_dt + poison);
        }
        __syncthreads();
        tile_store<R>((q < 0 ? a.traj : a.vel) + s * a.N * D, V, D, a.div_magic, TS, tile_start, a.N);
        __syncthreads();
      }
      if (a.score) {
        T lp0 = (T)0;
        for (int e = 0; e < 2 * D; ++e) {
          const int d = e >> 1, sgn = e & 1;
          field_copy<T>(U + col, P + col, D);
          lds_put(U + col, d, TS, lds_get<T>(P + col, d, TS) + (sgn == 0 ? half_dx : -half_dx));
          const T ps = field_poison<T>(U + col, D);
          const T ildj = flow_pass<H, K, true, FAST, T>(a.m, tab, U, O, ts);
          const T lp = base_logprob<T>(lds_col<T>(U + col, TS), D) + ildj;
          if (sgn == 0) lp0 = lp;
          else lds_put(V + col, d, TS, (lp0 - lp) * inv_dx + ps);
        }
        __syncthreads();
        tile_store<R>(a.score + s * a.N * D, V, D, a.div_magic, TS, tile_start, a.N);
        __syncthreads();
      }
    }
  }
}


// ---------------------------------------------------------------------------
// loss_pwl_kernel: the fused loss terms at dim 2 on the conditioner tables.
// Same terms and arithmetic as loss_kernel; a sample pair lives in registers,
// the passes of a term use up to three table sets (conditions t - dt/2,
// t + dt/2, t), each L x 22 KB in LDS.  Base noise comes from `pts` or from the
// Philox stream (one counter block = the pair's four normals when aligned).
// ---------------------------------------------------------------------------
struct LossPwlArgs {
  ModelArgs m;
  CnfLossSpec spec;
  const float* pts;
  const float* t;
  double* sums;
  const float* tables;        // [n_sets][n_slices][L][PWL_TBL]
  int64_t B, n_slices, pts_slice_stride;
  uint64_t seed;
  int64_t first_sample;
  int32_t n_sets, tiles_per_slice;
  DensityMix mix;             // the density-error terms' mixture (density_mix_consts)
};

template <int K, bool FAST>
__global__ __launch_bounds__(PWL_MAX_THREADS) void loss_pwl_kernel(const LossPwlArgs a) {
  using M = Math<FAST>;
  typedef v2f T;
  const int NT = blockDim.x, TS = 2 * NT;
  extern __shared__ __attribute__((aligned(16))) float lds_raw[];
  constexpr int HDR = (hdr_floats(K) + 3) & ~3;
  const int tid = threadIdx.x;
  const int L = a.m.L;
  float* tab = lds_raw;
  float* tbl = lds_raw + HDR;                               // n_sets x L tables
  float* R = tbl + a.n_sets * L * PWL_LTBL;                 // 2 x TS scratch columns: r3 for drift_field (registers spill)
  for (int i = tid; i < hdr_floats(K); i += NT) tab[i] = table_of<float>(a.m)[i];
  const SplineConsts sc = sc_scalars(sc_of<float>(a.m));
  const int kind = a.spec.kind;
  const bool kin = kind <= CNF_TERM_FLOW_MATCHING;
  const float dt = a.spec.dt, dx = a.spec.dx;
  const int64_t set_stride = a.n_slices * L * (int64_t)PWL_TBL;
  const int col = 2 * tid;

  const int total = (int)a.n_slices * a.tiles_per_slice;
  const int per_block = (total + gridDim.x - 1) / gridDim.x;
  const int t0 = blockIdx.x * per_block;
  const int t1 = t0 + per_block < total ? t0 + per_block : total;
  int cur = -1;
  SliceSum ssum;
  for (int tile = t0; tile < t1; ++tile) {
    const int slice = tile / a.tiles_per_slice;
    __syncthreads();                                        // the previous tile is done with R (and the tables)
    if (slice != cur) {
      for (int s = 0; s < a.n_sets; ++s)
        pwl_stage(tbl + s * L * PWL_LTBL, a.tables + s * set_stride + (int64_t)slice * L * PWL_TBL, L, tid, NT);
      cur = slice;
      __syncthreads();
    }
    const float* gslice = a.tables + (int64_t)slice * L * PWL_TBL;
    const int64_t j = (int64_t)(tile - slice * a.tiles_per_slice) * TS + col;
    const bool v0 = j < a.B, v1 = j + 1 < a.B;
    const float t = a.t[slice];
    // the pair's points: x = (n0.x, n1.x), y = (n0.y, n1.y)
    f4 x = {0.f, 0.f, 0.f, 0.f};
    const int64_t g = slice * a.pts_slice_stride + j;       // sample index in pts / offset in the stream
    if (a.pts) {
      const float* src = a.pts + 2 * g;
      if (v1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) x = *reinterpret_cast<const f4*>(src);
      else { if (v0) { x[0] = src[0]; x[1] = src[1]; } if (v1) { x[2] = src[2]; x[3] = src[3]; } }
    } else {
      const uint64_t e0 = (uint64_t)(a.first_sample + g) * 2u;
      if ((e0 & 3) == 0) {                                  // one Philox block holds the pair
        float z[4];
        philox_normals4(a.seed, e0 >> 2, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = z[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = normal_at(a.seed, e0 + q);
      }
      if (!v0) { x[0] = 0.f; x[1] = 0.f; }
      if (!v1) { x[2] = 0.f; x[3] = 0.f; }
    }
    const T n0 = {x[0], x[2]}, n1 = {x[1], x[3]};
    auto n = [&](int q) { return q == 0 ? n0 : n1; };

    T acc = splat<T>(0.0f);
    const bool data = kind == CNF_TERM_NEG_LOGPROB || kind == CNF_TERM_DENSITY_L2_DATA;    // points are data
    const int n_fwd = data ? 0 : (kind == CNF_TERM_KINETIC ? 2 : (kin ? 3 : 1));
    T fldj = splat<T>(0.0f);
    T y0 = n0, y1 = n1, va = splat<T>(0.0f), vb = splat<T>(0.0f);     // (va, vb): r1, then the velocity
    auto y = [&](int q) { return q == 0 ? y0 : y1; };
    for (int p = 0; p < n_fwd; ++p) {                                  // set p: conditions t - dt/2, t + dt/2, t (kin) or t
      y0 = n0; y1 = n1;
      fldj = flow2_tables<K, false, FAST, false, true>(tab, tbl + p * L * PWL_LTBL, gslice + p * set_stride, L, sc, y0, y1);
      if (kin) {
        if (p == 0) { va = y0; vb = y1; }
        else if (p == 1) { const float inv_dt = 1.0f / dt; va = (y0 - va) * inv_dt; vb = (y1 - vb) * inv_dt; }
      }
    }
    const int tset = kin ? 2 : 0;                                       // the set of condition t
    if (kind == CNF_TERM_KINETIC) {
      acc = vfma(va, va, vb * vb);
    } else if (kind == CNF_TERM_POTENTIAL) {
      acc = potential<FAST, T>(y, 2, a.spec.subtype, a.spec.a).v;
    } else if (kind == CNF_TERM_REVERSE_KL) {
      acc = base_logprob<T>(n, 2) - fldj - rkl_mixture<FAST, T>(y, 2, t, a.spec.T, a.spec.beta).logmix;
    } else if (kind == CNF_TERM_DENSITY_L2) {
      acc = density_l2_residual<FAST, T>(base_logprob<T>(n, 2) - fldj,
                                         density_mixture<FAST, T>(y, 2, t, a.mix));
    }
    // data->base passes: NEG_LOGPROB / DENSITY_L2_DATA (one, on the points themselves) or the central differences of
    // log_prob at r3 +- dx/2 e_d (applications.py:264-273); r3 = (y0, y1) of the pass at condition t
    const bool neg = data;
    const int n_tb = neg ? 1 : ((kind == CNF_TERM_KINETIC_SCORE || kind == CNF_TERM_FLOW_MATCHING) ? 4 : 0);
    if (kind == CNF_TERM_FLOW_MATCHING) { lds_put(R + col, 0, TS, y0); lds_put(R + col, 1, TS, y1); }
    T lp0 = splat<T>(0.0f);
    for (int e = 0; e < n_tb; ++e) {
      const int d = e >> 1, sgn = e & 1;
      T u0 = neg ? n0 : y0, u1 = neg ? n1 : y1;
      if (!neg) {
        const float h = sgn == 0 ? 0.5f * dx : -0.5f * dx;
        if (d == 0) u0 = u0 + h; else u1 = u1 + h;
      }
      // (the mixture at the data point waits in the scratch columns: nothing more is live across the pass)
      if (kind == CNF_TERM_DENSITY_L2_DATA) lds_put(R + col, 0, TS, density_mixture<FAST, T>(n, 2, t, a.mix));
      const T ildj = flow2_tables<K, true, FAST, false, true>(tab, tbl + tset * L * PWL_LTBL, gslice + tset * set_stride, L, sc, u0, u1);
      const T lp = base_logprob<T>([&](int q) { return q == 0 ? u0 : u1; }, 2) + ildj;
      if (kind == CNF_TERM_DENSITY_L2_DATA) acc = density_l2_residual<FAST, T>(lp, lds_get<T>(R + col, 0, TS));
      else if (neg) acc = -lp;
      else if (sgn == 0) lp0 = lp;
      else {
        const T dr = drift_field<T>(lds_col<T>(R + col, TS), d, kind == CNF_TERM_FLOW_MATCHING ? a.spec.subtype : -1, a.spec.a);
        const T u = score_residual(d == 0 ? va : vb, (lp0 - lp) * (1.0f / dx), a.spec.coef, dr);
        acc = vfma(u, u, acc);
      }
    }
    // tile reduction: lanes -> wave (shuffles) -> the wave's running sum of the slice
    float part = (v0 ? acc.x : 0.0f) + (v1 ? acc.y : 0.0f);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    ssum.add(a.sums, slice, part);
  }
  ssum.flush(a.sums);
}

}  // namespace cnf

// ===========================================================================
// C ABI
// ===========================================================================
using namespace cnf;

void first_table_enqueue(CnfModel* m, hipStream_t stream) {
  hipLaunchKernelGGL(first_table_kernel<FT_K>, dim3(FT_BLOCKS), dim3(32 * FT_PPB), 0, stream,
                     reinterpret_cast<const double*>(m->prep + m->tabd_off), m->prep + m->ft_off,
                     (double)m->cfg.range_min, (double)m->cfg.range_max);
  m->ft_built = 1;
  m->ft_wanted = 1;
}

extern "C" int cnf_model_set_params(CnfModel* m, const float* params, void* stream) {
  if (!m || !params) return CNF_ERR_INVALID;
  const int K = m->cfg.num_bins;
  const int64_t n_w = m->n_params - (3 * K + 1);
  int blocks = (int)((n_w + 255) / 256);
  if (blocks < 1) blocks = 1;
  if (blocks > 256) blocks = 256;
  blocks += 1;                                  // (+ the block that normalises the `first` spline)
  hipLaunchKernelGGL(prepare_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, params, m->prep, K,
                     m->n_params, (double)m->cfg.range_min, (double)m->cfg.range_max,
                     (double)m->cfg.min_bin_size, (double)m->cfg.min_knot_slope, m->cfg.dim,
                     m->cfg.num_layers, m->cfg.mlp_num_layers, m->per_layer, m->per_layer_q, m->mfma_off,
                     m->tabd_off, m->cfg.hidden_size, m->cfg.periodized, m->ft_off);
  if (m->cfg.periodized && m->cfg.dim > 1)
    hipLaunchKernelGGL(circular_slopes_kernel, dim3((unsigned)(m->cfg.num_layers * (m->cfg.dim - 1))), dim3(64), 0,
                       (hipStream_t)stream, params, m->prep, K, m->cfg.hidden_size, m->cfg.dim, m->cfg.num_layers,
                       m->cfg.mlp_num_layers, m->per_layer);
  // The `first` spline's inverse table (cnf_first_table.h), behind prepare_kernel, which has cleared its status words,
  // and in front of the event: wait_for_params covers it.  Only for a model whose launches have asked for the table
  // (run_flow_pwl builds the first one itself): the captured default training step is 0.076 ms of kernels, and a
  // 9 us builder behind every parameter load of a model that never samples through the table kernel would be a
  // tenth of it.
  if (m->ft_off > 0) {
    m->ft_built = 0;
    if (m->ft_wanted && pwl_config_ok(m)) first_table_enqueue(m, (hipStream_t)stream);
  }
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  // (inside a stream capture the record would become a graph node and leave the event unusable outside the graph:
  //  a captured step is ordered by its own stream)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
  if (cap == hipStreamCaptureStatusNone && hipEventRecord(m->prep_event, (hipStream_t)stream) != hipSuccess) return CNF_ERR_HIP;
  m->prep_stream = stream;
  m->params_set = 1;
  return CNF_OK;
}


constexpr int CNF_MFMA_SMALL_WAVES = 4;        // waves of single-lane work per SIMD up to which use_mfma = 2 picks MFMA

// Two samples per lane (packed fp32) once the batch fills every SIMD with at
// least one wave of sample pairs; one sample per lane below that.
static int samples_per_lane(const CnfModel* m, int64_t B) {
  if (m->force_spl == 1 || m->force_spl == 2) return m->force_spl;
  // the small-launch regime of the MFMA conditioner (launch_flow) is one sample per lane
  if (m->use_mfma == 2 && m->mfma_off > 0 && m->cfg.hidden_size == 16 && m->cfg.num_bins == 5 &&
      B <= (int64_t)m->num_cus * 4 * 64 * CNF_MFMA_SMALL_WAVES) return 1;
  return (m->fast_math && B >= (int64_t)m->num_cus * 4 * 64 * 2) ? 2 : 1;
}

// (the one tail of every kernel family's launch, `launch`, and its profiling scope: cnf_common.h)
typedef void (*FlowKernel)(const FlowArgs);

// flow_dpar_kernel: D >= 3, base -> data, packed-VALU conditioner, hardware transcendentals.  Chosen (use_dpar
// = 1) while the one-sample-per-lane kernel would leave the chip under-filled.
static int launch_flow_dpar(CnfModel* m, const FlowArgs& a, hipStream_t stream) {
  const int D = m->cfg.dim;
  if (D < 3 || !m->fast_math || m->use_mfma == 1 || !m->use_dpar || m->cfg.periodized) return CNF_ERR_UNSUPPORTED;
  // measured crossover with the one-sample-per-lane kernel (MI355X, D = 3 and D = 10, scripts/exp_dim10.py):
  // between 131 072 and 524 288 samples; 512 samples per CU
  if (m->use_dpar == 1 && a.B > (int64_t)m->num_cus * 512) return CNF_ERR_UNSUPPORTED;
  int nw = D - 1;
  if (nw > 16) nw = 16;
  const int spl = (m->force_spl == 1 || m->force_spl == 2) ? m->force_spl : (a.B >= (int64_t)m->num_cus * 128 ? 2 : 1);
  const int64_t ts = 64 * spl;
  const size_t lds = (size_t)(hdr_floats(m->cfg.num_bins) + (2 * D + nw) * ts) * sizeof(float);
  if (lds > 64 * 1024) return CNF_ERR_UNSUPPORTED;
  int64_t grid = (a.B + ts - 1) / ts;
  const int64_t cap = (int64_t)m->num_cus * 8;
  if (grid > cap) grid = cap;
  return with_shape(m->cfg, [&](auto h, auto k) -> int {
    constexpr int H = decltype(h)::value, K = decltype(k)::value;
    const FlowKernel kern = spl == 2 ? flow_dpar_kernel<H, K, true, v2f> : flow_dpar_kernel<H, K, true, float>;
    return launch(m, kern, grid, 64 * nw, lds, stream, a, CNF_PATH_DPAR, a.gate != nullptr, a.B);
  });
}

// LDS of the precise position path beyond the tile: the 2^(-i/32) table and the float64 `first` table
static size_t precise_lds_bytes(int K) { return sizeof(double) * (size_t)(cnf::EXP2_N + hdr_floats(K)); }

// flow_kernel's instantiation for a launch, each selection written once.  `precise` is honoured for TO_BASE alone:
// the precise position path exists for the data -> base direction.
// The packed-VALU conditioner of shape (H, K):
template <int H, int K, bool TO_BASE, bool PRECISE = false>
static FlowKernel flow_kernel_of(bool precise, bool fast, int spl) {
  if constexpr (TO_BASE && !PRECISE)
    if (precise) return flow_kernel_of<H, K, true, true>(true, fast, spl);
  if (!fast) return flow_kernel<H, K, TO_BASE, false, float, false, PRECISE>;
  return spl == 2 ? flow_kernel<H, K, TO_BASE, true, v2f, false, PRECISE>
                  : flow_kernel<H, K, TO_BASE, true, float, false, PRECISE>;
}
// The MFMA conditioner (H = 16, K = 5, hardware transcendentals).  d2: dim 2 at one sample per lane, the reference's
// per-batch call pattern, has its own instantiation.
template <bool TO_BASE, bool PRECISE = false>
static FlowKernel flow_mfma_kernel_of(bool precise, int spl, bool d2) {
  if constexpr (TO_BASE && !PRECISE)
    if (precise) return flow_mfma_kernel_of<true, true>(true, spl, d2);
  if (spl == 2) return flow_kernel<16, 5, TO_BASE, true, v2f, true, PRECISE>;
  return d2 ? flow_kernel<16, 5, TO_BASE, true, float, true, PRECISE, false, 2>
            : flow_kernel<16, 5, TO_BASE, true, float, true, PRECISE>;
}

template <bool TO_BASE>
static int launch_flow(CnfModel* m, const FlowArgs& a, int spl, hipStream_t stream) {
  const int64_t ts = (int64_t)TILE * spl;
  const int64_t n_tiles = (a.B + ts - 1) / ts;
  int64_t grid = n_tiles;
  const int64_t cap = (int64_t)m->num_cus * 8;
  if (grid > cap) grid = cap;
  const bool gated = a.gate != nullptr;
  if (m->cfg.periodized) {
    // RQSFlow(periodized=True): one sample per lane, hardware transcendentals, plain fp32 positions; sin / cos of
    // the conditioner inputs by ocml.  (fast_math off: the float64 entry points are the exact mode.)
    if (!m->fast_math) return CNF_ERR_UNSUPPORTED;
    const int64_t tiles1 = (a.B + TILE - 1) / TILE;
    const int64_t grid1 = tiles1 < cap ? tiles1 : cap;
    const size_t lds1 = (size_t)(hdr_floats(m->cfg.num_bins) + 2 * a.m.D * TILE) * sizeof(float);
    return with_shape(m->cfg, [&](auto h, auto k) -> int {
      constexpr int H = decltype(h)::value, K = decltype(k)::value;
      return launch(m, flow_kernel<H, K, TO_BASE, true, float, false, false, true>, grid1, TILE, lds1, stream, a,
                    CNF_PATH_MLP1, gated);
    });
  }
  const bool precise = TO_BASE && m->precise;
  const size_t lds = (size_t)(hdr_floats(m->cfg.num_bins) + 2 * a.m.D * ts) * sizeof(float) +
                     (precise ? precise_lds_bytes(m->cfg.num_bins) + sizeof(float) * a.m.D * ts : 0);
  // launches of up to 4 waves of single-lane work per SIMD: the MFMA conditioner, one sample per lane (measured
  // crossover with the packed-VALU kernel, dim 2 and dim 10: profiles/r02_experiments/exp_latency.log)
  const bool small = a.B <= (int64_t)m->num_cus * 4 * 64 * CNF_MFMA_SMALL_WAVES;
  if (m->fast_math && (m->use_mfma == 1 || (m->use_mfma == 2 && small)) && m->mfma_off > 0 &&
      m->cfg.hidden_size == 16 && m->cfg.num_bins == 5)
    return launch(m, flow_mfma_kernel_of<TO_BASE>(precise, spl, m->cfg.dim == 2 && spl == 1), grid, TILE, lds, stream, a,
                  CNF_PATH_MFMA, gated, a.B);
  return with_shape(m->cfg, [&](auto h, auto k) -> int {
    constexpr int H = decltype(h)::value, K = decltype(k)::value;
    return launch(m, flow_kernel_of<H, K, TO_BASE>(precise, m->fast_math != 0, spl), grid, TILE, lds, stream, a,
                  spl == 2 ? CNF_PATH_MLP2 : CNF_PATH_MLP1, gated, a.B);
  });
}

// How a call on the tables walks its slices: `chunk` slices per build + kernel pair, `tps` tiles per slice, on the
// stream's workspace `tables`.
struct SlicePlan { int64_t tps, chunk; float* tables; };

// The plan for n_slices slices of slice_len points in tiles of `tile` points, each slice taking sets_per_slice table
// sets; CNF_ERR_UNSUPPORTED when the call does not qualify (the caller then runs the MLP kernel).  No HIP call.
static int slice_plan(CnfModel* m, hipStream_t stream, int64_t slice_len, int64_t n_slices, int64_t tile,
                      int sets_per_slice, SlicePlan* p) {
  const int64_t PWL_MAX_SLICES = 2048;      // slices per build + kernel pair
  p->tps = (slice_len + tile - 1) / tile;
  const int64_t total = n_slices * p->tps;
  if (total > (1 << 30)) return CNF_ERR_UNSUPPORTED;
  // the tables cost one small kernel per launch: worth it once every CU has a tile,
  // and only while a slice is long enough to amortise building its tables
  // (crossover with the MLP kernel: B / 26 G/s = 20 us of table building + B / 62 G/s  ->  B ~ 0.9 M samples)
  if (m->use_pwl == 1 && (total < 2 * (int64_t)m->num_cus || slice_len < 4 * tile)) return CNF_ERR_UNSUPPORTED;
  // at most PWL_MAX_SLICES slices per kernel pair: the workspace stays bounded (2 048 x L x 48 KB) however many
  // slices a call has
  p->chunk = n_slices < PWL_MAX_SLICES ? n_slices : PWL_MAX_SLICES;
  // the stream's reservation decides: none (or one too small to keep every CU busy) -> the MLP kernel
  int64_t sets = 0;
  pwl_workspace(m, stream, &p->tables, &sets);
  if (sets / sets_per_slice < p->chunk) p->chunk = sets / sets_per_slice;
  if (p->chunk < 1) return CNF_ERR_UNSUPPORTED;
  if (m->use_pwl == 1 && p->chunk < n_slices && p->chunk * p->tps < (int64_t)m->num_cus) return CNF_ERR_UNSUPPORTED;
  return CNF_OK;
}

// Enqueues the tables of ns slices, conditions c[0 .. ns) + offset, into `tables`
// with the lean builder (one wave per table) from PWL_LEAN_MIN_TABLES tables up, below it the reference builder (512
// threads per table); cnf_model_set_pwl_builder forces either.  Both write the same bytes.
// A lone wave takes ~30 us for its table, with 16 tables in flight per CU (one round up to 4 096 tables); the
// reference builder takes ~11 us per round of 2 tables per CU, 512 tables: 10.6 us against ~30 at 32 and 96 tables,
// 13 against ~32 at 512, 36 against 39 at 1 536, 46 against 41 at 2 048, 89 against 56 at 4 096 (measured: profiles/r06_lean_builder has both
// builders from 32 to 4 096 tables).  The sampling step's chunks (4 096 and 3 616 tables) are above the crossover, the
// loss and backward paths (32 - 96) below.
constexpr int64_t PWL_LEAN_MIN_TABLES = 2048;
static void build_tables(CnfModel* m, hipStream_t stream, const float* c, float offset, int64_t ns, float* tables) {
  const int L = m->cfg.num_layers;
  const float* w = m->prep + cnf::hdr_floats(5);
  const bool lean = m->pwl_builder == 0 ? ns * L >= PWL_LEAN_MIN_TABLES : m->pwl_builder != 1;
  m->last_pwl_builder = lean ? 2 : 1;
  const dim3 grid((unsigned)(ns * L));
  if (!lean)
    hipLaunchKernelGGL(cnf::pwl_build_kernel, grid, dim3(512), 0, stream, w, m->per_layer, c, offset, L,
                       m->scd.sp_offset, tables);
  else
    hipLaunchKernelGGL(cnf::pwl_build_lean_kernel<64>, grid, dim3(64), 0, stream, w, m->per_layer, c, offset, L,
                       m->scd.sp_offset, tables);
}

typedef void (*PwlKernel)(const cnf::PwlArgs);

// flow_pwl_kernel's instantiation for a launch.  full: every row of the L tables is in LDS, else the first PWL_LROWS
// rows; l2: L = 2 (every configuration of the reference), full, has its own instantiation with the layer loop unrolled
template <bool TO_BASE, bool PRECISE, bool SEEDED>
static PwlKernel flow_pwl_kernel_of(bool full, bool l2) {
  constexpr int ALL = cnf::PWL_NPIECE, WIN = cnf::PWL_LROWS;
  if (l2) return cnf::flow_pwl_kernel<5, TO_BASE, true, PRECISE, ALL, 2, SEEDED>;
  return full ? cnf::flow_pwl_kernel<5, TO_BASE, true, PRECISE, ALL, 0, SEEDED>
              : cnf::flow_pwl_kernel<5, TO_BASE, true, PRECISE, WIN, 0, SEEDED>;
}
// precise: the precise position path (data -> base); seeded: base noise drawn in the kernel (base -> data)
static PwlKernel flow_pwl_kernel_of(bool to_base, bool precise, bool seeded, bool full, bool l2) {
  if (precise) return flow_pwl_kernel_of<true, true, false>(full, l2);
  if (to_base) return flow_pwl_kernel_of<true, false, false>(full, l2);
  return seeded ? flow_pwl_kernel_of<false, false, true>(full, l2) : flow_pwl_kernel_of<false, false, false>(full, l2);
}

// The piecewise-linear path (cnf_pwl.h): dim 2, H = 16, K = 5, two MLP layers, a condition that is
// uniform over slices of even length, 16-byte aligned points.  Returns CNF_ERR_UNSUPPORTED when the
// launch does not qualify (the caller then runs the MLP kernel).
// `detect`: the condition is per-sample in form (c_block == 1); the caller passes c_block = B here.  The
// uniformity check is enqueued first and the table kernels run only if it finds c uniform; *gate / *gate_epoch
// return the stamp for the MLP kernel the caller enqueues behind them (which runs only if c is NOT uniform).
// Where a base -> data call takes its points from when `in` is null: the cnf_fill_normal stream of `seed`
struct NoiseSrc { uint64_t seed; int64_t first_sample, slice_stride; };

static int run_flow_pwl(CnfModel* m, bool to_base, const float* in, const float* c, int64_t c_block,
                        float* out, float* aux, int aux_mode, int64_t B, hipStream_t stream,
                        bool detect = false, const uint32_t** gate = nullptr, uint32_t* gate_epoch = nullptr,
                        const NoiseSrc* noise = nullptr, const float* built = nullptr, bool in_shared = false) {
  // built: the slices' tables are in the stream's workspace already (cnf_internal_build_tables: one chunk);
  // in_shared: `in` holds ONE slice of points that every slice reads
  if (!pwl_config_ok(m)) return CNF_ERR_UNSUPPORTED;
  const int L = m->cfg.num_layers;
  const bool precise = to_base && m->precise;
  // every row of the L tables in LDS if that fits (L <= 3), else the first PWL_LROWS rows
  auto lds_for = [&](int lrows, bool first_table) {
    return (size_t)cnf::pwl_flow_lds_floats(5, L, lrows, first_table) * sizeof(float) + (precise ? precise_lds_bytes(5) : 0);
  };
  const bool full = lds_for(cnf::PWL_NPIECE, false) <= 160 * 1024;
  // the `first` spline's inverse table: the sampling direction's L = 2 instantiations, unless the knob asks for the
  // closed form (the kernel then asks the table's certified word).  The model's first such launch enqueues the builder
  // here, on its own stream and behind the parameters it has waited for; cnf_model_set_params does from then on.
  const float* ft = !to_base && full && L == 2 && m->ft_off > 0 && m->first_table_mode == 0 ? m->prep + m->ft_off : nullptr;
  if (ft && !m->ft_built) first_table_enqueue(m, stream);
  size_t lds = lds_for(full ? cnf::PWL_NPIECE : cnf::PWL_LROWS, ft != nullptr);
  if (lds > 160 * 1024) return CNF_ERR_UNSUPPORTED;
  const int64_t slice_len = c_block < B ? c_block : B;
  const int64_t n_slices = (B + slice_len - 1) / slice_len;
  if (n_slices > 1 && (slice_len & 1)) return CNF_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(in) & 15) || (reinterpret_cast<uintptr_t>(out) & 15) ||
      (reinterpret_cast<uintptr_t>(aux) & 7))
    return CNF_ERR_UNSUPPORTED;
  // Measured (MI355X, 256 x 65 536): the kernel is VALU-bound and runs best at 4 waves per SIMD -- one
  // 1024-thread workgroup per CU 58.9 G samples/s; 6 waves (3 x 512) 56.9; 2 waves 47.8.  Asking for at
  // least 82 KB of LDS keeps a second workgroup off the CU.
  // (profiles/r02_experiments: other workgroup sizes and LDS requests -- 2 / 4 / 6 waves per SIMD -- were all slower)
  const int pwl_threads = cnf::PWL_MAX_THREADS;
  const size_t pwl_min_lds = 82 * 1024;
  SlicePlan plan;
  if (slice_plan(m, stream, slice_len, n_slices, 2 * pwl_threads, 1, &plan) != CNF_OK) return CNF_ERR_UNSUPPORTED;
  const int64_t tps = plan.tps, chunk = plan.chunk;
  float* tables = plan.tables;
  if (built && (chunk < n_slices || built != tables)) return CNF_ERR_UNSUPPORTED;
  if (pwl_min_lds > lds) lds = pwl_min_lds;
  const PwlKernel kern = flow_pwl_kernel_of(to_base, precise, noise != nullptr, full, full && L == 2);
  if (!ensure_lds(kern, lds)) return CNF_ERR_UNSUPPORTED;
  uint32_t* flag = nullptr;
  uint32_t epoch = 0;
  if (detect) {
    int64_t sets = 0;
    pwl_workspace(m, stream, &tables, &sets, &flag, &epoch);
    int64_t g = (B + 4095) / 4096;
    if (g > 4 * (int64_t)m->num_cus) g = 4 * (int64_t)m->num_cus;
    hipLaunchKernelGGL(cnf::cond_uniform_kernel, dim3((unsigned)g), dim3(256), 0, stream, c, B, flag, epoch);
    *gate = flag; *gate_epoch = epoch;
  }
  m->last_path = detect ? CNF_PATH_DETECT : CNF_PATH_TABLES;
  for (int64_t s0 = 0; s0 < n_slices; s0 += chunk) {
    const int64_t ns = n_slices - s0 < chunk ? n_slices - s0 : chunk;
    const int64_t first = s0 * slice_len;
    ProfScope ps(m, stream, true, (B - first) < ns * slice_len ? (B - first) : ns * slice_len, CNF_PATH_TABLES);
    if (!built) build_tables(m, stream, c + s0, 0.0f, ns, tables);
    ps.built();
    cnf::PwlArgs a;
    a.m = model_args(m);
    a.in_shared = in_shared ? 1 : 0;
    a.in = in ? in + (in_shared ? 0 : first * 2) : nullptr; a.out = out ? out + first * 2 : nullptr; a.aux = aux ? aux + first : nullptr;
    a.seed = noise ? noise->seed : 0; a.slice_stride = noise ? noise->slice_stride : 0;
    a.first_sample = noise ? noise->first_sample + s0 * noise->slice_stride : 0;
    a.tables = tables; a.ft = ft;
    a.B = (B - first) < ns * slice_len ? (B - first) : ns * slice_len;
    a.slice_len = slice_len;
    a.n_slices = (int32_t)ns; a.tiles_per_slice = (int32_t)tps; a.aux_mode = aux_mode;
    a.gate = flag; a.gate_epoch = epoch; a.gate_want = 0;        // tables: only if no block stamped a difference
    const int64_t tiles = ns * tps;
    const int64_t want = (int64_t)m->num_cus;
    const int64_t grid = tiles < want ? tiles : want;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(pwl_threads), lds, stream, a);
    ps.done();
  }
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// base -> data over n_slices slices of slice_len points each, all reading the ONE slice of points `in`, on tables
// already built in the stream's workspace (cnf_kinetic_potential_vjp)
int cnf_internal_flow_shared(CnfModel* m, hipStream_t stream, const float* in, const float* c, int64_t slice_len,
                             int64_t n_slices, const float* tables, float* out) {
  return run_flow_pwl(m, false, in, c, slice_len, out, nullptr, 0, n_slices * slice_len, stream, false, nullptr, nullptr,
                      nullptr, tables, true);
}

// (one chunk of a term that pwl_term_on_tables has put on the tables: the reservation is the one question left)
int cnf_internal_build_tables(CnfModel* m, hipStream_t stream, const float* c, int64_t n, float** tables) {
  if (!pwl_config_ok(m) || n < 1) return CNF_ERR_UNSUPPORTED;
  int64_t sets = 0;
  pwl_workspace(m, stream, tables, &sets);
  if (sets < n) return CNF_ERR_UNSUPPORTED;
  build_tables(m, stream, c, 0.0f, n, *tables);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// Test / measurement entry point (cnf_ot_amd_debug.h): the table sets of n conditions c[0 .. n) + c_offset, built by the
// builder the knob selects, into the caller's device buffer out[n, L, PWL_TBL]
extern "C" int cnf_internal_build_tables_into(CnfModel* m, void* stream, const float* c, float c_offset, int64_t n,
                                              float* out) {
  if (!m || !c || !out || n < 1 || n * m->cfg.num_layers > (1 << 30)) return CNF_ERR_INVALID;
  if (!m->params_set) return CNF_ERR_INVALID;
  if (!pwl_network(m->cfg) || (reinterpret_cast<uintptr_t>(out) & 15)) return CNF_ERR_UNSUPPORTED;
  if (wait_for_params(m, (hipStream_t)stream) != CNF_OK) return CNF_ERR_HIP;
  build_tables(m, (hipStream_t)stream, c, c_offset, n, out);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// The arguments of a flow_kernel launch over B points in tiles of tile_samples: no gate, no finite differences,
// points read from `in`; a caller sets what differs.
template <class R>
static FlowArgsT<R> flow_args(const CnfModel* m, const R* in, const R* c, int64_t c_block, R* out, R* aux, int aux_mode,
                              int64_t B, int64_t tile_samples) {
  FlowArgsT<R> a;
  a.m = model_args(m);
  a.in = in; a.c = c; a.out = out; a.aux = aux;
  a.B = B; a.c_block = c_block; a.aux_mode = aux_mode; a.div_magic = m->div_magic;
  if (c_block >= B) a.c_mode = C_SINGLE;
  else if (c_block == 1) a.c_mode = C_PER_SAMPLE;
  else if (c_block % tile_samples == 0) a.c_mode = C_TILE_UNIFORM;
  else a.c_mode = C_GENERIC;
  a.gate = nullptr; a.gate_epoch = 0; a.gate_want = 0;
  a.fd2 = 0; a.fd_h = 0; a.fd_inv_dx = 0;
  a.seed = 0; a.first_sample = 0; a.slice_stride = 0;
  return a;
}

static int run_flow(CnfModel* m, bool to_base, const float* in, const float* c, int64_t c_block,
                    float* out, float* aux, int aux_mode, int64_t B, void* stream, const NoiseSrc* noise = nullptr) {
  if (!m || (!in && !noise) || (in && noise) || !c || B < 0 || c_block < 1) return CNF_ERR_INVALID;
  if (noise && (to_base || noise->first_sample < 0 || noise->slice_stride < 0)) return CNF_ERR_INVALID;
  if (noise && c_block == 1 && B > 1 && noise->slice_stride != 1) return CNF_ERR_INVALID;      // per-sample conditions: one run of the stream
  if (!out && !aux) return CNF_ERR_INVALID;
  if (!m->params_set) return CNF_ERR_INVALID;
  if (B == 0) return CNF_OK;
  if (wait_for_params(m, (hipStream_t)stream) != CNF_OK) return CNF_ERR_HIP;
  const uint32_t* gate = nullptr;
  uint32_t gate_epoch = 0;
  if (c_block == 1 && B > 1) {
    // per-sample conditions: uniform in every reference call (one time broadcast to cond[B,1]).  When the launch
    // is one the table path would take as a single slice, enqueue the check + the table kernels + (below) the MLP
    // kernel, gated on the device by the check's result.
    const int r = run_flow_pwl(m, to_base, in, c, B, out, aux, aux_mode, B, (hipStream_t)stream, true, &gate, &gate_epoch, noise);
    if (r != CNF_OK && r != CNF_ERR_UNSUPPORTED) return r;
  } else {
    const int r = run_flow_pwl(m, to_base, in, c, c_block, out, aux, aux_mode, B, (hipStream_t)stream, false, nullptr, nullptr, noise);
    if (r != CNF_ERR_UNSUPPORTED) return r;
  }
  int spl = m->fast_math ? samples_per_lane(m, B) : 1;
  // two samples per lane double the LDS tile: fall back when it would not fit
  if (spl == 2 && (size_t)(hdr_floats(m->cfg.num_bins) + 3 * m->cfg.dim * TILE * 2) * sizeof(float) +
                      precise_lds_bytes(m->cfg.num_bins) > 160 * 1024) spl = 1;
  FlowArgs a = flow_args<float>(m, in, c, c_block, out, aux, aux_mode, B, TILE * spl);
  a.gate = gate; a.gate_epoch = gate_epoch; a.gate_want = 1;     // MLP kernel: only if a difference was stamped
  if (noise) { a.seed = noise->seed; a.first_sample = noise->first_sample; a.slice_stride = noise->slice_stride; }
  if (!to_base) {
    const int r = launch_flow_dpar(m, a, (hipStream_t)stream);
    if (r != CNF_ERR_UNSUPPORTED) return r;
  }
  return to_base ? launch_flow<true>(m, a, spl, (hipStream_t)stream)
                 : launch_flow<false>(m, a, spl, (hipStream_t)stream);
}

extern "C" int cnf_forward_logdet(CnfModel* m, const float* x, const float* c, int64_t c_block,
                                  float* y, float* logdet, int64_t B, void* stream) {
  return run_flow(m, false, x, c, c_block, y, logdet, AUX_LOGDET, B, stream);
}

extern "C" int cnf_inverse_logdet(CnfModel* m, const float* y, const float* c, int64_t c_block,
                                  float* x, float* logdet, int64_t B, void* stream) {
  return run_flow(m, true, y, c, c_block, x, logdet, AUX_LOGDET, B, stream);
}

extern "C" int cnf_log_prob(CnfModel* m, const float* value, const float* c, int64_t c_block,
                            float* logp, int64_t B, void* stream) {
  if (!logp) return CNF_ERR_INVALID;
  return run_flow(m, true, value, c, c_block, nullptr, logp, AUX_LOGPROB, B, stream);
}

extern "C" int cnf_sample_logprob(CnfModel* m, const float* noise, const float* c, int64_t c_block,
                                  float* y, float* logp, int64_t B, void* stream) {
  if (!y) return CNF_ERR_INVALID;
  return run_flow(m, false, noise, c, c_block, y, logp, AUX_LOGPROB, B, stream);
}

extern "C" int cnf_sample_logprob_seeded(CnfModel* m, uint64_t seed, int64_t first_sample, int64_t slice_stride,
                                         const float* c, int64_t c_block, float* y, float* logp, int64_t B,
                                         void* stream) {
  if (!y) return CNF_ERR_INVALID;
  const NoiseSrc noise{seed, first_sample, slice_stride};
  return run_flow(m, false, nullptr, c, c_block, y, logp, AUX_LOGPROB, B, stream, &noise);
}

extern "C" int cnf_logprob_fd(CnfModel* m, const float* pts, const float* c, int64_t c_block, float dx,
                              float* score, int64_t B, void* stream) {
  if (!m || !pts || !c || !score || B < 0 || c_block < 1 || !(dx > 0.f)) return CNF_ERR_INVALID;
  if (!m->params_set) return CNF_ERR_INVALID;
  if (B == 0) return CNF_OK;
  const int D = m->cfg.dim;
  if (B * 2 * D >= ((int64_t)1 << 40)) return CNF_ERR_INVALID;
  if (wait_for_params(m, (hipStream_t)stream) != CNF_OK) return CNF_ERR_HIP;
  const int64_t n_eval = B * 2 * D;                 // evaluation points
  int spl = m->fast_math ? samples_per_lane(m, n_eval) : 1;
  if (spl == 2 && (size_t)(hdr_floats(m->cfg.num_bins) + 2 * D * TILE * 2) * sizeof(float) > 160 * 1024) spl = 1;
  FlowArgs a = flow_args<float>(m, pts, c, c_block, nullptr, score, AUX_LOGPROB, n_eval, TILE * spl);
  a.fd2 = 2 * D; a.fd_h = 0.5f * dx; a.fd_inv_dx = 1.0f / dx;
  a.c_mode = c_block >= B ? C_SINGLE : C_GENERIC;       // c_block counts points r_i, not evaluation points
  // plain fp32: the difference of two nearby log_prob values cancels what the precise position path would fix
  const int precise = m->precise;
  m->precise = 0;
  const int r = launch_flow<true>(m, a, spl, (hipStream_t)stream);
  m->precise = precise;
  return r;
}


// The loss terms on the conditioner tables (loss_pwl_kernel): same qualification as run_flow_pwl.
static int loss_terms_pwl(CnfModel* m, const CnfLossSpec* spec, const float* pts, int64_t slice_stride,
                          uint64_t seed, int64_t first_sample, const float* t, int64_t n_slices, int64_t B,
                          double* sums, hipStream_t stream) {
  if (!pwl_config_ok(m)) return CNF_ERR_UNSUPPORTED;
  const int L = m->cfg.num_layers;
  const int kind = spec->kind;
  const bool kin = kind <= CNF_TERM_FLOW_MATCHING;
  const int n_sets = kind == CNF_TERM_KINETIC ? 2 : (kin ? 3 : 1);
  const int threads = cnf::PWL_MAX_THREADS;
  const int64_t ts = 2 * threads;
  const size_t lds = (size_t)(((cnf::hdr_floats(5) + 3) & ~3) + n_sets * L * cnf::PWL_LTBL + 2 * ts) * sizeof(float);
  if (lds > 160 * 1024) return CNF_ERR_UNSUPPORTED;
  SlicePlan plan;
  if (slice_plan(m, stream, B, n_slices, ts, n_sets, &plan) != CNF_OK) return CNF_ERR_UNSUPPORTED;
  const int64_t tps = plan.tps, chunk = plan.chunk;
  float* tables = plan.tables;
  if (!ensure_lds(cnf::loss_pwl_kernel<5, true>, lds)) return CNF_ERR_UNSUPPORTED;
  m->last_path = CNF_PATH_LOSS_TABLES;
  for (int64_t s0 = 0; s0 < n_slices; s0 += chunk) {
    const int64_t ns = n_slices - s0 < chunk ? n_slices - s0 : chunk;
    const int64_t set_stride = ns * L * (int64_t)cnf::PWL_TBL;
    for (int s = 0; s < n_sets; ++s) {          // conditions t - dt/2, t + dt/2, t (kinetic kinds) or t
      const float off = !kin ? 0.0f : (s == 0 ? -0.5f * spec->dt : (s == 1 ? 0.5f * spec->dt : 0.0f));
      build_tables(m, stream, t + s0, off, ns, tables + s * set_stride);
    }
    cnf::LossPwlArgs a;
    a.m = model_args(m); a.spec = *spec; a.t = t + s0; a.sums = sums + s0; a.tables = tables;
    // slice s of the chunk is slice s0 + s of the call: its points / stream positions start s0 * stride later
    a.pts = pts ? pts + s0 * slice_stride * 2 : nullptr;
    a.B = B; a.n_slices = ns; a.pts_slice_stride = slice_stride;
    a.seed = seed; a.first_sample = first_sample + s0 * slice_stride;
    a.n_sets = n_sets; a.tiles_per_slice = (int32_t)tps;
    a.mix = cnf::density_mix_consts(*spec, 2);
    const int64_t tiles = ns * tps;
    const int64_t grid = tiles < m->num_cus ? tiles : m->num_cus;
    hipLaunchKernelGGL((cnf::loss_pwl_kernel<5, true>), dim3((unsigned)grid), dim3(threads), lds, stream, a);
  }
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

static int loss_terms_impl(CnfModel* m, const CnfLossSpec* spec, const float* pts, int64_t slice_stride,
                           uint64_t seed, int64_t first_sample, const float* t, int64_t n_slices, int64_t B,
                           double* sums, void* stream_) {
  if (!m || !spec || !t || !sums || n_slices < 0 || B < 0 || slice_stride < 0 || first_sample < 0) return CNF_ERR_INVALID;
  if (!m->params_set) return CNF_ERR_INVALID;
  if (term_spec_check(spec, m->cfg.dim) != CNF_OK) return CNF_ERR_INVALID;
  if (m->cfg.periodized) return CNF_ERR_UNSUPPORTED;      // flow functions only (include/cnf_ot_amd.h: CnfConfig)
  const int D = m->cfg.dim;
  hipStream_t stream = (hipStream_t)stream_;
  if (n_slices == 0) return CNF_OK;
  if (hipMemsetAsync(sums, 0, sizeof(double) * (size_t)n_slices, stream) != hipSuccess) return CNF_ERR_HIP;
  if (B == 0) return CNF_OK;
  if (wait_for_params(m, stream) != CNF_OK) return CNF_ERR_HIP;
  {
    const int r = loss_terms_pwl(m, spec, pts, slice_stride, seed, first_sample, t, n_slices, B, sums, stream);
    if (r != CNF_ERR_UNSUPPORTED) return r;
  }
  LossArgs a;
  a.m = model_args(m); a.spec = *spec; a.pts = pts; a.t = t; a.sums = sums;
  a.B = B; a.n_slices = n_slices; a.pts_slice_stride = slice_stride;
  a.div_magic = m->div_magic; a.seed = seed; a.first_sample = first_sample;
  a.mix = density_mix_consts(*spec, D);
  // five D x TS buffers: keep a workgroup under ~64 KB of LDS
  int spl = (m->fast_math && n_slices * B >= (int64_t)m->num_cus * 4 * 64 * 2) ? 2 : 1;
  if (m->force_spl == 1 || m->force_spl == 2) spl = m->fast_math ? m->force_spl : 1;
  if (spl == 2 && (size_t)(5 * D * TILE * 2) * sizeof(float) > 64 * 1024) spl = 1;
  const int64_t ts = (int64_t)TILE * spl;
  const size_t lds = (size_t)(hdr_floats(m->cfg.num_bins) + 5 * D * ts) * sizeof(float);
  if (lds > 160 * 1024) return CNF_ERR_UNSUPPORTED;
  int64_t grid = ((B + ts - 1) / ts) * n_slices;
  const int64_t cap = (int64_t)m->num_cus * 8;
  if (grid > cap) grid = cap;
  return with_shape(m->cfg, [&](auto h, auto k) -> int {
    constexpr int H = decltype(h)::value, K = decltype(k)::value;
    typedef void (*LossKernel)(const LossArgs);
    LossKernel kern = loss_kernel<H, K, false, float>;
    if (m->fast_math) kern = spl == 2 ? loss_kernel<H, K, true, v2f> : loss_kernel<H, K, true, float>;
    return launch(m, kern, grid, TILE, lds, stream, a, CNF_PATH_LOSS_MLP);
  });
}

extern "C" int cnf_loss_terms(CnfModel* m, const CnfLossSpec* spec, const float* pts, int pts_shared,
                              const float* t, int64_t n_slices, int64_t B, double* sums, void* stream) {
  if (!pts) return CNF_ERR_INVALID;
  return loss_terms_impl(m, spec, pts, pts_shared ? 0 : B, 0, 0, t, n_slices, B, sums, stream);
}

extern "C" int cnf_loss_terms_seeded(CnfModel* m, const CnfLossSpec* spec, uint64_t seed, int64_t first_sample,
                                     int64_t slice_stride, const float* t, int64_t n_slices, int64_t B,
                                     double* sums, void* stream) {
  if (spec && (spec->kind == CNF_TERM_NEG_LOGPROB || spec->kind == CNF_TERM_DENSITY_L2_DATA))
    return CNF_ERR_INVALID;                                                  // those terms take data points
  return loss_terms_impl(m, spec, nullptr, slice_stride, seed, first_sample, t, n_slices, B, sums, stream);
}

// ---- float64 instantiation: the reference's own dtype (solvers.py:23) ---------
// Exact-mode entry points: double IO, double table/constants, ocml math, one
// sample per lane.  Parameters stay the float32 vector given to
// cnf_model_set_params (each weight is widened exactly).
template <bool TO_BASE>
static int launch_flow_f64(CnfModel* m, const FlowArgsD& a, hipStream_t stream) {
  const int64_t n_tiles = (a.B + TILE - 1) / TILE;
  int64_t grid = n_tiles;
  const int64_t cap = (int64_t)m->num_cus * 8;
  if (grid > cap) grid = cap;
  const size_t lds = (size_t)(hdr_floats(m->cfg.num_bins) + 2 * a.m.D * TILE) * sizeof(double);
  return with_shape(m->cfg, [&](auto h, auto k) -> int {
    constexpr int H = decltype(h)::value, K = decltype(k)::value;
    typedef void (*FlowKernelD)(const FlowArgsD);
    const FlowKernelD kern = m->cfg.periodized ? flow_kernel<H, K, TO_BASE, false, double, false, false, true>
                                               : flow_kernel<H, K, TO_BASE, false, double>;
    return launch(m, kern, grid, TILE, lds, stream, a, CNF_PATH_F64);
  });
}

static int run_flow_f64(CnfModel* m, bool to_base, const double* in, const double* c, int64_t c_block,
                        double* out, double* aux, int aux_mode, int64_t B, void* stream) {
  if (!m || !in || !c || B < 0 || c_block < 1) return CNF_ERR_INVALID;
  if (!out && !aux) return CNF_ERR_INVALID;
  if (!m->params_set) return CNF_ERR_INVALID;
  if (B == 0) return CNF_OK;
  if (wait_for_params(m, (hipStream_t)stream) != CNF_OK) return CNF_ERR_HIP;
  const FlowArgsD a = flow_args<double>(m, in, c, c_block, out, aux, aux_mode, B, TILE);
  return to_base ? launch_flow_f64<true>(m, a, (hipStream_t)stream) : launch_flow_f64<false>(m, a, (hipStream_t)stream);
}

extern "C" int cnf_forward_logdet_f64(CnfModel* m, const double* x, const double* c, int64_t c_block, double* y,
                                      double* logdet, int64_t B, void* stream) {
  return run_flow_f64(m, false, x, c, c_block, y, logdet, AUX_LOGDET, B, stream);
}
extern "C" int cnf_inverse_logdet_f64(CnfModel* m, const double* y, const double* c, int64_t c_block, double* x,
                                      double* logdet, int64_t B, void* stream) {
  return run_flow_f64(m, true, y, c, c_block, x, logdet, AUX_LOGDET, B, stream);
}
extern "C" int cnf_log_prob_f64(CnfModel* m, const double* value, const double* c, int64_t c_block, double* logp,
                                int64_t B, void* stream) {
  if (!logp) return CNF_ERR_INVALID;
  return run_flow_f64(m, true, value, c, c_block, nullptr, logp, AUX_LOGPROB, B, stream);
}
extern "C" int cnf_sample_logprob_f64(CnfModel* m, const double* noise, const double* c, int64_t c_block, double* y,
                                      double* logp, int64_t B, void* stream) {
  if (!y) return CNF_ERR_INVALID;
  return run_flow_f64(m, false, noise, c, c_block, y, logp, AUX_LOGPROB, B, stream);
}

// ---- fields and trajectories (fields_kernel) ----------------------------------------------------------------------
// The configurations the kernel serves: the dims of the fused loss kernel, hardware transcendentals for float32, not
// periodized; everything else is CNF_ERR_UNSUPPORTED and composed from the flow calls by the caller.
template <class R>
static size_t fields_lds_bytes(const CnfModel* m) {
  const int D = m->cfg.dim;
  return std::is_same<R, double>::value
             ? (size_t)(hdr_floats(m->cfg.num_bins) + 5 * D * TILE) * sizeof(double)
             : (size_t)(hdr_floats(m->cfg.num_bins) + 6 * D * TILE) * sizeof(float) + precise_lds_bytes(m->cfg.num_bins);
}

// Checked before anything else a call does, the empty call included: one model gives one answer for every N and S.
template <class R>
static bool fields_supported(const CnfModel* m) {
  constexpr bool F64 = std::is_same<R, double>::value;
  if (m->cfg.periodized || m->cfg.dim > 14 || (!F64 && !m->fast_math)) return false;
  if (fields_lds_bytes<R>(m) > 160 * 1024) return false;
  return shape_compiled(m->cfg);
}

template <class R>
static int launch_fields(CnfModel* m, cnf::FieldArgsT<R>& a, hipStream_t stream) {
  constexpr bool F64 = std::is_same<R, double>::value;
  if (!fields_supported<R>(m)) return CNF_ERR_UNSUPPORTED;
  const size_t lds = fields_lds_bytes<R>(m);
  if (wait_for_params(m, stream) != CNF_OK) return CNF_ERR_HIP;
  a.m = model_args(m);
  a.div_magic = m->div_magic;
  const int64_t tiles = (a.N + TILE - 1) / TILE;
  // trajectories: a workgroup that walks all S times runs the data -> base pass once, one per time runs it S times
  // but S workgroups side by side -- the latter while the tiles alone leave compute units idle
  a.slice_chunk = (a.fixed_base && tiles >= 2 * (int64_t)m->num_cus) ? (int32_t)(a.S < (1 << 20) ? a.S : (1 << 20)) : 1;
  const int64_t items = tiles * ((a.S + a.slice_chunk - 1) / a.slice_chunk);
  const int64_t grid = balanced_grid(items, (int64_t)m->num_cus * 8);
  return with_shape(m->cfg, [&](auto h, auto k) -> int {      // float32: hardware transcendentals; float64: ocml
    return launch(m, cnf::fields_kernel<decltype(h)::value, decltype(k)::value, !F64, R>, grid, TILE, lds, stream, a,
                  F64 ? CNF_PATH_F64 : CNF_PATH_FIELDS);
  });
}

template <class R>
static int eulerian_fields_impl(CnfModel* m, const CnfFieldGrid* g, const R* pts, int64_t N, const R* t, int64_t S,
                                R dt, R dx, R* rho, R* logp, R* vel, R* score, void* stream) {
  if (!m || !t || N < 0 || S < 0 || (g != nullptr) == (pts != nullptr)) return CNF_ERR_INVALID;
  if (!rho && !logp && !vel && !score) return CNF_ERR_INVALID;
  if (!m->params_set) return CNF_ERR_INVALID;
  if ((vel && !(dt > 0)) || (score && !(dx > 0))) return CNF_ERR_INVALID;
  const int D = m->cfg.dim;
  cnf::FieldArgsT<R> a = {};
  a.n_sec = 1; a.sec_axis = -1;
  if (g) {
    if (g->nx < 1 || g->ny < 1 || (int64_t)g->nx * g->ny != N || !g->fixed) return CNF_ERR_INVALID;
    if (g->axis_x < 0 || g->axis_x >= D || g->axis_y < 0 || g->axis_y >= D || g->axis_x == g->axis_y) return CNF_ERR_INVALID;
    if (g->n_sec < 1 || (g->sec == nullptr) != (g->sec_axis < 0)) return CNF_ERR_INVALID;
    if (g->sec && (g->sec_axis >= D || g->sec_axis == g->axis_x || g->sec_axis == g->axis_y)) return CNF_ERR_INVALID;
    if (!g->sec && g->n_sec != 1) return CNF_ERR_INVALID;
    if (g->n_sec > 1 && (logp || vel || score)) return CNF_ERR_INVALID;      // a mean over sections: the density alone
    a.fixed = static_cast<const R*>(g->fixed); a.sec = static_cast<const R*>(g->sec);
    a.lo_x = g->lo_x; a.lo_y = g->lo_y; a.step_x = g->step_x; a.step_y = g->step_y;
    a.nx = g->nx; a.axis_x = g->axis_x; a.axis_y = g->axis_y; a.sec_axis = g->sec_axis; a.n_sec = g->n_sec;
  }
  if (!fields_supported<R>(m)) return CNF_ERR_UNSUPPORTED;
  if (N == 0 || S == 0) return CNF_OK;
  a.pts = pts; a.t = t; a.rho = rho; a.logp = logp; a.vel = vel; a.score = score; a.traj = nullptr;
  a.N = N; a.S = S; a.fixed_base = 0; a.t0 = 0; a.dt = vel ? dt : (R)1; a.dx = score ? dx : (R)1;
  return launch_fields<R>(m, a, (hipStream_t)stream);
}

template <class R>
static int trajectories_impl(CnfModel* m, const R* r0, int64_t N, R t0, const R* t, int64_t S, R dt, R* traj, R* vel,
                             void* stream) {
  if (!m || !r0 || !t || N < 0 || S < 0 || (!traj && !vel)) return CNF_ERR_INVALID;
  if (!m->params_set || (vel && !(dt > 0))) return CNF_ERR_INVALID;
  if (!fields_supported<R>(m)) return CNF_ERR_UNSUPPORTED;
  if (N == 0 || S == 0) return CNF_OK;
  cnf::FieldArgsT<R> a = {};
  a.pts = r0; a.t = t; a.traj = traj; a.vel = vel;
  a.N = N; a.S = S; a.n_sec = 1; a.sec_axis = -1; a.fixed_base = 1; a.t0 = t0; a.dt = vel ? dt : (R)1; a.dx = (R)1;
  return launch_fields<R>(m, a, (hipStream_t)stream);
}

extern "C" int cnf_eulerian_fields(CnfModel* m, const CnfFieldGrid* grid, const float* pts, int64_t N, const float* t,
                                   int64_t S, float dt, float dx, float* rho, float* logp, float* vel, float* score,
                                   void* stream) {
  return eulerian_fields_impl<float>(m, grid, pts, N, t, S, dt, dx, rho, logp, vel, score, stream);
}
extern "C" int cnf_eulerian_fields_f64(CnfModel* m, const CnfFieldGrid* grid, const double* pts, int64_t N,
                                       const double* t, int64_t S, double dt, double dx, double* rho, double* logp,
                                       double* vel, double* score, void* stream) {
  return eulerian_fields_impl<double>(m, grid, pts, N, t, S, dt, dx, rho, logp, vel, score, stream);
}
extern "C" int cnf_trajectories(CnfModel* m, const float* r0, int64_t N, float t0, const float* t, int64_t S, float dt,
                                float* traj, float* vel, void* stream) {
  return trajectories_impl<float>(m, r0, N, t0, t, S, dt, traj, vel, stream);
}
extern "C" int cnf_trajectories_f64(CnfModel* m, const double* r0, int64_t N, double t0, const double* t, int64_t S,
                                    double dt, double* traj, double* vel, void* stream) {
  return trajectories_impl<double>(m, r0, N, t0, t, S, dt, traj, vel, stream);
}
