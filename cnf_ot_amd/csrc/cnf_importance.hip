// cnf_importance.hip -- importance-sampling diagnostics of a trained flow against a density known in closed form
// (the reference's kl_ess, tests/test_fit_prob.py:50-56, "metrics used in the tori paper": draw y ~ q = the flow,
// weight w = p(y) / q(y), report Z = mean w, KL = mean(log q - log p) + log Z, ESS = (sum w)^2 / sum w^2).  The
// reference forms w in linear space, where it underflows as soon as the flow is far from the target; here the
// statistic is a running (max, scaled sums) state of the LOG-weights l = log p - log q,
//   (m, s1, s2, c, n) = (max l, sum exp(l - m), sum exp(2 (l - m)), sum l, count),
// merged in a fixed order lanes -> wave -> workgroup -> slice, all in float64: one launch over the samples, one
// small finishing launch, nothing but 5 doubles per (slice, chunk) in between.  A unit of its own: the kernels of
// cnf_flow.hip change their generated code when their unit changes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "cnf_flow_tile.h"
#include "cnf_host.h"

namespace cnf {

// The raw state and its merge.  The empty state is (-inf, 0, 0, 0, 0); merging it is a no-op, and two empty states
// merge to the empty state without ever forming -inf - (-inf).  `bad`: a non-finite log-weight was seen (it is
// counted in n and enters nothing else: the slice's four statistics become NaN at the end).
struct ImpState {
  double m, s1, s2, c, n;
  int bad;
};
__device__ __forceinline__ ImpState imp_empty() {
  return ImpState{-std::numeric_limits<double>::infinity(), 0.0, 0.0, 0.0, 0.0, 0};
}
__device__ __forceinline__ ImpState imp_merge(const ImpState& a, const ImpState& b) {
  ImpState r;
  r.m = fmax(a.m, b.m);
  r.c = a.c + b.c;
  r.n = a.n + b.n;
  r.bad = a.bad | b.bad;
  if (r.m == -std::numeric_limits<double>::infinity()) { r.s1 = 0.0; r.s2 = 0.0; return r; }    // both empty
  const double ea = exp(a.m - r.m), eb = exp(b.m - r.m);       // (an empty side: exp(-inf) = 0 times its zero sums)
  r.s1 = a.s1 * ea + b.s1 * eb;
  r.s2 = a.s2 * (ea * ea) + b.s2 * (eb * eb);
  return r;
}
// one sample's log-weight
__device__ __forceinline__ void imp_add(ImpState& s, double l) {
  if (!(fabs(l) <= std::numeric_limits<double>::max())) { s.bad = 1; s.n += 1.0; return; }       // NaN or +-inf
  s = imp_merge(s, ImpState{l, 1.0, 1.0, l, 1.0, 0});
}
__device__ __forceinline__ double shfl_down_f64(double v, int off) {
  const long long b = __double_as_longlong(v);
  const int lo = __shfl_down((int)(uint32_t)b, off, 64), hi = __shfl_down((int)(uint32_t)(b >> 32), off, 64);
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}
// lanes -> lane 0 of the wave: a fixed binary tree (lane k takes lane k + off, off = 32, 16, .. 1)
__device__ __forceinline__ ImpState imp_wave_merge(ImpState s) {
#pragma unroll 1
  for (int off = 32; off > 0; off >>= 1) {
    ImpState o;
    o.m = shfl_down_f64(s.m, off); o.s1 = shfl_down_f64(s.s1, off); o.s2 = shfl_down_f64(s.s2, off);
    o.c = shfl_down_f64(s.c, off); o.n = shfl_down_f64(s.n, off); o.bad = __shfl_down(s.bad, off, 64);
    s = imp_merge(s, o);
  }
  return s;
}
constexpr int IMP_COLS = 5;        // doubles of a `stats` row
constexpr int IMP_PART = 6;        // doubles of a workspace partial: the row and the `bad` flag
__device__ __forceinline__ void imp_store(double* p, const ImpState& s) {
  p[0] = s.m; p[1] = s.s1; p[2] = s.s2; p[3] = s.c; p[4] = s.n; p[5] = s.bad ? 1.0 : 0.0;
}
__device__ __forceinline__ ImpState imp_load(const double* p) {
  return ImpState{p[0], p[1], p[2], p[3], p[4], p[5] != 0.0 ? 1 : 0};
}

struct ImportanceArgs {
  ModelArgs m;
  CnfTargetSpec tg;
  const float* noise;   // base noise, or null: drawn in the kernel (the cnf_fill_normal stream of `seed`)
  const float* t;       // [n_slices]
  double* part;         // workspace [n_slices][chunks][IMP_PART]
  int64_t B;            // samples per slice
  int64_t n_slices;
  int64_t slice_stride; // samples between slices in the noise (0: every slice the same draw)
  int64_t chunks;       // partials per slice: chunk p of a slice owns its tiles p, p + chunks, ...
  uint32_t div_magic;
  uint64_t seed;
  int64_t first_sample;
};

// ---------------------------------------------------------------------------
// importance_kernel: one work item = (slice, chunk); tiles of 256 samples of the slice, one sample per lane.  Per
// tile: the base noise into LDS, its log N(x; 0, I) in float64, one base -> data pass, the target's log-density in
// float64 at the fp32 sample (cnf_terms.h: target_logprob), l = log p - log q into the lane's running state.  After
// the item's last tile: lanes -> wave -> workgroup, one partial to the workspace.  LDS: [hdr][U][O], each D x 256.
// ---------------------------------------------------------------------------
template <int H, int K, bool FAST>
__global__ __launch_bounds__(TILE, 2) void importance_kernel(const ImportanceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double wave_part[TILE / 64][IMP_PART];
  constexpr int HDR = hdr_floats(K);
  const int D = a.m.D;
  float* tab = lds;
  float* U = lds + HDR;
  float* O = U + D * TILE;
  for (int i = threadIdx.x; i < HDR; i += TILE) tab[i] = a.m.prep[i];
  const int col = threadIdx.x;
  const int64_t tiles_per_slice = (a.B + TILE - 1) / TILE;
  const int64_t n_items = a.n_slices * a.chunks;
  for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int64_t slice = item / a.chunks, chunk = item - slice * a.chunks;
    const float t = a.t[slice];
    const double scale = a.tg.scale ? a.tg.scale[slice] : 1.0;
    ImpState st = imp_empty();
    for (int64_t tile = chunk; tile < tiles_per_slice; tile += a.chunks) {
      const int64_t tile_start = tile * TILE;
      __syncthreads();
      if (a.noise)
        tile_load<float>(a.noise + slice * a.slice_stride * D, U, D, a.div_magic, TILE, tile_start, a.B);
      else
        tile_noise(a.seed, (uint64_t)(a.first_sample + slice * a.slice_stride + tile_start) * (uint64_t)D, U, D,
                   a.div_magic, TILE, a.B - tile_start);
      __syncthreads();
      const double lbase = base_logprob<double>(lds_col<float>(U + col, TILE), D);
      const float fldj = flow_pass<H, K, false, FAST, float>(a.m, tab, U, O, t);
      const double lq = lbase - (double)fldj;
      const double lp = target_logprob(a.tg, lds_col<float>(U + col, TILE), D, scale);
      if (tile_start + col < a.B) imp_add(st, lp - lq);
    }
    st = imp_wave_merge(st);
    __syncthreads();          // (the previous item's partial has been read)
    if ((threadIdx.x & 63) == 0) imp_store(wave_part[threadIdx.x >> 6], st);
    __syncthreads();
    if (threadIdx.x == 0) {
      ImpState s = imp_load(wave_part[0]);
      for (int w = 1; w < TILE / 64; ++w) s = imp_merge(s, imp_load(wave_part[w]));
      imp_store(a.part + item * IMP_PART, s);
    }
  }
}

// One wave per slice: lane k merges the slice's partials k, k + 64, ... in ascending order, the lanes merge by the
// same tree as above, lane 0 writes the row.  A slice that saw a non-finite log-weight: NaN in its first four columns.
__global__ __launch_bounds__(64) void importance_finish_kernel(const double* __restrict__ part, int64_t chunks,
                                                                double* __restrict__ stats) {
  const int64_t slice = blockIdx.x;
  ImpState s = imp_empty();
  for (int64_t p = threadIdx.x; p < chunks; p += 64) s = imp_merge(s, imp_load(part + (slice * chunks + p) * IMP_PART));
  s = imp_wave_merge(s);
  if (threadIdx.x == 0) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double* o = stats + slice * IMP_COLS;
    o[0] = s.bad ? nan : s.m; o[1] = s.bad ? nan : s.s1; o[2] = s.bad ? nan : s.s2; o[3] = s.bad ? nan : s.c;
    o[4] = s.n;
  }
}

}  // namespace cnf

using namespace cnf;

// Partials per slice: one per tile up to IMP_MAX_CHUNKS, where a chunk starts taking several tiles.  A function of B
// alone -- not of the device, nor of the other slices of the call -- so that the merge order, and with it every bit
// of a slice's row, is the same on any GPU and in any call the slice is part of.  1 024 chunks of one slice fill a
// 256-CU device with 4 workgroups per CU.
constexpr int64_t IMP_MAX_CHUNKS = 1024;
static int64_t importance_chunks(int64_t B) {
  const int64_t tps = (B + TILE - 1) / TILE;
  return tps < 1 ? 1 : (tps < IMP_MAX_CHUNKS ? tps : IMP_MAX_CHUNKS);
}

extern "C" int cnf_importance_workspace(int64_t n_slices, int64_t B, int32_t D, int64_t* bytes) {
  if (!bytes || n_slices < 0 || B < 0 || D < 1 || D > CNF_TARGET_MAX_DIM) return CNF_ERR_INVALID;
  if (n_slices > (int64_t)1 << 31 || B > (int64_t)1 << 40) return CNF_ERR_INVALID;
  const int64_t rows = n_slices > 0 ? n_slices * importance_chunks(B) : 1;
  *bytes = rows * IMP_PART * (int64_t)sizeof(double);
  return CNF_OK;
}

static int importance_impl(CnfModel* m, const CnfTargetSpec* tg, const float* noise, int64_t slice_stride, uint64_t seed,
                           int64_t first_sample, const float* t, int64_t n_slices, int64_t B, double* stats,
                           void* workspace, int64_t workspace_bytes, void* stream_) {
  if (!m || !tg || !t || !stats || !workspace || n_slices < 0 || B < 0 || slice_stride < 0 || first_sample < 0)
    return CNF_ERR_INVALID;
  if (!m->params_set) return CNF_ERR_INVALID;
  const int D = m->cfg.dim;
  if (D > CNF_TARGET_MAX_DIM) return CNF_ERR_INVALID;                 // the target struct holds no such density
  if (tg->n_comp < 1 || tg->n_comp > CNF_TARGET_MAX_COMP) return CNF_ERR_INVALID;
  for (int d = 0; d < D; ++d)
    if (!(tg->W[d][d] > 0.0) || !std::isfinite(tg->W[d][d])) return CNF_ERR_INVALID;
  int64_t need = 0;
  if (cnf_importance_workspace(n_slices, B, D, &need) != CNF_OK || workspace_bytes < need) return CNF_ERR_INVALID;
  if (m->cfg.periodized) return CNF_ERR_UNSUPPORTED;      // flow functions only (include/cnf_ot_amd.h: CnfConfig)
  if (!shape_compiled(m->cfg)) return CNF_ERR_UNSUPPORTED;
  if (n_slices == 0 || B == 0) return CNF_OK;
  hipStream_t stream = (hipStream_t)stream_;
  if (wait_for_params(m, stream) != CNF_OK) return CNF_ERR_HIP;
  ImportanceArgs a;
  a.m = model_args(m); a.tg = *tg; a.noise = noise; a.t = t; a.part = (double*)workspace;
  a.B = B; a.n_slices = n_slices; a.slice_stride = slice_stride; a.chunks = importance_chunks(B);
  a.div_magic = m->div_magic; a.seed = seed; a.first_sample = first_sample;
  const size_t lds = (size_t)(hdr_floats(m->cfg.num_bins) + 2 * D * TILE) * sizeof(float);
  int64_t grid = n_slices * a.chunks;
  const int64_t cap = (int64_t)m->num_cus * 8;
  if (grid > cap) grid = cap;
  const int r = with_shape(m->cfg, [&](auto h, auto k) -> int {
    constexpr int H = decltype(h)::value, K = decltype(k)::value;
    typedef void (*ImportanceKernel)(const ImportanceArgs);
    ImportanceKernel kern = m->fast_math ? importance_kernel<H, K, true> : importance_kernel<H, K, false>;
    return launch(m, kern, grid, TILE, lds, stream, a, CNF_PATH_IMPORTANCE);
  });
  if (r != CNF_OK) return r;
  hipLaunchKernelGGL(importance_finish_kernel, dim3((unsigned)n_slices), dim3(64), 0, stream, a.part, a.chunks, stats);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_importance_stats(CnfModel* m, const CnfTargetSpec* target, const float* noise, int noise_shared,
                                    const float* t, int64_t n_slices, int64_t B, double* stats, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  if (!noise) return CNF_ERR_INVALID;
  return importance_impl(m, target, noise, noise_shared ? 0 : B, 0, 0, t, n_slices, B, stats, workspace,
                         workspace_bytes, stream);
}

extern "C" int cnf_importance_stats_seeded(CnfModel* m, const CnfTargetSpec* target, uint64_t seed, int64_t first_sample,
                                           int64_t slice_stride, const float* t, int64_t n_slices, int64_t B,
                                           double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  return importance_impl(m, target, nullptr, slice_stride, seed, first_sample, t, n_slices, B, stats, workspace,
                         workspace_bytes, stream);
}
