// cnf_common.h -- structs shared by the translation units of libcnf_ot_amd.so that work on a CnfModel (cnf_model.hip,
// cnf_rng.hip, cnf_flow.hip, cnf_grad.hip, cnf_grad_pwl.hip, cnf_importance.hip): the model object, the kernels' view
// of it, the dim-2 table route, the list of compiled shapes, the argument checks and the launch tails (the model-free
// cnf_step.hip uses those too).  The declarations of functions that cross units: cnf_host.h.
#pragma once
#include <mutex>
#include <map>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "cnf_device.h"
#include "cnf_terms.h"
#include "../../include/cnf_ot_amd.h"

namespace cnf {

constexpr int TILE = 256;

struct ModelArgs {
  const float* prep;     // prepared model buffer
  const float* wq;       // MFMA-layout weights (inside prep), or null
  int64_t per_layer;     // floats of conditioner weights per flow layer
  int64_t per_layer_q;   // floats of MFMA-layout weights per flow layer
  int32_t D, L, M;
  SplineConsts sc;
  SplineConstsT<double> scd;   // the same constants in float64 (exact-mode kernels)
  const double* tabd;          // float64 copy of the `first` table (inside prep)
  const double* e2tab;         // 2^(-i/32), i = 0 .. 1024 (inside prep): the precise position path
};

template <class R> __device__ __forceinline__ const SplineConstsT<R>& sc_of(const ModelArgs& a);
template <> __device__ __forceinline__ const SplineConstsT<float>& sc_of<float>(const ModelArgs& a) { return a.sc; }
template <> __device__ __forceinline__ const SplineConstsT<double>& sc_of<double>(const ModelArgs& a) { return a.scd; }
template <class R> __device__ __forceinline__ const R* table_of(const ModelArgs& a);
template <> __device__ __forceinline__ const float* table_of<float>(const ModelArgs& a) { return a.prep; }
template <> __device__ __forceinline__ const double* table_of<double>(const ModelArgs& a) { return a.tabd; }

}  // namespace cnf

struct CnfModel {
  // (opaque to callers; see include/cnf_ot_amd.h)
  CnfConfig cfg;
  cnf::SplineConsts sc;
  cnf::SplineConstsT<double> scd;
  int64_t tabd_off;       // offset (in floats, 8-byte aligned) of the float64 table inside prep
  int64_t e2_off;         // offset (in floats, 8-byte aligned) of the 2^(-i/32) table inside prep
  int precise;            // 1 (default): data -> base entry points run the precise position path
  int64_t ft_off;         // offset (in floats, 16-byte aligned) of the `first` spline's inverse table (cnf_first_table.h)
                          // inside prep, behind every other section; 0: this model has no kernel that reads one
  int ft_built;           // the table's builder has been enqueued for the current parameters
  int ft_wanted;          // a launch has asked for the table: from then on cnf_model_set_params builds it (a model that
                          // only trains never pays for the builder)
  int first_table_mode;   // 0 (default): the table where certified; 1: always the closed form
  float* prep;            // device
  int64_t n_params;
  int64_t per_layer;
  int device;
  int num_cus;
  int fast_math;          // 1: hardware transcendentals (default), 0: ocml
  int force_spl;          // 0: automatic; 1 / 2: samples per lane (tests, bench)
  int use_mfma;           // 1: MFMA conditioner where available (H = 16, K = 5, fast math)
  uint32_t div_magic;     // ceil(2^32 / D)
  int64_t per_layer_q;    // MFMA-layout floats per flow layer (0: not available)
  int64_t mfma_off;       // offset of the MFMA-layout weights inside prep (floats)
  int params_set;
  float* grad_slabs;      // per-wave gradient slabs (cnf_grad_enable), or null
  int64_t grad_max_blocks;
  int use_pwl;            // 1: piecewise-linear conditioner tables at dim 2 (cnf_pwl.h)
  int use_dpar;           // 1: wave-per-dimension kernel for small base -> data launches at dim >= 3
  int pwl_builder;        // table builder: 0 by table count (default), 1 the reference builder, 2 the lean one
  int last_pwl_builder;   // the builder (1 / 2) of the most recent table build, 0 before the first
  // table workspaces [sets][L][PWL_TBL], one per stream (calls on different streams never share one).
  // Allocated ONLY by cnf_model_reserve; the compute entry points look theirs up and never allocate.
  // cnf_grad_enable: per-piece gradient statistics of the table backward (cnf_grad_pwl.hip), PWL_STAT_SLICES slices
  float* pwl_stats;
  // retired: blocks of this stream outgrown by a later reservation, kept alive for graphs captured on them
  struct PwlWorkspace { float* tables; int64_t sets; uint32_t epoch; std::vector<float*> retired; };
  std::mutex pwl_mu;
  std::unordered_map<void*, PwlWorkspace> pwl_ws;
  // cnf_model_set_params records `prep_event` after its kernel; a compute call on another stream waits for it
  hipEvent_t prep_event;
  void* prep_stream;
  int last_path;          // CnfPath of the most recent compute call (cnf_model_last_path)
  // cnf_model_set_profiling: HIP events around the kernels of the flow entry points
  struct ProfRec { hipEvent_t e0, e1, e2; int64_t samples; int path; };
  int profiling;
  std::vector<ProfRec> prof;
};

// which kernels a compute call ran (cnf_model_last_path)
enum CnfPath {
  CNF_PATH_NONE = 0,
  CNF_PATH_MLP1 = 1,        // flow_kernel, one sample per lane
  CNF_PATH_MLP2 = 2,        // flow_kernel, packed fp32, two samples per lane
  CNF_PATH_MFMA = 3,        // flow_kernel with the MFMA conditioner
  CNF_PATH_TABLES = 4,      // pwl_build_kernel + flow_pwl_kernel
  CNF_PATH_LOSS_MLP = 5,    // loss_kernel
  CNF_PATH_LOSS_TABLES = 6, // pwl_build_kernel + loss_pwl_kernel
  CNF_PATH_F64 = 7,         // float64 instantiation
  CNF_PATH_DPAR = 9,        // flow_dpar_kernel: one wave per conditioned dimension (dim >= 3, base -> data)
  CNF_PATH_DETECT = 8,      // per-sample condition: uniformity check + table kernels + MLP kernel, gated on the device
  CNF_PATH_FIELDS = 10,     // fields_kernel (cnf_eulerian_fields, cnf_trajectories)
  CNF_PATH_SCORE = 11,      // score_kernel (cnf_score)
  CNF_PATH_IMPORTANCE = 12, // importance_kernel + importance_finish_kernel (cnf_importance_stats)
};

// ---- The dim-2 conditioner-table route, stated once (host code; no HIP call anywhere below) -------------------------
// The network the tables exist for (cnf_pwl.h: hidden width PWL_H = 16, 5 bins, two MLP layers; the sin / cos
// features of a periodized model are not piecewise linear in u) ...
static inline bool pwl_network(const CnfConfig& g) {
  return g.dim == 2 && g.hidden_size == 16 && g.num_bins == 5 && g.mlp_num_layers == 2 && !g.periodized;
}
// ... and the one its backward (vjp_pwl_kernel) exists for: what cnf_grad_enable allocates pwl_stats for
static inline bool pwl_backward_network(const CnfConfig& g) { return pwl_network(g) && g.num_layers <= 4; }
// This model has a table path under its current knobs ...
static inline bool pwl_config_ok(const CnfModel* m) { return m->use_pwl && m->fast_math && pwl_network(m->cfg); }
// ... and a table backward (after cnf_grad_enable; without pwl_stats the MLP backward remains)
static inline bool pwl_backward_ok(const CnfModel* m) {
  return pwl_config_ok(m) && pwl_backward_network(m->cfg) && m->pwl_stats != nullptr;
}
// A pass on the tables is worth it while a slice amortises its tables and their per-piece finishing (measured
// crossover: see DESIGN.md)
// (measured, scripts/exp_vjp_crossover.py, round 3's kernel: 131 072 points 0.049 vs 0.044 ms for the MLP backward,
// 262 144 points 0.056 vs 0.066 -- 32 slices of 8 192: 0.062 vs 0.066 --, 524 288 points 0.072 vs 0.110; slices of
// 4 096 points lose until there are ~100 of them.  Round 2's kernel crossed over at twice that.)
constexpr int64_t PWL_MIN_SLICE = 8192, PWL_MIN_POINTS = 262144;
// Whether a term composed from table launches -- slices of slice_len points, n_points over all slices of all its
// passes -- is taken by the table kernels under the model's use_pwl mode (0: never; 1: from the thresholds up; 2: at
// every size); with_grad: by the table backward too.  What cnf_pass_vjp, cnf_neg_logprob_vjp and
// cnf_kinetic_potential_vjp ask before their own conditions (alignment, odd slice lengths, slab room, slice count).
static inline bool pwl_term_on_tables(const CnfModel* m, int64_t slice_len, int64_t n_points, bool with_grad) {
  if (with_grad ? !pwl_backward_ok(m) : !pwl_config_ok(m)) return false;
  return m->use_pwl != 1 || (slice_len >= PWL_MIN_SLICE && n_points >= PWL_MIN_POINTS);
}

#ifdef CNF_MINIMAL_CONFIGS   /* faster builds while iterating on the kernels */
#define CNF_KERNEL_CONFIGS(X) X(16, 5)
#else
#define CNF_KERNEL_CONFIGS(X) \
  X(8, 5) X(16, 4) X(16, 5) X(16, 8) X(16, 10) X(32, 5) X(32, 8) X(64, 5)
#endif

// The list's one expansion.  Calls f(std::integral_constant<int, H>{}, std::integral_constant<int, K>{}) for the
// compiled shape of cfg and returns its result; CNF_ERR_UNSUPPORTED when the shape is not compiled.  A launch site is
// a generic lambda that names its kernels with decltype(h)::value and decltype(k)::value.
template <class F>
static inline int with_shape(const CnfConfig& cfg, F&& f) {
#define X(HH, KK)                                      \
  if (cfg.hidden_size == HH && cfg.num_bins == KK)     \
    return f(std::integral_constant<int, HH>{}, std::integral_constant<int, KK>{});
  CNF_KERNEL_CONFIGS(X)
#undef X
  return CNF_ERR_UNSUPPORTED;
}
static inline bool shape_compiled(const CnfConfig& cfg) {
  return with_shape(cfg, [](auto, auto) { return CNF_OK; }) == CNF_OK;
}

// Dynamic LDS above the 64 KB default needs an explicit opt-in per kernel; the
// CU has 160 KB.  Returns false if the request cannot be met.
// The attribute is set once per (kernel, device) for the whole CU (a launch then needs no runtime call but
// the launch itself).
template <class K>
static inline bool ensure_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) return false;
  if (bytes <= 64 * 1024) return true;
  static std::mutex mu;
  // keyed by (kernel, device): kernels of one signature share this instantiation
  static std::map<std::pair<const void*, int>, bool> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair((const void*)kernel, dev);
  auto it = done.find(key);
  if (it != done.end()) return it->second;
  const bool ok = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
  done[key] = ok;
  return ok;
}

// profiling helpers: a record is opened before the (optional) build kernel and closed after the flow kernel
// (samples < 0: a launch that is not recorded)
struct ProfScope {
  CnfModel* m; hipStream_t s; CnfModel::ProfRec r; bool on;
  ProfScope(CnfModel* m_, hipStream_t s_, bool with_build, int64_t samples, int path) : m(m_), s(s_), on(false) {
    r.e0 = r.e1 = r.e2 = nullptr; r.samples = samples; r.path = path;
    if (!m->profiling || samples < 0 || m->prof.size() >= 4096) return;
    if (hipEventCreate(&r.e1) != hipSuccess || hipEventCreate(&r.e2) != hipSuccess) return;
    if (with_build) { if (hipEventCreate(&r.e0) != hipSuccess) return; (void)hipEventRecord(r.e0, s); }
    else (void)hipEventRecord(r.e1, s);
    on = true;
  }
  void built() { if (on && r.e0) (void)hipEventRecord(r.e1, s); }
  void done() { if (on) { (void)hipEventRecord(r.e2, s); m->prof.push_back(r); on = false; } }
};

// The one tail of every kernel family's launch: report `path` (cnf_model_last_path) -- unless the launch is gated on
// the device: its call has reported CNF_PATH_DETECT --, opt in to the LDS, launch `threads` per workgroup and map the
// launch error.  prof_samples >= 0: a kernel of the flow entry points, timed under cnf_model_set_profiling.
template <class K, class A>
static int launch(CnfModel* m, K kernel, int64_t grid, int threads, size_t lds, hipStream_t stream, const A& a, int path,
                  bool gated = false, int64_t prof_samples = -1) {
  if (!gated) m->last_path = path;
  if (!ensure_lds(kernel, lds)) return CNF_ERR_UNSUPPORTED;
  ProfScope ps(m, stream, false, prof_samples, path);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, stream, a);
  ps.done();
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// ... and its sibling for the kernels that report no path (the backward's, whose entry points set theirs themselves, and
// the step's, which have no model): the launch and the mapped error.  ensure_lds, where needed, is the caller's.
template <class K, class... A>
static int launch_plain(K kernel, int64_t grid, int threads, size_t lds, hipStream_t stream, const A&... a) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, stream, a...);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// Workgroups of `kernel` (threads, dynamic LDS bytes) that fit on one CU at a time (registers, LDS, waves), cached.
template <class K>
static inline int resident_blocks_per_cu(K kernel, int threads, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<const void*, int, size_t, int>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple((const void*)kernel, threads, lds, dev);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)kernel, threads, lds) != hipSuccess || n < 1) n = 1;
  // The API has been seen one workgroup per CU high (MI355X_MICROARCH.md: kernels with 81-112 SGPRs; here: 6 reported
  // for 27.8 KB of LDS per workgroup, 5 resident -- profiles/r03b_cfg4), and a grid one round larger than what is
  // resident costs a whole extra round: bound it by the two limits that can be computed here.
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, (const void*)kernel) == hipSuccess) {
    const size_t per_wg = ((lds + fa.sharedSizeBytes + 511) / 512) * 512;              // LDS allocation granularity
    if (per_wg > 0) { const int by_lds = (int)((160 * 1024) / per_wg); if (by_lds >= 1 && by_lds < n) n = by_lds; }
    const int regs = ((fa.numRegs > 0 ? fa.numRegs : 1) + 7) / 8 * 8;                  // unified VGPR file: 512 per SIMD lane
    int waves_per_simd = 512 / regs; if (waves_per_simd > 8) waves_per_simd = 8;
    const int by_regs = waves_per_simd * 4 / ((threads + 63) / 64);
    if (by_regs >= 1 && by_regs < n) n = by_regs;
  }
  cache[key] = n;
  return n;
}

// Grid of a kernel that walks `n_tiles` equal tiles with a grid-stride loop: as many workgroups as are resident at
// once (`capacity`), never more -- a grid of 2 048 single-wave workgroups on 1 536 slots ran a second, quarter-filled
// round as long as the first (profiles/r03a_cfg4).  With every slot taken the tiles that do not divide evenly (config
// 4: 10 923 tiles on 2 048 slots) end as a thinly populated last round in which a wave has its SIMD to itself and runs
// ~1.7 x as fast; giving every workgroup the same count instead (1 821 workgroups x 6 tiles) cost config 4's
// value_and_grad 7 % (1.56 vs 1.455 ms).
static inline int64_t balanced_grid(int64_t n_tiles, int64_t capacity) {
  if (capacity < 1) capacity = 1;
  if (n_tiles < 1) n_tiles = 1;
  return n_tiles < capacity ? n_tiles : capacity;
}

// Argument checks of a term spec (cnf_terms.h computes the terms; anything else must never reach a kernel)
static inline bool potential_ok(int subtype) { return subtype >= CNF_POT_QUADRATIC && subtype <= CNF_POT_OBSTACLE; }
// the reference raises for the 2-D / 3-D fields at other dimensions (applications.py:359,365); SMILE is 2-D by construction
static inline bool drift_ok(int subtype, int D) {
  if (subtype == CNF_DRIFT_SMILE || subtype == CNF_DRIFT_NONGRADIENT) return D == 2;
  if (subtype == CNF_DRIFT_LORENZ) return D == 3;
  return subtype == CNF_DRIFT_OU;
}
// CNF_OK or CNF_ERR_INVALID: the checks of cnf_loss_terms (term_grad_spec_check adds those of the gradient entries)
static inline int term_spec_check(const CnfLossSpec* spec, int D) {
  if (!spec || spec->kind < CNF_TERM_KINETIC || spec->kind > CNF_TERM_DENSITY_L2_DATA) return CNF_ERR_INVALID;
  if (spec->kind <= CNF_TERM_FLOW_MATCHING && !(spec->dt > 0.f)) return CNF_ERR_INVALID;
  if ((spec->kind == CNF_TERM_KINETIC_SCORE || spec->kind == CNF_TERM_FLOW_MATCHING) && !(spec->dx > 0.f))
    return CNF_ERR_INVALID;
  if (spec->kind == CNF_TERM_FLOW_MATCHING && !drift_ok(spec->subtype, D)) return CNF_ERR_INVALID;
  if (spec->kind == CNF_TERM_POTENTIAL && !potential_ok(spec->subtype)) return CNF_ERR_INVALID;
  if (spec->kind == CNF_TERM_REVERSE_KL && (!(spec->T > 0.f) || !(spec->beta > 0.f))) return CNF_ERR_INVALID;
  if ((spec->kind == CNF_TERM_DENSITY_L2 || spec->kind == CNF_TERM_DENSITY_L2_DATA) &&
      (!(spec->coef > 0.f) || !(spec->a > 0.f) || !(spec->T > 0.f)))
    return CNF_ERR_INVALID;
  return CNF_OK;
}
// the checks of cnf_loss_terms_grad(_multi): the density-error terms are evaluation terms and have no backward
static inline int term_grad_spec_check(const CnfLossSpec* spec, int D) {
  if (term_spec_check(spec, D) != CNF_OK || spec->kind > CNF_TERM_NEG_LOGPROB) return CNF_ERR_INVALID;
  return CNF_OK;
}

// Orders a compute call after the last cnf_model_set_params when that ran on a different stream.
static inline int wait_for_params(CnfModel* m, hipStream_t stream) {
  if (m->prep_event && m->prep_stream != (void*)stream)
    if (hipStreamWaitEvent(stream, m->prep_event, 0) != hipSuccess) return CNF_ERR_HIP;
  return CNF_OK;
}

// The checks of a backward entry point on its model, in this order for those asked for in `what`: CHECK_MODEL -- the
// parameters are set and the backward serves the config; CHECK_SLABS -- cnf_grad_enable has made room for gradient
// slabs; CHECK_WAIT -- wait_for_params.  An entry point asks CHECK_MODEL before and the rest after its own return for
// an empty call; where one keeps another order, that check is written out there.
enum { CHECK_MODEL = 1, CHECK_SLABS = 2, CHECK_WAIT = 4 };
static inline int backward_check(CnfModel* m, int what, hipStream_t stream) {
  if ((what & CHECK_MODEL) && !m->params_set) return CNF_ERR_INVALID;
  if ((what & CHECK_MODEL) && !cnf_grad_supported(&m->cfg)) return CNF_ERR_UNSUPPORTED;
  if ((what & CHECK_SLABS) && !m->grad_slabs) return CNF_ERR_INVALID;
  return (what & CHECK_WAIT) ? wait_for_params(m, stream) : CNF_OK;
}

// Zeroes a call's n_sums sums on its stream: CNF_ERR_HIP (< 0), 1 when the call has work to launch, or 0 -- no sum
// or no point: what an empty call returns (CNF_OK).
static inline int zero_sums(double* sums, int64_t n_sums, int64_t n_points, hipStream_t stream) {
  if (n_sums > 0 && hipMemsetAsync(sums, 0, sizeof(double) * (size_t)n_sums, stream) != hipSuccess) return CNF_ERR_HIP;
  return n_sums > 0 && n_points > 0;
}

static inline cnf::ModelArgs model_args(const CnfModel* m) {
  cnf::ModelArgs a;
  a.prep = m->prep; a.per_layer = m->per_layer;
  a.wq = m->mfma_off > 0 ? m->prep + m->mfma_off : nullptr; a.per_layer_q = m->per_layer_q;
  a.D = m->cfg.dim; a.L = m->cfg.num_layers; a.M = m->cfg.mlp_num_layers;
  a.sc = m->sc; a.scd = m->scd;
  a.tabd = reinterpret_cast<const double*>(m->prep + m->tabd_off);
  a.e2tab = reinterpret_cast<const double*>(m->prep + m->e2_off);
  return a;
}
