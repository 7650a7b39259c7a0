// cnf_model.hip -- the model object of libcnf_ot_amd.so, host code only: configuration checks, cnf_model_create /
// destroy, profiling, the knobs, and the per-stream reservation of the dim-2 conditioner-table workspaces
// (cnf_model_reserve, pwl_workspace).  The parameter snapshot (cnf_model_set_params and its two kernels) is in
// cnf_flow.hip.  Declarations: include/cnf_ot_amd.h.
#include "cnf_host.h"
#include "cnf_pwl.h"
#include "cnf_first_table.h"

#include <math.h>
#include <new>
#include <stdlib.h>
#include <string.h>

// ===========================================================================
// C ABI
// ===========================================================================
using namespace cnf;

static int config_valid(const CnfConfig* c) {
  if (!c) return 0;
  if (c->dim < 1 || c->dim > 64) return 0;
  if (c->num_layers < 1 || c->num_layers > 64) return 0;
  if (c->hidden_size < 1 || c->mlp_num_layers < 1 || c->mlp_num_layers > 16) return 0;
  if (c->num_bins < 1 || c->num_bins > 64) return 0;
  if (!(c->range_min < c->range_max)) return 0;
  if (!(c->min_bin_size > 0.f) || !(c->min_knot_slope > 0.f) || !(c->min_knot_slope < 1.f)) return 0;
  if (c->num_bins * c->min_bin_size > c->range_max - c->range_min) return 0;   // distrax raises
  if (c->periodized != 0 && c->periodized != 1) return 0;
  return 1;
}

extern "C" int cnf_config_supported(const CnfConfig* c) {
  return config_valid(c) && shape_compiled(*c) ? 1 : 0;
}

extern "C" void cnf_config_default(CnfConfig* c, int32_t dim) {
  if (!c) return;
  c->dim = dim; c->num_layers = 2; c->hidden_size = 16; c->mlp_num_layers = 2; c->num_bins = 5;
  c->range_min = -10.f; c->range_max = 10.f; c->min_bin_size = 1e-4f; c->min_knot_slope = 1e-4f;
  c->periodized = 0;
}

extern "C" int64_t cnf_param_count(const CnfConfig* c) {
  if (!config_valid(c)) return CNF_ERR_INVALID;
  const int P = 3 * c->num_bins + 1;
  int64_t n = P;
  for (int d = 1; d < c->dim; ++d)
    n += (int64_t)c->num_layers * cond_floats_p(d, c->hidden_size, c->mlp_num_layers, P, c->periodized != 0);
  return n;
}

extern "C" const char* cnf_strerror(int code) {
  switch (code) {
    case CNF_OK: return "ok";
    case CNF_ERR_INVALID: return "invalid argument";
    case CNF_ERR_UNSUPPORTED: return "no kernel compiled for this (hidden_size, num_bins)";
    case CNF_ERR_NOMEM: return "out of memory";
    case CNF_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
  }
}

extern "C" const char* cnf_build_arch(void) { return "gfx950"; }

extern "C" int cnf_model_create(const CnfConfig* cfg, CnfModel** out) {
  if (!out) return CNF_ERR_INVALID;
  *out = nullptr;
  if (!config_valid(cfg)) return CNF_ERR_INVALID;
  if (!cnf_config_supported(cfg)) return CNF_ERR_UNSUPPORTED;
  CnfModel* m = new (std::nothrow) CnfModel();       // value-initialised: scalars and pointers start at zero
  if (!m) return CNF_ERR_NOMEM;
  m->cfg = *cfg;
  const int K = cfg->num_bins, P = 3 * K + 1;
  m->n_params = cnf_param_count(cfg);
  m->per_layer = 0;
  for (int d = 1; d < cfg->dim; ++d)
    m->per_layer += cond_floats_p(d, cfg->hidden_size, cfg->mlp_num_layers, P, cfg->periodized != 0);
  m->sc.lo = cfg->range_min; m->sc.hi = cfg->range_max;
  m->sc.min_bin = cfg->min_bin_size; m->sc.min_slope = cfg->min_knot_slope;
  m->sc.span_eff = (float)(((double)cfg->range_max - (double)cfg->range_min) - (double)K * (double)cfg->min_bin_size);
  m->sc.sp_offset = (float)log(exp(1.0 - (double)cfg->min_knot_slope) - 1.0);
  m->fast_math = 1;
  if (hipGetDevice(&m->device) != hipSuccess) { delete m; return CNF_ERR_HIP; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, m->device) != hipSuccess) { delete m; return CNF_ERR_HIP; }
  m->num_cus = prop.multiProcessorCount;
  // The MFMA conditioner: fp32 MFMA and fp32 VALU do not overlap on gfx950 (their busy times add up:
  // profiles/r01c), so at equal peak rate the packed-VALU conditioner is 4-5 % faster once the chip is full.  A
  // launch of one wave per SIMD is a different regime: a lone wave issues one VALU instruction per 8 cycles
  // (profiles/r01_issue_probe), and the MFMA form has ~45 % fewer of them and no scalar weight loads to wait
  // for -- 6.1 vs 9.8 us per 65 536-sample call (profiles/r02_experiments/exp_latency.log).  2 = by launch size.
  m->use_mfma = 2;
  m->use_pwl = 1;
  m->use_dpar = 1;
  // (D = 1 would need 2^32: encoded as 0, tile_load/tile_store take s = e)
  m->div_magic = cfg->dim == 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + (uint64_t)cfg->dim - 1) / (uint64_t)cfg->dim);
  m->per_layer_q = 0; m->mfma_off = 0;
  size_t q_floats = 0;
  if (cfg->hidden_size == 16 && P == 16 && cfg->dim > 1 && !cfg->periodized) {      // (no MFMA form of the sin / cos layer)
    for (int d = 1; d < cfg->dim; ++d) m->per_layer_q += cond_floats_mfma(d, cfg->mlp_num_layers);
    m->mfma_off = (hdr_floats(K) + (m->n_params - P) + 3) & ~(int64_t)3;
    q_floats = (size_t)m->per_layer_q * cfg->num_layers;
  }
  // float64 copy of the `first` table (exact-mode kernels), 8-byte aligned, after everything else
  m->tabd_off = (hdr_floats(K) + (m->n_params - P) + 4 + (int64_t)q_floats + 1) & ~(int64_t)1;
  // 2^(-i/32), i = 0 .. 1024, float64: the table of the precise position path (cnf_device.h)
  m->e2_off = m->tabd_off + 2 * hdr_floats(K);
  m->precise = 1;
  // the `first` spline's inverse table (cnf_first_table.h), behind everything else: only for the models whose kernels
  // read one (the dim-2 table path at L = 2)
  int64_t n_floats = m->e2_off + 2 * cnf::EXP2_N;
  if (pwl_network(*cfg) && cfg->num_layers == 2 && K == cnf::FT_K) {
    m->ft_off = (n_floats + 3) & ~(int64_t)3;
    n_floats = m->ft_off + cnf::FT_FLOATS;
  }
  const size_t bytes = (size_t)n_floats * sizeof(float) + 64;
  m->scd.lo = (double)cfg->range_min; m->scd.hi = (double)cfg->range_max;
  m->scd.min_bin = (double)cfg->min_bin_size; m->scd.min_slope = (double)cfg->min_knot_slope;
  m->scd.span_eff = (m->scd.hi - m->scd.lo) - (double)K * m->scd.min_bin;
  m->scd.sp_offset = log(exp(1.0 - m->scd.min_slope) - 1.0);
  if (hipMalloc((void**)&m->prep, bytes) != hipSuccess) { delete m; return CNF_ERR_NOMEM; }
  {
    double e2[cnf::EXP2_N];
    for (int i = 0; i < cnf::EXP2_N; ++i) e2[i] = exp2(-(double)i / (double)cnf::EXP2_STEPS);
    if (hipMemcpy(m->prep + m->e2_off, e2, sizeof(e2), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(m->prep); delete m; return CNF_ERR_HIP;
    }
  }
  if (hipEventCreateWithFlags(&m->prep_event, hipEventDisableTiming) != hipSuccess) {
    (void)hipFree(m->prep); delete m; return CNF_ERR_HIP;
  }
  *out = m;
  return CNF_OK;
}

static void prof_clear(CnfModel* m) {
  for (auto& r : m->prof) {
    if (r.e0) (void)hipEventDestroy(r.e0);
    if (r.e1) (void)hipEventDestroy(r.e1);
    if (r.e2) (void)hipEventDestroy(r.e2);
  }
  m->prof.clear();
}

extern "C" void cnf_model_destroy(CnfModel* m) {
  if (!m) return;
  if (m->prep) (void)hipFree(m->prep);
  if (m->grad_slabs) (void)hipFree(m->grad_slabs);
  if (m->pwl_stats) (void)hipFree(m->pwl_stats);
  for (auto& kv : m->pwl_ws) {
    if (kv.second.tables) (void)hipFree(kv.second.tables);
    for (float* p : kv.second.retired) (void)hipFree(p);
  }
  if (m->prep_event) (void)hipEventDestroy(m->prep_event);
  prof_clear(m);
  delete m;
}

/* Which kernels the most recent compute call of this model ran: a CnfPath value (cnf_common.h).
 * Tests use it to assert that a forced path was really taken; bench.py labels its roofline with it. */
extern "C" int cnf_model_last_path(const CnfModel* m) { return m ? m->last_path : CNF_ERR_INVALID; }

/* Internal (bench.py): with profiling on, the flow entry points record HIP events around their kernels
 * (table path: before the table build, between build and flow kernel, after the flow kernel), at most
 * 4096 launches.  cnf_model_read_profile waits for them and returns the SUMS in milliseconds of the
 * dominant (flow) kernel and of the table build, the number of kernel launches and the samples they
 * processed, then clears the records. */
extern "C" int cnf_model_set_profiling(CnfModel* m, int on) {
  if (!m) return CNF_ERR_INVALID;
  m->profiling = on ? 1 : 0;
  if (!on) prof_clear(m);
  return CNF_OK;
}

extern "C" int cnf_model_read_profile(CnfModel* m, double* flow_ms, double* build_ms, int64_t* launches,
                                      int64_t* samples) {
  if (!m) return CNF_ERR_INVALID;
  double f = 0.0, b = 0.0;
  int64_t n = 0, smp = 0;
  for (auto& r : m->prof) {
    if (hipEventSynchronize(r.e2) != hipSuccess) return CNF_ERR_HIP;
    float ms = 0.f;
    if (r.e0) { if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) return CNF_ERR_HIP; b += ms; }
    if (hipEventElapsedTime(&ms, r.e1, r.e2) != hipSuccess) return CNF_ERR_HIP;
    f += ms; ++n; smp += r.samples;
  }
  prof_clear(m);
  if (flow_ms) *flow_ms = f;
  if (build_ms) *build_ms = b;
  if (launches) *launches = n;
  if (samples) *samples = smp;
  return CNF_OK;
}

/* Internal knob used by the tests and the bench: 1 = hardware transcendentals
 * (default), 0 = ocml expf/logf/sqrtf + IEEE division. */
extern "C" int cnf_model_set_fast_math(CnfModel* m, int on) {
  if (!m) return CNF_ERR_INVALID;
  m->fast_math = on ? 1 : 0;
  return CNF_OK;
}

/* Internal knob: 1 = MFMA conditioner wherever available, 0 = packed-VALU conditioner, 2 = MFMA for launches
 * that leave the chip under-filled (default). */
extern "C" int cnf_model_set_mfma(CnfModel* m, int mode) {
  if (!m || mode < 0 || mode > 2) return CNF_ERR_INVALID;
  m->use_mfma = mode;
  return CNF_OK;
}

/* Internal knob: 1 = piecewise-linear conditioner tables at dim 2 for large launches (default),
 * 2 = for every launch they apply to (tests), 0 = always evaluate the MLP. */
extern "C" int cnf_model_set_pwl(CnfModel* m, int mode) {
  if (!m || mode < 0 || mode > 2) return CNF_ERR_INVALID;
  m->use_pwl = mode;
  return CNF_OK;
}

/* Internal knob: the `first` spline of the sampling direction's L = 2 table kernels -- 0 (default) = from its inverse
 * table where the builder has certified it (cnf_first_table.h), 1 = always the closed form. */
extern "C" int cnf_model_set_first_table(CnfModel* m, int mode) {
  if (!m || mode < 0 || mode > 1) return CNF_ERR_INVALID;
  m->first_table_mode = mode;
  return CNF_OK;
}

extern "C" int64_t cnf_internal_first_table_floats(void) { return cnf::FT_FLOATS; }

/* Test entry point: the inverse table as the last cnf_model_set_params left it -- status words, grid, rows
 * (cnf_first_table.h) -- copied to the host buffer out[cnf_internal_first_table_floats()]; waits for the copy.
 * Builds the table first if no launch has asked for it yet.  CNF_ERR_UNSUPPORTED: the model has no table path. */
extern "C" int cnf_internal_first_table(CnfModel* m, void* stream, float* out) {
  if (!m || !out || !m->params_set) return CNF_ERR_INVALID;
  if (m->ft_off <= 0 || !pwl_config_ok(m)) return CNF_ERR_UNSUPPORTED;
  if (wait_for_params(m, (hipStream_t)stream) != CNF_OK) return CNF_ERR_HIP;
  if (!m->ft_built) first_table_enqueue(m, (hipStream_t)stream);      // (as the model's first table launch would)
  if (hipMemcpyAsync(out, m->prep + m->ft_off, sizeof(float) * (size_t)cnf::FT_FLOATS, hipMemcpyDeviceToHost,
                     (hipStream_t)stream) != hipSuccess) return CNF_ERR_HIP;
  return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

/* Internal knob: which kernel builds the dim-2 tables -- 0 = by table count (default; build_tables in cnf_flow.hip),
 * 1 = the reference builder (pwl_build_kernel), 2 = the lean builder (pwl_build_lean_kernel<64>).  Both write the same
 * bytes. */
extern "C" int cnf_model_set_pwl_builder(CnfModel* m, int mode) {
  if (!m || mode < 0 || mode > 2) return CNF_ERR_INVALID;
  m->pwl_builder = mode;
  return CNF_OK;
}

/* The builder the most recent table build ran (1 / 2); 0 before the first build.  A plain field, like last_path:
 * meaningful only while one host thread calls into the model. */
extern "C" int cnf_model_last_pwl_builder(const CnfModel* m) { return m ? m->last_pwl_builder : CNF_ERR_INVALID; }

/* 1 (default): cnf_log_prob / cnf_inverse_logdet (data -> base) carry the knot positions, the offset in the
 * bin and the base term in float64 (cnf_device.h "precise position path"); 0: plain fp32 throughout. */
extern "C" int cnf_model_set_precise(CnfModel* m, int on) {
  if (!m) return CNF_ERR_INVALID;
  m->precise = on ? 1 : 0;
  return CNF_OK;
}

/* Internal knob: wave-per-dimension kernel for base -> data at dim >= 3: 1 = by batch size (default),
 * 2 = always, 0 = never. */
extern "C" int cnf_model_set_dpar(CnfModel* m, int mode) {
  if (!m || mode < 0 || mode > 2) return CNF_ERR_INVALID;
  m->use_dpar = mode;
  return CNF_OK;
}

/* Internal knob: 0 = choose by batch size, 1 / 2 = force samples per lane. */
extern "C" int cnf_model_set_samples_per_lane(CnfModel* m, int spl) {
  if (!m || spl < 0 || spl > 2) return CNF_ERR_INVALID;
  m->force_spl = spl;
  return CNF_OK;
}


void pwl_workspace(CnfModel* m, hipStream_t stream, float** tables, int64_t* sets, uint32_t** flag, uint32_t* epoch) {
  std::lock_guard<std::mutex> lock(m->pwl_mu);
  auto it = m->pwl_ws.find((void*)stream);
  if (it == m->pwl_ws.end()) { *tables = nullptr; *sets = 0; return; }
  *tables = it->second.tables; *sets = it->second.sets;
  // the uniform-condition stamp lives behind the tables; a call that uses it takes a fresh epoch
  if (flag) { *flag = reinterpret_cast<uint32_t*>(it->second.tables + it->second.sets * m->cfg.num_layers * (int64_t)cnf::PWL_TBL);
              *epoch = ++it->second.epoch; }
}

extern "C" int64_t cnf_model_table_bytes(const CnfModel* m) {
  return m ? (int64_t)sizeof(float) * m->cfg.num_layers * cnf::PWL_TBL : 0;
}

extern "C" int cnf_model_reserve(CnfModel* m, void* stream, int64_t n_sets) {
  if (!m || n_sets < 0) return CNF_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->pwl_mu);
  CnfModel::PwlWorkspace& ws = m->pwl_ws[stream];          // value-initialised on first use
  if (ws.sets >= n_sets && n_sets > 0) return CNF_OK;
  if (ws.tables && n_sets > 0) {
    // Growing: the old block is RETIRED, not freed -- a HIP graph captured on this stream has its address baked into
    // kernel arguments and may be replayed at any later time (a stream synchronisation protects running kernels, not
    // future replays).  Retired blocks live until cnf_model_destroy or an explicit release (n_sets = 0); reservations
    // grow geometrically (FlowEngine.reserve), so they add up to less than the current block.
    ws.retired.push_back(ws.tables);
    ws.tables = nullptr; ws.sets = 0;
  }
  if (n_sets == 0) {      // explicit release: the caller vouches that nothing (no graph either) uses this stream's tables
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return CNF_ERR_HIP;
    if (ws.tables) (void)hipFree(ws.tables);
    for (float* p : ws.retired) (void)hipFree(p);
    m->pwl_ws.erase(stream);
    return CNF_OK;
  }
  if (hipMalloc((void**)&ws.tables, (size_t)cnf_model_table_bytes(m) * (size_t)n_sets + 64) != hipSuccess) {
    ws.tables = nullptr; ws.sets = 0;        // (calls on this stream fall back to the MLP kernels; retired blocks stay)
    return CNF_ERR_NOMEM;
  }
  // the stamp of cond_uniform_kernel starts at 0; epochs count from 1
  if (hipMemset(reinterpret_cast<char*>(ws.tables) + (size_t)cnf_model_table_bytes(m) * (size_t)n_sets, 0, 64) != hipSuccess) {
    (void)hipFree(ws.tables); ws.tables = nullptr; ws.sets = 0;
    return CNF_ERR_HIP;
  }
  ws.sets = n_sets; ws.epoch = 0;
  return CNF_OK;
}

extern "C" int64_t cnf_model_reserved(CnfModel* m, void* stream) {
  if (!m) return CNF_ERR_INVALID;
  float* t; int64_t sets;
  pwl_workspace(m, (hipStream_t)stream, &t, &sets);
  return sets;
}

static_assert(cnf::PWL_H == 16, "pwl_network (cnf_common.h) states the tables' network");

extern "C" int cnf_model_has_tables(const CnfModel* m) { return m && pwl_network(m->cfg) ? 1 : 0; }

extern "C" int cnf_model_term_on_tables(const CnfModel* m, int64_t slice_len, int64_t n_points, int with_grad) {
  return m && pwl_term_on_tables(m, slice_len, n_points, with_grad != 0) ? 1 : 0;
}
