/*
 * cnf_ot_amd.h -- C ABI of the MI355X-native conditional RQS flow engine.
 *
 * This is the drop-in boundary for cnf_ot's flow-model call surface: the
 * namedtuple of pure functions returned by RQSFlow(...) and wrapped by
 * hk.multi_transform (reference: cnf_ot/models/flows.py:213-226, consumed by
 * cnf_ot/mfc/applications.py and cnf_ot/mfc/solvers.py:48-53).  Every entry
 * point below names the reference interface it replaces.  The reference is
 * pure Python (no FFI of its own): the binding a maintainer would add is the
 * ctypes stub shown in INTEGRATION.md; cnf_ot_amd/_capi.py is that stub.
 *
 * Conventions
 *  - plain C types only; all tensor arguments are DEVICE pointers to
 *    contiguous row-major float32 unless a parameter says otherwise;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *    every compute entry point only enqueues work on that stream: no
 *    allocation, no synchronisation, graph-capturable.  Device memory is
 *    allocated by cnf_model_create, cnf_model_reserve and cnf_grad_enable only;
 *  - return value: 0 on success, negative CNF_ERR_* otherwise; nothing throws;
 *  - a CnfModel may be used from several host threads as long as each uses its
 *    own stream and nobody calls cnf_model_set_params concurrently; a compute
 *    call on another stream than the last cnf_model_set_params is ordered after
 *    it (event wait), but set_params does not wait for compute calls still in
 *    flight on OTHER streams -- finish those first.
 *
 * Condition argument (`c`, `c_block`): the condition of sample i is
 * c[i / c_block].  c_block == 1 is the per-sample form the reference uses for
 * sampling (cond[B,1] under vmap, conditional.py:400); c_block >= B is the
 * broadcast form it uses for log_prob (cond[1], autoregressive.py:96);
 * c_block == slice length fuses many time-slices into one launch (the shape of
 * cnf_ot/utils.py:311-340).
 */
#ifndef CNF_OT_AMD_H
#define CNF_OT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNF_OK 0
#define CNF_ERR_INVALID (-22)     /* bad argument / shape               */
#define CNF_ERR_UNSUPPORTED (-95) /* config has no compiled kernel      */
#define CNF_ERR_NOMEM (-12)
#define CNF_ERR_HIP (-5)          /* a HIP runtime call failed          */

/* Network configuration: RQSFlow(event_shape=(dim,), num_layers,
 * hidden_sizes=[hidden_size]*mlp_num_layers, num_bins) -- flows.py:178-199,
 * solvers.py:41-47; keys of config/mfc.yaml:29-33.  Spline constants are the
 * ones flows.py:124-132 passes to distrax.RationalQuadraticSpline. */
typedef struct CnfConfig {
  int32_t dim;            /* D: general.dim                         */
  int32_t num_layers;     /* L: cnf.flow_num_layers                 */
  int32_t hidden_size;    /* H: cnf.hidden_size                     */
  int32_t mlp_num_layers; /* M: cnf.mlp_num_layers (>= 1)           */
  int32_t num_bins;       /* K: cnf.num_bins                        */
  float range_min;        /* -10  (flows.py:127)                    */
  float range_max;        /* +10  (flows.py:128)                    */
  float min_bin_size;     /* 1e-4 (distrax default)                 */
  float min_knot_slope;   /* 1e-4 (flows.py:130)                    */
  int32_t periodized;     /* 0; 1 = RQSFlow(periodized=True), flows.py:58-64,127-131: the conditioner MLP sees
                           * [sin(x), cos(x)] of its input x = [c, v] (first linear layer: 2 (1 + d) rows, sin
                           * rows first), boundary_slopes='circular' (the last knot slope is the first); the
                           * caller sets range_min = 0, range_max = 2 pi (a float here: 6.2831855, 1.7e-7 above the reference's
                           * double).  Flow functions only (forward / inverse
                           * / log_prob / sample_logprob, float32 and float64): the loss, gradient and
                           * vector-Jacobian entry points return CNF_ERR_UNSUPPORTED -- no reference call site
                           * passes periodized=True. */
} CnfConfig;

typedef struct CnfModel CnfModel;

/* Fills the reference's defaults (config/mfc.yaml:29-33, flows.py:124-132). */
void cnf_config_default(CnfConfig *cfg, int32_t dim);

/* Number of float32 parameters of the flat layout below; < 0 on bad config.
 * 1 200 at dim=2, 11 824 at dim=10 (solvers.py:135-136 prints this count).
 *
 * Flat layout (this library's own order; it is NOT the order in which haiku
 * creates the parameters -- hk's init traces log_prob, which visits layer L-1
 * first (conditional.py:163-166) -- nor jax's key-sorted flattening: import a
 * haiku tree BY NAME, INTEGRATION.md / cnf_ot_amd/params.py from_tree):
 *   first[P]   then for l in 0..L-1, d in 1..D-1 (module names flows.py:46-86,146-158):
 *   mlp_layer{l}_d{d}/~/linear_0 w[(1+d)][H], b[H]; .../linear_{m} w[H][H],
 *   b[H] (m=1..M-1); linear_out_layer{l}_d{d} w[H][P], b[P];   P = 3K+1. */
int64_t cnf_param_count(const CnfConfig *cfg);

/* Replaces: RQSFlow(...) + hk.multi_transform (flows.py:178-226,
 * solvers.py:41-48).  Allocates the model's private device buffer (prepared
 * `first` knot table + a copy of the conditioner weights) on the current
 * device.  CNF_ERR_UNSUPPORTED if no kernel is compiled for (D,H,K). */
int cnf_model_create(const CnfConfig *cfg, CnfModel **out);
void cnf_model_destroy(CnfModel *m);

/* Replaces: passing `params` to model.apply.* (pure-function convention,
 * applications.py:85,153-158,233-239).  `params` is a device pointer to
 * cnf_param_count() float32 in the flat layout; enqueues a small kernel that
 * normalises the shared, condition-independent `first` spline once (float64
 * on device) and snapshots the weights.  Must precede compute calls; call
 * again after every optimiser step. */
int cnf_model_set_params(CnfModel *m, const float *params, void *stream);

/* Workspace of the dim-2 table path (no reference counterpart: the reference
 * re-evaluates the conditioner MLP per sample, flows.py:57-84).  Large dim-2
 * calls whose condition is uniform over slices read the conditioner from exact
 * piecewise-linear tables, one SET (num_layers tables, cnf_model_table_bytes()
 * bytes) per time-slice and condition; the fused loss terms need up to three
 * sets per slice (t - dt/2, t + dt/2, t).  cnf_model_reserve(m, stream, n_sets)
 * makes room for n_sets sets for calls on `stream` (grows only; n_sets = 0
 * releases it).  It allocates: call it outside graph capture.  A block that a
 * larger reservation replaces stays allocated until cnf_model_destroy (or the
 * release), so a graph captured on the smaller one can still be replayed; the
 * release (n_sets = 0) synchronises `stream`, frees everything and invalidates
 * graphs captured on this model's table path.  Compute calls never allocate: a call with more slices than
 * the reservation holds is processed in chunks, and without a (useful)
 * reservation the same result comes from the MLP kernels.  2 048 sets cover the
 * largest chunk a call is ever split into. */
int cnf_model_reserve(CnfModel *m, void *stream, int64_t n_sets);
int64_t cnf_model_reserved(CnfModel *m, void *stream);
int64_t cnf_model_table_bytes(const CnfModel *m);

/* The library's own answer to "will this run on the tables?", for a caller that composes a loss term from table
 * launches (cnf_sample / cnf_inverse_logdet + cnf_term_residual + cnf_pass_vjp, or cnf_neg_logprob_vjp /
 * cnf_kinetic_potential_vjp) instead of one fused cnf_loss_terms(_grad) launch.  cnf_model_has_tables: 1 if the
 * model's network is the one the tables exist for (dim 2, the reference's conditioner), whatever the knobs say -- a
 * reservation is of use.  cnf_model_term_on_tables: 1 if a term with slices of slice_len points, n_points over all
 * slices of all its passes, is taken by the table kernels as the model stands; with_grad: by the table backward too
 * (after cnf_grad_enable, which allocates its statistics).  Those entry points ask the same question before their
 * own conditions (alignment, odd slice lengths, more than 128 slice sets), so a 1 is not a promise: compose the
 * term from the other calls when one of them still returns CNF_ERR_UNSUPPORTED.  Neither makes a HIP call: both are
 * legal inside a stream capture. */
int cnf_model_has_tables(const CnfModel *m);
int cnf_model_term_on_tables(const CnfModel *m, int64_t slice_len, int64_t n_points, int with_grad);

/* Numerics of the data -> base direction (cnf_log_prob, cnf_inverse_logdet).
 * log_prob = sum_d -x_d^2/2 + ildj multiplies the error of the recovered base
 * point by |x| (up to 5), and an all-fp32 evaluation of the softmax-normalised
 * knots leaves ~2e-6 in x: max |d log_prob| 1.1e-5 .. 1.5e-5 against a float64
 * evaluation of the reference algorithm (conditional.py:316-321 in float64,
 * solvers.py:23) on 65 536 samples.  on = 1 (the default): the softmax terms are
 * evaluated to ~1e-9, and the knot prefix sums, the bin corner, the offset in
 * the bin, the result and the base term are carried in float64 (the conditioner
 * MLP, the slopes and the log-det terms stay fp32): max |d log_prob| ~2e-6, at
 * ~1.5x the time of a data -> base call.  on = 0: plain fp32 throughout (what
 * the fused loss terms use internally for their score differences). */
int cnf_model_set_precise(CnfModel *m, int on);

/* Which kernels the most recent compute call on this model ran: 1/2 = MLP flow
 * kernel with one / two samples per lane, 3 = MFMA conditioner, 4 = conditioner
 * tables, 5/6 = fused loss kernel on the MLP / on tables, 7 = float64, 10 = the fused field kernel,
 * 11 = the exact-score kernel (cnf_score), 12 = the importance-sampling kernel (cnf_importance_stats). */
int cnf_model_last_path(const CnfModel *m);

/* Replaces: model.apply.forward(params, x, c) = flow.bijector.forward, and
 * flow.bijector.forward_and_log_det (flows.py:221-223, conditional.py:233-237,
 * 169-177; autoregressive.py:109-136).  base -> data.  y [B,D]; logdet [B]
 * may be NULL. */
int cnf_forward_logdet(CnfModel *m, const float *x, const float *c,
                       int64_t c_block, float *y, float *logdet, int64_t B,
                       void *stream);

/* Replaces: model.apply.inverse(params, y, c) = flow.bijector.inverse /
 * inverse_and_log_det (conditional.py:239-243,159-167;
 * autoregressive.py:76-107).  data -> base.  logdet may be NULL. */
int cnf_inverse_logdet(CnfModel *m, const float *y, const float *c,
                       int64_t c_block, float *x, float *logdet, int64_t B,
                       void *stream);

/* Replaces: model.apply.log_prob(params, value, cond)
 * (conditional.py:316-321; call sites applications.py:85,272). */
int cnf_log_prob(CnfModel *m, const float *value, const float *c,
                 int64_t c_block, float *logp, int64_t B, void *stream);

/* Replaces: model.apply.sample / sample_and_log_prob(params, cond=, seed=,
 * sample_shape=(B,)) (conditional.py:323-402; call sites
 * applications.py:153-158,233-239, utils.py:330-336) for base noise the caller
 * supplies (noise [B,D] ~ N(0,I), e.g. from cnf_fill_normal).  y [B,D];
 * logp [B] may be NULL (= sample).  THE METRIC KERNEL of BASELINE.json. */
int cnf_sample_logprob(CnfModel *m, const float *noise, const float *c,
                       int64_t c_block, float *y, float *logp, int64_t B,
                       void *stream);

/* Replaces: model.apply.sample / sample_and_log_prob(params, cond=, seed=, sample_shape=(B,)) as the reference
 * calls them (conditional.py:376-402: the base draw happens INSIDE the call): the same as cnf_fill_normal +
 * cnf_sample_logprob, bit for bit, with the noise drawn in the flow kernel -- no noise tensor in HBM (12 instead
 * of 20 bytes per sample at dim 2) and one launch instead of two.  Sample i of the call is sample
 *   first_sample + (i / c_block) * slice_stride + i % c_block
 * of the cnf_fill_normal stream of `seed` (element (sample) * D + d): slice_stride = c_block (or one slice,
 * c_block >= B) draws B consecutive samples, slice_stride = 0 gives every slice the same draw (the reused rng of
 * applications.py:392-400).  Per-sample conditions (c_block = 1) need slice_stride = 1.  logp may be NULL. */
int cnf_sample_logprob_seeded(CnfModel *m, uint64_t seed, int64_t first_sample,
                              int64_t slice_stride, const float *c,
                              int64_t c_block, float *y, float *logp, int64_t B,
                              void *stream);

/* float64 instantiation of the four functions above: the reference computes in
 * float64 (jax.config.update("jax_enable_x64", True), solvers.py:23).  Double
 * IO, double spline table and constants, ocml math, one sample per lane:
 * agrees with a float64 evaluation of the reference algorithm to ~1e-12, at a
 * fraction of the fp32 kernels' speed.  The parameters are the float32 vector
 * given to cnf_model_set_params (each weight is widened exactly). */
int cnf_forward_logdet_f64(CnfModel *m, const double *x, const double *c,
                           int64_t c_block, double *y, double *logdet, int64_t B,
                           void *stream);
int cnf_inverse_logdet_f64(CnfModel *m, const double *y, const double *c,
                           int64_t c_block, double *x, double *logdet, int64_t B,
                           void *stream);
int cnf_log_prob_f64(CnfModel *m, const double *value, const double *c,
                     int64_t c_block, double *logp, int64_t B, void *stream);
int cnf_sample_logprob_f64(CnfModel *m, const double *noise, const double *c,
                           int64_t c_block, double *y, double *logp, int64_t B,
                           void *stream);

/* Replaces: the base draw `Independent(Normal(0,1)).sample(seed=rng, B)`
 * (conditional.py:378,399).  JAX's threefry stream cannot be reproduced
 * (JAX absent, stream version-dependent); the build's stream is
 * Philox4x32-10 + Box-Muller, a pure function of (seed, element index):
 * out[i] = normal(seed, first_element + i).  Sharding a batch over GPUs with
 * first_element = rank_offset * D gives results independent of the GPU count. */
int cnf_fill_normal(uint64_t seed, uint64_t first_element, int64_t n,
                    float *out, void *stream);

/* The same draw as JAX makes it: jax.random.normal(key, shape, float64) with
 * prod(shape) = `size`, key data (key0, key1) (jax.random.PRNGKey(seed) is
 * (seed >> 32, seed & 0xffffffff)), classic (non-partitionable) threefry bit
 * generation; elements [first_element, first_element + n) of the flattened
 * draw, as float32 and / or float64 (either pointer may be NULL).  Threefry-2x32
 * is pinned by the Random123 known answers; the bits -> normal mapping restates
 * jax._src.random and could not be compared with JAX itself (not installable
 * where this was built): use it to reproduce a reference run's base noise, and
 * verify on a JAX box before relying on bit-level agreement. */
int cnf_fill_normal_threefry(uint32_t key0, uint32_t key1, uint64_t size,
                             uint64_t first_element, int64_t n, float *out_f32,
                             double *out_f64, void *stream);

/* ---- fused Monte-Carlo loss terms (cnf_ot/mfc/applications.py) ------------
 * One launch evaluates one term over n_slices time-slices x B samples and
 * returns, per slice, the SUM over that slice's samples (double, device); the
 * caller divides by the global sample count and composes the losses
 * (applications.py:377-441), after an all-reduce when samples are sharded.
 * No [B,D] intermediate reaches HBM. */
enum CnfTermKind {
  /* kinetic_loss_fn, applications.py:220-242 (and utils.py:311-340):
   * sum_{i,d} ((F(x_i,t+dt/2) - F(x_i,t-dt/2)) / dt)^2 on the SAME base noise */
  CNF_TERM_KINETIC = 0,
  /* kinetic_with_score_loss_fn, applications.py:245-276 (utils.py:343-389):
   * v = (r2-r1)/dt + coef * score(r3), score_d by central differences of
   * log_prob at r3 +- dx/2 e_d; sum_{i,d} v^2; coef = 1/beta */
  CNF_TERM_KINETIC_SCORE = 1,
  /* flow_matching_loss_fn, applications.py:279-374: as above with coef = sigma
   * and sum_{i,d} (v - drift_d(r3))^2; drift by `subtype` */
  CNF_TERM_FLOW_MATCHING = 2,
  /* potential_loss_fn, applications.py:176-205: sum_i V(F(x_i,t)) */
  CNF_TERM_POTENTIAL = 3,
  /* reverse_kl_loss_fn, applications.py:129-163:
   * sum_i log_prob_i - log(N(y_i;0,2/beta (T+1) I)(T-t)/T + N(y_i;0,2/beta I) t/T) */
  CNF_TERM_REVERSE_KL = 4,
  /* kl_loss_fn, applications.py:11-86 (after the host mixed the samples):
   * sum_i -log_prob(value_i; t); pts are DATA points, not base noise */
  CNF_TERM_NEG_LOGPROB = 5,
  /* rmse_mc_loss_fn, solvers.py:239-279 (the fp evaluation; the caller takes
   * sqrt(sum / n)): one base -> data pass at t, as REVERSE_KL, giving y_i and
   * lp_i; sum_i (exp(lp_i) - p_mix(y_i; t))^2 with the mixture in linear space
   *   p_mix(y; t) = (1 - t) N(y; 0, v0 I) + t N(y; 0, vT I),
   *   vT = exp(-2 a T) (v0 - 1/(2a)) + 1/(2a),  v0 = coef
   * (the reference hard-codes v0 = 4; its weights are 1 - cond and cond, t is
   * not divided by T, and may lie outside [0, 1]).  An evaluation term: no
   * gradient entry accepts it. */
  CNF_TERM_DENSITY_L2 = 6,
  /* rmse_grid_loss_fn, solvers.py:284-305: the same residual at DATA points
   * (pts as for NEG_LOGPROB; one data -> base pass gives log_prob at the point
   * itself): sum_i (exp(log_prob(pts_i; t)) - p_mix(pts_i; t))^2.  No gradient. */
  CNF_TERM_DENSITY_L2_DATA = 7
};
enum CnfPotential { CNF_POT_QUADRATIC = 0, CNF_POT_DOUBLE_WELL = 1, CNF_POT_OBSTACLE = 2 };
/* drift of flow_matching_loss_fn: OU = -a r (applications.py:310, README);
 * SMILE = the 2-D field that overwrites it (applications.py:353-357);
 * NONGRADIENT (:358-363, dim 2); LORENZ (:364-372, dim 3) */
enum CnfDrift { CNF_DRIFT_OU = 0, CNF_DRIFT_SMILE = 1, CNF_DRIFT_NONGRADIENT = 2, CNF_DRIFT_LORENZ = 3 };

typedef struct CnfLossSpec {
  int32_t kind;      /* CnfTermKind                                         */
  int32_t subtype;   /* CnfPotential or CnfDrift                            */
  float dt, dx;      /* finite-difference steps (general.dt / general.dx)   */
  float coef;        /* 1/beta (KINETIC_SCORE), sigma (FLOW_MATCHING) or the
                        source variance v0 (DENSITY_L2, DENSITY_L2_DATA)    */
  float a;           /* potential / drift parameter (rwpo.a, fp.a)          */
  float T, beta;     /* REVERSE_KL; T also the horizon of the DENSITY_L2s   */
} CnfLossSpec;

/* pts: [n_slices * B, D] when pts_shared == 0 (each slice its own draw, the
 * key-split of utils.py:328), [B, D] when pts_shared != 0 (every slice reuses
 * the same draw: the reused rng of applications.py:392-400).  t: [n_slices].
 * sums: [n_slices] doubles, overwritten.  CNF_ERR_INVALID (nothing enqueued) for a spec
 * the reference does not define: a kind outside CnfTermKind, dt <= 0 (the kinetic
 * and score terms), dx <= 0 (the score terms), a potential subtype outside
 * CnfPotential, a drift subtype outside CnfDrift or one for another dimension
 * (SMILE, NONGRADIENT: dim 2; LORENZ: dim 3), a reverse-KL term with T <= 0 or
 * beta <= 0, a density-error term (DENSITY_L2, DENSITY_L2_DATA) with coef <= 0,
 * a <= 0 or T <= 0. */
int cnf_loss_terms(CnfModel *m, const CnfLossSpec *spec, const float *pts,
                   int pts_shared, const float *t, int64_t n_slices, int64_t B,
                   double *sums, void *stream);

/* Same as cnf_loss_terms with the base noise drawn inside the kernel (no noise
 * tensor in HBM): sample i of slice s is sample (first_sample + s * slice_stride
 * + i) of the cnf_fill_normal stream of `seed`.  slice_stride = 0: every slice
 * reuses the same draw (applications.py:392-400); slice_stride = batch size:
 * each slice its own draw (the key split of utils.py:328).  Not for
 * CNF_TERM_NEG_LOGPROB or CNF_TERM_DENSITY_L2_DATA (whose points are data):
 * CNF_ERR_INVALID. */
int cnf_loss_terms_seeded(CnfModel *m, const CnfLossSpec *spec, uint64_t seed,
                          int64_t first_sample, int64_t slice_stride,
                          const float *t, int64_t n_slices, int64_t B,
                          double *sums, void *stream);

/* ---- value_and_grad + Adam (cnf_ot/mfc/solvers.py:90-97) -------------------
 * Backward pass of the loss terms, for the reference's network (hidden 16, two
 * hidden layers, 5 bins; dim <= 14 -- the first layer's inputs + bias row are 16 MFMA rows, and the tile's working set
 * must fit one CU's LDS): cnf_grad_supported() tells.  A model's gradient
 * slabs are shared state: do not run two gradient calls of the same model
 * concurrently on different streams.  More exactly: the gradient entry points of ONE CnfModel (cnf_loss_terms_grad[_multi],
 * cnf_pass_vjp, cnf_neg_logprob_vjp, cnf_kinetic_potential_vjp, cnf_logprob_fd_vjp, cnf_score_fd_vjp) must be ORDERED
 * on one stream, or across streams by events: the adjoint maximum, the per-piece statistics and the slabs exist once
 * per model, not once per stream (only the table workspaces of cnf_model_reserve are per stream), and nothing in the
 * library orders two such calls.  A step that is warmed up and captured on a side stream (solvers.CapturedUpdate)
 * relies on its wait_stream pairs around every warm-up step, and on the capture's own fork and join, for that order
 * against the caller's stream.
 *
 * cnf_grad_enable allocates the per-wave gradient slabs (the only allocation;
 * call once, outside any graph capture; max_blocks <= 0: a default).
 *
 * cnf_loss_terms_grad = cnf_loss_terms (same arguments and spec checks, same `sums`; the evaluation terms
 * CNF_TERM_DENSITY_L2 and CNF_TERM_DENSITY_L2_DATA have no backward: CNF_ERR_INVALID, nothing enqueued, here and in
 * cnf_loss_terms_grad_multi and cnf_term_residual) PLUS
 *   grad[p] += scale * d(sum over all slices and samples of the term)/d params[p]
 * `grad` (device, cnf_param_count() floats) is ACCUMULATED into, so the caller
 * zeroes it once and adds every term of a composite loss with its coefficient
 * as `scale`.  `params` is the same flat vector that was given to
 * cnf_model_set_params.  Results are deterministic (no float atomics). */
int cnf_grad_supported(const CnfConfig *cfg);
int cnf_grad_enable(CnfModel *m, int64_t max_blocks);
int cnf_loss_terms_grad(CnfModel *m, const CnfLossSpec *spec, const float *pts,
                        int pts_shared, const float *t, int64_t n_slices,
                        int64_t B, float scale, double *sums, float *grad,
                        const float *params, void *stream);

/* Up to 4 terms of one composite loss (applications.py:377-441) in ONE launch: term i with its own points, slices,
 * batch and coefficient (arrays of n_terms entries; sums[i] has n_slices[i] doubles).  The terms' tiles share the grid,
 * so several small terms run side by side instead of one under-filled launch after the other -- a default-config
 * training step (config/mfc.yaml: batch 2 048) is three terms of 8 tiles each.  Same result as n_terms calls of
 * cnf_loss_terms_grad up to the order of the float32 additions into `grad`. */
int cnf_loss_terms_grad_multi(CnfModel *m, int32_t n_terms, const CnfLossSpec *specs,
                              const float *const *pts, const int32_t *pts_shared,
                              const float *const *t, const int64_t *n_slices,
                              const int64_t *B, const float *scale,
                              double *const *sums, float *grad, const float *params,
                              void *stream);

/* Replaces the autodiff helpers of the Flow tuple (flows.py:203-211):
 *   forward_jac = vmap(jacfwd(flow.bijector.forward)),
 *   inverse_jac = vmap(jacfwd(flow.bijector.inverse)),
 *   gauge_potential = jacfwd(log|det J| of forward)
 * through one primitive, the vector-Jacobian product of a flow pass w.r.t. its
 * input points:  xbar[b,:] = ybar[b,:] . dF/dx(b) + ldbar[b] * d logdet/dx(b).
 * to_base = 0: F = flow.bijector.forward (base -> data); 1: the inverse.
 * ybar [B,D] and ldbar [B] may each be NULL (= 0), not both.  Row i of the
 * Jacobian is the call with ybar = e_i.  Same config support as the gradients. */
int cnf_input_vjp(CnfModel *m, int to_base, const float *pts, const float *c,
                  int64_t c_block, const float *ybar, const float *ldbar,
                  float *xbar, int64_t B, void *stream);

/* The backward of a differentiable flow op: cnf_input_vjp PLUS the parameter
 * gradient of the same pass,
 *   grad[p] += sum_b ( ybar[b,:] . dF/dp(b) + ldbar[b] * d logdet/dp(b) ),
 * so that any loss composed on the host from flow passes (e.g. under
 * torch.autograd: cnf_ot_amd/autograd.py) gets exact gradients -- what
 * jax.value_and_grad gives the reference for losses not in applications.py.
 * xbar may be NULL; grad is accumulated (needs cnf_grad_enable).
 * At dim 2, with a condition that is uniform over slices (c_block >= 8 192) and >= 262 144 points, and tables
 * reserved on the stream for min(n_slices, 128) slices (cnf_model_reserve), the pass runs on the conditioner tables:
 * per-piece sufficient statistics in 64-bit fixed point instead of per-sample weight gradients --
 * same result to ~1e-6, about twice as fast, bitwise reproducible.  Nothing is allocated here: the statistics
 * buffer comes with cnf_grad_enable. */
int cnf_pass_vjp(CnfModel *m, int to_base, const float *pts, const float *c,
                 int64_t c_block, const float *ybar, const float *ldbar,
                 float *xbar, float *grad, const float *params, int64_t B,
                 void *stream);

/* Value and gradient of the density-fit term in ONE launch over the data (kl_loss_fn, applications.py:11-86, under
 * jax.value_and_grad, solvers.py:94):
 *   sums[s] = -sum_{i in slice s} log_prob(pts_i; c_s),   grad[p] += loss_coef * d(sum_s sums[s]) / dp
 * -- the table form of cnf_pass_vjp in the data -> base direction with the output adjoints formed in the kernel
 * (ybar = loss_coef * base point, ldbar = -loss_coef), so neither cnf_inverse_logdet nor cnf_term_residual nor the
 * adjoint scan run, and the tables are built once.  Same conditions as the table form of cnf_pass_vjp;
 * CNF_ERR_UNSUPPORTED where it does not apply: the caller composes the term from those three calls. */
int cnf_neg_logprob_vjp(CnfModel *m, const float *pts, const float *c,
                        int64_t c_block, float loss_coef, double *sums,
                        float *grad, const float *params, int64_t B,
                        void *stream);

/* Value and gradient of the kinetic (+ potential) term of ot_loss_fn in one call (kinetic_loss_fn / potential_loss_fn,
 * applications.py:176-242, as ot_loss_fn combines them, :388-402, under jax.value_and_grad, solvers.py:94): the ONE
 * base draw z [count, 2] pushed to the S times t_s - dt/2, t_s + dt/2 and -- with subtype >= 0 (CnfPotential) -- t_s:
 *   kin[s] = sum_i |(r2_i - r1_i) / dt|^2,  pot[s] = sum_i V(r3_i),
 *   grad[p] += c_kin d(sum_s kin[s]) / dp + c_pot d(sum_s pot[s]) / dp.
 * c: the 2 S (3 S) conditions [t - dt/2 | t + dt/2 | t] as the caller rounds them.  One table build, one forward
 * launch in which all slices read the same z (no repeated copy of it), the term epilogues, which also leave the largest
 * adjoint for the backward (no scan), and one backward launch -- what cnf_sample + cnf_term_residual + cnf_pass_vjp do
 * in six launches over 2 (3) S repeated copies of z.  work: 4 x 2 (3) S x count floats, 16-byte aligned (the pushed
 * points and their adjoints).  pot == NULL iff subtype < 0; subtype > 2: CNF_ERR_INVALID.  grad == NULL: the terms' values alone (the loss without
 * jax.value_and_grad; work: 2 x 2 (3) S x count floats).  CNF_ERR_UNSUPPORTED (nothing written) where the table
 * backward does not apply or 2 (3) S > 128: compose the term from those calls. */
int cnf_kinetic_potential_vjp(CnfModel *m, const float *z, int64_t count,
                              const float *c, int32_t S, float dt, float c_kin,
                              int32_t subtype, float pot_a, float c_pot,
                              double *kin, double *pot, float *grad,
                              const float *params, float *work, void *stream);

/* The score of the flow's density by central differences, the way the reference
 * forms it (kinetic_with_score_loss_fn / flow_matching_loss_fn,
 * applications.py:264-273; utils.py:366-381):
 *   score[i, d] = (log_prob(r_i + dx/2 e_d) - log_prob(r_i - dx/2 e_d)) / dx
 * for B points r_i [B, D] (the 2 D evaluation points of a point are generated in
 * the kernel: 2 D B flow passes spread over the whole GPU, nothing but `score`
 * [B, D] is written).  cnf_logprob_fd_vjp is its backward:
 *   pts_bar[i, :] = sum_d gbar[i, d] * d score[i, d] / d r_i      (may be NULL)
 *   grad[p]      += sum_{i,d} gbar[i, d] * d score[i, d] / d params[p]
 * (needs cnf_grad_enable; same config support as the other gradients). */
int cnf_logprob_fd(CnfModel *m, const float *pts, const float *c,
                   int64_t c_block, float dx, float *score, int64_t B,
                   void *stream);
int cnf_logprob_fd_vjp(CnfModel *m, const float *pts, const float *c,
                       int64_t c_block, float dx, const float *gbar,
                       float *pts_bar, float *grad, const float *params,
                       int64_t B, void *stream);

/* The exact score of the flow's density and, optionally, log_prob, from ONE launch:
 *   score[s*count + i, :] = grad_x log_prob(x_si; c[s]),   log_prob[s*count + i]  (may be NULL)
 * for n_slices conditions c[s] and `count` points per slice: pts [n_slices*count, D], or, with pts_shared != 0,
 * the same [count, D] points for every slice (a grid at several times).  This is the derivative that the
 * reference's difference quotient (log_prob(r + dx/2 e_d) - log_prob(r - dx/2 e_d)) / dx approximates
 * (utils.py:366-381, applications.py:264-273; cnf_logprob_fd is that quotient): with z = F^-1(x, c),
 *   log_prob = -|z|^2 / 2 - D/2 log 2 pi + ildj,   grad_x log_prob = (dz/dx)^T (-z) + grad_x ildj,
 * one data -> base pass with its layer inputs kept and its reverse pass seeded with (-z, 1) -- what
 * cnf_inverse_logdet + a negation + cnf_input_vjp(to_base = 1) compose from two forward passes; no dx, and one
 * reverse pass where the quotient takes 2 D forward passes.  An evaluation quantity: the loss terms keep the
 * reference's quotient.  fp32: the base point z and ildj come from the plain-fp32 pass (not the precise position
 * path); log_prob alone is summed in float64 from those fp32 values and rounded once, so it is close to, but not
 * bit for bit, what cnf_log_prob gives under cnf_model_set_precise(0).  A non-finite point gives a non-finite score
 * row and log_prob for that point only.
 * Checks come first: CNF_ERR_INVALID for NULL pts / c / score, negative sizes or parameters not set;
 * CNF_ERR_UNSUPPORTED (nothing written or enqueued) where cnf_grad_supported is false.  n_slices == 0 or count == 0:
 * CNF_OK, no launch.  Neither allocates nor synchronises (legal inside a stream capture) and needs no
 * cnf_grad_enable: no gradient slab is written. */
int cnf_score(CnfModel *m, const float *pts, int32_t pts_shared, const float *c,
              int64_t n_slices, int64_t count, float *score, float *log_prob, void *stream);

/* The score terms' value AND backward in one launch (value_and_grad of kinetic_with_score_loss_fn /
 * flow_matching_loss_fn, applications.py:245-374, composed from separate flow launches -- the form
 * cnf_ot_amd.applications uses from dim 6 up).  r [3n, D] = the samples at t - dt/2 | t + dt/2 | t from one
 * base -> data launch; per slice of `count` points (condition c[slice])
 *   sums[s] = sum_{i,d} u_{i,d}^2,  u = (r2 - r1)/dt + coef * score_d(r3) - drift_d(r3),
 * score by central differences of log_prob as in cnf_logprob_fd, drift = CNF_DRIFT_OU (-a r) or -1 (none).
 * For d(loss) = loss_coef * d(sum of sums):  rbar [3n, D] receives the adjoints of r (all three blocks, the
 * r3 block complete: drift, score and the 2 D evaluation points' input adjoints), grad the parameter gradient
 * (accumulated; needs cnf_grad_enable).  Equals cnf_logprob_fd + cnf_score_residual + cnf_logprob_fd_vjp, but
 * the 2 D n evaluation points are pushed through the flow ONCE: the kernel that differentiates them forms the
 * score from its own forward passes (no separate forward launch, no score / sbar tensors). */
int cnf_score_fd_vjp(CnfModel *m, const float *r, const float *c, int64_t count,
                     float dt, float dx, float coef, int32_t drift, float a,
                     float loss_coef, double *sums, float *rbar, float *grad,
                     const float *params, int64_t n, void *stream);

/* Epilogues of loss terms composed from separate flow launches (what
 * cnf_ot_amd.applications does from dim 6 up, where a rank's few samples cannot
 * fill the GPU from inside one fused kernel).  Model-independent, like
 * cnf_adam_step.
 *
 * cnf_score_residual: r [3n, D] = the samples at t - dt/2 | t + dt/2 | t (one
 * base -> data launch), score [n, D] from cnf_logprob_fd; per slice of `count`
 * samples  sums[s] = sum_{i,d} ((r2 - r1)/dt + coef score - drift_d(r3))^2
 * (kinetic_with_score_loss_fn / flow_matching_loss_fn, applications.py:245-374;
 * drift = CnfDrift, or -1 for none; anything else, or a drift for another
 * dimension, is CNF_ERR_INVALID).  With rbar / sbar non-NULL it also writes
 * the adjoints of r and score for d(loss) = loss_coef * d(sum of sums): the
 * seeds of cnf_logprob_fd_vjp and cnf_pass_vjp.
 *
 * cnf_rkl_residual: y [n, D], lp [n] from cnf_sample_logprob;
 * sum = sum_i lp_i - log(mixture(y_i)) of reverse_kl_loss_fn
 * (applications.py:129-163), adjoints ybar / lpbar likewise.  The mixture is
 * a log-sum-exp over the WEIGHTED exponents: at t == 0 and t == T the
 * component of weight zero drops out, and sum, ybar stay finite wherever the
 * remaining density is representable as a float32 logarithm. */
/* cnf_term_residual: value and adjoints of the kinetic / potential / density-fit terms composed from separate flow
 * launches (kinetic_loss_fn applications.py:220-242: r = [r1 | r2], 2 n points, p0 = dt; potential_loss_fn :176-205:
 * r = n points, subtype = CnfPotential (else CNF_ERR_INVALID), p0 = a; kl_loss_fn :11-86: r = the recovered base
 * points, aux = ildj).
 * sums [ceil(n / count)] per slice; rbar (and auxbar for the density fit) receive loss_coef * d(sum) / d(.) when
 * non-NULL. */
int cnf_term_residual(int32_t kind, const float *r, const float *aux, int64_t n,
                      int64_t count, int32_t D, int32_t subtype, float p0,
                      float loss_coef, double *sums, float *rbar, float *auxbar,
                      void *stream);
int cnf_score_residual(const float *r, const float *score, int64_t n,
                       int64_t count, int32_t D, float dt, float coef,
                       int32_t drift, float a, float loss_coef, double *sums,
                       float *rbar, float *sbar, void *stream);
/* cnf_score_residual with an interaction force inside the square (the interacting Fokker-Planck residual):
 * force [n, D] = the force at the n samples r3 (cnf_interaction, self mode, per slice),
 *   u = (r2 - r1)/dt + coef score - drift_d(r3) + strength force,   sums[s] = sum_{i,d} u_{i,d}^2,
 * for every drift cnf_score_residual takes.  With rbar / sbar / fbar non-NULL (all three or none) it also writes
 * fbar [n, D] = strength * u_bar, the adjoint of the force: the seed of cnf_interaction_vjp.  CNF_ERR_INVALID: what
 * cnf_score_residual refuses, a NULL force, an fbar that does not match rbar. */
int cnf_score_residual_force(const float *r, const float *score, const float *force, float strength,
                             int64_t n, int64_t count, int32_t D, float dt, float coef,
                             int32_t drift, float a, float loss_coef, double *sums, float *rbar,
                             float *sbar, float *fbar, void *stream);
int cnf_rkl_residual(const float *y, const float *lp, int64_t n, int32_t D,
                     float t, float T, float beta, float loss_coef, double *sum,
                     float *ybar, float *lpbar, void *stream);

/* optax.adam(lr) update in place (solvers.py:55,95-96): b1 = 0.9, b2 = 0.999,
 * eps = 1e-8 are optax's defaults; `step` counts from 1. */
int cnf_adam_step(float *params, const float *grad, float *mu, float *nu,
                  int64_t n, float lr, float b1, float b2, float eps,
                  int64_t step, void *stream);

/* ---- a training step as ONE device-side program (cnf_ot/mfc/solvers.py:90-105: the reference's step is one jitted
 * XLA program; here: one HIP graph, captured once and replayed) ----------------------------------------------------
 * What changes from step to step must not be a kernel argument of a captured step: the random key and the step
 * count live in device memory, `state` = uint64[2] = { step count, key }.  The caller writes state[1] (one 8-byte
 * copy) before a step; cnf_step_begin increments the count; the draws below read the key on the device:
 *   cnf_fill_normal_dev     out[i] = element first_element + i of the cnf_fill_normal stream of the key
 *                           (base noise; conditional.py:378,399)
 *   cnf_fill_uniform_dev    out[i] = scale * uniform[0, 1)        (the time batch, applications.py:392,414,434)
 *   cnf_mixture_source_dev  out[i, :] = z[i, :] + centre of a uniformly drawn component of the 8-mode source
 *                           (dim 2; applications.py:34-71); comp (optional) receives the component indices
 * cnf_adam_step_dev is cnf_adam_step with `step` = state[0]; cnf_weighted_sum (out = sum v[i] w[i], one block, fixed
 * order) composes a loss from its terms' partial sums without a BLAS call inside the capture. */
int cnf_step_begin(uint64_t *state, void *stream);
int cnf_fill_normal_dev(const uint64_t *state, uint64_t first_element, int64_t n,
                        float *out, void *stream);
int cnf_fill_uniform_dev(const uint64_t *state, uint64_t first, int64_t n,
                         float scale, float *out, void *stream);
int cnf_mixture_source_dev(const uint64_t *state, uint64_t first_sample, int64_t n,
                           const float *z, float *out, int32_t *comp, void *stream);
int cnf_adam_step_dev(float *params, const float *grad, float *mu, float *nu,
                      int64_t n, float lr, float b1, float b2, float eps,
                      const uint64_t *state, void *stream);
int cnf_weighted_sum(const double *v, const double *w, int64_t n, double *out,
                     void *stream);

/* ---- the exact 2-D rwpo solution for evaluation (cnf_ot/mfc/2d_WPO_ref_solution.py:60-187, solvers.py:170-232) ----
 * The regularized Wasserstein proximal problem's solution by the Hopf-Cole kernel formula, as the reference's offline
 * generator sums it on a uniform grid, with eps = 1 / beta and g = the potential of potential_loss_fn (CnfPotential,
 * `a` as the loss spec carries it):
 *   h(y)      = sum_z exp(-(g(z) + |y - z|^2 / (2T)) / (2 eps)) dz^2     over |z_i - y_i| <= window
 *   rho_T(x)  = sum_y exp(-(g(x) + |x - y|^2 / (2T)) / (2 eps)) rho0(y) / h(y) dz^2
 *   score_T   = -grad g(x) / (2 eps) - (x - m(x)) / (2 eps T),  m = the rho0 / h weighted mean of y
 *   w0        = -(x - m0(x)) / T + eps x,  m0 weighted by exp(-g(y) / (2 eps))
 *   wT        = -grad g - eps score_T
 *   true_value = -2 eps sum_y rho0(y) (log h(y) - log(4 pi eps T)) dz^2    (the optimal rwpo energy)
 *   ic_mass    = sum_y rho0(y) dz^2                                        (how much of rho0 the y grid holds)
 * rho0 = N(0, var0 I).  Grids are index-based: y = k dz for |k| <= n_y = round(y_range / dz), z = k dz for
 * |k| <= n_y + n_w, n_w = round(window / dz), a z term counted iff its index offset is <= n_w per coordinate.
 * Outputs (device, float64) on the tensor grid x1 [n1] x x2 [n2], x1 fastest: log_rho [n2, n1] (the log: nothing
 * underflows); score, w0, wT [n2, n1, 2], each optional (NULL: not computed); true_value, ic_mass: one double each,
 * optional.  n1 = n2 = 0 (x1, x2, log_rho NULL): the true value and the mass only.  Every sum is a float64
 * log-sum-exp in a fixed order: no atomics, repeated calls are bit-identical.
 * cnf_hopf_cole_workspace: the device workspace cnf_hopf_cole_2d needs, in bytes (~8 ((2 n_y + 2 n_w + 1)^2 + ...)).
 * CNF_ERR_INVALID: T, beta, var0, dz, window or y_range <= 0 or not finite; an unknown potential; n_y, n_w, n1 or
 * n2 above 2^19; only one of n1, n2 zero; a required pointer NULL; the workspace too small. */
int cnf_hopf_cole_workspace(double dz, double window, double y_range,
                            int64_t n1, int64_t n2, int64_t *bytes);
int cnf_hopf_cole_2d(int32_t subtype, float a, double T, double beta,
                     double var0, double dz, double window, double y_range,
                     const double *x1, int64_t n1, const double *x2,
                     int64_t n2, double *log_rho, double *score, double *w0,
                     double *wT, double *true_value, double *ic_mass,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* The same solution at every time of times [S] (a HOST array, 0 <= t <= T), from the quantities above: h, the
 * potential table and the value once per call, then for 0 < t < T, with lg = -g / (2 eps) on the whole z grid:
 *   log eta_t(x)    = log sum_z exp(lg(z) - |x - z|^2 / (4 eps (T - t))) dz^2 - log(4 pi eps (T - t)),  m_b = mean of z
 *   log etahat_t(x) = log sum_y exp(log rho0(y) - log h(y) - |x - y|^2 / (4 eps t)) dz^2 + log(T / t),  m_f = mean of y
 *   log_rho = log eta_t + log etahat_t
 *   drift   = -(x - m_b) / (T - t)             (2 eps grad log eta_t: the optimal control; -grad g at T)
 *   score   = -(x - m_b) / (2 eps (T - t)) - (x - m_f) / (2 eps t)
 *   vel     = drift - eps score                (the current velocity: what a flow's velocity field must equal;
 *                                               kinetic_with_score_loss_fn penalises |v + score / beta|^2)
 * The endpoints are exact, with no narrow kernel.  t == T: log_rho, score and vel are cnf_hopf_cole_2d's log_rho,
 * score and wT bit for bit, drift = -grad g.  t == 0: log_rho = log rho0(x), score = -x / var0, drift =
 * -(x - m0) / T with w0's m0, vel = drift + eps x / var0.  (cnf_hopf_cole_2d's w0 = drift + eps x is the generator's
 * form, the velocity at 0 for var0 = 1 only: vel(0) - w0 = eps x (1 / var0 - 1).)
 * Outputs (device, float64): log_rho [S, n2, n1]; score, drift, vel [S, n2, n1, 2], each optional.  The interior
 * times are summed 8 per launch from one staged copy of the source table: five launches per 8 times, whatever S;
 * a time equal to T adds one epilogue launch.  Fixed summation order, no atomics: repeated calls are bit-identical and
 * a call with S times equals S calls with one.  No allocation, no synchronisation.
 * CNF_ERR_INVALID (nothing is written): cnf_hopf_cole_2d's cases; n1 or n2 == 0; S < 1 or above 2^19; times NULL; a
 * time < 0, > T or not finite; an interior time with sqrt(2 eps min(t, T - t)) < 1.5 dz (the narrower Gaussian kernel
 * has that standard deviation; the uniform rule's aliasing error is about 2 exp(-2 pi^2 sigma^2 / dz^2), 1e-19 at
 * sigma = 1.5 dz, so from there up the quadrature is exact at float64 level). */
int cnf_hopf_cole_path_workspace(double dz, double window, double y_range,
                                 int64_t n1, int64_t n2, int64_t *bytes);
int cnf_hopf_cole_path_2d(int32_t subtype, float a, double T, double beta,
                          double var0, double dz, double window, double y_range,
                          const double *times, int64_t S, const double *x1,
                          int64_t n1, const double *x2, int64_t n2,
                          double *log_rho, double *score, double *drift,
                          double *vel, double *true_value, double *ic_mass,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* ---- fields and characteristics of a trained flow (cnf_ot/utils.py:598-798 as solvers.py:309-493 calls it) --------
 * The arrays under the reference's figures, for S times in ONE launch; nothing but the results reaches HBM.
 *
 * cnf_eulerian_fields: fields at N fixed points of data space, at each of the times t [S].  Replaces the
 * log_prob_fn(params, XY, cond=t_i) loops of plot_density_and_trajectory (utils.py:615-625),
 * plot_high_dim_density_and_trajectory (:662-678) and plot_proj_density (:711-745), and what plot_velocity_field /
 * plot_traj_and_velocity (:754-797) evaluate on their grids.  The points are either pts [N, D] or -- grid != NULL,
 * pts == NULL, N = nx * ny -- a regular 2-D grid generated in the kernel: point i * nx + j has coordinate axis_x =
 * lo_x + j * step_x, coordinate axis_y = lo_y + i * step_y (the reference's meshgrid + hstack; a float64 product and
 * sum rounded to the kernel's type, numpy.linspace's arithmetic), the other coordinates `fixed` [D] (device; the
 * entries of the grid's axes are ignored), and coordinate sec_axis = sec [n_sec] (device) when sec != NULL
 * (sec == NULL: sec_axis = -1, n_sec = 1).  Per (time t_j, point r) one data -> base pass at t_j gives the base
 * point xi and log_prob.  Outputs, each optional (NULL: not computed, its passes not run), at least one:
 *   rho   [S, N]     mean over the sections of exp(log_prob) (plot_proj_density's prob / len(section)); the sections
 *                    are summed in float64 in a fixed order inside one thread: no atomics, calls are bit-identical
 *   logp  [S, N]     log_prob                                                             (n_sec = 1 only)
 *   vel   [S, N, D]  (F(xi, t_j + dt/2) - F(xi, t_j - dt/2)) / dt, two base -> data passes on xi  (n_sec = 1 only)
 *   score [S, N, D]  (log_prob(r + dx/2 e_d) - log_prob(r - dx/2 e_d)) / dx, 2 D data -> base passes in plain fp32
 *                    as in cnf_logprob_fd                                                  (n_sec = 1 only)
 * The float32 kernel runs the density pass on the precise position path (cnf_model_set_precise's "on") and needs
 * hardware transcendentals (the default); the _f64 entry points are the exact mode (all device arrays double,
 * `fixed` and `sec` included).  A non-finite point gives NaN results for that point only.
 *
 * cnf_trajectories: the characteristics r(t) = F(F^-1(r0, t0), t) of plot_density_and_trajectory (utils.py:619,
 * 626-627) and plot_high_dim_density_and_trajectory (:670, 679-680): one data -> base pass at t0 per point (per time
 * while the launch is too small to fill the GPU otherwise), then the base -> data passes on the same xi: traj
 * [S, N, D], and with vel != NULL the central-difference velocity along each trajectory, vel [S, N, D] as above.
 * traj or vel may be NULL, not both.
 *
 * CNF_ERR_UNSUPPORTED (nothing enqueued): dim > 14, periodized, or float32 without hardware transcendentals --
 * compose the result from cnf_log_prob / cnf_inverse_logdet / cnf_forward_logdet / cnf_logprob_fd.
 * CNF_ERR_INVALID: both or neither of grid / pts, no output, a grid that does not have N points, axes outside the
 * event or equal, dt <= 0 with vel, dx <= 0 with score, more than one section with anything but rho. */
typedef struct CnfFieldGrid {
  double lo_x, lo_y, step_x, step_y;
  int32_t nx, ny;
  int32_t axis_x, axis_y; /* the event axes the grid spans                                  */
  int32_t sec_axis;       /* the axis of the sections, -1 for none                          */
  int32_t n_sec;          /* >= 1                                                           */
  const void *fixed;      /* device [D], of the entry point's real type                     */
  const void *sec;        /* device [n_sec], of the entry point's real type, or NULL        */
} CnfFieldGrid;
int cnf_eulerian_fields(CnfModel *m, const CnfFieldGrid *grid, const float *pts,
                        int64_t N, const float *t, int64_t S, float dt, float dx,
                        float *rho, float *logp, float *vel, float *score,
                        void *stream);
int cnf_eulerian_fields_f64(CnfModel *m, const CnfFieldGrid *grid, const double *pts,
                            int64_t N, const double *t, int64_t S, double dt,
                            double dx, double *rho, double *logp, double *vel,
                            double *score, void *stream);
int cnf_trajectories(CnfModel *m, const float *r0, int64_t N, float t0,
                     const float *t, int64_t S, float dt, float *traj, float *vel,
                     void *stream);
int cnf_trajectories_f64(CnfModel *m, const double *r0, int64_t N, double t0,
                         const double *t, int64_t S, double dt, double *traj,
                         double *vel, void *stream);

/* ---- a particle reference for the Fokker-Planck problems (applications.py:279-374; the reference's tests/test_lorenz.py
 * sketches it) ----------------------------------------------------------------------------------------------------
 * flow_matching_loss_fn fits v_flow + sigma grad log rho = drift, the continuity form of
 * d rho / dt = -div(rho drift) + sigma lap rho: the density is the law of dX = drift(X) dt + sqrt(2 sigma) dW.
 * cnf_fp_particles integrates N particles of dimension D from X_0 ~ N(0, var0 I) by n_steps Euler-Maruyama steps
 *   x <- x + h drift(x) + sqrt(2 sigma h) z
 * in float64, drift = CnfDrift with parameter `a` exactly as the loss kernels evaluate it (one definition; its float32
 * constants a, 28/9 and 8/3 widened).  The normals are the cnf_fill_normal(seed, .) stream widened exactly: global
 * particle p = first_particle + i owns elements [p R, p R + (n_steps + 1) D), R = (n_steps + 1) D rounded up to a
 * multiple of 4; the first D give x0 = sqrt(var0) z, step k = 1.. the next D each.  x0 [N, D] (device, double;
 * optional) replaces the drawn start without moving the steps' stream positions.  first_particle splits an ensemble
 * over ranks or calls.  snap_step [S] (HOST, strictly ascending, in [0, n_steps], S <= 64) travels in the kernel
 * arguments: step 0 is the start, and nothing is integrated past the last snapshot.  Outputs (device), each optional,
 * at least one, overwritten:
 *   pos  [S, N, D]           double
 *   sums [S, 2 + D + D D]    double: the number of finite particles, of non-finite ones, sum x_d, sum x_d x_e --
 *                            raw sums, so the shards of an ensemble add
 *   hist [S, ny, nx]         uint32 counts on `grid` (lo, step, n and axis_x / axis_y; its other members are ignored):
 *                            cell j is centred on the grid point lo + j step, its index is
 *                            floor((x - (lo - step / 2)) / step) by an IEEE float64 division; particles outside the
 *                            grid are not counted
 * A particle whose state is not finite at a snapshot enters neither that snapshot's sums nor its histogram and is
 * counted as non-finite.  Two calls are bit-identical: the counts are integers, and the sums are formed over a fixed
 * partition of the call's particles into chunks of 256, the chunks' partials added in ascending order, whatever the
 * launch.  `workspace` (needed with sums; cnf_fp_particles_workspace(N, D, S) bytes) is the caller's: no allocation,
 * no synchronisation.
 * cnf_point_stats: the same sums and hist over given points pts [S, N, D] (device, float32, widened) -- what the
 * flow's own samples go through -- by the same accumulation code.
 * CNF_ERR_INVALID (nothing enqueued): a drift outside CnfDrift or one for another dimension (SMILE, NONGRADIENT: 2;
 * LORENZ: 3); D < 1 or > 14; h, var0 or N <= 0 or not finite (N above 2^31); sigma < 0; n_steps < 0 (or above 2^30);
 * first_particle < 0; S < 1 or > 64; snapshot steps that do not ascend or lie outside [0, n_steps]; no output; hist
 * without a grid, with n < 1, a step <= 0 or more than 2^24 cells; axes equal or outside the event; sums with a
 * workspace that is NULL or too small. */
int cnf_fp_particles_workspace(int64_t N, int32_t D, int32_t S, int64_t *bytes);
int cnf_fp_particles(int32_t drift, int32_t D, float a, double sigma, double h,
                     int64_t n_steps, double var0, uint64_t seed,
                     int64_t first_particle, int64_t N, const double *x0,
                     const int64_t *snap_step, int32_t S,
                     const CnfFieldGrid *grid, double *pos, double *sums,
                     uint32_t *hist, void *workspace, int64_t workspace_bytes,
                     void *stream);
int cnf_point_stats(const float *pts, int64_t N, int32_t D, int32_t S,
                    const CnfFieldGrid *grid, double *sums, uint32_t *hist,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* ---- a finite-volume reference for the 2-D Fokker-Planck problems (applications.py:279-374, drifts :310, :353-363) ----
 * The same PDE, d rho / dt = -div(rho drift) + sigma lap rho, solved on the grid of cnf_fp_particles' histogram: points
 * lo + i step, cell (j, i) centred on its point, arrays [ny, nx] row-major, float64.  No noise floor.
 * Flux (Scharfetter-Gummel / Chang-Cooper): B(z) = z / expm1(z) (1 - z / 2 for |z| < 1e-8), Pe = b step / sigma with b
 * the normal drift (CnfDrift, parameter `a`, evaluated in float64) at the face's midpoint; the face between cells i - 1
 * and i carries F = cL rho_{i-1} - cR rho_i, cL = sigma / step^2 B(-Pe), cR = sigma / step^2 B(Pe).  The faces of the
 * box carry no flux.  Step: rho' = rho + dt ((F_w - F_e) + (G_s - G_n)), that order, no contraction.
 *
 * cnf_fp_grid_coeffs writes the coefficient block `coef` (cnf_fp_grid_coeffs_bytes(nx, ny) bytes; `grid`: lo, step, nx,
 * ny; its other members are ignored): cxL, cxR [ny, nx + 1] (face f of a row lies between cells f - 1 and f), then cyL,
 * cyR [ny + 1, nx]; the box's faces hold zeros.  rate (one device double): the largest outflow rate, the sum of the
 * four coefficients that multiply a cell's own rho.  A step with dt rate <= 1 is a convex combination: rho stays >= 0.
 * cnf_fp_grid_steps advances rho [ny, nx] in place by n_steps steps of dt, steps_per_launch = K in {1, 2, 4, 8} steps
 * per launch (a workgroup takes K steps on its tile with a halo of K cells; n_steps mod K steps run with smaller K);
 * every K gives the same bits.  workspace: cnf_fp_grid_steps_workspace(nx, ny) bytes, the second buffer of the launches.
 * cnf_fp_grid_stats: per snapshot of rho [S, ny, nx], stats [S, 7] = mass, min, sum rho x, y, xx, xy, yy -- the sums
 * times step_x step_y, min the smallest cell value -- in a fixed order: two calls are bit-identical.
 * No allocation, no synchronisation, no atomics.
 * CNF_ERR_INVALID (nothing enqueued): D != 2; a drift other than OU, SMILE, NONGRADIENT; sigma <= 0; sigma or a not
 * finite; nx or ny outside 1..2^14; a step <= 0; a NULL array; a block or workspace too small; dt <= 0; n_steps < 0; K
 * outside {1, 2, 4, 8}; S outside 1..64. */
int cnf_fp_grid_coeffs_bytes(int32_t nx, int32_t ny, int64_t *bytes);
int cnf_fp_grid_coeffs(int32_t drift, int32_t D, float a, double sigma,
                       const CnfFieldGrid *grid, double *coef, int64_t coef_bytes,
                       double *rate, void *stream);
int cnf_fp_grid_steps_workspace(int32_t nx, int32_t ny, int64_t *bytes);
int cnf_fp_grid_steps(const double *coef, int32_t nx, int32_t ny, double dt,
                      int64_t n_steps, int32_t steps_per_launch, double *rho,
                      void *workspace, int64_t workspace_bytes, void *stream);
int cnf_fp_grid_stats(const CnfFieldGrid *grid, const double *rho, int32_t S,
                      double *stats, void *stream);

/* ---- importance-sampling diagnostics against a density known in closed form ----------------------------------------
 * The reference's kl_ess (tests/test_fit_prob.py:50-56, "metrics used in the tori paper"): draw y_i from the flow,
 * weight w_i = p_target(y_i) / q_flow(y_i), and report Z = mean w, KL = mean(log q - log p) + log Z and the effective
 * sample size ESS = (sum w)^2 / sum w^2.  It forms target_prob / exp(log_model_prob) in linear space: with the flow
 * far from its target (early in training, high dimension) sum w underflows to 0, Z = 0 and ESS = NaN.  Here the
 * statistic is carried in log space, as a state that merges exactly over lanes, waves, workgroups, calls and ranks.
 *
 * The target family, CnfTargetSpec: a Gaussian mixture whose components share one covariance shape,
 *   log p_s(y) = logsumexp_m(log_weight[m] - |W (y - mean[m])|^2 / (2 scale_s)) - D/2 log(2 pi scale_s) + log_det_W,
 * W lower triangular with Sigma^-1 = W^T W (rows and columns < D are read; the diagonal must be positive and
 * finite), log_det_W = log|det W|, log_weight normalised by the host (logsumexp = 0; -inf: a component of weight 0),
 * scale [n_slices] an optional DEVICE array of per-slice variance factors (slice s has covariance scale[s] Sigma;
 * NULL: 1).  It holds every closed-form density of the reference's problems: N(0, v I), the Gaussian source N(-3 1, A)
 * and the 8-mode mixture source (applications.py:28-71), and the OU solution N(0, v(t) I) at all times through scale.
 * The struct is a HOST argument, passed to the kernel by value.
 *
 * cnf_importance_stats: n_slices times t [n_slices] (device), B samples per time from base noise [n_slices * B, D]
 * ([B, D] with noise_shared != 0: every slice the same draw); one base -> data pass per sample gives y and
 * log q = log N(noise; 0, I) - log|det J|; the target is evaluated in float64 at the fp32 sample.  With
 * l_i = log p_s(y_i) - log q(y_i), stats [n_slices, 5] (device, double, overwritten) is the raw, mergeable state
 *   m = max_i l_i,  s1 = sum exp(l_i - m),  s2 = sum exp(2 (l_i - m)),  c = sum l_i,  n = the sample count,
 * from which log Z = log s1 + m - log n, KL = -c / n + log Z, ESS = s1^2 / s2.  Two states merge by bringing s1
 * and s2 to the common maximum and adding; the empty state (-inf, 0, 0, 0, 0) is the identity.  A slice with any
 * non-finite l_i has NaN in its first four columns: nothing is hidden.  All sums are float64 in a fixed order that
 * depends on B alone -- not on the device, nor on the other slices of the call; no atomics: repeated calls are
 * bit-identical on any device, and a slice's row is the same whatever else the call holds.
 * cnf_importance_stats_seeded: the same with the noise drawn in the kernel, by the convention of
 * cnf_loss_terms_seeded: sample i of slice s is sample first_sample + s * slice_stride + i of the cnf_fill_normal
 * stream of `seed` -- bit for bit cnf_fill_normal followed by cnf_importance_stats.
 * cnf_importance_workspace: the bytes of device workspace a call with these sizes needs (> 0); no HIP call.  The
 * workspace is the caller's: the compute calls neither allocate nor synchronise (legal inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL model, target, noise, t, stats or workspace; a
 * negative size, first_sample or slice_stride; n_comp outside 1..8; a diagonal entry of W (below the model's dim)
 * that is not positive and finite; a model of dim > 14; a workspace smaller than cnf_importance_workspace says;
 * parameters not set.  CNF_ERR_UNSUPPORTED: a periodized model, as for the loss terms.  n_slices == 0 or B == 0:
 * CNF_OK, nothing launched, stats untouched.  Runs the conditioner MLP at every dimension (the dim-2 tables pay from
 * launches far larger than an evaluation's). */
#define CNF_TARGET_MAX_COMP 8
#define CNF_TARGET_MAX_DIM 14
typedef struct CnfTargetSpec {
  int32_t n_comp;                                       /* 1 .. CNF_TARGET_MAX_COMP                      */
  int32_t reserved;
  double mean[CNF_TARGET_MAX_COMP][CNF_TARGET_MAX_DIM];
  double log_weight[CNF_TARGET_MAX_COMP];
  double W[CNF_TARGET_MAX_DIM][CNF_TARGET_MAX_DIM];     /* lower triangular: Sigma^-1 = W^T W            */
  double log_det_W;
  const double *scale;                                  /* device [n_slices], or NULL                    */
} CnfTargetSpec;
int cnf_importance_workspace(int64_t n_slices, int64_t B, int32_t D, int64_t *bytes);
int cnf_importance_stats(CnfModel *m, const CnfTargetSpec *target, const float *noise,
                         int noise_shared, const float *t, int64_t n_slices, int64_t B,
                         double *stats, void *workspace, int64_t workspace_bytes,
                         void *stream);
int cnf_importance_stats_seeded(CnfModel *m, const CnfTargetSpec *target, uint64_t seed,
                                int64_t first_sample, int64_t slice_stride, const float *t,
                                int64_t n_slices, int64_t B, double *stats, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* ---- kernel two-sample statistics between point clouds: MMD^2 and the energy distance, with gradients ---------------
 * What compares a flow with a target that exists only as SAMPLES (the reference: with samples of the target alone "we
 * need to shift to other integral probability metric, e.g. MMD", tests/test_wasserstein_geodesic.py:165-169).
 * Model-free.  For S independent sets, x [S, N, D] against y [S, M, D] (device, float32), and the kernel
 *   kind CNF_MMD_GAUSSIAN:  k(x, y) = sum_b exp(-|x - y|^2 / (2 bw_b^2)),  b < n_bw <= 8
 *   kind CNF_MMD_ENERGY:    k(x, y) = -|x - y|                             (n_bw and bw are ignored)
 * cnf_mmd2 writes sums [S, 3] (device, double, overwritten), the RAW sums
 *   sxx = sum_{i != j} k(x_i, x_j),   syy = sum_{i != j} k(y_i, y_j),   sxy = sum_{i, j} k(x_i, y_j);
 * the caller forms the unbiased MMD^2 = sxx / (N (N - 1)) + syy / (M (M - 1)) - 2 sxy / (N M), which with the energy
 * kernel is the energy distance 2 E|x - y| - E|x - x'| - E|y - y'|.  With xgrad [S, N, D] (device, float32, optional,
 * overwritten) it also writes d MMD^2 / d x_i; the derivative of k in its first argument is -(x - y) / bw_b^2 k_b
 * per bandwidth and -(x - y) / |x - y| for the energy kernel (0 for coincident points).  The diagonal i == j of the xx
 * and yy sums is left out by index.  Distances are formed from coordinate differences in float32; no float32
 * accumulator holds more than 64 pair terms before it is added into a double.  One launch computes the three blocks
 * of all sets, the columns of a block split over cnf_mmd_splits(S, N, M, D) workgroups (a function of the sizes
 * alone); a second adds the splits and the rows in a fixed order: no atomics, two calls are bit-identical, and the
 * result does not depend on what the workspace held.  The spec is a HOST argument.
 * cnf_mmd_workspace: the bytes of device workspace (8-byte aligned) such a call needs; no HIP call.  The workspace is
 * the caller's: cnf_mmd2 neither allocates nor synchronises (legal inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL spec, x, y, sums or workspace; D outside 1..14; N or
 * M < 2 (or above 2^24); S outside 1..64; an unknown kind; n_bw outside 1..8 or a bandwidth that is not positive and
 * finite (or whose square leaves float32's range); a workspace smaller than cnf_mmd_workspace says. */
#define CNF_MMD_MAX_BW 8
typedef enum { CNF_MMD_GAUSSIAN = 0, CNF_MMD_ENERGY = 1 } CnfMmdKind;
typedef struct CnfMmdSpec {
  int32_t kind;                 /* CnfMmdKind                                   */
  int32_t n_bw;                 /* Gaussian: 1 .. CNF_MMD_MAX_BW; energy: ignored */
  float bw[CNF_MMD_MAX_BW];
} CnfMmdSpec;
int cnf_mmd_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t want_grad, int64_t *bytes);
/* the column splits of a block at these sizes (>= 1), or CNF_ERR_INVALID */
int cnf_mmd_splits(int32_t S, int64_t N, int64_t M, int32_t D);
int cnf_mmd2(const CnfMmdSpec *spec, int32_t S, const float *x, int64_t N, const float *y,
             int64_t M, int32_t D, double *sums, float *xgrad, void *workspace,
             int64_t workspace_bytes, void *stream);

/* ---- the permutation test of the kernel two-sample statistic: P relabellings of the pooled sample at once -----------
 * What turns a value of MMD^2 into a p-value.  With the pooled sample z = (x, y) of set s, n = N + M points (pooled
 * index i < N: x_i, otherwise y_{i - N}), its zero-diagonal kernel matrix K (cnf_mmd2's kernel value, in the same
 * float32 operations and order) and a label vector s in {+1, -1}^n (+1: "first sample"),
 *   q = s' K s,   r = 1' K s,   t = 1' K 1,
 *   sum_xx = (t + 2 r + q) / 4,   sum_yy = (t - 2 r + q) / 4,   sum_xy = (t - q) / 4,
 *   MMD^2 = sum_xx / (N_s (N_s - 1)) + sum_yy / (M_s (M_s - 1)) - 2 sum_xy / (N_s M_s),
 * N_s the number of +1 labels and M_s = n - N_s.  For P label vectors C = K S' is a matrix product whose left factor is
 * generated on the fly and never stored: each kernel value is formed once and used P times, on the exact-fp32 MFMA.
 * labels [n, P / 32] (device, uint32, shared by all S sets): bit b of word w of point j is label vector 32 w + b, set
 * where point j belongs to the first sample under that vector.  The counts N_p, M_p are read from the labels; any
 * split with N_p >= 2 and M_p >= 2 is legal, and for a vector outside that range stats is NaN for that vector alone.
 * cnf_mmd_perm writes stats [S, P] (device, double, overwritten): MMD^2_u (with the energy kernel, the energy
 * distance) per set and label vector; and, with raw (device, double, optional, overwritten), raw [S, P, 2] = (q, r)
 * followed by t [S] -- what a rank or a call is audited from.  t is computed by the call, not taken from the labels.
 * No float32 accumulator holds more than 64 pair terms before it is added into a double; the column splits are
 * cnf_mmd_perm_splits(S, N, M, D) (a function of the sizes alone); the partial sums are added in a fixed ascending
 * order: no atomics, two calls are bit-identical, the result does not depend on what the workspace held, and a label
 * vector's q and r do not depend on P, on its position among the vectors or on the other vectors.  The spec is a HOST
 * argument.  cnf_mmd_perm_workspace: the bytes of device workspace (8-byte aligned) such a call needs; no HIP call.
 * cnf_mmd_perm neither allocates nor synchronises (legal inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL spec, x, y, labels, stats or workspace; D outside
 * 1..14; S outside 1..64; N or M < 2; N + M > 2^20; P not a multiple of 32 or outside 32..1024; what cnf_mmd2 refuses
 * in a spec; a workspace smaller than cnf_mmd_perm_workspace says. */
int cnf_mmd_perm_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t P, int64_t *bytes);
/* the column splits of the pooled sample at these sizes (>= 1), or CNF_ERR_INVALID */
int cnf_mmd_perm_splits(int32_t S, int64_t N, int64_t M, int32_t D);
int cnf_mmd_perm(const CnfMmdSpec *spec, int32_t S, const float *x, int64_t N, const float *y,
                 int64_t M, int32_t D, const uint32_t *labels, int32_t P, double *stats, double *raw,
                 void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the Sinkhorn divergence between point clouds: the optimal-transport reference of the ot problems ---------------
 * Debiased entropic optimal transport with the cost C(x, y) = |x - y|^2 / 2 and uniform weights, in the log domain.
 * Model-free.  For S independent sets, x [S, N, D] against y [S, M, D] (device, float32) and a HOST array
 * eps[n_iters], four potentials per set, all 0 at the start: f [N], g [M] (x against y), p [N] (x against x), q [M]
 * (y against y).  With T(h; rows, cols, e)_i = -e log((1 / n_cols) sum_j exp((h_j - C(row_i, col_j)) / e)), iteration
 * k = 0 .. n_iters - 1 updates the four simultaneously from the old state,
 *   f <- (f + T(g; x, y, eps_k)) / 2,  g <- (g + T(f; y, x, eps_k)) / 2,
 *   p <- (p + T(p; x, x, eps_k)) / 2,  q <- (q + T(q; y, y, eps_k)) / 2,
 * and a final pass at eps[n_iters - 1] takes f* = T(g), g* = T(f), p* = T(p), q* = T(q) without averaging.  The
 * iteration count and every eps are the caller's: the call decides nothing about convergence.
 * cnf_sinkhorn writes
 *   sums [S, 6] (device, double, overwritten): sum f*, sum g*, sum p*, sum q*, max(|f* - f|, |g* - g|) and
 *     max(|p* - p|, |q* - q|) over the final pass (the convergence diagnostic).  The caller forms
 *     OT_eps(x, y) = sum f* / N + sum g* / M and S_eps(x, y) = (sum f* - sum p*) / N + (sum g* - sum q*) / M;
 *   potentials [S, 2 N + 2 M] (device, float32, or NULL): per set f* [N], g* [M], p* [N], q* [M];
 *   xmap [S, N, D] (device, float32, or NULL): the barycentric map Txy(x_i) = sum_j w_ij y_j of the final pass,
 *     w_ij = exp((g_j - C_ij) / eps) normalised over j;
 *   xgrad [S, N, D] (device, float32, or NULL): (Txx(x_i) - Txy(x_i)) / N, Txx the same map of x onto itself under p.
 *     It is the ENVELOPE gradient of S_eps in x_i (potentials held fixed): exact at the fixed point of the recursion,
 *     approximate before it.
 * Every iteration is one pair launch over the four blocks of all sets, the columns of a block split over
 * cnf_sinkhorn_splits(S, N, M, D) workgroups (a function of the sizes alone), and one merge launch; every eps goes to
 * its launches by value.  No atomics: two calls are bit-identical, the sums do not depend on which optional outputs
 * are asked for, and the result does not depend on what the workspace held.
 * cnf_sinkhorn_workspace: the bytes of device workspace (8-byte aligned) a call needs; no HIP call.  The workspace
 * is the caller's: cnf_sinkhorn neither allocates, synchronises nor reads the device (legal inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL x, y, eps, sums or workspace; S outside 1..64; D
 * outside 1..14; N or M outside 2..2^20; n_iters outside 1..512; an eps that is not finite and > 0, or for which 1 / eps
 * or log2(e) / eps is not a finite normal float32; a workspace smaller than cnf_sinkhorn_workspace says. */
int cnf_sinkhorn_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int64_t *bytes);
/* the column splits of a block at these sizes (>= 1), or CNF_ERR_INVALID */
int cnf_sinkhorn_splits(int32_t S, int64_t N, int64_t M, int32_t D);
int cnf_sinkhorn(int32_t S, const float *x, int64_t N, const float *y, int64_t M, int32_t D,
                 const double *eps, int32_t n_iters, double *sums, float *potentials,
                 float *xgrad, float *xmap, void *workspace, int64_t workspace_bytes,
                 void *stream);

/* ---- the sliced Wasserstein distance between point clouds: transport units at N log N ------------------------------
 * What the reference's tests/test_wasserstein_geodesic.py:165-169 leaves open for a target known only by its samples,
 * in the units of cnf_sinkhorn (cost |.|^2 / 2) and without an eps, an iteration count or N x M pairs.  Model-free.
 * For S independent sets, x [S, N, D] against y [S, M, D] (device, float32, uniform weights) and P directions
 * theta [P, D] (device, float32) that the CALLER supplies: the library neither draws nor normalises them.
 * Per set s and projection p:
 *   keys   k_i = x[i, 0] theta[p, 0], then k_i = fmaf(x[i, d], theta[p, d], k_i) for d = 1 .. D - 1 in ascending d, in
 *          float32, and last k_i = fmaf(k_i, 0, k_i): a finite key is unchanged by it, an infinite one becomes NaN.
 *          l_j the same for y.
 *   order  both key arrays ascending; TIES go by the sample's index.  (A NaN sorts by its bit pattern.)
 *   value  w[s, p] = 1/2 sum_i sum_j o_ij (k_(i) - l_(j))^2 over the sorted keys, with
 *          o_ij = max(0, min((i + 1) M, (j + 1) N) - max(i M, j N)) / (N M)
 *          in 64-bit integers up to the division: the quantile-function integral of one-dimensional optimal
 *          transport, for equal and for unequal sizes.  Differences and sums in double.
 * cnf_sliced_w2 writes
 *   sums [S, P + 2] (device, double, overwritten): the P values w[s, :], their mean SW[s] (summed in ascending p) and
 *     their maximum, the max-sliced value over the given directions;
 *   grad [S, N, D] (device, float32, or NULL): grad[s, i, :] = (1 / P) sum_p a[s, p, i] theta[p, :] + 0 SW[s], with
 *     a = sum_j o_ij (k_i - l_j) at the rank sample i took: the ENVELOPE gradient of SW in x_i, the two permutations
 *     held fixed (exact wherever the keys are distinct), accumulated in double in ascending p and rounded once.
 * The cost convention is |.|^2 / 2: for unit directions drawn uniformly, SW <= W2^2 / (2 D), and with the D coordinate
 * axes as directions sqrt(2 w[s, d]) is the exact W2 of marginal d.
 * Non-finite input: a NaN or infinite coordinate of set s makes every key it enters NaN, hence every value of that
 * set it reaches, and through the 0 SW[s] term every gradient row of that set; other sets are untouched.
 * G projections are in flight at a time (the workspace grows with G).  The running gradient is carried between
 * groups as DOUBLES in the workspace, so values and gradient are bit-identical for every G; no atomics: two calls are
 * bit-identical, and the result does not depend on what the workspace held.
 * cnf_sliced_workspace: the bytes of device workspace a call with this G needs (want_grad: grad != NULL); no HIP call.
 * The workspace is the caller's: cnf_sliced_w2 neither allocates, synchronises nor reads the device (legal inside a
 * stream capture).  cnf_sliced_tile: the keys per sorted tile (a build constant; clouds above it take merge passes).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL x, y, theta, sums or workspace; S outside 1..64; D
 * outside 1..14; N or M outside 1..2^20; P outside 1..1024; G outside 1..P (cnf_sliced_workspace: 1..1024); a workspace
 * smaller than cnf_sliced_workspace says.
 * Out of scope: weights, more than one rank, N > 2^20, costs other than |.|^2 / 2, drawing directions on the device. */
int cnf_sliced_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t G, int32_t want_grad,
                         int64_t *bytes);
int cnf_sliced_tile(void);
int cnf_sliced_w2(int32_t S, const float *x, int64_t N, const float *y, int64_t M, int32_t D,
                  const float *theta, int32_t P, int32_t G, double *sums, float *grad,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* ---- k nearest neighbours between point clouds: entropy, cross entropy and KL in nats from samples alone ------------
 * The reference's note (tests/test_wasserstein_geodesic.py:165-169), "with samples of the target alone KL cannot be
 * computed", holds for the plug-in formula, not for the nearest-neighbour estimators.  Model-free.  For S independent
 * sets, x [S, N, D] and optionally y [S, M, D] (device, float32), two blocks per set:
 *   self   rho_j(i) = the distance from x_i to its j-th nearest OTHER point of x (the diagonal is left out by index; a
 *          duplicate of x_i at another index is a neighbour at distance 0);
 *   cross  nu_j(i)  = the distance from x_i to its j-th nearest point of y.
 * Squared distances are formed from coordinate differences in float32: diff = x - c, d2 = diff_0^2, then
 * d2 = fmaf(diff_d, diff_d, d2) in ascending d (the distance of cnf_mmd2).  ORDER: neighbours are ascending by (d2 as
 * computed, index); of two equal d2 the smaller index comes first.  Rank j depends neither on k nor on what else is
 * asked for.
 * cnf_knn writes
 *   dist_xx, dist_xy [S, N, k] (device, float32, each or NULL): (float)sqrt((double)d2), ranks 1..k;
 *   idx_xx, idx_xy [S, N, k] (device, int32, each or NULL): the neighbour's row in x (self) or y (cross);
 *   sums [S, 2, k, 2] (device, double, overwritten): per block (self, cross) and rank j,
 *     sums[s, b, j, 0] = sum over the rows i with d2_j(i) > 0 of 0.5 log((double)d2_j(i)), and
 *     sums[s, b, j, 1] = the number of rows with d2_j(i) == 0.
 * From them, with psi the digamma function, log V_D = (D / 2) log pi - lgamma(D / 2 + 1) the log volume of the unit
 * ball, and the means taken over the rows counted in the sum, the caller forms
 *   the Kozachenko-Leonenko entropy           H(x)    ~ psi(N) - psi(j) + log V_D + D mean_i log rho_j(i),
 *   the Leonenko-Pronzato-Savani cross entropy H(x, y) ~ log M  - psi(j) + log V_D + D mean_i log nu_j(i),
 *   and KL(x || y) ~ H(x, y) - H(x), the Wang-Kulkarni-Verdu estimator with the psi corrections.
 * With M == 0 and y == NULL the self block alone is computed and the cross half of sums is written as zeros.
 * One launch scans both blocks of all sets, the columns of a block split over cnf_knn_splits(S, N, M, D) workgroups (a
 * function of the sizes alone); a second merges a row's splits in ascending order, a third adds the rows in a fixed
 * order: no atomics, two calls are bit-identical, the numbers do not depend on which optional outputs are asked for,
 * and the result does not depend on what the workspace held.  There is no gradient.
 * cnf_knn_workspace: the bytes of device workspace (8-byte aligned) such a call needs; no HIP call.  The workspace is
 * the caller's: cnf_knn neither allocates nor synchronises (legal inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL x, sums or workspace; y NULL with M != 0 or y given
 * with M == 0; dist_xy or idx_xy given with M == 0; S outside 1..64; D outside 1..14; k outside 1..CNF_KNN_MAX_K; N
 * outside k + 1..2^20; M outside k..2^20 and not 0; a workspace smaller than cnf_knn_workspace says. */
#define CNF_KNN_MAX_K 16
int cnf_knn_workspace(int32_t S, int64_t N, int64_t M, int32_t D, int32_t k, int64_t *bytes);
/* the column splits of a block at these sizes (>= 1), or CNF_ERR_INVALID */
int cnf_knn_splits(int32_t S, int64_t N, int64_t M, int32_t D);
int cnf_knn(int32_t S, const float *x, int64_t N, const float *y, int64_t M, int32_t D, int32_t k,
            float *dist_xx, int32_t *idx_xx, float *dist_xy, int32_t *idx_xy, double *sums,
            void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the mean-field interaction energy of a point cloud, its field and its force -------------------------------------
 * The nonlocal cost of a mean-field control problem, F[rho] = 1/2 int int W(x - y) rho(x) rho(y) dx dy, on samples: a
 * double sum with first variation W * rho (a field) and Wasserstein gradient grad (W * rho) (a force).  Model-free.
 * The pair kernel is a function of r = |x - y| with SIGNED amplitudes (W > 0: congestion, W < 0: aggregation):
 *   kind CNF_INTERACTION_GAUSSIAN:     W = sum_b amp_b exp(-r^2 / (2 bw_b^2)),  b < n_terms <= 4
 *   kind CNF_INTERACTION_EXPONENTIAL:  W = sum_b amp_b exp(-r / bw_b)           (Morse: n_terms = 2, amp = (C_r, -C_a));
 *                                      grad W is 0 at a coincident pair (r^2 <= 1e-30)
 *   kind CNF_INTERACTION_QUADRATIC:    W = amp_0 r^2 / 2                        (n_terms and bw are ignored)
 *   kind CNF_INTERACTION_POWER:        W = sum_b amp_b u^(pw_b / 2) / pw_b (pw_b != 0) + sum_b amp_b ln(u) / 2 (pw_b == 0),
 *                                      u = r^2 + eps^2, eps = bw[0] ONE softening length (Plummer; bw[1..] are ignored), so
 *                                      grad W = (x - y) sum_b amp_b u^(pw_b / 2 - 1): softened power laws and the log kernel,
 *                                      which the force passes through continuously at pw = 0.  pw = 2 - D: Newtonian /
 *                                      Coulomb; pw = 0: log (Keller-Segel, log-gases); two terms of opposite sign: an
 *                                      attractive-repulsive power law r^a / a - r^b / b; pw = 2, eps = 0: the quadratic
 *                                      kind.  eps = 0 only with every pw_b >= 2; a coincident pair then contributes
 *                                      W(0) = 0 and a zero force.  u is clamped below at 1e-30, the unit's rule for
 *                                      a coincident pair: an eps below 1e-15 acts as that clamp at r = 0
 * For S independent sets x [S, N, D] (device, float32), one entry with two modes:
 *   self mode  (q == NULL, Q == 0): the rows are the particles themselves; the pair i == j is skipped by INDEX (a
 *              duplicate of x_i at another index does interact); n = N - 1;
 *   query mode (q [S, Q, D], Q >= 1): the rows are the points q against the sources x; nothing is skipped; n = N.
 * cnf_interaction writes
 *   sums [S] (device, double, overwritten): sum_i sum_j W(row_i - x_j), the RAW double sum over the rows; in self mode
 *     the caller forms F = sums / (2 N (N - 1)), and because W is even dF / dx_i = force_i / N;
 *   pot [S, rows] (device, float32, or NULL): (1 / n) sum_j W(row_i - x_j), that is (W * rho)(row_i);
 *   force [S, rows, D] (device, float32, or NULL): (1 / n) sum_j grad W(row_i - x_j), that is grad (W * rho)(row_i).
 * Distances are formed from coordinate differences in float32 in the fmaf order of cnf_mmd2; no float32 accumulator
 * holds more than 64 pair terms before it is added into a double.  One launch computes all sets, the columns split over
 * cnf_interaction_splits(S, N, Q, D) workgroups (a function of the sizes alone); a second adds a row's splits in
 * ascending order and the rows in a fixed order: no atomics, two calls are bit-identical, sums does not depend on
 * whether pot or force are asked for, and the result does not depend on what the workspace held.  The spec is a HOST
 * argument.
 * cnf_interaction_workspace: the bytes of device workspace (8-byte aligned) a call needs -- want_rows != 0: a call
 * that asks for force (pot needs no more than sums); no HIP call.  The workspace is the caller's: cnf_interaction
 * neither allocates nor synchronises (legal inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL spec, x, sums or workspace; q NULL with Q != 0 or q
 * given with Q == 0; S outside 1..64; D outside 1..14; N outside 2..2^20; Q outside 1..2^20 and not 0; an unknown
 * kind; n_terms outside 1..4; an amp that is zero or not finite; a bw that is not positive and finite, whose 1 / bw^2
 * leaves float32's range or for which amp / bw^2 (Gaussian) or amp / bw (exponential) does; a workspace smaller than
 * cnf_interaction_workspace says.  For the power kind: a pw that is not finite or has |pw| > 16; an eps = bw[0] that is
 * negative or not finite, or 0 unless every pw_b >= 2; a force coefficient amp_b eps^(pw_b - 2) or a value coefficient
 * amp_b eps^pw_b / pw_b (pw_b = 0: amp_b ln eps; also amp_b eps^(pw_b - 2) / pw_b, the value's sum before its factor u)
 * outside float32's range.
 * Out of scope: weighted particles, truly singular kernels (eps = 0 with a pw < 2), per-term softening lengths, more
 * than one rank, D > 14, N > 2^20. */
#define CNF_INTERACTION_MAX_TERMS 4
typedef enum {
  CNF_INTERACTION_GAUSSIAN = 0, CNF_INTERACTION_EXPONENTIAL = 1, CNF_INTERACTION_QUADRATIC = 2,
  CNF_INTERACTION_POWER = 4     /* (3 is not a kind) */
} CnfInteractionKind;
typedef struct CnfInteractionSpec {
  int32_t kind;                 /* CnfInteractionKind                                     */
  int32_t n_terms;              /* 1 .. CNF_INTERACTION_MAX_TERMS; quadratic: ignored     */
  float amp[CNF_INTERACTION_MAX_TERMS];
  float bw[CNF_INTERACTION_MAX_TERMS];   /* power: bw[0] = the softening length eps          */
  float pw[CNF_INTERACTION_MAX_TERMS];   /* power: the exponents; the other kinds ignore it  */
} CnfInteractionSpec;
int cnf_interaction_workspace(int32_t S, int64_t N, int64_t Q, int32_t D, int32_t want_rows,
                              int64_t *bytes);
/* the column splits at these sizes (>= 1), or CNF_ERR_INVALID */
int cnf_interaction_splits(int32_t S, int64_t N, int64_t Q, int32_t D);
int cnf_interaction(const CnfInteractionSpec *spec, int32_t S, const float *x, int64_t N,
                    const float *q, int64_t Q, int32_t D, double *sums, float *pot, float *force,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the vector-Jacobian product of the self-mode force ---------------------------------------------------------------
 * For S sets x [S, N, D] and an adjoint g [S, N, D] of the force f_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j)
 * that cnf_interaction writes in self mode, cnf_interaction_vjp OVERWRITES
 *   xbar [S, N, D] (device, float32):  xbar_k = (1 / (N - 1)) sum_{j != k} H(x_k - x_j) (g_k - g_j),
 * H(d) v = c1 v + d (d . v) c2 the pair Hessian of W (W is even) with, r = |d| and e_b the term's exponential,
 *   Gaussian:     c1 = sum_b (-amp_b / bw_b^2) e_b,  c2 = sum_b (amp_b / bw_b^4) e_b
 *   exponential:  c1 = w / r,  c2 = w' / r^2 - w / r^3,  w = sum_b (-amp_b / bw_b) e_b,  w' = sum_b (amp_b / bw_b^2) e_b;
 *                 both 0 at a coincident pair (r^2 <= 1e-30), the force's own rule
 *   quadratic:    c1 = amp_0,  c2 = 0
 *   power:        c1 = sum_b amp_b u^(pw_b / 2 - 1),  c2 = sum_b amp_b (pw_b - 2) u^(pw_b / 2 - 2),  u = r^2 + eps^2
 * the exact gradient of sum_i g_i . f_i in x for fixed g.  (For the exponential kind in dimension 1 it does not contain
 * the delta term of the kink of W at 0: the discrete objective has none.)  The pair j == k contributes 0 by itself.
 * Built as cnf_interaction's pair pass: the same workgroup geometry and cnf_interaction_splits(S, N, 0, D) column
 * splits, one v_exp_f32 per term and pair, float32 accumulators for 64 columns, then doubles, a fixed-order merge, no
 * atomics: two calls are bit-identical and the result does not depend on what the workspace held.  The spec is a HOST
 * argument; the workspace (cnf_interaction_vjp_workspace bytes, 8-byte aligned) is the caller's: no allocation, no
 * synchronisation (legal inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: everything cnf_interaction refuses in self mode (spec, S, N,
 * D), a NULL g or xbar, a Hessian coefficient amp / bw^4 (Gaussian), amp / bw^2 (exponential) or amp_b (pw_b - 2)
 * eps^(pw_b - 4) (power; none for pw_b = 2) outside float32's range, a workspace smaller than
 * cnf_interaction_vjp_workspace says.
 * Out of scope: query mode, more than one rank. */
int cnf_interaction_vjp_workspace(int32_t S, int64_t N, int32_t D, int64_t *bytes);
int cnf_interaction_vjp(const CnfInteractionSpec *spec, int32_t S, const float *x, const float *g,
                        int64_t N, int32_t D, float *xbar, void *workspace, int64_t workspace_bytes,
                        void *stream);

/* ---- the kernel Stein discrepancy of point sets against a score ------------------------------------------------------
 * For S sets x [S, N, D] and the score s [S, N, D] = grad log p at those points (p known through s alone), with the
 * base kernel k(x, y) = phi(r^2), r^2 = |d|^2, d = x - y, and phi', phi'', phi''' its derivatives in r^2, the Stein kernel
 *   k_p(x, y) = phi (s_x . s_y) + 2 phi' d . (s_y - s_x) - 4 phi'' r^2 - 2 D phi'
 *   k_p(x, x) = phi(0) |s_x|^2 - 2 D phi'(0)
 *   kind CNF_STEIN_IMQ:       phi = sum_b w_b (bw_b^2 + r^2)^beta,  -1 < beta < 0,  b < n_terms <= 4
 *   kind CNF_STEIN_GAUSSIAN:  phi = sum_b w_b exp(-r^2 / (2 bw_b^2))           (beta is ignored)
 * cnf_stein writes
 *   sums [S, 2] (device, doubles):  sum_{i != j} k_p(x_i, x_j)  and  sum_i k_p(x_i, x_i)
 *       (KSD^2_U = sums[0] / (N (N - 1)),  KSD^2_V = (sums[0] + sums[1]) / N^2)
 *   rows [S, N] (float32, or NULL):  (1 / (N - 1)) sum_{j != i} k_p(x_i, x_j)
 *   grad_x, grad_s [S, N, D] (float32, both or neither):  the gradients of KSD^2_U in x_i and in s_i, s held an
 *       independent input: 2 / (N (N - 1)) times the sum over j != i of
 *         d / d s_i:  phi s_j - 2 phi' d
 *         d / d x_i:  (2 phi' s_i . s_j + 4 phi'' d . (s_j - s_i) - 8 phi''' r^2 - (8 + 4 D) phi'') d + 2 phi' (s_j - s_i)
 * The pair i == j is skipped by index; duplicated points at other indices do interact.  Built as cnf_interaction's pair
 * pass: blockIdx.y the set, a 256-lane workgroup owning rows held in registers (two per lane for D <= 8, one above) and
 * one of cnf_stein_splits(S, N, D) column splits, a column's x_j and s_j through the scalar cache, float32 accumulators
 * for 64 columns, then doubles, a fixed-order merge, no atomics: two calls are bit-identical, sums does not depend on
 * what else is asked for, and nothing depends on what the workspace held.  The IMQ kind: one v_log_f32, one v_exp_f32
 * and one v_rcp_f32 per pair and term give all four of phi .. phi'''; the Gaussian kind: one v_exp_f32.  The spec is a
 * HOST argument; the workspace (cnf_stein_workspace bytes, 8-byte aligned) is the caller's: no allocation, no
 * synchronisation (legal inside a stream capture).  Non-finite inputs propagate to the outputs of their own set.
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL spec, x, score, sums or workspace; S outside 1..64, N
 * outside 2..2^20, D outside 1..14; an unknown kind; n_terms outside 1..4; a w_b that is not positive and finite; a
 * bw_b that is not positive and finite; (IMQ) beta outside (-1, 0) or a w_b bw_b^(2 beta - 6), bw_b^2 or 1 / bw_b^2
 * outside float32's range; (Gaussian) a w_b / bw_b^6 outside float32's range; one of grad_x, grad_s without the other; a
 * workspace smaller than cnf_stein_workspace says (want_grad != 0: a call that asks for the gradients).
 * Out of scope: weighted points, D > 14, N > 2^20, more than one rank, other kernels. */
#define CNF_STEIN_MAX_TERMS 4
enum { CNF_STEIN_IMQ = 1, CNF_STEIN_GAUSSIAN = 2 };
typedef struct CnfSteinSpec {
  int32_t kind;                 /* CNF_STEIN_IMQ or CNF_STEIN_GAUSSIAN */
  int32_t n_terms;              /* 1 .. CNF_STEIN_MAX_TERMS            */
  float w[CNF_STEIN_MAX_TERMS];
  float bw[CNF_STEIN_MAX_TERMS];         /* IMQ: c_b; Gaussian: h_b    */
  float beta;                   /* IMQ: the exponent, in (-1, 0)       */
} CnfSteinSpec;
int cnf_stein_workspace(int32_t S, int64_t N, int32_t D, int32_t want_grad, int64_t *bytes);
int cnf_stein_splits(int32_t S, int64_t N, int32_t D);
int cnf_stein(const CnfSteinSpec *spec, int32_t S, const float *x, const float *score, int64_t N, int32_t D,
              double *sums, float *rows, float *grad_x, float *grad_s, void *workspace, int64_t workspace_bytes,
              void *stream);

/* ---- the wild bootstrap of the kernel Stein discrepancy: P Rademacher sign vectors at once --------------------------
 * What turns a value of KSD^2_U into a p-value.  With H the Stein kernel matrix of set s with its diagonal zeroed
 * (cnf_stein's k_p, in the same float32 operations and order, without the gradient's phi''') and a sign vector e in
 * {+1, -1}^N, the wild bootstrap of the degenerate U-statistic is
 *   B(e) = e' H e / (N (N - 1)),   KSD^2_U = B(1).
 * For P sign vectors C = H E' is a matrix product whose left factor is generated on the fly and never stored: each
 * Stein kernel value is formed once and used P times, on the exact-fp32 MFMA.
 * signs [N, P / 32] (device, uint32, shared by all S sets): bit b of word w of point j is sign vector 32 w + b, set
 * where e_j = +1 under that vector.
 * cnf_stein_boot writes stats [S, P] (device, double, overwritten): e' H e / (N (N - 1)) per set and sign vector; and,
 * with raw (device, double, optional, overwritten), q [S, P] = e' H e, then t [S] = 1' H 1, then the diagonal sum [S] =
 * sum_i k_p(x_i, x_i) (cnf_stein's sums[1]) -- what a rank, a call or the V-statistic (q + diagonal) / N^2 is audited
 * from.  t is computed by the call, not taken from the signs.
 * No float32 accumulator holds more than 64 pair terms before it is added into a double; the column splits are
 * cnf_stein_boot_splits(S, N, D) (a function of the sizes alone); the partial sums are added in a fixed ascending
 * order: no atomics, two calls are bit-identical, the result does not depend on what the workspace held, a sign
 * vector's q does not depend on P, on its position among the vectors or on the other vectors, and q is unchanged bit
 * for bit when a vector is complemented.  The spec is a HOST argument.  cnf_stein_boot_workspace: the bytes of device
 * workspace (8-byte aligned) such a call needs; no HIP call.  cnf_stein_boot neither allocates nor synchronises (legal
 * inside a stream capture).  Non-finite inputs propagate to the outputs of their own set.
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL spec, x, score, signs, stats or workspace; S outside
 * 1..64; N outside 2..2^20; D outside 1..14; P not a multiple of 32 or outside 32..1024; what cnf_stein refuses in a
 * spec; a workspace smaller than cnf_stein_boot_workspace says.
 * Out of scope: H's symmetry, other weights than Rademacher signs, dependent or block bootstraps, signs drawn on the
 * device or per set, gradients, more than one rank, N > 2^20. */
int cnf_stein_boot_workspace(int32_t S, int64_t N, int32_t D, int32_t P, int64_t *bytes);
/* the column splits of a set at these sizes (>= 1), or CNF_ERR_INVALID */
int cnf_stein_boot_splits(int32_t S, int64_t N, int32_t D);
int cnf_stein_boot(const CnfSteinSpec *spec, int32_t S, const float *x, const float *score, int64_t N, int32_t D,
                   const uint32_t *signs, int32_t P, double *stats, double *raw,
                   void *workspace, int64_t workspace_bytes, void *stream);

/* ---- a Gaussian kernel density estimate of point sets: log-density and score ----------------------------------------
 * What turns an ensemble into FIELDS at given points in the full dimension.  For S sets of sources x [S, N, D], queries
 * q [S, Q, D] and bandwidths h_b, b < n_bw <= 4, per (set, b, query i):
 *   t_ij     = -|q_i - x_j|^2 / (2 h_b^2)        (the difference first, then the square)
 *   m        = max_j t_ij,   s = sum_j exp(t_ij - m),   w_ij = exp(t_ij - m) / s
 *   log_rho  = m + log s - log n_eff - (D / 2) log(2 pi h_b^2)        [S, n_bw, Q]     float32, or NULL
 *   score_d  = sum_j w_ij (x_jd - q_id) / h_b^2                       [S, n_bw, Q, D]  float32, or NULL
 *   sums     = sum_i log_rho                                          [S, n_bw]        float64, or NULL
 * (sums adds the float32 log_rho values in double).  q == NULL is self mode: the queries are the sources and Q must
 * equal N.  With spec->loo != 0 (self mode only) the pair j == i is skipped by index -- duplicated points at other
 * indices do interact -- and n_eff = N - 1: the leave-one-out estimate, whose sums / N is the likelihood that bandwidth
 * selection maximises.  Otherwise n_eff = N.
 * Where every t_ij of a row is -inf in float32 (no source within reach: a distance that overflows, or one that times
 * 1 / (2 h_b^2) does): log_rho = -inf and score = 0.  A query with a NaN coordinate gives NaN for that query only; a
 * set with a NaN source coordinate gives NaN for that set only.
 * Built as cnf_sinkhorn's pair pass: blockIdx.y the set, a 256-lane workgroup owning query rows held in registers (two
 * per lane where n_bw (1 + D) <= 16, one above) and one of cnf_kde_splits(S, N, Q, D) column splits, a source through
 * the scalar cache, float32 pair math with exp2 on the precomputed -log2 e / (2 h_b^2), float32 sums for 64 columns,
 * then doubles.  All bandwidths share d2_ij and ONE running minimum of it per row, from which each bandwidth's sums are
 * rescaled.  A merge kernel brings a row's splits together in ascending order; a finish kernel forms sums in a fixed
 * order.  No float atomics: two calls are bit-identical, no output depends on which others are asked for, and nothing
 * depends on what the workspace held.  The spec is a HOST argument; the workspace (cnf_kde_workspace bytes, 8-byte
 * aligned; want_score != 0: a call that asks for the score) is the caller's: no allocation, no synchronisation (legal
 * inside a stream capture).
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: a NULL spec, x or workspace; log_rho, score and sums all NULL;
 * S outside 1..64, N outside 1..2^20 (2..2^20 with loo), Q outside 1..2^20, D outside 1..14, n_bw outside 1..4; q ==
 * NULL with Q != N; loo with q != NULL; a bandwidth that is not positive and finite or whose 1 / (2 h^2) is not a
 * normal float32; a workspace smaller than cnf_kde_workspace says.
 * Out of scope: gradients in the particles, per-set bandwidths, weighted sources, other kernels, more than one rank. */
#define CNF_KDE_MAX_BW 4
typedef struct CnfKdeSpec {
  int32_t n_bw;                 /* 1 .. CNF_KDE_MAX_BW                              */
  int32_t loo;                  /* != 0: leave-one-out (self mode only)             */
  float bw[CNF_KDE_MAX_BW];     /* h_b                                              */
} CnfKdeSpec;
int cnf_kde_workspace(int32_t S, int64_t N, int64_t Q, int32_t D, int32_t n_bw, int32_t want_score, int64_t *bytes);
int cnf_kde_splits(int32_t S, int64_t N, int64_t Q, int32_t D);
int cnf_kde(const CnfKdeSpec *spec, int32_t S, const float *x, int64_t N, const float *q, int64_t Q, int32_t D,
            float *log_rho, float *score, double *sums, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- a particle reference for the interacting (McKean-Vlasov) Fokker-Planck equation --------------------------------
 *   d rho / dt = -div(rho (drift - kappa grad (W * rho))) + sigma lap rho
 * (aggregation-diffusion, crowd aversion, swarming: the forward half of a mean-field game).  It replaces a loop of one
 * cnf_interaction call in query mode plus a composed float64 update per step, and is the ground truth an interacting
 * fp training term would be held to.  R independent replicas of N particles of dimension D, replica r particle i:
 *   x_i <- x_i + h (drift(x_i) - kappa G_i) + sqrt(2 sigma h) z,   G_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j)
 * State and update are float64, drift as in cnf_fp_particles; per coordinate v = fma(-kappa, G_d, drift_d),
 * xn_d = fma(h, v, x_d) for every d from the OLD x, then x_d = fma(sqrt(2 sigma h), z, xn_d): kappa = 0 is
 * cnf_fp_particles' step bit for bit.  The pair force is formed exactly as cnf_interaction forms it in self mode, by
 * the same kernel, on the float32 rounding of the current positions (a replica is one of its sets, so replicas never
 * interact; the pair i == j is skipped by index); then G_d = (cf (split 0 + split 1 + ...)) / (N - 1) in double, cf =
 * amp_0 for the quadratic kind and 1 otherwise, with NO float32 rounding of the force in between.
 * Normals: cnf_fp_particles' stream layout with global particle p = first_particle + r N + i.
 * snap_step [S] as in cnf_fp_particles; nothing is integrated past the last snapshot.  Outputs (device), overwritten:
 *   state [R, N, D]              double, required: the positions, advanced in place; on return those of the last snapshot
 *   sums  [S, R, 3 + D + D D]    double, required: per snapshot and replica the number of finite particles, of
 *                                non-finite ones, sum x_d, sum x_d x_e, and sum_i sum_{j != i} W(x_i - x_j) over the
 *                                finite i from that step's pair pass (double row partials): F = last / (2 N (N - 1))
 *   pos   [S, R, N, D]           double or NULL
 *   hist  [S, ny, nx]            uint32 or NULL: counts on `grid` pooled over the replicas, as cnf_fp_particles'
 * The sums go over a fixed partition into chunks of 256 particles WITHIN a replica, the chunks' partials added in
 * ascending order: two calls are bit-identical, and one call with R replicas equals R calls with one (first_particle
 * moved by N each).  A particle that is not finite is counted as such at snapshots and is NOT masked out of the pair
 * pass: every force of its own replica is non-finite one step later (and the replica's W sum from the same step on).
 * Each step is two launches on `stream` (the pair pass, then the step kernel, ordered by the stream alone; the last
 * snapshot's pair pass computes no force) after one that draws the start, and one that adds the chunks' partials at
 * the end.  x0 [R, N, D] (device, double; optional) replaces the drawn start.
 * The caller passes `state`; `workspace` (cnf_mv_particles_workspace(R, N, D, S) bytes, 8-byte aligned) holds the pair
 * partials, the chunks' partials and the float32 mirror of the state: no allocation, no synchronisation.
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: every refusal of cnf_fp_particles (drift, D, h, var0, sigma,
 * a, n_steps, first_particle, S, snapshot steps, hist and its grid; a drift defined at another D) and of
 * cnf_interaction (a NULL or bad spec, D outside 1..14, N outside 2..2^20, R outside 1..64); a kappa that is not
 * finite; a NULL state, sums or workspace or a workspace that is too small; a stream element index
 * (first_particle + R N) (n_steps + 1) D, rounded up, that would not fit in 63 bits.
 * Out of scope: more than one rank, weighted particles, truly singular kernels (the power kind with eps = 0 and a
 * pw < 2), per-term softening lengths, float64 pair forces, the captured step, N > 2^20. */
int cnf_mv_particles_workspace(int32_t R, int64_t N, int32_t D, int32_t S, int64_t *bytes);
int cnf_mv_particles(const CnfInteractionSpec *spec, double kappa, int32_t drift, int32_t D, float a,
                     double sigma, double h, int64_t n_steps, double var0, uint64_t seed,
                     int64_t first_particle, int32_t R, int64_t N, const double *x0,
                     const int64_t *snap_step, int32_t S, const CnfFieldGrid *grid, double *state,
                     double *pos, double *sums, uint32_t *hist, void *workspace,
                     int64_t workspace_bytes, void *stream);

/* ---- a particle reference for the rwpo problems at any dimension (the reference's cost_rwpo, cnf_ot/mfc/solvers.py:
 * 190-220, is its nested Monte-Carlo at dim 2) ---------------------------------------------------------------------------
 * With eps = 1 / beta the optimal path measure of the rwpo problem is Brownian motion of variance 2 eps t started from
 * rho0 = N(0, var0 I), reweighted by exp(-g(X_T) / (2 eps)) / h(X_0), h(y) = E exp(-g(y + sqrt(2 eps T) xi) / (2 eps)):
 * the optimal energy is -2 eps E log h, X_T given X_0 = y is the weighted inner ensemble, the path between the endpoints
 * is a Brownian bridge and the control at time 0 is (E[X_T | y] - y) / T.  Everything is float64; g is CnfPotential
 * `subtype` with parameter `a` exactly as the loss kernels evaluate it (one definition, a widened).
 * Outer particle i: y = sqrt(var0) z.  Inner draw k < K from the symmetric two-centre Gaussian proposal:
 *   z_k = shrink y + sg_k m + sqrt(prop_var) xi_k,   m = centre [D] (HOST; NULL: 0), sg_k = +1 if its normal is >= 0 else -1
 * and with s^2 = 2 T / beta
 *   l_k = -beta g(z_k) / 2 - |z_k - y|^2 / (2 s^2) + (D / 2) log(prop_var / s^2)
 *         - logaddexp(-|z_k - shrink y - m|^2 / (2 prop_var), -|z_k - shrink y + m|^2 / (2 prop_var)) + log 2
 *   log_h[i] = logsumexp_k l_k - log K,  w_k = exp(l_k - lse),  ess[i] = 1 / sum w_k^2,  mean_T[i] = sum w_k z_k
 * (shrink = 1, prop_var = s^2, no centre: the plain Brownian proposal, every l_k = -beta g(z_k) / 2).
 * sel[i] is the smallest k whose cumulative sum of exp(l_j - max_j l_j) over j <= k, ascending, exceeds u[i] times the
 * total (K - 1 if rounding leaves none); the endpoint is z* = z_sel.  The path runs from (0, y) through the strictly
 * ascending times [S] (HOST, in [0, T]):
 *   x <- x + (t - t_prev) / (T - t_prev) (z* - x) + sqrt(2 eps (t - t_prev) (T - t) / (T - t_prev)) zeta
 * t = 0 gives y and t = T gives z*, both exactly.
 * Normals: global particle p = first_particle + i owns R = 4 (ceil(D / 4) + K ceil((D + 1) / 4) + ceil(S D / 4))
 * elements of the cnf_fill_normal(seed, .) stream from p R, widened exactly: D for y (padded to a block); per draw
 * xi_k [D], then the sign normal (padded to a block); then D per snapshot, used or not.  S enters R: pass the same S
 * (and times) to look at the same draws.  u [N] (device, in [0, 1)) is an input: a result is a function of its arguments.
 * Outputs (device), each optional, at least one, overwritten:
 *   log_h, ess [N]; mean_T [N, D]             double -- without u as with it
 *   sel [N]                                   int32, needs u
 *   pos [S, N, D], sums [S, 2 + D + D D], hist [S, ny, nx]: cnf_fp_particles' outputs of the bridge's positions by the
 *                                             same code, layout and non-finite rule; need u, S >= 1 and the workspace
 * No output depends on the launch, on N or on first_particle: two calls are bit-identical, a call split at any
 * first_particle reproduces the per-particle outputs bit for bit and the sums as cnf_fp_particles' split does.  Two
 * launches (the inner ensembles, one wave per outer particle; the bridges, one particle per lane) and the chunk sum.
 * `workspace` (cnf_rwpo_particles_workspace(N, D, S) bytes, 8-byte aligned; needed with pos, sums or hist) holds the
 * chunks' partials and z* [N, D]: no allocation, no synchronisation.
 * Checks come first.  CNF_ERR_INVALID, nothing enqueued: an unknown potential; D outside 1..14; T, beta, var0 or
 * prop_var not positive and finite; shrink, a or a centre entry not finite; K < 1 or above 2^20; N < 1 or above 2^31;
 * first_particle < 0 or a stream element index that would not fit in 63 bits; S outside 0..64, or 0 with pos, sums or
 * hist; times NULL with S > 0, not ascending, not finite or outside [0, T]; sel, pos, sums or hist without u; no
 * output at all; cnf_fp_particles' histogram refusals; a workspace that is NULL or too small when it is needed.
 * Out of scope: the interaction cost (the measure is no longer a reweighted Brownian motion), adaptive or learned
 * proposals, weighted output clouds, the control at interior times, more than one rank beyond first_particle. */
int cnf_rwpo_particles_workspace(int64_t N, int32_t D, int32_t S, int64_t *bytes);
int cnf_rwpo_particles(int32_t subtype, int32_t D, float a, double T, double beta, double var0,
                       double shrink, double prop_var, const double *centre /* host [D] or NULL */,
                       int64_t K, uint64_t seed, int64_t first_particle, int64_t N,
                       const double *u /* device [N] in [0,1), or NULL */,
                       const double *times /* host [S] */, int32_t S, const CnfFieldGrid *grid,
                       double *log_h, double *ess, double *mean_T, int32_t *sel,
                       double *pos, double *sums, uint32_t *hist,
                       void *workspace, int64_t workspace_bytes, void *stream);

const char *cnf_strerror(int code);
/* "gfx950" etc.: the offload arch this library was compiled for. */
const char *cnf_build_arch(void);
/* 1 if a kernel is compiled for this (dim, hidden_size, num_bins). */
int cnf_config_supported(const CnfConfig *cfg);

#ifdef __cplusplus
}
#endif
#endif /* CNF_OT_AMD_H */
