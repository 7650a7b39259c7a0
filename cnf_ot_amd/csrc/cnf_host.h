// cnf_host.h -- the functions of libcnf_ot_amd.so that one translation unit defines and another calls.  Each is
// defined in exactly one .hip and declared here and nowhere else.
#pragma once
#include "cnf_common.h"

// ---- cnf_model.hip --------------------------------------------------------------------------------------------------
// This stream's table workspace (cnf_model_reserve).  Lookup only: the compute entry points never allocate,
// free or synchronise.  *sets = 0 when the stream has no reservation.
void pwl_workspace(CnfModel* m, hipStream_t stream, float** tables, int64_t* sets, uint32_t** flag = nullptr,
                   uint32_t* epoch = nullptr);

// ---- cnf_grad.hip (called by cnf_grad_pwl.hip) ----------------------------------------------------------------------
// grad_finish_kernel: grad += the sum of the first n_slabs gradient slabs (amax != null: the table backward's, whose
// adjoint maximum it clears)
int grad_finish(const CnfModel* m, int64_t n_slabs, const float* params, float* grad, uint32_t* amax, hipStream_t stream);

// ---- cnf_grad_pwl.hip (called by cnf_grad.hip) ----------------------------------------------------------------------
// bytes of CnfModel::pwl_stats for a flow of L layers (cnf_grad_enable allocates and clears them)
size_t pwl_stats_bytes(int L);
// The table form of cnf_pass_vjp (its conditions: with the definition).  CNF_ERR_UNSUPPORTED: the caller runs the MLP
// backward.  seed_sums != null: the density-fit form; built != null: on tables already built (cnf_kinetic_potential_vjp).
int pass_vjp_pwl(CnfModel* m, int to_base, const float* pts, const float* c, int64_t c_block, const float* ybar,
                 const float* ldbar, float* xbar, float* grad, const float* params, int64_t B, hipStream_t stream,
                 float seed_coef = 0.0f, double* seed_sums = nullptr, const float* built = nullptr);

// ---- cnf_step.hip (called by cnf_grad_pwl.hip) ----------------------------------------------------------------------
// term_residual_kernel over n checked rows, the arguments of cnf_term_residual (its sums already zeroed); amax != null:
// the kernel also leaves the largest |rbar| and the non-finite flag there, as adjoint_max_kernel would
int term_residual_launch(int32_t kind, const float* r, const float* aux, int64_t n, int64_t count, int32_t D,
                         int32_t subtype, float p0, float loss_coef, double* sums, float* rbar, float* auxbar,
                         uint32_t* amax, hipStream_t stream);

// ---- cnf_flow.hip (called by cnf_grad_pwl.hip) ----------------------------------------------------------------------
// builds the dim-2 conditioner tables (cnf_pwl.h) of n slices -- conditions c[0 .. n) on the device --
// into the stream's reserved workspace and returns them; CNF_ERR_UNSUPPORTED if the configuration has no table path
// or the stream's reservation (cnf_model_reserve) is smaller than n.  Used by the table form of cnf_pass_vjp.
int cnf_internal_build_tables(CnfModel* m, hipStream_t stream, const float* c, int64_t n, float** tables);
// base -> data over n_slices slices of slice_len points each, all reading the ONE slice of points `in`, on tables
// already built in the stream's workspace (cnf_kinetic_potential_vjp)
int cnf_internal_flow_shared(CnfModel* m, hipStream_t stream, const float* in, const float* c, int64_t slice_len,
                             int64_t n_slices, const float* tables, float* out);

// Enqueues first_table_kernel (cnf_first_table.h) for the model's current parameters on `stream`, which must be ordered
// behind the last cnf_model_set_params, and marks the table built and wanted.  A kernel enqueue only.
void first_table_enqueue(CnfModel* m, hipStream_t stream);

// ---- cnf_importance.hip ---------------------------------------------------------------------------------------------
// importance_kernel and importance_finish_kernel behind cnf_importance_workspace / cnf_importance_stats(_seeded)
// (include/cnf_ot_amd.h).  The unit calls into no other and none calls into it: it shares the headers -- the tile
// helpers and flow_pass (cnf_flow_tile.h), target_logprob (cnf_terms.h), with_shape and launch (cnf_common.h) -- and
// stands apart so that the kernels of cnf_flow.hip keep their generated code.

// ---- the pair passes (cnf_mmd, cnf_knn, cnf_sinkhorn, cnf_interaction, cnf_interaction_vjp, cnf_stein, cnf_kde) -------
// Every row of a point set against every column, in column splits, with a fixed-order finish.  What they decide alike
// -- the workgroup's geometry, the column splits, a split's tiles, the block tree sum, the dispatch on the dimension --
// is cnf_pairs.h: a header without kernels, so no unit's kernels depend on another's.

// ---- cnf_mmd.hip ----------------------------------------------------------------------------------------------------
// mmd_kernel and mmd_finish_kernel behind cnf_mmd_workspace / cnf_mmd_splits / cnf_mmd2 (include/cnf_ot_amd.h).
// Model-free, like cnf_fp_particles.hip: the unit calls into no other and none calls into it.

// ---- cnf_mmd_perm.hip -----------------------------------------------------------------------------------------------
// perm_counts_kernel, perm_kernel and perm_finish_kernel behind cnf_mmd_perm_workspace / cnf_mmd_perm_splits /
// cnf_mmd_perm (include/cnf_ot_amd.h): the first pair pass on the matrix cores.  It restates cnf_mmd.hip's pair value
// and calls into no other unit.

// ---- cnf_stein_boot.hip ---------------------------------------------------------------------------------------------
// boot_kernel and boot_finish_kernel behind cnf_stein_boot_workspace / cnf_stein_boot_splits / cnf_stein_boot
// (include/cnf_ot_amd.h): the second pair pass on the matrix cores.  It restates cnf_stein.hip's pair value and spec
// checks and cnf_mmd_perm.hip's skeleton, and calls into no other unit.

// ---- cnf_sinkhorn.hip -----------------------------------------------------------------------------------------------
// sinkhorn_pair_kernel, sinkhorn_merge_kernel and sinkhorn_finish_kernel behind cnf_sinkhorn_workspace /
// cnf_sinkhorn_splits / cnf_sinkhorn (include/cnf_ot_amd.h).  Model-free as well; it shares launch_plain (cnf_common.h).

// ---- cnf_sliced.hip -------------------------------------------------------------------------------------------------
// sliced_sort_kernel, sliced_merge_kernel, sliced_w2_kernel and the three finish kernels behind cnf_sliced_workspace /
// cnf_sliced_tile / cnf_sliced_w2 (include/cnf_ot_amd.h).  Model-free as well; it shares launch_plain (cnf_common.h).

// ---- cnf_interaction.hip (called by cnf_mv_particles.hip) -----------------------------------------------------------
// What ia_finish_kernel, or another reader of the pair pass's workspace, needs: row partials [S][P][rows] doubles from
// the workspace's start, force partials [S][P][rows][D] from double `force_off` on; a row's W sum is cv times its
// splits added in ascending order, its grad W sum cf times them
struct IaPairLayout {
  int32_t P;
  int64_t force_off;
  double cv, cf;
};
// cnf_interaction's checks of spec and shape and its pair launch (ia_kernel) WITHOUT the finish: the partials of S sets
// x [S, N, D] (q, Q: query mode) into `workspace` (cnf_interaction_workspace bytes; force: with the force partials) and
// the layout into *lay.  x == NULL: the checks and the layout alone, nothing enqueued.  CNF_ERR_INVALID as
// cnf_interaction (nothing enqueued).
int interaction_pairs(const CnfInteractionSpec* spec, int32_t S, const float* x, int64_t N, const float* q, int64_t Q,
                      int32_t D, bool force, void* workspace, int64_t workspace_bytes, hipStream_t stream,
                      IaPairLayout* lay);

// ---- cnf_interaction_vjp.hip ------------------------------------------------------------------------------------------
// iv_kernel and iv_finish_kernel behind cnf_interaction_vjp_workspace / cnf_interaction_vjp (include/cnf_ot_amd.h).
// Model-free: the unit calls into no other and none calls into it; it shares cnf_interaction_pairs.h (the rows per
// lane, the column splits in the interaction's arguments, the spec and shape checks) with cnf_interaction.hip.
