// cnf_host.h -- the functions of libcnf_ot_amd.so that one translation unit defines and another calls.  Each is
// defined in exactly one .hip and declared here and nowhere else.
#pragma once
#include "cnf_common.h"

// ---- cnf_model.hip --------------------------------------------------------------------------------------------------
// This stream's table workspace (cnf_model_reserve).  Lookup only: the compute entry points never allocate,
// free or synchronise.  *sets = 0 when the stream has no reservation.
void pwl_workspace(CnfModel* m, hipStream_t stream, float** tables, int64_t* sets, uint32_t** flag = nullptr,
                   uint32_t* epoch = nullptr);

// ---- cnf_flow.hip (called by cnf_grad.hip) --------------------------------------------------------------------------
// builds the dim-2 conditioner tables (cnf_pwl.h) of n slices -- conditions c[0 .. n) on the device --
// into the stream's reserved workspace and returns them; CNF_ERR_UNSUPPORTED if the configuration has no table path
// or the stream's reservation (cnf_model_reserve) is smaller than n.  Used by the table form of cnf_pass_vjp.
int cnf_internal_build_tables(CnfModel* m, hipStream_t stream, const float* c, int64_t n, float** tables);
// base -> data over n_slices slices of slice_len points each, all reading the ONE slice of points `in`, on tables
// already built in the stream's workspace (cnf_kinetic_potential_vjp)
int cnf_internal_flow_shared(CnfModel* m, hipStream_t stream, const float* in, const float* c, int64_t slice_len,
                             int64_t n_slices, const float* tables, float* out);

// ---- cnf_importance.hip ---------------------------------------------------------------------------------------------
// importance_kernel and importance_finish_kernel behind cnf_importance_workspace / cnf_importance_stats(_seeded)
// (include/cnf_ot_amd.h).  The unit calls into no other and none calls into it: it shares the headers -- the tile
// helpers and flow_pass (cnf_flow_tile.h), target_logprob (cnf_terms.h), with_shape and launch (cnf_common.h) -- and
// stands apart so that the kernels of cnf_flow.hip keep their generated code.

// ---- cnf_mmd.hip ----------------------------------------------------------------------------------------------------
// mmd_kernel and mmd_finish_kernel behind cnf_mmd_workspace / cnf_mmd_splits / cnf_mmd2 (include/cnf_ot_amd.h).
// Model-free, like cnf_fp_particles.hip: the unit calls into no other and none calls into it.
