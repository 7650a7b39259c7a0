// cnf_interaction.hip -- the mean-field interaction energy of a point cloud, F = 1/2 sum sum W(x_i - x_j) / (N (N - 1)),
// its first variation (W * rho)(row_i) and its Wasserstein gradient grad (W * rho)(row_i), for a pair kernel of r = |x - y|
//   Gaussian     W = sum_b amp_b exp(-r^2 / (2 bw_b^2)),   exponential  W = sum_b amp_b exp(-r / bw_b)  (Morse: two terms),
//   quadratic    W = amp_0 r^2 / 2,        power  W = sum_b amp_b u^(pw_b / 2) / pw_b (ln(u) / 2 for pw_b = 0), u = r^2 + eps^2,
// with SIGNED amplitudes: repulsion, aggregation, swarming.  The one cost of a mean-field control problem that is not
// local in the density.  Model-free, like cnf_mmd.hip, and built like it.
//
// Two modes, one kernel.  Self mode: the rows are the particles x themselves and the pair i == j is skipped by INDEX
// (only in the tiles that meet the workgroup's own rows); query mode: the rows are the points q, nothing is skipped.
// A workgroup owns IA_ROWS rows of one set and one of P column splits; a lane holds IA_R rows in registers, so a column
// read serves IA_R pairs per lane and a row's sum and force are that lane's alone: no atomics.  A column is the same
// for every lane of the wave -- its address comes from blockIdx and loop counters only -- so it is read through the
// scalar cache into SGPRs.  Distances come from coordinate differences, in cnf_mmd2's fmaf order.  One v_exp_f32 per term
// and pair; the exponential kind adds one v_rsq_f32 per pair, the power kind one v_log_f32.  The term count is
// wave-uniform and chosen per TILE, inside the kernel, so the unit has 14 x 4 x 2 kernels where a templated count would
// have four times as many.  float32
// accumulators live for one tile of IA_TILE = 64 columns and are then added into doubles.  The full square is computed:
// the per-row field and force are the product, and a triangle would need transposed accumulation.
//
// Each (split, row) writes one double (and D doubles of force) to the workspace; ia_finish_kernel adds a row's splits
// in ascending order -- that is pot and force -- then the rows in a fixed strided order and a fixed tree -- that is
// sums: bitwise reproducible, and every workspace word it reads was written by this call.  P depends on the sizes alone.
// What it shares with the other pair passes -- the workgroup's geometry, the split rule, a split's tiles, the finish's
// tree, the dispatch on D -- is cnf_pairs.h's.
#include "cnf_host.h"
#include "cnf_interaction_pairs.h"
#include "cnf_terms.h"

#include <math.h>

// Every fused multiply-add below is written as one (fmaf): with the compiler free to contract, the instantiations with
// and without the force would round the same value differently
#pragma clang fp contract(off)

namespace cnf {
namespace {

// The geometry (cnf_interaction_pairs.h, shared with cnf_interaction_vjp.hip: IA_THREADS = 256; IA_R = 2; IA_TILE = 64;)
// this unit's kernels are written for
static_assert(IA_THREADS == 256 && IA_R == 2 && IA_TILE == 64 && IA_ROWS % IA_TILE == 0, "ia_kernel's tile geometry");

// Workspace, in doubles: row partials [S][P][rows], then force partials [S][P][rows][D]
int64_t ia_row_doubles(int32_t S, int64_t rows, int32_t P) { return (int64_t)S * P * rows; }
int64_t ia_workspace_doubles(int32_t S, int64_t rows, int64_t N, int32_t D, bool force) {
  const int32_t P = ia_splits(S, rows, N);
  return ia_row_doubles(S, rows, P) * (force ? 1 + D : 1);
}

// n <= IA_TILE columns starting at column c0 of `col` against the lane's rows; the float32 tile sums into the doubles.
// The quadratic kind accumulates r^2 and (x - y); amp_0 joins the finish kernel's coefficients.
template <int D, int KIND, bool FORCE, bool DIAG, int NT>
__device__ __forceinline__ void ia_tile(const float* __restrict__ col, int64_t c0, int n, int first_local,
                                        const float (&x)[IA_R][D], const IaCoef& k, const IaPower& pk,
                                        double (&sum)[IA_R], double (&gsum)[IA_R][D]) {
  float ks[IA_R], g[IA_R][D];
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
    ks[r] = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) g[r][d] = 0.0f;
  }
  const float* p = col + c0 * D;               // wave-uniform: scalar loads
  // columns in flight: at most 14 SGPRs of coordinates beside the 12 of coefficients
  // (the power kind at D = 3: 3 columns, for its u and L beside the coefficients -- with 4 two SGPRs were spilled)
  constexpr int U = KIND == CNF_INTERACTION_POWER && D == 3 ? 3 : D <= 3 ? 4 : D == 4 ? 3 : D <= 6 ? 2 : 1;
#pragma unroll U
  for (int j = 0; j < n; ++j) {
    float c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = p[j * D + d];
    float diff[IA_R][D], d2[IA_R], v[IA_R], w[IA_R];
#pragma unroll
    for (int r = 0; r < IA_R; ++r) {
#pragma unroll
      for (int d = 0; d < D; ++d) diff[r][d] = x[r][d] - c[d];
      if constexpr (KIND == CNF_INTERACTION_POWER) d2[r] = fmaf(diff[r][0], diff[r][0], pk.eps2);   // u = d2 + eps^2
      else d2[r] = diff[r][0] * diff[r][0];
#pragma unroll
      for (int d = 1; d < D; ++d) d2[r] = fmaf(diff[r][d], diff[r][d], d2[r]);
    }
    if constexpr (KIND == CNF_INTERACTION_QUADRATIC) {
#pragma unroll
      for (int r = 0; r < IA_R; ++r) {
        v[r] = d2[r];
        w[r] = 1.0f;
      }
    } else if constexpr (KIND == CNF_INTERACTION_POWER) {
      // One v_log_f32 per pair, one v_exp_f32 per term: t_b = u^(pw_b / 2 - 1), the loop of the other kinds; the value
      // is u sum_b amp_b t_b + cl L after it (a per-term choice between a power and a log term, though wave-uniform,
      // compiled to both forms and a select per term and pair; the log terms' coefficients are added on the host instead).
      // The clamp is what keeps a coincident pair with eps = 0 (every pw_b >= 2, so nc_b >= 0 and cl = 0) finite:
      // u = 1e-30 gives a finite L and t_b <= 1, so the pair adds W(0) = 0 (below 1e-30 sum_b |amp_b|) and, with
      // diff = 0, a zero force; log2(0) = -inf times nc_b = 0 would be NaN
      float u[IA_R], L[IA_R];
#pragma unroll
      for (int r = 0; r < IA_R; ++r) {
        u[r] = fmaxf(d2[r], 1e-30f);
        L[r] = __builtin_amdgcn_logf(u[r]);
        v[r] = 0.0f;
        w[r] = 0.0f;
      }
#pragma unroll
      for (int b = 0; b < NT; ++b) {
#pragma unroll
        for (int r = 0; r < IA_R; ++r) {
          const float t = __builtin_amdgcn_exp2f(L[r] * k.nc[b]);
          v[r] = fmaf(t, k.amp[b], v[r]);
          if constexpr (FORCE) w[r] = fmaf(t, k.ga[b], w[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < IA_R; ++r) v[r] = fmaf(u[r], v[r], L[r] * pk.cl);
    } else {
      float a[IA_R], inv[IA_R];
#pragma unroll
      for (int r = 0; r < IA_R; ++r) {
        if constexpr (KIND == CNF_INTERACTION_EXPONENTIAL) {   // grad W is 0 at a coincident pair (cnf_mmd's energy rule)
          inv[r] = d2[r] > 1e-30f ? __builtin_amdgcn_rsqf(d2[r]) : 0.0f;
          a[r] = d2[r] * inv[r];
        } else {
          inv[r] = 1.0f;
          a[r] = d2[r];
        }
        v[r] = 0.0f;
        w[r] = 0.0f;
      }
#pragma unroll
      for (int b = 0; b < NT; ++b) {
#pragma unroll
        for (int r = 0; r < IA_R; ++r) {
          const float e = __builtin_amdgcn_exp2f(a[r] * k.nc[b]);
          v[r] = fmaf(e, k.amp[b], v[r]);
          if constexpr (FORCE) w[r] = fmaf(e, k.ga[b], w[r]);
        }
      }
      if constexpr (FORCE && KIND == CNF_INTERACTION_EXPONENTIAL) {
#pragma unroll
        for (int r = 0; r < IA_R; ++r) w[r] = w[r] * inv[r];
      }
    }
#pragma unroll
    for (int r = 0; r < IA_R; ++r) {
      // (the force's diagonal term is diff = 0 times a finite w: nothing to mask)
      if constexpr (DIAG) v[r] = first_local + j == r * IA_THREADS + (int)threadIdx.x ? 0.0f : v[r];
      ks[r] += v[r];
      if constexpr (FORCE) {
#pragma unroll
        for (int d = 0; d < D; ++d) g[r][d] = fmaf(diff[r][d], w[r], g[r][d]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
    sum[r] += (double)ks[r];
    if constexpr (FORCE) {
#pragma unroll
      for (int d = 0; d < D; ++d) gsum[r][d] += (double)g[r][d];
    }
  }
}

// The tile for the spec's term count: a wave-uniform switch per tile of 64 columns, so the pair loop itself is straight
// code for its count (a count tested per column kept every column's scalar load and its wait between two branches)
template <int D, int KIND, bool FORCE, bool DIAG>
__device__ __forceinline__ void ia_tile_terms(const float* __restrict__ col, int64_t c0, int n, int first_local,
                                              const float (&x)[IA_R][D], const IaCoef& k, const IaPower& pk,
                                              double (&sum)[IA_R], double (&gsum)[IA_R][D]) {
  if constexpr (KIND == CNF_INTERACTION_QUADRATIC) {
    ia_tile<D, KIND, FORCE, DIAG, 1>(col, c0, n, first_local, x, k, pk, sum, gsum);
  } else {
    switch (k.nt) {
      case 1: ia_tile<D, KIND, FORCE, DIAG, 1>(col, c0, n, first_local, x, k, pk, sum, gsum); break;
      case 2: ia_tile<D, KIND, FORCE, DIAG, 2>(col, c0, n, first_local, x, k, pk, sum, gsum); break;
      case 3: ia_tile<D, KIND, FORCE, DIAG, 3>(col, c0, n, first_local, x, k, pk, sum, gsum); break;
      default: ia_tile<D, KIND, FORCE, DIAG, 4>(col, c0, n, first_local, x, k, pk, sum, gsum); break;
    }
  }
}

// grid (row groups x P, S): blockIdx.y = the set, blockIdx.x = row group * P + split.  rows_p == col: self mode.
template <int D, int KIND, bool FORCE>
__global__ __launch_bounds__(IA_THREADS) void ia_kernel(const float* __restrict__ x, const float* __restrict__ q,
                                                        int64_t N, int64_t n_rows, int32_t P, const IaCoef k,
                                                        double* __restrict__ ws, int64_t force_off,
                                                        const IaPower pk) {
  const int s = (int)blockIdx.y;
  const int64_t rg = blockIdx.x / (unsigned)P;
  const int p = (int)(blockIdx.x % (unsigned)P);
  const int64_t row0 = rg * IA_ROWS;
  const bool self = q == nullptr;
  const float* col = x + (int64_t)s * N * D;
  const float* rows_p = self ? col : q + (int64_t)s * n_rows * D;
  const auto [t0, t1] = pair_tile_range<int64_t>(N, P, p);
  float xr[IA_R][D];
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
    const int64_t i = row0 + r * IA_THREADS + (int64_t)threadIdx.x;
#pragma unroll
    for (int d = 0; d < D; ++d) xr[r][d] = i < n_rows ? rows_p[i * D + d] : 0.0f;
  }
  double sum[IA_R], gsum[IA_R][D];
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
    sum[r] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) gsum[r][d] = 0.0;
  }
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t c0 = t * IA_TILE;
    const int n = (int)(N - c0 < IA_TILE ? N - c0 : IA_TILE);
    // IA_TILE divides IA_ROWS and row0 is a multiple of IA_ROWS: a tile lies inside the workgroup's rows or outside
    if (self && c0 >= row0 && c0 < row0 + IA_ROWS)
      ia_tile_terms<D, KIND, FORCE, true>(col, c0, n, (int)(c0 - row0), xr, k, pk, sum, gsum);
    else
      ia_tile_terms<D, KIND, FORCE, false>(col, c0, n, 0, xr, k, pk, sum, gsum);
  }
  double* part = ws + ((int64_t)s * P + p) * n_rows;
  double* gpart = ws + force_off + ((int64_t)s * P + p) * n_rows * D;
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
    const int64_t i = row0 + r * IA_THREADS + (int64_t)threadIdx.x;
    if (i < n_rows) {
      part[i] = sum[r];
      if constexpr (FORCE) {
#pragma unroll
        for (int d = 0; d < D; ++d) gpart[i * D + d] = gsum[r][d];
      }
    }
  }
}

// Workgroups [0, S): a row's splits added in ascending order -- pot[s, i] = cv / n times that -- thread t taking rows
// t, t + 256, ... and the threads' totals meeting in a fixed tree: sums[s] = cv times the total.  The workgroups after
// them: force = cf / n times a component's splits.
__global__ __launch_bounds__(IA_THREADS) void ia_finish_kernel(const double* __restrict__ ws, int32_t S, int64_t n_rows,
                                                               int32_t D, int32_t P, int64_t force_off, double cv,
                                                               double cf, double inv_n, double* __restrict__ sums,
                                                               float* __restrict__ pot, float* __restrict__ force) {
  __shared__ double s_acc[IA_THREADS];
  const int t = (int)threadIdx.x;
  if ((int)blockIdx.x < S) {
    const int64_t s = blockIdx.x;
    const double* part = ws + s * P * n_rows;
    double acc = 0.0;
    for (int64_t i = t; i < n_rows; i += IA_THREADS) {
      double v = part[i];
      for (int p = 1; p < P; ++p) v += part[p * n_rows + i];
      if (pot) pot[s * n_rows + i] = (float)(cv * v * inv_n);
      acc += v;
    }
    const double total = pair_block_sum<IA_THREADS>(s_acc, t, acc);
    if (t == 0) sums[s] = cv * total;
    return;
  }
  if (!force) return;
  const int64_t per_set = n_rows * D;
  const int64_t e = ((int64_t)blockIdx.x - S) * IA_THREADS + t;
  if (e >= (int64_t)S * per_set) return;
  const int64_t s = e / per_set, r = e % per_set;
  const double* g = ws + force_off + s * P * per_set + r;
  double a = g[0];
  for (int p = 1; p < P; ++p) a += g[p * per_set];
  force[e] = (float)(cf * a * inv_n);
}

struct IaLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *q;
  int64_t N, rows;
  int32_t P;
  IaCoef k;
  IaPower pk;
  double* ws;
  int64_t force_off;
  bool force;
};

template <int D, int KIND> void ia_launch_force(const IaLaunch& a) {
  if (a.force)
    hipLaunchKernelGGL((ia_kernel<D, KIND, true>), a.grid, dim3(IA_THREADS), 0, a.st, a.x, a.q, a.N, a.rows, a.P, a.k, a.ws,
                       a.force_off, a.pk);
  else
    hipLaunchKernelGGL((ia_kernel<D, KIND, false>), a.grid, dim3(IA_THREADS), 0, a.st, a.x, a.q, a.N, a.rows, a.P, a.k, a.ws,
                       a.force_off, a.pk);
}
template <int D> void ia_launch_kind(int kind, const IaLaunch& a) {
  if (kind == CNF_INTERACTION_GAUSSIAN) ia_launch_force<D, CNF_INTERACTION_GAUSSIAN>(a);
  else if (kind == CNF_INTERACTION_EXPONENTIAL) ia_launch_force<D, CNF_INTERACTION_EXPONENTIAL>(a);
  else if (kind == CNF_INTERACTION_POWER) ia_launch_force<D, CNF_INTERACTION_POWER>(a);
  else ia_launch_force<D, CNF_INTERACTION_QUADRATIC>(a);   // (ia_coef has refused every other kind)
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_interaction_workspace(int32_t S, int64_t N, int64_t Q, int32_t D, int32_t want_rows, int64_t* bytes) {
  if (!bytes || !ia_shape_ok(S, N, Q, D)) return CNF_ERR_INVALID;
  *bytes = ia_workspace_doubles(S, Q > 0 ? Q : N, N, D, want_rows != 0) * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_interaction_splits(int32_t S, int64_t N, int64_t Q, int32_t D) {
  return ia_shape_ok(S, N, Q, D) ? ia_splits(S, Q > 0 ? Q : N, N) : CNF_ERR_INVALID;
}

int interaction_pairs(const CnfInteractionSpec* spec, int32_t S, const float* x, int64_t N, const float* q, int64_t Q,
                      int32_t D, bool force, void* workspace, int64_t workspace_bytes, hipStream_t stream,
                      IaPairLayout* lay) {
  if (!spec || !lay || !ia_shape_ok(S, N, Q, D)) return CNF_ERR_INVALID;
  IaLaunch a{};
  if (!ia_coef(spec, &a.k, &a.pk)) return CNF_ERR_INVALID;
  a.force = force;
  a.rows = Q > 0 ? Q : N;
  a.P = ia_splits(S, a.rows, N);
  a.force_off = ia_row_doubles(S, a.rows, a.P);
  const bool quad = spec->kind == CNF_INTERACTION_QUADRATIC;
  lay->P = a.P;
  lay->force_off = a.force_off;
  lay->cv = quad ? 0.5 * (double)spec->amp[0] : 1.0;
  lay->cf = quad ? (double)spec->amp[0] : 1.0;
  if (!x) return CNF_OK;
  if (!workspace || workspace_bytes < ia_workspace_doubles(S, a.rows, N, D, a.force) * (int64_t)sizeof(double))
    return CNF_ERR_INVALID;
  a.grid = dim3((unsigned)(row_groups(a.rows) * a.P), (unsigned)S);
  a.st = stream;
  a.x = x; a.q = q; a.N = N;
  a.ws = (double*)workspace;
  pair_dispatch_dim(D, [&](auto d) { ia_launch_kind<decltype(d)::value>(spec->kind, a); });
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_interaction(const CnfInteractionSpec* spec, int32_t S, const float* x, int64_t N, const float* q,
                               int64_t Q, int32_t D, double* sums, float* pot, float* force, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  if (!spec || !x || !sums || !workspace || !ia_shape_ok(S, N, Q, D)) return CNF_ERR_INVALID;
  if ((q == nullptr) != (Q == 0)) return CNF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  IaPairLayout lay{};
  const int rc = interaction_pairs(spec, S, x, N, q, Q, D, force != nullptr, workspace, workspace_bytes, st, &lay);
  if (rc != CNF_OK) return rc;
  const int64_t rows = Q > 0 ? Q : N;
  const double inv_n = 1.0 / (double)(Q > 0 ? N : N - 1);
  const int64_t force_wgs = force ? ((int64_t)S * rows * D + IA_THREADS - 1) / IA_THREADS : 0;
  hipLaunchKernelGGL(ia_finish_kernel, dim3((unsigned)(S + force_wgs)), dim3(IA_THREADS), 0, st, (const double*)workspace,
                     S, rows, D, lay.P, lay.force_off, lay.cv, lay.cf, inv_n, sums, pot, force);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
