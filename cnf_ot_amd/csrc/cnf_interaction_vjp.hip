// cnf_interaction_vjp.hip -- the vector-Jacobian product of cnf_interaction's self-mode force.  With the force
//   f_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j)
// of a point cloud and an adjoint g_i of it, the adjoint of the points is, W being even,
//   xbar_k = (1 / (N - 1)) sum_{j != k} H(x_k - x_j) (g_k - g_j),    H(d) v = c1 v + d (d . v) c2,
// H the pair Hessian of W: with r = |d| and e_b the term's exponential, as ia_tile (cnf_interaction.hip) forms it,
//   Gaussian     c1 = sum_b (-amp_b / bw_b^2) e_b  (ia_tile's w)      c2 = sum_b (amp_b / bw_b^4) e_b
//   exponential  c1 = w / r,  c2 = w' / r^2 - w / r^3 = (w' - c1) / r^2,   w = sum_b (-amp_b / bw_b) e_b,
//                w' = sum_b (amp_b / bw_b^2) e_b;  both 0 at a coincident pair (d^2 <= 1e-30: ia_tile's rule)
//   quadratic    c1 = amp_0 (it joins the finish kernel's coefficient),  c2 = 0
//   power        c1 = sum_b amp_b t_b,  c2 = (sum_b amp_b (pw_b - 2) t_b) / u,   t_b = u^(pw_b / 2 - 1), u = d^2 + eps^2
// What a loss needs that has the force inside a square (the interacting Fokker-Planck residual): a
// second pair sum, which composed in torch is a double backward through an N x N x D pair tensor.  The pair j == k
// contributes d = 0 and g_k - g_k = 0: nothing is masked.
//
// Built as ia_kernel is.  A workgroup owns IA_ROWS rows of one set and one of P column splits; a lane keeps IA_R rows
// of x AND g in registers; a column's x_j and g_j are the same for every lane of the wave and come through the scalar
// cache.  One v_exp_f32 per term and pair; the exponential kind adds one v_rsq_f32 per pair, the power kind one v_log_f32
// and one v_rcp_f32.  The term count is wave-uniform and switched per TILE.  float32 accumulators live for one tile of
// IA_TILE = 64 columns and are then added into doubles.  Each (split, row) writes D doubles to the workspace;
// iv_finish_kernel adds a row's splits in ascending order: no atomics, bitwise reproducible, and every workspace word it
// reads was written by this call.
// What it shares with the other pair passes -- the workgroup's geometry, the split rule, a split's tiles, the
// dispatch on D -- is cnf_pairs.h's.
#include "cnf_host.h"
#include "cnf_interaction_pairs.h"

#include <math.h>

// (as cnf_interaction.hip: every fused multiply-add is written as one)
#pragma clang fp contract(off)

namespace cnf {
namespace {

// Term b of a pair: e_b = exp2(nc_b a) with IaCoef's nc_b and a (the power kind: a = log2 u); c1's sum += k1_b e_b,
// c2's sum += k2_b e_b
struct IvCoef {
  float nc[IA_MAX_TERMS], k1[IA_MAX_TERMS], k2[IA_MAX_TERMS];
  int32_t nt;
};

// Workspace, in doubles: the partials [S][P][N][D]
int64_t iv_workspace_doubles(int32_t S, int64_t N, int32_t D) { return (int64_t)S * ia_splits(S, N, N) * N * D; }

// n <= IA_TILE columns starting at column c0 against the lane's rows; the float32 tile sums into the doubles
template <int D, int KIND, int NT>
__device__ __forceinline__ void iv_tile(const float* __restrict__ colx, const float* __restrict__ colg, int64_t c0, int n,
                                        const float (&x)[IA_R][D], const float (&g)[IA_R][D], const IvCoef& k,
                                        const float eps2, double (&acc)[IA_R][D]) {
  float o[IA_R][D];
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
#pragma unroll
    for (int d = 0; d < D; ++d) o[r][d] = 0.0f;
  }
  const float* px = colx + c0 * D;             // wave-uniform: scalar loads
  const float* pg = colg + c0 * D;
  // columns in flight: at most 14 SGPRs of x_j and g_j beside the 12 of coefficients
  constexpr int U = D == 1 ? 4 : D == 2 ? 3 : D == 3 ? 2 : 1;
#pragma unroll U
  for (int j = 0; j < n; ++j) {
    float c[D], h[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      c[d] = px[j * D + d];
      h[d] = pg[j * D + d];
    }
#pragma unroll
    for (int r = 0; r < IA_R; ++r) {
      float diff[D], dv[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        diff[d] = x[r][d] - c[d];
        dv[d] = g[r][d] - h[d];
      }
      if constexpr (KIND == CNF_INTERACTION_QUADRATIC) {
#pragma unroll
        for (int d = 0; d < D; ++d) o[r][d] += dv[d];
      } else {
        // (the power kind: u = d2 + eps^2, the softening joining the first product)
        float d2 = KIND == CNF_INTERACTION_POWER ? fmaf(diff[0], diff[0], eps2) : diff[0] * diff[0], dot = diff[0] * dv[0];
#pragma unroll
        for (int d = 1; d < D; ++d) {
          d2 = fmaf(diff[d], diff[d], d2);
          dot = fmaf(diff[d], dv[d], dot);
        }
        float a = d2, inv = 1.0f;
        if constexpr (KIND == CNF_INTERACTION_EXPONENTIAL) {
          inv = d2 > 1e-30f ? __builtin_amdgcn_rsqf(d2) : 0.0f;
          a = d2 * inv;
        }
        if constexpr (KIND == CNF_INTERACTION_POWER) {      // (ia_tile's clamp: a coincident pair with eps = 0 stays finite)
          const float u = fmaxf(d2, 1e-30f);
          inv = __builtin_amdgcn_rcpf(u);
          a = __builtin_amdgcn_logf(u);
        }
        float c1 = 0.0f, c2 = 0.0f;
#pragma unroll
        for (int b = 0; b < NT; ++b) {
          const float e = __builtin_amdgcn_exp2f(a * k.nc[b]);
          c1 = fmaf(e, k.k1[b], c1);
          c2 = fmaf(e, k.k2[b], c2);
        }
        if constexpr (KIND == CNF_INTERACTION_EXPONENTIAL) {
          c1 = c1 * inv;                       // w / r
          c2 = (c2 - c1) * (inv * inv);        // (w' - w / r) / r^2
        }
        if constexpr (KIND == CNF_INTERACTION_POWER) c2 = c2 * inv;   // u^(q - 1) = t / u
        const float s = dot * c2;
#pragma unroll
        for (int d = 0; d < D; ++d) o[r][d] = fmaf(diff[d], s, fmaf(dv[d], c1, o[r][d]));
      }
    }
  }
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
#pragma unroll
    for (int d = 0; d < D; ++d) acc[r][d] += (double)o[r][d];
  }
}

// The tile for the spec's term count: a wave-uniform switch per tile, so the pair loop is straight code for its count
template <int D, int KIND>
__device__ __forceinline__ void iv_tile_terms(const float* __restrict__ colx, const float* __restrict__ colg, int64_t c0,
                                              int n, const float (&x)[IA_R][D], const float (&g)[IA_R][D],
                                              const IvCoef& k, const float eps2, double (&acc)[IA_R][D]) {
  if constexpr (KIND == CNF_INTERACTION_QUADRATIC) {
    iv_tile<D, KIND, 1>(colx, colg, c0, n, x, g, k, eps2, acc);
  } else {
    switch (k.nt) {
      case 1: iv_tile<D, KIND, 1>(colx, colg, c0, n, x, g, k, eps2, acc); break;
      case 2: iv_tile<D, KIND, 2>(colx, colg, c0, n, x, g, k, eps2, acc); break;
      case 3: iv_tile<D, KIND, 3>(colx, colg, c0, n, x, g, k, eps2, acc); break;
      default: iv_tile<D, KIND, 4>(colx, colg, c0, n, x, g, k, eps2, acc); break;
    }
  }
}

// grid (row groups x P, S): blockIdx.y = the set, blockIdx.x = row group * P + split.  eps2 (IaPower's; the power kind
// alone reads it) is the last argument, so the other kinds' arguments stay where they were
template <int D, int KIND>
__global__ __launch_bounds__(IA_THREADS) void iv_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        int64_t N, int32_t P, const IvCoef k, double* __restrict__ ws,
                                                        const float eps2) {
  const int s = (int)blockIdx.y;
  const int64_t rg = blockIdx.x / (unsigned)P;
  const int p = (int)(blockIdx.x % (unsigned)P);
  const int64_t row0 = rg * IA_ROWS;
  const float* colx = x + (int64_t)s * N * D;
  const float* colg = g + (int64_t)s * N * D;
  const auto [t0, t1] = pair_tile_range<int64_t>(N, P, p);
  float xr[IA_R][D], gr[IA_R][D];
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
    const int64_t i = row0 + r * IA_THREADS + (int64_t)threadIdx.x;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      xr[r][d] = i < N ? colx[i * D + d] : 0.0f;
      gr[r][d] = i < N ? colg[i * D + d] : 0.0f;
    }
  }
  double acc[IA_R][D];
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
#pragma unroll
    for (int d = 0; d < D; ++d) acc[r][d] = 0.0;
  }
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t c0 = t * IA_TILE;
    const int n = (int)(N - c0 < IA_TILE ? N - c0 : IA_TILE);
    iv_tile_terms<D, KIND>(colx, colg, c0, n, xr, gr, k, eps2, acc);
  }
  double* part = ws + ((int64_t)s * P + p) * N * D;
#pragma unroll
  for (int r = 0; r < IA_R; ++r) {
    const int64_t i = row0 + r * IA_THREADS + (int64_t)threadIdx.x;
    if (i < N) {
#pragma unroll
      for (int d = 0; d < D; ++d) part[i * D + d] = acc[r][d];
    }
  }
}

// xbar = cf / (N - 1) times a component's splits, added in ascending order
__global__ __launch_bounds__(IA_THREADS) void iv_finish_kernel(const double* __restrict__ ws, int64_t total, int64_t per_set,
                                                               int32_t P, double cf, double inv_n,
                                                               float* __restrict__ xbar) {
  const int64_t e = (int64_t)blockIdx.x * IA_THREADS + (int64_t)threadIdx.x;
  if (e >= total) return;
  const int64_t s = e / per_set, r = e % per_set;
  const double* part = ws + s * P * per_set + r;
  double a = part[0];
  for (int p = 1; p < P; ++p) a += part[p * per_set];
  xbar[e] = (float)(cf * a * inv_n);
}

struct IvLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *g;
  int64_t N;
  int32_t P;
  IvCoef k;
  double* ws;
  float eps2;
};

template <int D> void iv_launch_kind(int kind, const IvLaunch& a) {
  if (kind == CNF_INTERACTION_GAUSSIAN)
    hipLaunchKernelGGL((iv_kernel<D, CNF_INTERACTION_GAUSSIAN>), a.grid, dim3(IA_THREADS), 0, a.st, a.x, a.g, a.N, a.P, a.k, a.ws, a.eps2);
  else if (kind == CNF_INTERACTION_EXPONENTIAL)
    hipLaunchKernelGGL((iv_kernel<D, CNF_INTERACTION_EXPONENTIAL>), a.grid, dim3(IA_THREADS), 0, a.st, a.x, a.g, a.N, a.P, a.k, a.ws, a.eps2);
  else if (kind == CNF_INTERACTION_POWER)
    hipLaunchKernelGGL((iv_kernel<D, CNF_INTERACTION_POWER>), a.grid, dim3(IA_THREADS), 0, a.st, a.x, a.g, a.N, a.P, a.k, a.ws, a.eps2);
  else                                         // (ia_coef has refused every other kind)
    hipLaunchKernelGGL((iv_kernel<D, CNF_INTERACTION_QUADRATIC>), a.grid, dim3(IA_THREADS), 0, a.st, a.x, a.g, a.N, a.P, a.k, a.ws, a.eps2);
}

// The spec as iv_kernel reads it; false for what cnf_interaction refuses in one and for a Hessian coefficient
// (amp / bw^4, Gaussian; amp / bw^2, exponential; amp (pw - 2) eps^(pw - 4), power) outside float32's range
bool iv_coef(const CnfInteractionSpec* spec, IvCoef* k, float* eps2) {
  IaCoef base;
  IaPower pk;
  *k = IvCoef{};
  *eps2 = 0.0f;
  if (spec->kind == CNF_INTERACTION_POWER) {
    base = IaCoef{};
    pk = IaPower{};
    if (!ia_coef_power(spec, &base, &pk, true)) return false;
    k->nt = base.nt;
    *eps2 = pk.eps2;
    for (int b = 0; b < base.nt; ++b) {
      k->nc[b] = base.nc[b];
      k->k1[b] = base.ga[b];
      k->k2[b] = (float)((double)spec->amp[b] * ((double)spec->pw[b] - 2.0));
      if (!std::isfinite(k->k2[b])) return false;
    }
    return true;
  }
  if (!ia_coef(spec, &base, &pk)) return false;
  k->nt = base.nt;
  for (int b = 0; b < base.nt; ++b) {
    const double ib = 1.0 / ((double)spec->bw[b] * (double)spec->bw[b]);
    k->nc[b] = base.nc[b];
    k->k1[b] = base.ga[b];
    k->k2[b] = (float)((double)spec->amp[b] * (spec->kind == CNF_INTERACTION_GAUSSIAN ? ib * ib : ib));
    if (!std::isfinite(k->k2[b])) return false;
  }
  return true;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_interaction_vjp_workspace(int32_t S, int64_t N, int32_t D, int64_t* bytes) {
  if (!bytes || !ia_shape_ok(S, N, 0, D)) return CNF_ERR_INVALID;
  *bytes = iv_workspace_doubles(S, N, D) * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_interaction_vjp(const CnfInteractionSpec* spec, int32_t S, const float* x, const float* g, int64_t N,
                                   int32_t D, float* xbar, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!spec || !x || !g || !xbar || !workspace || !ia_shape_ok(S, N, 0, D)) return CNF_ERR_INVALID;
  IvLaunch a{};
  if (!iv_coef(spec, &a.k, &a.eps2)) return CNF_ERR_INVALID;
  if (workspace_bytes < iv_workspace_doubles(S, N, D) * (int64_t)sizeof(double)) return CNF_ERR_INVALID;
  a.P = ia_splits(S, N, N);
  a.grid = dim3((unsigned)(row_groups(N) * a.P), (unsigned)S);
  a.st = (hipStream_t)stream;
  a.x = x; a.g = g; a.N = N;
  a.ws = (double*)workspace;
  pair_dispatch_dim(D, [&](auto d) { iv_launch_kind<decltype(d)::value>(spec->kind, a); });
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  const int64_t per_set = N * D, total = (int64_t)S * per_set;
  const double cf = spec->kind == CNF_INTERACTION_QUADRATIC ? (double)spec->amp[0] : 1.0;
  hipLaunchKernelGGL(iv_finish_kernel, dim3((unsigned)((total + IA_THREADS - 1) / IA_THREADS)), dim3(IA_THREADS), 0, a.st,
                     (const double*)workspace, total, per_set, a.P, cf, 1.0 / (double)(N - 1), xbar);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
