// cnf_stein.hip -- the kernel Stein discrepancy of point sets against a score (include/cnf_ot_amd.h has the entry).
// With the base kernel k(x, y) = phi(q), q = |d|^2, d = x - y, and p0 .. p3 = phi, phi', phi'', phi''' at q,
//   k_p(x, y) = p0 (s_x . s_y) + 2 p1 d . (s_y - s_x) - 4 p2 q - 2 D p1
// and, per ordered pair i != j and times 2 / (N (N - 1)) in the finish kernel, the gradients of KSD^2_U
//   d / d s_i:  p0 s_j - 2 p1 d
//   d / d x_i:  (2 p1 s_i . s_j + 4 p2 d . (s_j - s_i) - 8 p3 q - (8 + 4 D) p2) d + 2 p1 (s_j - s_i)
//   IMQ       p0 = sum_b w_b u_b^beta, u_b = c_b^2 + q: per term ONE v_log_f32 (L = log2 u_b), one v_exp_f32
//             (t = exp2(beta L)) and one v_rcp_f32 (1 / u_b); the other three powers are t / u_b, t / u_b^2, t / u_b^3
//             times w_b beta, w_b beta (beta - 1), w_b beta (beta - 1) (beta - 2)
//   Gaussian  p0 = sum_b w_b e_b, e_b = exp2(nc_b q): one v_exp_f32 per term; p1 .. p3 are e_b times
//             -w_b / (2 h_b^2), w_b / (4 h_b^4), -w_b / (8 h_b^6)
// Composed in torch the same statistic is several N x N matrices and their backward.
//
// Built as ia_kernel and iv_kernel are.  A workgroup owns ST_THREADS * R rows of one set and one
// of P column splits; a lane keeps R rows of x AND s in registers (R = st_rows(D): two for D <= 8, one above, where two
// rows with the gradients take 230 VGPRs and more, past 256 into the AGPRs from D = 12: DESIGN.md 5.3q); a column's x_j and s_j are the same for every lane of the
// wave and come through the scalar cache.  The pair i == j is skipped by index: its four kernel values are set to 0, so
// a duplicated point at another index does interact.  The term count is wave-uniform and switched per TILE.  float32
// accumulators live for one tile of IA_TILE = 64 columns and are then added into doubles.  Each (split, row) writes one
// double (and 2 D of the gradients) to the workspace; st_finish_kernel adds a row's splits in ascending order and the
// rows in a fixed tree: no atomics, bitwise reproducible, and every workspace word it reads was written by this call.
// What it shares with the other pair passes -- the workgroup's geometry, the split rule, a split's tiles, the finish's
// tree, the dispatch on D -- is cnf_pairs.h's.
#include "cnf_host.h"
#include "cnf_interaction_pairs.h"

#include <math.h>

// (as cnf_interaction.hip: every fused multiply-add is written as one)
#pragma clang fp contract(off)

namespace cnf {
namespace {

constexpr int ST_THREADS = IA_THREADS;
constexpr int ST_R_MAX_D = 8;                  // the largest D with two rows per lane
constexpr int st_rows(int D) { return D <= ST_R_MAX_D ? 2 : 1; }

// Term b of a pair: a_b = c_b^2 (IMQ: u_b = q + a_b) or nc_b = -log2 e / (2 h_b^2) (Gaussian: e_b = exp2(a_b q));
// p_m += k_m[b] times the term's m-th factor
struct StCoef {
  float a[CNF_STEIN_MAX_TERMS], k0[CNF_STEIN_MAX_TERMS], k1[CNF_STEIN_MAX_TERMS], k2[CNF_STEIN_MAX_TERMS],
      k3[CNF_STEIN_MAX_TERMS];
  float beta;
  int32_t nt;
};

inline int64_t st_row_groups(int64_t n, int32_t D) { return pair_row_groups(n, ST_THREADS * st_rows(D)); }

// Column splits (pair_splits) for this unit's row groups
inline int32_t st_splits(int32_t S, int64_t N, int32_t D) {
  return pair_splits((int64_t)S * st_row_groups(N, D), pair_tiles(N));
}

// Workspace, in doubles: the value partials [S][P][N], then (grad) those of grad_x and of grad_s, [S][P][N][D] each
int64_t st_value_doubles(int32_t S, int64_t N, int32_t P) { return (int64_t)S * P * N; }
int64_t st_workspace_doubles(int32_t S, int64_t N, int32_t D, bool grad) {
  const int32_t P = st_splits(S, N, D);
  return st_value_doubles(S, N, P) * (grad ? 1 + 2 * D : 1);
}

// n <= IA_TILE columns starting at column c0 against the lane's rows; the float32 tile sums into the doubles
template <int D, int KIND, int NT, bool GRAD, int R>
__device__ __forceinline__ void st_tile(const float* __restrict__ colx, const float* __restrict__ cols, int c0, int n,
                                        const int (&row)[R], const float (&x)[R][D], const float (&s)[R][D],
                                        const StCoef& k, double (&acc)[R], double (&accx)[R][GRAD ? D : 1],
                                        double (&accs)[R][GRAD ? D : 1]) {
  float ov[R], ox[R][GRAD ? D : 1], os[R][GRAD ? D : 1];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ov[r] = 0.0f;
#pragma unroll
    for (int d = 0; d < (GRAD ? D : 1); ++d) ox[r][d] = os[r][d] = 0.0f;
  }
  const float* px = colx + (int64_t)c0 * D;    // wave-uniform: scalar loads
  const float* ps = cols + (int64_t)c0 * D;
  // columns in flight: at most 12 SGPRs of x_j and s_j beside the 22 of coefficients (three columns at D = 2 spill SGPRs)
  constexpr int U = D == 1 ? 4 : D <= 3 ? 2 : 1;
#pragma unroll U
  for (int j = 0; j < n; ++j) {
    float c[D], h[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      c[d] = px[j * D + d];
      h[d] = ps[j * D + d];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float diff[D], ds[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        diff[d] = x[r][d] - c[d];
        ds[d] = h[d] - s[r][d];
      }
      float q = diff[0] * diff[0], ss = s[r][0] * h[0], dds = diff[0] * ds[0];
#pragma unroll
      for (int d = 1; d < D; ++d) {
        q = fmaf(diff[d], diff[d], q);
        ss = fmaf(s[r][d], h[d], ss);
        dds = fmaf(diff[d], ds[d], dds);
      }
      float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        if constexpr (KIND == CNF_STEIN_IMQ) {
          const float u = q + k.a[b];
          const float inv = __builtin_amdgcn_rcpf(u);
          const float t0 = __builtin_amdgcn_exp2f(k.beta * __builtin_amdgcn_logf(u));
          const float t1 = t0 * inv, t2 = t1 * inv;
          p0 = fmaf(t0, k.k0[b], p0);
          p1 = fmaf(t1, k.k1[b], p1);
          p2 = fmaf(t2, k.k2[b], p2);
          if constexpr (GRAD) p3 = fmaf(t2 * inv, k.k3[b], p3);
        } else {
          const float e = __builtin_amdgcn_exp2f(q * k.a[b]);
          p0 = fmaf(e, k.k0[b], p0);
          p1 = fmaf(e, k.k1[b], p1);
          p2 = fmaf(e, k.k2[b], p2);
          if constexpr (GRAD) p3 = fmaf(e, k.k3[b], p3);
        }
      }
      if (c0 + j == row[r]) p0 = p1 = p2 = p3 = 0.0f;      // the pair i == j, by index
      const float p2q = p2 * q;
      ov[r] += fmaf(p0, ss, fmaf(p1, fmaf(2.0f, dds, -2.0f * D), -4.0f * p2q));
      if constexpr (GRAD) {
        const float m = 2.0f * p1;
        const float A = fmaf(m, ss, fmaf(4.0f * p2, dds, fmaf(-8.0f * p3, q, -(8.0f + 4.0f * D) * p2)));
#pragma unroll
        for (int d = 0; d < D; ++d) {
          os[r][d] = fmaf(p0, h[d], fmaf(-m, diff[d], os[r][d]));
          ox[r][d] = fmaf(A, diff[d], fmaf(m, ds[d], ox[r][d]));
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    acc[r] += (double)ov[r];
    if constexpr (GRAD) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        accx[r][d] += (double)ox[r][d];
        accs[r][d] += (double)os[r][d];
      }
    }
  }
}

// The tile for the spec's term count: a wave-uniform switch per tile, so the pair loop is straight code for its count
template <int D, int KIND, bool GRAD, int R>
__device__ __forceinline__ void st_tile_terms(const float* __restrict__ colx, const float* __restrict__ cols, int c0, int n,
                                              const int (&row)[R], const float (&x)[R][D], const float (&s)[R][D],
                                              const StCoef& k, double (&acc)[R], double (&accx)[R][GRAD ? D : 1],
                                              double (&accs)[R][GRAD ? D : 1]) {
  switch (k.nt) {
    case 1: st_tile<D, KIND, 1, GRAD, R>(colx, cols, c0, n, row, x, s, k, acc, accx, accs); break;
    case 2: st_tile<D, KIND, 2, GRAD, R>(colx, cols, c0, n, row, x, s, k, acc, accx, accs); break;
    case 3: st_tile<D, KIND, 3, GRAD, R>(colx, cols, c0, n, row, x, s, k, acc, accx, accs); break;
    default: st_tile<D, KIND, 4, GRAD, R>(colx, cols, c0, n, row, x, s, k, acc, accx, accs); break;
  }
}

// grid (row groups x P, S): blockIdx.y = the set, blockIdx.x = row group * P + split
template <int D, int KIND, bool GRAD>
__global__ __launch_bounds__(ST_THREADS) void st_kernel(const float* __restrict__ x, const float* __restrict__ score,
                                                        int32_t N, int32_t P, const StCoef k, double* __restrict__ ws) {
  constexpr int R = st_rows(D);
  constexpr int GD = GRAD ? D : 1;
  const int s = (int)blockIdx.y;
  const int rg = (int)(blockIdx.x / (unsigned)P);
  const int p = (int)(blockIdx.x % (unsigned)P);
  const int row0 = rg * (ST_THREADS * R);
  const float* colx = x + (int64_t)s * N * D;
  const float* cols = score + (int64_t)s * N * D;
  const auto [t0, t1] = pair_tile_range<int>(N, P, p);
  float xr[R][D], sr[R][D];
  int row[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = row[r] = row0 + r * ST_THREADS + (int)threadIdx.x;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      xr[r][d] = i < N ? colx[(int64_t)i * D + d] : 0.0f;
      sr[r][d] = i < N ? cols[(int64_t)i * D + d] : 0.0f;
    }
  }
  double acc[R], accx[R][GD], accs[R][GD];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    acc[r] = 0.0;
#pragma unroll
    for (int d = 0; d < GD; ++d) accx[r][d] = accs[r][d] = 0.0;
  }
  for (int t = t0; t < t1; ++t) {
    const int c0 = t * IA_TILE;
    const int n = N - c0 < IA_TILE ? N - c0 : IA_TILE;
    st_tile_terms<D, KIND, GRAD, R>(colx, cols, c0, n, row, xr, sr, k, acc, accx, accs);
  }
  double* part = ws + ((int64_t)s * P + p) * N;
  const int64_t per_grad = (int64_t)gridDim.y * P * N;     // st_value_doubles(S, N, P)
  double* partx = ws + per_grad + ((int64_t)s * P + p) * N * D;
  double* parts = partx + per_grad * D;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = row[r];
    if (i < N) {
      part[i] = acc[r];
      if constexpr (GRAD) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          partx[(int64_t)i * D + d] = accx[r][d];
          parts[(int64_t)i * D + d] = accs[r][d];
        }
      }
    }
  }
}

// Workgroups [0, S): a row's splits added in ascending order -- rows[s, i] = that / (N - 1) -- thread t taking rows
// t, t + 256, ... and the threads' totals meeting in a fixed tree: sums[s, 0]; the diagonal phi(0) |s_i|^2 - 2 D phi'(0)
// the same way: sums[s, 1].  The workgroups after them: both gradients = cg times a component's splits.
__global__ __launch_bounds__(ST_THREADS) void st_finish_kernel(const double* __restrict__ ws, const float* __restrict__ score,
                                                               int32_t S, int64_t N, int32_t D, int32_t P, double phi0,
                                                               double dphi0, double inv_n, double cg,
                                                               double* __restrict__ sums, float* __restrict__ rows,
                                                               float* __restrict__ grad_x, float* __restrict__ grad_s) {
  __shared__ double s_acc[ST_THREADS], s_diag[ST_THREADS];
  const int t = (int)threadIdx.x;
  if ((int)blockIdx.x < S) {
    const int64_t s = blockIdx.x;
    const double* part = ws + s * P * N;
    const float* sc = score + s * N * D;
    double acc = 0.0, diag = 0.0;
    for (int64_t i = t; i < N; i += ST_THREADS) {
      double v = part[i];
      for (int p = 1; p < P; ++p) v += part[p * N + i];
      if (rows) rows[s * N + i] = (float)(v * inv_n);
      acc += v;
      double n2 = 0.0;
      for (int d = 0; d < D; ++d) n2 += (double)sc[i * D + d] * (double)sc[i * D + d];
      diag += phi0 * n2 - 2.0 * D * dphi0;
    }
    s_acc[t] = acc;
    s_diag[t] = diag;
    pair_block_tree<ST_THREADS>(t, s_acc, s_diag);
    if (t == 0) {
      sums[2 * s] = s_acc[0];
      sums[2 * s + 1] = s_diag[0];
    }
    return;
  }
  if (!grad_x) return;
  const int64_t per_set = N * D, total = (int64_t)S * per_set;
  int64_t e = ((int64_t)blockIdx.x - S) * ST_THREADS + t;
  if (e >= 2 * total) return;
  const bool second = e >= total;              // grad_s follows grad_x, in the workspace as in the grid
  if (second) e -= total;
  const int64_t s = e / per_set, r = e % per_set;
  const double* g = ws + (int64_t)S * P * N * (second ? 1 + D : 1) + s * P * per_set + r;
  double a = g[0];
  for (int p = 1; p < P; ++p) a += g[p * per_set];
  (second ? grad_s : grad_x)[e] = (float)(cg * a);
}

struct StLaunch {
  dim3 grid;
  hipStream_t st;
  const float *x, *score;
  int32_t N, P;
  StCoef k;
  double* ws;
  bool grad;
};

template <int D, int KIND> void st_launch_grad(const StLaunch& a) {
  if (a.grad)
    hipLaunchKernelGGL((st_kernel<D, KIND, true>), a.grid, dim3(ST_THREADS), 0, a.st, a.x, a.score, a.N, a.P, a.k, a.ws);
  else
    hipLaunchKernelGGL((st_kernel<D, KIND, false>), a.grid, dim3(ST_THREADS), 0, a.st, a.x, a.score, a.N, a.P, a.k, a.ws);
}
template <int D> void st_launch_kind(int kind, const StLaunch& a) {
  if (kind == CNF_STEIN_IMQ) st_launch_grad<D, CNF_STEIN_IMQ>(a);
  else st_launch_grad<D, CNF_STEIN_GAUSSIAN>(a);             // (st_coef has refused every other kind)
}

inline bool st_shape_ok(int32_t S, int64_t N, int32_t D) { return ia_shape_ok(S, N, 0, D); }

// The spec as st_kernel reads it and phi(0), phi'(0) for the diagonal; false for what cnf_stein refuses in one
bool st_coef(const CnfSteinSpec* spec, StCoef* k, double* phi0, double* dphi0) {
  *k = StCoef{};
  *phi0 = *dphi0 = 0.0;
  if (spec->kind != CNF_STEIN_IMQ && spec->kind != CNF_STEIN_GAUSSIAN) return false;
  if (spec->n_terms < 1 || spec->n_terms > CNF_STEIN_MAX_TERMS) return false;
  const double beta = (double)spec->beta;
  if (spec->kind == CNF_STEIN_IMQ && !(beta > -1.0 && beta < 0.0)) return false;
  k->nt = spec->n_terms;
  k->beta = spec->kind == CNF_STEIN_IMQ ? spec->beta : 0.0f;
  for (int b = 0; b < k->nt; ++b) {
    const double w = (double)spec->w[b], bw = (double)spec->bw[b];
    if (!(w > 0.0) || !std::isfinite(w) || !(bw > 0.0) || !std::isfinite(bw)) return false;
    double c[4];
    if (spec->kind == CNF_STEIN_IMQ) {
      const double c2 = bw * bw;
      // (a coincident pair has u = c^2: 1 / u, and the last power times its coefficient, stay in float32's range)
      if (!fits_float(c2) || !(c2 >= 1.1754943508222875e-38) || !fits_float(1.0 / c2)) return false;
      c[0] = w; c[1] = w * beta; c[2] = c[1] * (beta - 1.0); c[3] = c[2] * (beta - 2.0);
      if (!fits_float(c[3] * std::pow(c2, beta - 3.0)) || !fits_float(w * std::pow(c2, beta))) return false;
      k->a[b] = (float)c2;
      *phi0 += w * std::pow(c2, beta);
      *dphi0 += c[1] * std::pow(c2, beta - 1.0);
    } else {
      const double ib = 1.0 / (2.0 * bw * bw);
      c[0] = w; c[1] = -w * ib; c[2] = w * ib * ib; c[3] = -w * ib * ib * ib;
      if (!fits_float(ib) || !fits_float(c[3])) return false;
      k->a[b] = (float)(-1.4426950408889634 * ib);
      if (!std::isfinite(k->a[b])) return false;
      *phi0 += w;
      *dphi0 += c[1];
    }
    k->k0[b] = (float)c[0]; k->k1[b] = (float)c[1]; k->k2[b] = (float)c[2]; k->k3[b] = (float)c[3];
  }
  return true;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_stein_workspace(int32_t S, int64_t N, int32_t D, int32_t want_grad, int64_t* bytes) {
  if (!bytes || !st_shape_ok(S, N, D)) return CNF_ERR_INVALID;
  *bytes = st_workspace_doubles(S, N, D, want_grad != 0) * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_stein_splits(int32_t S, int64_t N, int32_t D) {
  return st_shape_ok(S, N, D) ? st_splits(S, N, D) : CNF_ERR_INVALID;
}

extern "C" int cnf_stein(const CnfSteinSpec* spec, int32_t S, const float* x, const float* score, int64_t N, int32_t D,
                         double* sums, float* rows, float* grad_x, float* grad_s, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  if (!spec || !x || !score || !sums || !workspace || !st_shape_ok(S, N, D)) return CNF_ERR_INVALID;
  if ((grad_x == nullptr) != (grad_s == nullptr)) return CNF_ERR_INVALID;
  StLaunch a{};
  double phi0, dphi0;
  if (!st_coef(spec, &a.k, &phi0, &dphi0)) return CNF_ERR_INVALID;
  a.grad = grad_x != nullptr;
  if (workspace_bytes < st_workspace_doubles(S, N, D, a.grad) * (int64_t)sizeof(double)) return CNF_ERR_INVALID;
  a.P = st_splits(S, N, D);
  a.grid = dim3((unsigned)(st_row_groups(N, D) * a.P), (unsigned)S);
  a.st = (hipStream_t)stream;
  a.x = x; a.score = score; a.N = (int32_t)N;
  a.ws = (double*)workspace;
  pair_dispatch_dim(D, [&](auto d) { st_launch_kind<decltype(d)::value>(spec->kind, a); });
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  const int64_t grad_wgs = a.grad ? (2 * (int64_t)S * N * D + ST_THREADS - 1) / ST_THREADS : 0;
  hipLaunchKernelGGL(st_finish_kernel, dim3((unsigned)(S + grad_wgs)), dim3(ST_THREADS), 0, a.st, (const double*)workspace,
                     score, S, N, D, a.P, phi0, dphi0, 1.0 / (double)(N - 1), 2.0 / ((double)N * (double)(N - 1)), sums, rows,
                     grad_x, grad_s);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
