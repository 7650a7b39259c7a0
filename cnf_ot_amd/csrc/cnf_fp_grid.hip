// cnf_fp_grid.hip -- a finite-volume reference for the 2-D Fokker-Planck problems: the PDE behind flow_matching_loss_fn
// (applications.py:279-374),
//   d rho / dt = -div(b rho) + sigma lap rho,   b = drift_field<double> (cnf_terms.h: the one definition),
// on the grid of density_on_grid / stats_grid: points x_i = lo_x + i dx, y_j = lo_y + j dy, cell (j, i) centred on its
// point, arrays [ny, nx] row-major, float64 throughout.  No noise floor: what cnf_fp_particles gives to 1 / sqrt(N).
//
// Flux (Scharfetter-Gummel / Chang-Cooper): with B(z) = z / expm1(z) and Pe = b dx / sigma, b the normal drift at the
// face's midpoint, the face between cells i - 1 and i carries F = cL rho_{i-1} - cR rho_i, cL = (sigma / dx^2) B(-Pe),
// cR = (sigma / dx^2) B(Pe); the same with dy for the faces between rows.  The faces of the box carry no flux.
// Step (explicit Euler): rho' = rho + dt ((F_w - F_e) + (G_s - G_n)), exactly that expression with no contraction
// (fpg_step_cell).  With dt R <= 1, R the largest sum of the four coefficients that multiply a cell's own rho, a step is
// a convex combination: rho stays >= 0 and sum rho is kept to rounding.
//
// Coefficients: four face arrays in one block, cxL and cxR [ny, nx + 1] (face f of row j lies between cells f - 1 and
// f), cyL and cyR [ny + 1, nx]; the box's faces (f = 0, nx; g = 0, ny) hold zeros, so every cell runs the same code.
//
// Steps: a workgroup owns an interior tile of FPG_TX x FPG_TY cells, loads it with a halo of K cells into LDS, takes
// K steps there between two LDS buffers and stores the interior.  After step s the cells less than s from the loaded
// region's edge are stale and are no longer computed or read: the halo is recomputed by every tile that needs it, the
// same expression of the same operands, so the result equals the K = 1 result bit for bit.  A launch reads one global
// buffer and writes the other; no kernel reads what another workgroup writes in the same launch.  No atomics, no
// grid-wide barrier.  A cell's eight coefficients stay in the lane's registers over the K steps.
#include "cnf_pairs.h"
#include "cnf_terms.h"

#include <math.h>

#include <cmath>

namespace cnf {
namespace {

constexpr int FPG_THREADS = 256;
constexpr int FPG_TX = 32, FPG_TY = 32;          // the interior tile
constexpr int FPG_MAX_K = 8;
constexpr int FPG_RED = 512;                     // lanes of the one-block reductions
constexpr int FPG_MAX_AXIS = 1 << 14;
constexpr int FPG_MAX_S = 64;

// The scheme's one statement.  c: the cell's west face (cL, cR), east, south, north.
__device__ __forceinline__ double fpg_step_cell(double r, double rw, double re, double rs, double rn,
                                                const double (&c)[8], double dt) {
#pragma clang fp contract(off)
  const double Fw = c[0] * rw - c[1] * r;
  const double Fe = c[2] * r - c[3] * re;
  const double Gs = c[4] * rs - c[5] * r;
  const double Gn = c[6] * r - c[7] * rn;
  return r + dt * ((Fw - Fe) + (Gs - Gn));
}

__device__ __forceinline__ double fpg_bernoulli(double z) {
#pragma clang fp contract(off)
  return fabs(z) < 1e-8 ? 1.0 - 0.5 * z : z / expm1(z);
}

struct FpgGrid {
  double lo_x, lo_y, dx, dy;
  int nx, ny;
};

// One lane per point (j, i) of the padded index space [ny + 1, nx + 1]: the face of row j between cells i - 1 and i,
// and the face of column i between cells j - 1 and j
template <int DRIFT>
__global__ __launch_bounds__(FPG_THREADS) void fpg_coeffs_kernel(const FpgGrid g, float a, double sigma, double* cxL,
                                                                 double* cxR, double* cyL, double* cyR) {
#pragma clang fp contract(off)
  const int64_t total = (int64_t)(g.ny + 1) * (g.nx + 1);
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e / (g.nx + 1)), i = (int)(e % (g.nx + 1));
  if (j < g.ny) {
    double l = 0.0, r = 0.0;
    if (i >= 1 && i < g.nx) {
      const double x = g.lo_x + ((double)i - 0.5) * g.dx, y = g.lo_y + (double)j * g.dy;
      const double b = drift_field<double>([&](int d) { return d == 0 ? x : y; }, 0, DRIFT, a);
      const double pe = b * g.dx / sigma, k = sigma / (g.dx * g.dx);
      l = k * fpg_bernoulli(-pe);
      r = k * fpg_bernoulli(pe);
    }
    cxL[(int64_t)j * (g.nx + 1) + i] = l;
    cxR[(int64_t)j * (g.nx + 1) + i] = r;
  }
  if (i < g.nx) {
    double l = 0.0, r = 0.0;
    if (j >= 1 && j < g.ny) {
      const double x = g.lo_x + (double)i * g.dx, y = g.lo_y + ((double)j - 0.5) * g.dy;
      const double b = drift_field<double>([&](int d) { return d == 0 ? x : y; }, 1, DRIFT, a);
      const double pe = b * g.dy / sigma, k = sigma / (g.dy * g.dy);
      l = k * fpg_bernoulli(-pe);
      r = k * fpg_bernoulli(pe);
    }
    cyL[(int64_t)j * g.nx + i] = l;
    cyR[(int64_t)j * g.nx + i] = r;
  }
}

// One block: the largest outflow rate, the four coefficients of a cell's own rho (east cL, west cR, north cL, south cR)
__global__ __launch_bounds__(FPG_RED) void fpg_rate_kernel(int nx, int ny, const double* cxL, const double* cxR,
                                                           const double* cyL, const double* cyR, double* rate) {
  __shared__ double s_m[FPG_RED];
  const int t = (int)threadIdx.x;
  const int64_t total = (int64_t)nx * ny;
  double m = 0.0;
  for (int64_t e = t; e < total; e += FPG_RED) {
    const int64_t j = e / nx, i = e % nx;
    const double out = ((cxL[j * (nx + 1) + i + 1] + cxR[j * (nx + 1) + i]) + cyL[(j + 1) * nx + i]) + cyR[j * nx + i];
    m = fmax(m, out);
  }
  s_m[t] = m;
  __syncthreads();
  for (int o = FPG_RED / 2; o > 0; o >>= 1) {
    if (t < o) s_m[t] = fmax(s_m[t], s_m[t + o]);
    __syncthreads();
  }
  if (t == 0) *rate = s_m[0];
}

struct FpgStep {
  const double *cxL, *cxR, *cyL, *cyR;
  const double* src;
  double* dst;
  double dt;
  int nx, ny;
};

template <int K>
__global__ __launch_bounds__(FPG_THREADS) void fpg_steps_kernel(const FpgStep p) {
  constexpr int EX = FPG_TX + 2 * K, EY = FPG_TY + 2 * K, CELLS = EX * EY;
  constexpr int CPT = (CELLS + FPG_THREADS - 1) / FPG_THREADS;      // cells per lane
  __shared__ double s_rho[2][CELLS];
  const int i0 = (int)blockIdx.x * FPG_TX - K, j0 = (int)blockIdx.y * FPG_TY - K;
  const int nx = p.nx, ny = p.ny;
  double c[CPT][8];
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int e = (int)threadIdx.x + q * FPG_THREADS;
    const int ej = e / EX, ei = e - ej * EX;
    const int i = i0 + ei, j = j0 + ej;
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) c[q][k] = 0.0;
    if (e < CELLS && i >= 0 && i < nx && j >= 0 && j < ny) {          // outside the box: rho = 0 and no flux, for good
      r = p.src[(int64_t)j * nx + i];
      const int64_t fx = (int64_t)j * (nx + 1) + i, fy = (int64_t)j * nx + i;
      c[q][0] = p.cxL[fx];
      c[q][1] = p.cxR[fx];
      c[q][2] = p.cxL[fx + 1];
      c[q][3] = p.cxR[fx + 1];
      c[q][4] = p.cyL[fy];
      c[q][5] = p.cyR[fy];
      c[q][6] = p.cyL[fy + nx];
      c[q][7] = p.cyR[fy + nx];
    }
    if (e < CELLS) s_rho[0][e] = r;
  }
  __syncthreads();
#pragma unroll
  for (int s = 1; s <= K; ++s) {
    const double* from = s_rho[(s - 1) & 1];
    double* to = s_rho[s & 1];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int e = (int)threadIdx.x + q * FPG_THREADS;
      const int ej = e / EX, ei = e - ej * EX;
      const int d = min(min(ei, EX - 1 - ei), min(ej, EY - 1 - ej));    // cells from the loaded region's edge
      if (e < CELLS && d >= s)
        to[e] = fpg_step_cell(from[e], from[e - 1], from[e + 1], from[e - EX], from[e + EX], c[q], p.dt);
    }
    __syncthreads();
  }
  const double* res = s_rho[K & 1];
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int e = (int)threadIdx.x + q * FPG_THREADS;
    const int ej = e / EX, ei = e - ej * EX;
    const int i = i0 + ei, j = j0 + ej;
    if (e < CELLS && ei >= K && ei < K + FPG_TX && ej >= K && ej < K + FPG_TY && i < nx && j < ny)
      p.dst[(int64_t)j * nx + i] = res[e];
  }
}

// One block per snapshot: mass, min, sum rho x, y, xx, xy, yy.  Lane t adds cells t, t + FPG_RED, ... in order, then
// the block's tree: a fixed order, two calls are bit-identical.
__global__ __launch_bounds__(FPG_RED) void fpg_stats_kernel(const FpgGrid g, const double* rho, double* stats) {
#pragma clang fp contract(off)
  __shared__ double s_a[6][FPG_RED];
  __shared__ double s_min[FPG_RED];
  const int t = (int)threadIdx.x;
  const int64_t total = (int64_t)g.nx * g.ny;
  const double* r = rho + (int64_t)blockIdx.x * total;
  double m = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0, lo = INFINITY;
  for (int64_t e = t; e < total; e += FPG_RED) {
    const double x = g.lo_x + (double)(e % g.nx) * g.dx, y = g.lo_y + (double)(e / g.nx) * g.dy, v = r[e];
    m += v;
    sx += v * x;
    sy += v * y;
    sxx += v * x * x;
    sxy += v * x * y;
    syy += v * y * y;
    lo = fmin(lo, v);
  }
  s_a[0][t] = m; s_a[1][t] = sx; s_a[2][t] = sy; s_a[3][t] = sxx; s_a[4][t] = sxy; s_a[5][t] = syy;
  s_min[t] = lo;
  pair_block_tree<FPG_RED>(t, s_a[0], s_a[1], s_a[2], s_a[3], s_a[4], s_a[5]);
  for (int o = FPG_RED / 2; o > 0; o >>= 1) {
    if (t < o) s_min[t] = fmin(s_min[t], s_min[t + o]);
    __syncthreads();
  }
  if (t == 0) {
    double* out = stats + (int64_t)blockIdx.x * 7;
    const double area = g.dx * g.dy;
    out[0] = s_a[0][0] * area;
    out[1] = s_min[0];
    for (int k = 1; k < 6; ++k) out[k + 1] = s_a[k][0] * area;
  }
}

bool fpg_shape_ok(int32_t nx, int32_t ny) { return nx >= 1 && ny >= 1 && nx <= FPG_MAX_AXIS && ny <= FPG_MAX_AXIS; }
int64_t fpg_coef_doubles(int64_t nx, int64_t ny) { return 2 * ny * (nx + 1) + 2 * (ny + 1) * nx; }

bool fpg_grid_of(const CnfFieldGrid* grid, FpgGrid* g) {
  if (!grid || !fpg_shape_ok(grid->nx, grid->ny)) return false;
  if (!(grid->step_x > 0.0) || !(grid->step_y > 0.0) || !std::isfinite(grid->step_x) || !std::isfinite(grid->step_y) ||
      !std::isfinite(grid->lo_x) || !std::isfinite(grid->lo_y))
    return false;
  *g = FpgGrid{grid->lo_x, grid->lo_y, grid->step_x, grid->step_y, grid->nx, grid->ny};
  return true;
}

struct FpgCoef {
  double *cxL, *cxR, *cyL, *cyR;
};
FpgCoef fpg_coef_of(const double* coef, int64_t nx, int64_t ny) {
  double* c = const_cast<double*>(coef);
  return FpgCoef{c, c + ny * (nx + 1), c + 2 * ny * (nx + 1), c + 2 * ny * (nx + 1) + (ny + 1) * nx};
}

template <int K> void fpg_launch(const FpgStep& p, hipStream_t st) {
  const dim3 grid((unsigned)((p.nx + FPG_TX - 1) / FPG_TX), (unsigned)((p.ny + FPG_TY - 1) / FPG_TY));
  hipLaunchKernelGGL((fpg_steps_kernel<K>), grid, dim3(FPG_THREADS), 0, st, p);
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_fp_grid_coeffs_bytes(int32_t nx, int32_t ny, int64_t* bytes) {
  if (!bytes || !fpg_shape_ok(nx, ny)) return CNF_ERR_INVALID;
  *bytes = fpg_coef_doubles(nx, ny) * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_fp_grid_coeffs(int32_t drift, int32_t D, float a, double sigma, const CnfFieldGrid* grid,
                                  double* coef, int64_t coef_bytes, double* rate, void* stream) {
  FpgGrid g;
  if (D != 2 || (drift != CNF_DRIFT_OU && drift != CNF_DRIFT_SMILE && drift != CNF_DRIFT_NONGRADIENT)) return CNF_ERR_INVALID;
  if (!fpg_grid_of(grid, &g) || !(sigma > 0.0) || !std::isfinite(sigma) || !std::isfinite(a)) return CNF_ERR_INVALID;
  if (!coef || !rate || coef_bytes < fpg_coef_doubles(g.nx, g.ny) * (int64_t)sizeof(double)) return CNF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const FpgCoef c = fpg_coef_of(coef, g.nx, g.ny);
  const int64_t total = (int64_t)(g.ny + 1) * (g.nx + 1);
  const dim3 blocks((unsigned)((total + FPG_THREADS - 1) / FPG_THREADS)), threads(FPG_THREADS);
  if (drift == CNF_DRIFT_OU)
    hipLaunchKernelGGL((fpg_coeffs_kernel<CNF_DRIFT_OU>), blocks, threads, 0, st, g, a, sigma, c.cxL, c.cxR, c.cyL, c.cyR);
  else if (drift == CNF_DRIFT_SMILE)
    hipLaunchKernelGGL((fpg_coeffs_kernel<CNF_DRIFT_SMILE>), blocks, threads, 0, st, g, a, sigma, c.cxL, c.cxR, c.cyL, c.cyR);
  else
    hipLaunchKernelGGL((fpg_coeffs_kernel<CNF_DRIFT_NONGRADIENT>), blocks, threads, 0, st, g, a, sigma, c.cxL, c.cxR, c.cyL,
                       c.cyR);
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  hipLaunchKernelGGL(fpg_rate_kernel, dim3(1), dim3(FPG_RED), 0, st, g.nx, g.ny, c.cxL, c.cxR, c.cyL, c.cyR, rate);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_fp_grid_steps_workspace(int32_t nx, int32_t ny, int64_t* bytes) {
  if (!bytes || !fpg_shape_ok(nx, ny)) return CNF_ERR_INVALID;
  *bytes = (int64_t)nx * ny * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_fp_grid_steps(const double* coef, int32_t nx, int32_t ny, double dt, int64_t n_steps,
                                 int32_t steps_per_launch, double* rho, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  const int K = steps_per_launch;
  if (!fpg_shape_ok(nx, ny) || !coef || !rho || !(dt > 0.0) || !std::isfinite(dt) || n_steps < 0) return CNF_ERR_INVALID;
  if (K != 1 && K != 2 && K != 4 && K != FPG_MAX_K) return CNF_ERR_INVALID;
  if (!workspace || workspace_bytes < (int64_t)nx * ny * (int64_t)sizeof(double)) return CNF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const FpgCoef c = fpg_coef_of(coef, nx, ny);
  double* buf[2] = {rho, (double*)workspace};
  int cur = 0;
  auto launch = [&](int k) {
    const FpgStep p{c.cxL, c.cxR, c.cyL, c.cyR, buf[cur], buf[cur ^ 1], dt, nx, ny};
    if (k == 8) fpg_launch<8>(p, st);
    else if (k == 4) fpg_launch<4>(p, st);
    else if (k == 2) fpg_launch<2>(p, st);
    else fpg_launch<1>(p, st);
    cur ^= 1;
    return hipGetLastError() == hipSuccess;
  };
  for (int64_t l = 0; l < n_steps / K; ++l)
    if (!launch(K)) return CNF_ERR_HIP;
  const int tail = (int)(n_steps % K);                   // the tail: the largest smaller variants that fit
  for (int k = FPG_MAX_K / 2; k >= 1; k >>= 1)
    if ((tail & k) && !launch(k)) return CNF_ERR_HIP;
  if (cur == 1 && hipMemcpyAsync(rho, workspace, (size_t)nx * ny * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return CNF_ERR_HIP;
  return CNF_OK;
}

extern "C" int cnf_fp_grid_stats(const CnfFieldGrid* grid, const double* rho, int32_t S, double* stats, void* stream) {
  FpgGrid g;
  if (!fpg_grid_of(grid, &g) || !rho || !stats || S < 1 || S > FPG_MAX_S) return CNF_ERR_INVALID;
  hipLaunchKernelGGL(fpg_stats_kernel, dim3((unsigned)S), dim3(FPG_RED), 0, (hipStream_t)stream, g, rho, stats);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
