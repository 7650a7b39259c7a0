// cnf_hopf_cole.hip -- the exact solution of the 2-D regularized Wasserstein proximal problem (rwpo) by the
// Hopf-Cole kernel formula: the discrete sums of the reference's offline generator
// (cnf_ot/mfc/2d_WPO_ref_solution.py:60-187) and the optimal value that solvers.py:170-232 estimates by Monte Carlo.
// With eps = 1 / beta, g the potential of potential_loss_fn (cnf_terms.h) and kappa = 1 / (4 eps T):
//   log h(y)      = log sum_{z: |z_i - y_i| <= window} exp(-g(z) / (2 eps) - kappa |y - z|^2) dz^2
//   log rho_T(x)  = -g(x) / (2 eps) + log sum_y exp(log rho0(y) - log h(y) - kappa |x - y|^2) dy^2
//   true value    = -2 eps sum_y rho0(y) (log h(y) - log(4 pi eps T)) dy^2
// The Gaussian factors over the two coordinates and so does the square window, so each sum is two 1-D passes (over
// coordinate 1 for every row of coordinate 2, then over coordinate 2), each a streaming log-sum-exp over the source
// index that also carries weighted means (the score's and w0's first moments).  This is the generator's discrete sum
// in another order, not an approximation of it.  Float64 throughout: the log-weights reach 1e2-1e4 at the grid edges.
// Every output is written by one lane in a fixed order: no atomics, repeated calls are bit-identical.
//
// cnf_hopf_cole_path_2d is the same solution at every time 0 <= t <= T: rho_t = eta_t etahat_t with
//   log eta_t(x)    = LSE_z(-g(z) / (2 eps) - |x - z|^2 / (4 eps (T - t))) + 2 log dz - log(4 pi eps (T - t))   (z grid)
//   log etahat_t(x) = LSE_y(log rho0(y) - log h(y) - |x - y|^2 / (4 eps t)) + 2 log dz + log(T / t)             (y grid)
// and the drift, score and current velocity from the two sums' first moments.  h, the potential table and the value are
// built once; per chunk of HC_TIMES interior times, hc_path_pass_kernel sums every time of the chunk from one staged
// source tile (the table is the same for all of them, only kappa changes).  t = 0 and t = T go through the T kernels.
#include "cnf_terms.h"

#include <math.h>

#include <algorithm>
#include <cmath>

namespace cnf {
namespace {

constexpr int HC_BLOCK = 128;    // lanes over the destination index
constexpr int HC_TILE = 2048;    // source log-weights staged in LDS per tile (16 KB)
constexpr int HC_RED = 1024;     // threads of the reduction block
constexpr int64_t HC_MAX_N = int64_t(1) << 19;   // n_y, n_w and the output extents are capped: workspace sizes fit

// One 1-D pass.  Row r, source k: log-weight lw[r * lw_rs + k * lw_ks] at coordinate (k - s_c) dz.
// Destination j: in window mode at (j - d_c) dz, summing the sources |k - s_c - (j - d_c)| <= n_w; in free mode at
// xd[j], summing every source.  Outputs (at r * o_rs + j * o_js): L = log sum_k exp(lw_k - kappa u_k^2), and the
// weighted means M of the source coordinate and C of `carry` (same layout as lw).
struct HcPass {
  const double* lw;
  const double* carry;
  int64_t lw_rs, lw_ks;
  int S, s_c;
  int n_dst, d_c, n_w;
  const double* xd;
  double dz, kappa;
  double *L, *M, *C;
  int64_t o_rs, o_js;
};

template <bool FREE, bool MEAN, bool CARRY>
__global__ __launch_bounds__(HC_BLOCK) void hc_pass_kernel(const HcPass p) {
  __shared__ double s_lw[HC_TILE];
  __shared__ double s_cy[CARRY ? HC_TILE : 1];
  const int r = blockIdx.x;
  const int j0 = blockIdx.y * HC_BLOCK, j = j0 + (int)threadIdx.x;
  const bool live = j < p.n_dst;
  // the sources this block stages [lo, hi) and the ones this lane sums [klo, khi)
  int lo = 0, hi = p.S, klo = 0, khi = live ? p.S : 0;
  const int sh = p.s_c - p.d_c;                       // window mode: source k = j + sh + o, |o| <= n_w
  if (!FREE) {
    const int jl = min(j0 + HC_BLOCK, p.n_dst) - 1;
    lo = max(0, j0 + sh - p.n_w);
    hi = min(p.S, jl + sh + p.n_w + 1);
    klo = max(0, j + sh - p.n_w);
    khi = live ? min(p.S, j + sh + p.n_w + 1) : klo;
  }
  const double x = (FREE && live) ? p.xd[j] : 0.0;
  const int cj = j + sh;                               // window mode: u = (k - cj) dz, an exact index difference
  const double nk = -p.kappa;
  auto logk = [&](int k) {
    const double u = FREE ? x - (double)(k - p.s_c) * p.dz : (double)(k - cj) * p.dz;
    return nk * u * u;
  };
  const double* row = p.lw + (int64_t)r * p.lw_rs;
  const double* crow = CARRY ? p.carry + (int64_t)r * p.lw_rs : nullptr;
  double m = -INFINITY, s = 0.0, sx = 0.0, sc = 0.0;
  for (int t0 = lo; t0 < hi; t0 += HC_TILE) {
    const int t1 = min(hi, t0 + HC_TILE);
    __syncthreads();
    for (int k = t0 + (int)threadIdx.x; k < t1; k += HC_BLOCK) {
      s_lw[k - t0] = row[(int64_t)k * p.lw_ks];
      if (CARRY) s_cy[k - t0] = crow[(int64_t)k * p.lw_ks];
    }
    __syncthreads();
    const int a = max(klo, t0), b = min(khi, t1);
    double mt = -INFINITY;                             // the tile's maximum: no exponentials
    for (int k = a; k < b; ++k) mt = fmax(mt, s_lw[k - t0] + logk(k));
    if (mt > m) {                                      // (m = -inf: the sums are still 0)
      const double f = exp(m - mt);
      s *= f; sx *= f; sc *= f;
      m = mt;
    }
    for (int k = a; k < b; ++k) {                      // one exponential per term
      const double e = exp(s_lw[k - t0] + logk(k) - m);
      s += e;
      if (MEAN) sx = fma(e, (double)(k - p.s_c) * p.dz, sx);
      if (CARRY) sc = fma(e, s_cy[k - t0], sc);
    }
  }
  if (!live) return;
  const int64_t o = (int64_t)r * p.o_rs + (int64_t)j * p.o_js;
  p.L[o] = m + log(s);
  if (MEAN) p.M[o] = sx / s;
  if (CARRY) p.C[o] = sc / s;
}

// lg[k2 * n + k1] = -g(z) / (2 eps) at z = ((k1 - c) dz, (k2 - c) dz)
__global__ __launch_bounds__(256) void hc_potential_kernel(double* lg, int n, int c, double dz, double half_beta,
                                                            int subtype, float a) {
  const int64_t total = (int64_t)n * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const double z1 = (double)((int)(i % n) - c) * dz, z2 = (double)((int)(i / n) - c) * dz;
    const Potential<double> g = potential<false, double>([&](int d) { return d == 0 ? z1 : z2; }, 2, subtype, a);
    lg[i] = -g.v * half_beta;
  }
}

// One block, fixed order: the true value and the IC mass from log h on the y grid; H becomes the second stage's
// log-weight log rho0(y) - log h(y) in place.
__global__ __launch_bounds__(HC_RED) void hc_value_kernel(double* H, int n, int c, double dz, double var0, double eps,
                                                          double T, double* true_value, double* ic_mass) {
  __shared__ double s_v[HC_RED], s_m[HC_RED];
  const int64_t total = (int64_t)n * n;
  const double l2dz = 2.0 * log(dz), lnorm0 = log(2.0 * M_PI * var0), lk = log(4.0 * M_PI * eps * T);
  double v = 0.0, mass = 0.0;
  for (int64_t i = threadIdx.x; i < total; i += HC_RED) {
    const double y1 = (double)((int)(i % n) - c) * dz, y2 = (double)((int)(i / n) - c) * dz;
    const double lr0 = -(y1 * y1 + y2 * y2) / (2.0 * var0) - lnorm0;
    const double lh = H[i] + l2dz;
    const double r0 = exp(lr0);
    v = fma(r0, lh - lk, v);
    mass += r0;
    H[i] = lr0 - lh;
  }
  s_v[threadIdx.x] = v;
  s_m[threadIdx.x] = mass;
  for (int w = HC_RED / 2; w > 0; w >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < w) {
      s_v[threadIdx.x] += s_v[threadIdx.x + w];
      s_m[threadIdx.x] += s_m[threadIdx.x + w];
    }
  }
  if (threadIdx.x == 0) {
    if (true_value) *true_value = -2.0 * eps * s_v[0] * dz * dz;
    if (ic_mass) *ic_mass = s_m[0] * dz * dz;
  }
}

// Per output point (x1 fastest): log rho_T, and the generator's fields from the first moments (:177-187):
//   score = -grad g / (2 eps) - (x - m) / (2 eps T),  w0 = -(x - m0) / T + eps x,  wT = -grad g - eps score
__global__ __launch_bounds__(256) void hc_finish_kernel(const double* x1, const double* x2, int n1, int n2,
                                                        const double* L, const double* m1, const double* m2,
                                                        const double* m01, const double* m02, double l2dz, double eps,
                                                        double T, int subtype, float a, double* log_rho, double* score,
                                                        double* w0, double* wT) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)n1 * n2) return;
  const double x[2] = {x1[i % n1], x2[i / n1]};
  const Potential<double> g = potential<false, double>([&](int d) { return x[d]; }, 2, subtype, a);
  log_rho[i] = L[i] + l2dz - g.v / (2.0 * eps);
  if (!score && !wT && !w0) return;
  const double m[2] = {m1 ? m1[i] : 0.0, m2 ? m2[i] : 0.0};
  for (int e = 0; e < 2; ++e) {
    const double ge = g.grad(x[e]);
    const double se = -ge / (2.0 * eps) - (x[e] - m[e]) / (2.0 * eps * T);
    if (score) score[2 * i + e] = se;
    if (wT) wT[2 * i + e] = -ge - eps * se;
    if (w0) w0[2 * i + e] = -(x[e] - (e == 0 ? m01[i] : m02[i])) / T + eps * x[e];
  }
}

constexpr int HC_TIMES = 8;      // interior times per launch of the path passes: 8 x (max, sum, two means) in registers

// A free-mode pass for up to HC_TIMES times at once.  Time q has kernel width kappa[q], reads the log-weights at
// lw + q * lw_ts (lw_ts = 0: one table for every time) and writes at q * o_ts; otherwise HcPass's layout.
struct HcPathPass {
  const double* lw;
  const double* carry;
  int64_t lw_ts, lw_rs, lw_ks;
  int S, s_c, n_dst, nt;
  const double* xd;
  double dz;
  double kappa[HC_TIMES];
  double *L, *M, *C;
  int64_t o_ts, o_rs, o_js;
};

// NT = HC_TIMES: the first pass.  The source row does not depend on the time, so a tile staged in LDS once serves all
// nt times: per term one LDS read and one squared distance, then one exponential per time.  NT = 1: the second pass,
// whose source is the first pass's per-time output; the time is blockIdx.z.  Per time the terms are summed in source
// order tile by tile (a max sweep, then the exponentials), whatever the other times of the launch are.
template <int NT, bool CARRY>
__global__ __launch_bounds__(HC_BLOCK) void hc_path_pass_kernel(const HcPathPass p) {
  __shared__ double s_lw[HC_TILE];
  __shared__ double s_cy[CARRY ? HC_TILE : 1];
  const int r = blockIdx.x, tz = blockIdx.z;
  const int j = blockIdx.y * HC_BLOCK + (int)threadIdx.x;
  const bool live = j < p.n_dst;
  const int khi = live ? p.S : 0;
  const double x = live ? p.xd[j] : 0.0;
  double nk[NT], m[NT], s[NT], sx[NT], sc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    nk[q] = -p.kappa[q];
    m[q] = -INFINITY;
    s[q] = sx[q] = sc[q] = 0.0;
  }
  if (NT == 1) {                                       // kappa[tz] without a dynamic index into the arguments
#pragma unroll
    for (int q = 1; q < HC_TIMES; ++q)
      if (tz == q) nk[0] = -p.kappa[q];
  }
  const int nt = NT == 1 ? 1 : p.nt;
  const double* row = p.lw + (int64_t)tz * p.lw_ts + (int64_t)r * p.lw_rs;
  const double* crow = CARRY ? p.carry + (int64_t)tz * p.lw_ts + (int64_t)r * p.lw_rs : nullptr;
  for (int t0 = 0; t0 < p.S; t0 += HC_TILE) {
    const int t1 = min(p.S, t0 + HC_TILE);
    __syncthreads();
    for (int k = t0 + (int)threadIdx.x; k < t1; k += HC_BLOCK) {
      s_lw[k - t0] = row[(int64_t)k * p.lw_ks];
      if (CARRY) s_cy[k - t0] = crow[(int64_t)k * p.lw_ks];
    }
    __syncthreads();
    const int b = min(khi, t1);
    double mt[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) mt[q] = -INFINITY;
    for (int k = t0; k < b; ++k) {                     // the tile's maxima: no exponentials
      const double u = x - (double)(k - p.s_c) * p.dz, u2 = u * u, w = s_lw[k - t0];
#pragma unroll
      for (int q = 0; q < NT; ++q)
        if (q < nt) mt[q] = fmax(mt[q], fma(nk[q], u2, w));
    }
#pragma unroll
    for (int q = 0; q < NT; ++q)
      if (q < nt && mt[q] > m[q]) {                    // (m = -inf: the sums are still 0)
        const double f = exp(m[q] - mt[q]);
        s[q] *= f; sx[q] *= f; sc[q] *= f;
        m[q] = mt[q];
      }
    for (int k = t0; k < b; ++k) {                     // one exponential per term and time
      const double z = (double)(k - p.s_c) * p.dz, u = x - z, u2 = u * u, w = s_lw[k - t0];
      const double cy = CARRY ? s_cy[k - t0] : 0.0;
#pragma unroll
      for (int q = 0; q < NT; ++q)
        if (q < nt) {
          const double e = exp(fma(nk[q], u2, w) - m[q]);
          s[q] += e;
          sx[q] = fma(e, z, sx[q]);
          if (CARRY) sc[q] = fma(e, cy, sc[q]);
        }
    }
  }
  if (!live) return;
#pragma unroll
  for (int q = 0; q < NT; ++q)
    if (q < nt) {
      const int64_t o = (int64_t)(NT == 1 ? tz : q) * p.o_ts + (int64_t)r * p.o_rs + (int64_t)j * p.o_js;
      p.L[o] = m[q] + log(s[q]);
      p.M[o] = sx[q] / s[q];
      if (CARRY) p.C[o] = sc[q] / s[q];
    }
}

// The times one hc_path_finish_kernel launch writes: output slab, time t, and how (HcTime)
enum HcTime { HC_T_INNER = 0, HC_T_ZERO = 1, HC_T_END = 2 };
struct HcPathSlots {
  int n;
  int mode[HC_TIMES];
  int64_t slab[HC_TIMES];
  double t[HC_TIMES];
};

// Per output point and time slot q (W: [6][HC_TIMES][n2 n1] = the log-sum and the means of coordinates 1 and 2 of the
// eta sum, then of the etahat sum):
//   0 < t < T   log rho = log eta + log etahat,  drift = -(x - mb) / (T - t),
//               score = -(x - mb) / (2 eps (T - t)) - (x - mf) / (2 eps t),  vel = drift - eps score
//   t = 0       rho0 itself: log rho0(x), score = -x / var0, drift = -(x - m0) / T (m0: the w0 pass's),
//               vel = drift + eps x / var0
//   t = T       drift = -grad g alone; hc_finish_kernel writes the rest into the slab
__global__ __launch_bounds__(256) void hc_path_finish_kernel(const HcPathSlots sl, const double* x1, const double* x2,
                                                             int n1, int n2, const double* W, const double* m01,
                                                             const double* m02, double l2dz, double eps, double T,
                                                             double var0, int subtype, float a, double* log_rho,
                                                             double* score, double* drift, double* vel) {
  const int64_t nn = (int64_t)n1 * n2;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nn) return;
  const double x[2] = {x1[i % n1], x2[i / n1]};
  const bool fields = score || drift || vel;
#pragma unroll
  for (int q = 0; q < HC_TIMES; ++q) {
    if (q >= sl.n) break;
    const int64_t o = sl.slab[q] * nn + i;
    const double t = sl.t[q];
    if (sl.mode[q] == HC_T_END) {
      if (drift) {
        const Potential<double> g = potential<false, double>([&](int d) { return x[d]; }, 2, subtype, a);
        for (int e = 0; e < 2; ++e) drift[2 * o + e] = -g.grad(x[e]);
      }
    } else if (sl.mode[q] == HC_T_ZERO) {
      log_rho[o] = -(x[0] * x[0] + x[1] * x[1]) / (2.0 * var0) - log(2.0 * M_PI * var0);
      if (!fields) continue;
      for (int e = 0; e < 2; ++e) {
        const double de = (drift || vel) ? -(x[e] - (e == 0 ? m01[i] : m02[i])) / T : 0.0, se = -x[e] / var0;
        if (score) score[2 * o + e] = se;
        if (drift) drift[2 * o + e] = de;
        if (vel) vel[2 * o + e] = de - eps * se;
      }
    } else {
      const double* w = W + (int64_t)q * nn + i;
      const int64_t ws = (int64_t)HC_TIMES * nn;
      const double tb = T - t;
      log_rho[o] = (w[0] + l2dz - log(4.0 * M_PI * eps * tb)) + (w[3 * ws] + l2dz + log(T / t));
      if (!fields) continue;
      for (int e = 0; e < 2; ++e) {
        const double xb = x[e] - w[(1 + e) * ws], xf = x[e] - w[(4 + e) * ws];
        const double de = -xb / tb, se = -xb / (2.0 * eps * tb) - xf / (2.0 * eps * t);
        if (score) score[2 * o + e] = se;
        if (drift) drift[2 * o + e] = de;
        if (vel) vel[2 * o + e] = de - eps * se;
      }
    }
  }
}

// Grid extents: n_y = round(y_range / dz), n_w = round(window / dz); 0 on invalid input
struct HcGrid {
  int64_t ny, nw, Ny, Nz, n1, n2;
  bool ok;
};

HcGrid hc_grid(double dz, double window, double y_range, int64_t n1, int64_t n2) {
  HcGrid g{};
  if (!(dz > 0.0) || !std::isfinite(dz) || !(window > 0.0) || !(y_range > 0.0) || !std::isfinite(window) || !std::isfinite(y_range)) return g;
  const double ry = y_range / dz, rw = window / dz;
  if (!(ry <= (double)HC_MAX_N) || !(rw <= (double)HC_MAX_N)) return g;
  if (n1 < 0 || n2 < 0 || n1 > HC_MAX_N || n2 > HC_MAX_N || ((n1 == 0) != (n2 == 0))) return g;
  g.ny = llround(ry);
  g.nw = llround(rw);
  g.Ny = 2 * g.ny + 1;
  g.Nz = g.Ny + 2 * g.nw;
  g.n1 = n1;
  g.n2 = n2;
  g.ok = true;
  return g;
}

int64_t hc_workspace_doubles(const HcGrid& g) {
  return g.Nz * g.Nz + g.Ny * g.Nz + g.Ny * g.Ny + 4 * g.n1 * g.Ny + 6 * g.n1 * g.n2;
}

template <bool FREE, bool MEAN, bool CARRY>
int hc_launch(const HcPass& p, int rows, hipStream_t stream) {
  const dim3 grid((unsigned)rows, (unsigned)((p.n_dst + HC_BLOCK - 1) / HC_BLOCK));
  hipLaunchKernelGGL((hc_pass_kernel<FREE, MEAN, CARRY>), grid, dim3(HC_BLOCK), 0, stream, p);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// The two free-mode passes from the y grid to the output grid: log-weights lw (row y2, column y1, row stride rs);
// L [x2, x1] and the means of y1 (C) and y2 (M) there.  Cbuf: 2 n1 Ny doubles.
int hc_to_outputs(const double* lw, int64_t rs, const HcGrid& g, const double* x1, const double* x2, double dz,
                  double kappa, bool means, double* Cbuf, double* L, double* M1, double* M2, hipStream_t stream) {
  const int Ny = (int)g.Ny, n1 = (int)g.n1, n2 = (int)g.n2, c = (int)g.ny;
  double *LC = Cbuf, *MC = Cbuf + g.n1 * g.Ny;     // [x1, y2]
  HcPass a{lw, nullptr, rs, 1, Ny, c, n1, 0, 0, x1, dz, kappa, LC, MC, nullptr, 1, Ny};
  int rc = means ? hc_launch<true, true, false>(a, Ny, stream) : hc_launch<true, false, false>(a, Ny, stream);
  if (rc != CNF_OK) return rc;
  HcPass b{LC, MC, Ny, 1, Ny, c, n2, 0, 0, x2, dz, kappa, L, M2, M1, 1, n1};
  return means ? hc_launch<true, true, true>(b, n1, stream) : hc_launch<true, false, false>(b, n1, stream);
}

// The workspace of cnf_hopf_cole_2d (hc_workspace_doubles)
struct HcBuffers {
  double* lg;      // [z2, z1]  -g(z) / (2 eps)
  double* LA;      // [y1, z2]  first pass of log h
  double* H;       // [y2, y1]  log h - 2 log dz, then log rho0 - log h
  double* Cbuf;    // [x1, y2] x 4
  double* D;       // [x2, x1] x 6
};

HcBuffers hc_buffers(const HcGrid& g, void* workspace) {
  HcBuffers w;
  w.lg = (double*)workspace;
  w.LA = w.lg + g.Nz * g.Nz;
  w.H = w.LA + g.Ny * g.Nz;
  w.Cbuf = w.H + g.Ny * g.Ny;
  w.D = w.Cbuf + 4 * g.n1 * g.Ny;
  return w;
}

// What does not depend on the outputs: the potential table, log h by two window passes, the value and the IC mass
int hc_h_and_value(const HcGrid& g, const HcBuffers& w, int32_t subtype, float a, double T, double beta, double var0,
                   double dz, double* true_value, double* ic_mass, hipStream_t st) {
  const double eps = 1.0 / beta, kappa = beta / (4.0 * T);
  const int ny = (int)g.ny, nw = (int)g.nw, Ny = (int)g.Ny, Nz = (int)g.Nz;
  const int64_t nzz = g.Nz * g.Nz;
  const unsigned fill_blocks = (unsigned)std::min<int64_t>((nzz + 255) / 256, 4096);
  hipLaunchKernelGGL(hc_potential_kernel, dim3(fill_blocks), dim3(256), 0, st, w.lg, Nz, ny + nw, dz, 0.5 * beta,
                     (int)subtype, a);
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  // log h: over z1 for every z2 (the window |z1 - y1| <= n_w), then over z2
  HcPass pa{w.lg, nullptr, Nz, 1, Nz, ny + nw, Ny, ny, nw, nullptr, dz, kappa, w.LA, nullptr, nullptr, 1, Nz};
  int rc = hc_launch<false, false, false>(pa, Nz, st);
  if (rc != CNF_OK) return rc;
  HcPass pb{w.LA, nullptr, Nz, 1, Nz, ny + nw, Ny, ny, nw, nullptr, dz, kappa, w.H, nullptr, nullptr, 1, Ny};
  if ((rc = hc_launch<false, false, false>(pb, Ny, st)) != CNF_OK) return rc;
  hipLaunchKernelGGL(hc_value_kernel, dim3(1), dim3(HC_RED), 0, st, w.H, Ny, ny, dz, var0, eps, T, true_value, ic_mass);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// The path's share of the workspace, after cnf_hopf_cole_2d's: per time of a chunk the two first passes' outputs
// ([x1, z2] and [x1, y2], log-sum and mean each) and six [x2, x1] results
int64_t hc_path_extra_doubles(const HcGrid& g) {
  return HC_TIMES * (2 * g.n1 * g.Nz + 2 * g.n1 * g.Ny + 6 * g.n1 * g.n2);
}

// The two passes from a table (row stride rs, S x S sources centred at index c) to the output grid for the nt times of
// a chunk: log-sum and means of the table's coordinates 1 and 2 at out, out + HC_TIMES nn, out + 2 HC_TIMES nn
int hc_path_to_outputs(const double* lw, int64_t rs, int S, int c, const HcGrid& g, const double* x1, const double* x2,
                       double dz, const double* kappa, int nt, double* Cbuf, double* out, hipStream_t stream) {
  const int n1 = (int)g.n1, n2 = (int)g.n2;
  const int64_t slab = g.n1 * S, nn = g.n1 * g.n2;
  double *LC = Cbuf, *MC = Cbuf + HC_TIMES * slab;     // [time][x1, source 2]
  HcPathPass pa{lw, nullptr, 0, rs, 1, S, c, n1, nt, x1, dz, {}, LC, MC, nullptr, slab, 1, S};
  HcPathPass pb{LC, MC, slab, S, 1, S, c, n2, nt, x2, dz, {}, out, out + 2 * HC_TIMES * nn, out + HC_TIMES * nn, nn, 1,
                n1};
  for (int q = 0; q < HC_TIMES; ++q) pa.kappa[q] = pb.kappa[q] = q < nt ? kappa[q] : 0.0;
  const dim3 ga((unsigned)S, (unsigned)((n1 + HC_BLOCK - 1) / HC_BLOCK), 1);
  hipLaunchKernelGGL((hc_path_pass_kernel<HC_TIMES, false>), ga, dim3(HC_BLOCK), 0, stream, pa);
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  const dim3 gb((unsigned)n1, (unsigned)((n2 + HC_BLOCK - 1) / HC_BLOCK), (unsigned)nt);
  hipLaunchKernelGGL((hc_path_pass_kernel<1, true>), gb, dim3(HC_BLOCK), 0, stream, pb);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// A time of the path: HC_T_*, or -1 where cnf_hopf_cole_path_2d refuses it.  Between the endpoints the two Gaussian
// kernels have standard deviations sqrt(2 eps (T - t)) and sqrt(2 eps t); the uniform rule's aliasing error for a
// Gaussian of standard deviation sigma is about 2 exp(-2 pi^2 sigma^2 / dz^2), 1e-19 at sigma = 1.5 dz, so from there
// up the quadrature is exact at float64 level, and below it the time is refused rather than summed badly.
int hc_time_mode(double t, double T, double eps, double dz) {
  if (!std::isfinite(t) || t < 0.0 || t > T) return -1;
  if (t == 0.0) return HC_T_ZERO;
  if (t == T) return HC_T_END;
  return std::sqrt(2.0 * eps * std::min(t, T - t)) < 1.5 * dz ? -1 : HC_T_INNER;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_hopf_cole_workspace(double dz, double window, double y_range, int64_t n1, int64_t n2,
                                       int64_t* bytes) {
  const HcGrid g = hc_grid(dz, window, y_range, n1, n2);
  if (!bytes || !g.ok) return CNF_ERR_INVALID;
  *bytes = hc_workspace_doubles(g) * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_hopf_cole_2d(int32_t subtype, float a, double T, double beta, double var0, double dz,
                                double window, double y_range, const double* x1, int64_t n1, const double* x2,
                                int64_t n2, double* log_rho, double* score, double* w0, double* wT,
                                double* true_value, double* ic_mass, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  const HcGrid g = hc_grid(dz, window, y_range, n1, n2);
  if (!g.ok || !(T > 0.0) || !(beta > 0.0) || !(var0 > 0.0) || !std::isfinite(T) || !std::isfinite(beta) ||
      !std::isfinite(var0) || !std::isfinite(a) || subtype < CNF_POT_QUADRATIC || subtype > CNF_POT_OBSTACLE)
    return CNF_ERR_INVALID;
  if (!workspace || workspace_bytes < hc_workspace_doubles(g) * (int64_t)sizeof(double)) return CNF_ERR_INVALID;
  const bool outputs = g.n1 > 0;
  if (outputs && (!x1 || !x2 || !log_rho)) return CNF_ERR_INVALID;
  if (!outputs && (score || w0 || wT)) return CNF_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const double eps = 1.0 / beta, kappa = beta / (4.0 * T);
  const int nw = (int)g.nw, Ny = (int)g.Ny, Nz = (int)g.Nz;
  const HcBuffers w = hc_buffers(g, workspace);
  double *lg = w.lg, *H = w.H, *Cbuf = w.Cbuf, *D = w.D;
  int rc = hc_h_and_value(g, w, subtype, a, T, beta, var0, dz, true_value, ic_mass, st);
  if (rc != CNF_OK) return rc;
  if (!outputs) return CNF_OK;
  const int64_t nn = g.n1 * g.n2;
  double *L = D, *M1 = D + nn, *M2 = D + 2 * nn, *L0 = D + 3 * nn, *M01 = D + 4 * nn, *M02 = D + 5 * nn;
  const bool means = score || wT;
  if ((rc = hc_to_outputs(H, Ny, g, x1, x2, dz, kappa, means, Cbuf, L, M1, M2, st)) != CNF_OK) return rc;
  if (w0) {       // m0: the y grid weighted by exp(-(g(y) + |x - y|^2 / (2T)) / (2 eps)), the y block of lg
    const double* lg_y = lg + (int64_t)nw * Nz + nw;
    if ((rc = hc_to_outputs(lg_y, Nz, g, x1, x2, dz, kappa, true, Cbuf + 2 * g.n1 * g.Ny, L0, M01, M02, st)) != CNF_OK)
      return rc;
  }
  hipLaunchKernelGGL(hc_finish_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, x1, x2, (int)g.n1,
                     (int)g.n2, L, means ? M1 : nullptr, means ? M2 : nullptr, M01, M02, 2.0 * log(dz), eps, T,
                     (int)subtype, a, log_rho, score, w0, wT);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_hopf_cole_path_workspace(double dz, double window, double y_range, int64_t n1, int64_t n2,
                                            int64_t* bytes) {
  const HcGrid g = hc_grid(dz, window, y_range, n1, n2);
  if (!bytes || !g.ok || g.n1 == 0) return CNF_ERR_INVALID;
  *bytes = (hc_workspace_doubles(g) + hc_path_extra_doubles(g)) * (int64_t)sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_hopf_cole_path_2d(int32_t subtype, float a, double T, double beta, double var0, double dz,
                                     double window, double y_range, const double* times, int64_t S, const double* x1,
                                     int64_t n1, const double* x2, int64_t n2, double* log_rho, double* score,
                                     double* drift, double* vel, double* true_value, double* ic_mass, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  const HcGrid g = hc_grid(dz, window, y_range, n1, n2);
  if (!g.ok || !(T > 0.0) || !(beta > 0.0) || !(var0 > 0.0) || !std::isfinite(T) || !std::isfinite(beta) ||
      !std::isfinite(var0) || !std::isfinite(a) || subtype < CNF_POT_QUADRATIC || subtype > CNF_POT_OBSTACLE)
    return CNF_ERR_INVALID;
  if (g.n1 == 0 || !times || S < 1 || S > HC_MAX_N || !x1 || !x2 || !log_rho) return CNF_ERR_INVALID;
  const int64_t base = hc_workspace_doubles(g);
  if (!workspace || workspace_bytes < (base + hc_path_extra_doubles(g)) * (int64_t)sizeof(double))
    return CNF_ERR_INVALID;
  const double eps = 1.0 / beta, kappa = beta / (4.0 * T);
  bool at0 = false, atT = false;
  for (int64_t s = 0; s < S; ++s) {
    const int mode = hc_time_mode(times[s], T, eps, dz);
    if (mode < 0) return CNF_ERR_INVALID;
    at0 |= mode == HC_T_ZERO;
    atT |= mode == HC_T_END;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nw = (int)g.nw, Ny = (int)g.Ny, Nz = (int)g.Nz;
  const HcBuffers w = hc_buffers(g, workspace);
  int rc = hc_h_and_value(g, w, subtype, a, T, beta, var0, dz, true_value, ic_mass, st);
  if (rc != CNF_OK) return rc;
  const int64_t nn = g.n1 * g.n2;
  double *L = w.D, *M1 = w.D + nn, *M2 = w.D + 2 * nn, *L0 = w.D + 3 * nn, *M01 = w.D + 4 * nn, *M02 = w.D + 5 * nn;
  // the endpoints, once per call: cnf_hopf_cole_2d's own passes at kappa = 1 / (4 eps T)
  const bool means = score || vel;
  if (atT && (rc = hc_to_outputs(w.H, Ny, g, x1, x2, dz, kappa, means, w.Cbuf, L, M1, M2, st)) != CNF_OK) return rc;
  if (at0 && (drift || vel)) {
    const double* lg_y = w.lg + (int64_t)nw * Nz + nw;
    if ((rc = hc_to_outputs(lg_y, Nz, g, x1, x2, dz, kappa, true, w.Cbuf + 2 * g.n1 * g.Ny, L0, M01, M02, st)) != CNF_OK)
      return rc;
  }
  double* CbB = (double*)workspace + base;                     // [2][HC_TIMES][x1, z2]
  double* CbF = CbB + 2 * HC_TIMES * g.n1 * g.Nz;              // [2][HC_TIMES][x1, y2]
  double* W = CbF + 2 * HC_TIMES * g.n1 * g.Ny;                // [6][HC_TIMES][x2, x1]
  const double l2dz = 2.0 * log(dz);
  const unsigned blocks = (unsigned)((nn + 255) / 256);
  auto finish = [&](HcPathSlots& sl) {
    if (sl.n == 0) return CNF_OK;
    hipLaunchKernelGGL(hc_path_finish_kernel, dim3(blocks), dim3(256), 0, st, sl, x1, x2, (int)g.n1, (int)g.n2, W, M01,
                       M02, l2dz, eps, T, var0, (int)subtype, a, log_rho, score, drift, vel);
    sl.n = 0;
    return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
  };
  auto chunk = [&](HcPathSlots& sl) {        // the interior times collected so far: four passes and the epilogue
    if (sl.n == 0) return CNF_OK;
    double kb[HC_TIMES], kf[HC_TIMES];
    for (int q = 0; q < sl.n; ++q) {
      kb[q] = beta / (4.0 * (T - sl.t[q]));
      kf[q] = beta / (4.0 * sl.t[q]);
    }
    int rc = hc_path_to_outputs(w.lg, Nz, Nz, (int)(g.ny + g.nw), g, x1, x2, dz, kb, sl.n, CbB, W, st);
    if (rc != CNF_OK) return rc;
    if ((rc = hc_path_to_outputs(w.H, Ny, Ny, (int)g.ny, g, x1, x2, dz, kf, sl.n, CbF, W + 3 * HC_TIMES * nn, st)) != CNF_OK)
      return rc;
    return finish(sl);
  };
  HcPathSlots inner{}, ends{};
  for (int64_t s = 0; s < S; ++s) {
    const int mode = hc_time_mode(times[s], T, eps, dz);
    HcPathSlots& sl = mode == HC_T_INNER ? inner : ends;
    sl.mode[sl.n] = mode;
    sl.slab[sl.n] = s;
    sl.t[sl.n] = times[s];
    ++sl.n;
    if (mode == HC_T_END) {                // log rho_T, score_T and wT exactly as cnf_hopf_cole_2d writes them
      hipLaunchKernelGGL(hc_finish_kernel, dim3(blocks), dim3(256), 0, st, x1, x2, (int)g.n1, (int)g.n2, L,
                         means ? M1 : nullptr, means ? M2 : nullptr, (const double*)nullptr, (const double*)nullptr,
                         l2dz, eps, T, (int)subtype, a, log_rho + s * nn, score ? score + 2 * s * nn : nullptr,
                         (double*)nullptr, vel ? vel + 2 * s * nn : nullptr);
      if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
    }
    if (sl.n == HC_TIMES && (rc = mode == HC_T_INNER ? chunk(sl) : finish(sl)) != CNF_OK) return rc;
  }
  if ((rc = chunk(inner)) != CNF_OK) return rc;
  return finish(ends);
}
