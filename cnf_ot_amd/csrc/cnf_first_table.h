// cnf_first_table.h -- the `first` spline's inverse as a certified interpolation table (dim-2 table path, sampling
// direction, L = 2: flow_pwl_kernel).
//
// The `first` spline is one unconditional rational-quadratic spline, the same for every layer, slice and launch until
// the next cnf_model_set_params: v -> (g^-1(v), -log g'(g^-1(v))) is a fixed 1-D function.  first_table_kernel
// tabulates it once per parameter load, in float64 from the float64 header prepare_kernel writes, and certifies the
// table against the float64 closed form; the flow kernel then replaces the per-sample quadratic root (v_sqrt_f32 and
// two v_rcp_f32 per sample and layer) by a grid lookup and a packed quintic Horner.  cnf_ot_amd/first_table.py states
// the construction in numpy; the tests hold this file to it.
//
// Format (behind every other section of the prepared model buffer):
//   [4 words]            FT_W_CERT: FT_CERTIFIED or 0, FT_W_FAILS / FT_W_DONE: the builder's block counters
//   [FT_CELLS x 4]       a cell's grid entry: ref, the next breakpoint (+inf: none), the byte offset of the cell's
//                        first row, 0 -- one ds_read_b128 per sample
//   [FT_ROWS x FT_ROW]   a piece's row (o0, l0, o1, l1, .., o5, l5): `out` and `ld` as quintics in dv = v - ref,
//                        three ds_read_b128 at immediate offsets from one address per sample.  At a stride of 48 B
//                        consecutive rows start 12 banks apart: the rows of 64 unrelated lanes start on 16 different
//                        bank groups, as the conditioner rows (PWL_ROW) do.
// FT_CELLS uniform cells over [range_min, range_max]; a cell that holds an interior y knot is split there (the spline
// is only C^1 at a knot), so there are FT_CELLS + K - 1 pieces.  A piece's quintic goes through its six
// Chebyshev-Lobatto nodes, end points included: neighbours agree at their common edge to rounding.  ref is the cell's
// midpoint, or the knot for both pieces of a split cell (|dv| <= one cell: nothing cancels); the kernel's comparison
// against the breakpoint is then a comparison against ref.
// Certified (one model-wide word): every piece within FT_BUDGET -- two fp32 ulps at the value's magnitude, below the
// rounding of the fp32 closed form -- of the float64 closed form at FT_PROBES interior points that are not nodes, with
// the coefficients as stored (rounded to fp32); no cell with two knots; no knot within ft_edge_guard(lo, hi) of a cell
// edge (the fp32 cell index is off by one near an edge, harmless unless a knot lies between); all finite.
#pragma once
#include "cnf_device.h"

namespace cnf {

constexpr int FT_K = 5;                          // the table path's bin count (pwl_network)
constexpr int FT_CELLS = 1024;
constexpr int FT_DEG = 5;
constexpr int FT_ROW = 2 * (FT_DEG + 1);         // 12 floats = 48 B
constexpr int FT_ROWS = FT_CELLS + FT_K - 1;
constexpr int FT_PROBES = 17;
constexpr double FT_BUDGET = 2.4e-7;
// How far from a cell edge the kernel's cell index, (int)fmaf(v, cs, c0) in fp32, can put v into the neighbouring cell:
// cs, c0 and the FMA's result are each rounded once, 2^-24 relative, on magnitudes |v| cs, |lo| cs and the index
// itself: at most 2^-24 (2 max(|lo|, |hi|) + (hi - lo)) in units of v.  The guard is twice that (4.8e-6 for
// [-10, 10]); it follows the configured range.
__host__ __device__ inline double ft_edge_guard(double lo, double hi) {
  const double m = fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
  return 1.1920928955078125e-7 * (2.0 * m + (hi - lo));
}
constexpr int FT_WORDS = 4;                      // status words in front of the table
enum { FT_W_CERT = 0, FT_W_FAILS = 1, FT_W_DONE = 2 };
constexpr uint32_t FT_CERTIFIED = 0x31305446u;
constexpr int FT_GRID_FLOATS = 4 * FT_CELLS;
constexpr int FT_LDS_FLOATS = FT_GRID_FLOATS + FT_ROWS * FT_ROW;       // what a workgroup stages: 65 728 B
constexpr int FT_FLOATS = FT_WORDS + FT_LDS_FLOATS;                    // floats in the prepared model buffer
static_assert(FT_ROW % 4 == 0 && FT_WORDS % 4 == 0, "grid entries and rows are read with 16-byte loads");

constexpr int FT_PPB = 8;                        // pieces per block of the builder, 32 lanes each
constexpr int FT_BLOCKS = (FT_ROWS + FT_PPB - 1) / FT_PPB;
static_assert(FT_BLOCKS * FT_PPB >= FT_CELLS, "block b also writes the grid entries of cells 8 b .. 8 b + 7");

// (g^-1(v), -log g') of bin k, float64 closed form: the flow kernel's root (rqs_bin_eval) without its fp32 rounding
__device__ __forceinline__ void ft_closed(const double* xk, const double* yk, const double* d, int k, double v,
                                          double& out, double& ld) {
  const double x0 = xk[k], y0 = yk[k];
  const double bw = xk[k + 1] - x0, bh = yk[k + 1] - y0, s = bh / bw;
  const double d0 = d[k], d1 = d[k + 1], st = d1 + d0 - 2.0 * s;
  const double dy = v - y0, c2 = 2.0 * s * dy;
  const double b = d0 * bh - st * dy, a = s * bh - b;
  const double z = c2 / (b + sqrt(b * b + a * (c2 + c2))), omz = 1.0 - z;
  const double num2 = d1 * z * z + 2.0 * s * z * omz + d0 * omz * omz;
  const double den = s + st * z * omz;
  out = x0 + bw * z;
  ld = -log(s * s * num2 / (den * den));
}

// One block per FT_PPB pieces, 32 lanes per piece: lanes 0-5 evaluate the closed form at the nodes, lanes 6-22 at the
// probes; lanes 0 / 1 turn the node values of out / ld into coefficients about ref (Newton's divided differences, then
// nested multiplication); the probe lanes compare.  The last block to finish writes the model-wide word
// (prepare_kernel, earlier on the same stream, has cleared the three words).
// (a template, so that every unit that includes this header may: the kernel is launched from cnf_flow.hip alone)
template <int K>
__global__ __launch_bounds__(32 * FT_PPB) void first_table_kernel(const double* __restrict__ tabd, float* __restrict__ ft,
                                                                 double lo, double hi) {
  static_assert(K == FT_K, "FT_ROWS counts the K - 1 knot splits");
  constexpr int N = FT_DEG + 1;
  __shared__ double xk[K + 1], yk[K + 1], dk[K + 1];
  __shared__ double fo[FT_PPB][N], fl[FT_PPB][N];
  __shared__ float cf[FT_PPB][FT_ROW];
  if (threadIdx.x <= K) {
    xk[threadIdx.x] = tabd[tab_off(F_XK, K) + threadIdx.x];
    yk[threadIdx.x] = tabd[tab_off(F_YK, K) + threadIdx.x];
    dk[threadIdx.x] = threadIdx.x < K ? tabd[tab_off(F_D0, K) + threadIdx.x] : tabd[tab_off(F_D1, K) + K - 1];
  }
  __syncthreads();
  const double cw = (hi - lo) / FT_CELLS, guard = ft_edge_guard(lo, hi);
  int kc[K - 1];
  bool fail = false;
#pragma unroll
  for (int j = 0; j < K - 1; ++j) {
    const double q = floor((yk[j + 1] - lo) / cw);
    const int c = q >= 0.0 && q < (double)FT_CELLS ? (int)q : 0;
    fail |= !(q >= 0.0 && q < (double)FT_CELLS);
    kc[j] = c;
    if (j > 0 && kc[j - 1] == c) fail = true;
    const double e0 = lo + c * cw, e1 = c + 1 < FT_CELLS ? lo + (c + 1) * cw : hi;
    if (!(yk[j + 1] - e0 >= guard) || !(e1 - yk[j + 1] >= guard)) fail = true;
  }
  const int lp = threadIdx.x >> 5, ln = threadIdx.x & 31;
  const int p = blockIdx.x * FT_PPB + lp;
  float* grid = ft + FT_WORDS;
  float* rows = grid + FT_GRID_FLOATS;

  // the piece: its cell, which part of it, its range [a, b], its bin and ref
  int m = 0, half = 0, knot = 0;
#pragma unroll
  for (int j = 0; j < K - 1; ++j) {
    const int q = kc[j] + j;
    if (q + 1 <= p) ++m;
    if (p == q + 1) { half = 2; knot = j + 1; }
    else if (p == q && half == 0) { half = 1; knot = j + 1; }
  }
  int c = p - m;
  c = c < 0 ? 0 : (c > FT_CELLS - 1 ? FT_CELLS - 1 : c);
  double a = lo + c * cw, b = c + 1 < FT_CELLS ? lo + (c + 1) * cw : hi;
  int bin = 0;
#pragma unroll
  for (int j = 0; j < K - 1; ++j) bin += kc[j] < c ? 1 : 0;
  double refd = 0.5 * (a + b);
  if (half == 1) { b = yk[knot]; refd = yk[knot]; bin = knot - 1; }
  if (half == 2) { a = yk[knot]; refd = yk[knot]; bin = knot; }
  if (bin > K - 1) bin = K - 1;
  const float ref32 = (float)refd;
  const double ref = (double)ref32;
  const double mid = 0.5 * (a + b), rad = 0.5 * (b - a);

  // -cos(i pi / 5): the Chebyshev-Lobatto nodes of degree 5
  const double nodes[N] = {-1.0, -0.8090169943749475, -0.30901699437494745, 0.30901699437494745, 0.8090169943749475, 1.0};
  double xs[N];                          // the nodes relative to ref; x: this lane's node or probe
  double x = mid + rad * ((2.0 * (double)(ln - N) + 1.0) / (double)FT_PROBES - 1.0);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double xn = i == 0 ? a : (i == N - 1 ? b : mid + rad * nodes[i]);
    xs[i] = xn - ref;
    if (ln == i) x = xn;
  }
  double vo, vl;
  ft_closed(xk, yk, dk, bin, x, vo, vl);
  if (ln < N) { fo[lp][ln] = vo; fl[lp][ln] = vl; }
  __syncthreads();
  if (ln < 2) {
    double cc[N], mm[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { cc[i] = ln == 0 ? fo[lp][i] : fl[lp][i]; mm[i] = 0.0; }
#pragma unroll
    for (int j = 1; j < N; ++j)
#pragma unroll
      for (int i = N - 1; i >= j; --i) cc[i] = (cc[i] - cc[i - 1]) / (xs[i] - xs[i - j]);
    mm[0] = cc[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) {
#pragma unroll
      for (int q = N - 1 - i; q >= 1; --q) mm[q] = mm[q - 1] - xs[i] * mm[q];
      mm[0] = cc[i] - xs[i] * mm[0];
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const float v = (float)mm[q];
      if (!(fabsf(v) <= 3.0e38f)) fail = true;      // NaN or inf
      cf[lp][2 * q + ln] = v;
      if (p < FT_ROWS) rows[(int64_t)p * FT_ROW + 2 * q + ln] = v;
    }
  }
  __syncthreads();
  if (ln >= N && ln < N + FT_PROBES && p < FT_ROWS) {
    const double dv = x - ref;
    double po = (double)cf[lp][2 * FT_DEG], pl = (double)cf[lp][2 * FT_DEG + 1];
#pragma unroll
    for (int q = FT_DEG - 1; q >= 0; --q) { po = po * dv + (double)cf[lp][2 * q]; pl = pl * dv + (double)cf[lp][2 * q + 1]; }
    if (!(fabs(po - vo) <= FT_BUDGET * fmax(1.0, fabs(vo)))) fail = true;
    if (!(fabs(pl - vl) <= FT_BUDGET * fmax(1.0, fabs(vl)))) fail = true;
  }
  if (ln == 31) {                        // the grid entry of cell 8 b + lp
    const int cell = blockIdx.x * FT_PPB + lp;
    if (cell < FT_CELLS) {
      int base = cell;
      bool split = false;
      double r = 0.5 * ((lo + cell * cw) + (cell + 1 < FT_CELLS ? lo + (cell + 1) * cw : hi));
#pragma unroll
      for (int j = 0; j < K - 1; ++j) {
        base += kc[j] < cell ? 1 : 0;
        if (kc[j] == cell && !split) { split = true; r = yk[j + 1]; }
      }
      f4 e;
      e.x = (float)r;
      e.y = split ? (float)r : __builtin_inff();
      e.z = __uint_as_float((uint32_t)(base * FT_ROW * 4));
      e.w = 0.0f;
      reinterpret_cast<f4*>(grid)[cell] = e;
    }
  }
  const int any = __syncthreads_or(p < FT_ROWS && fail ? 1 : 0);
  if (threadIdx.x == 0) {
    uint32_t* words = reinterpret_cast<uint32_t*>(ft);
    if (any) atomicAdd(&words[FT_W_FAILS], 1u);
    __threadfence();
    if (atomicAdd(&words[FT_W_DONE], 1u) == gridDim.x - 1) {
      __threadfence();
      words[FT_W_CERT] = atomicAdd(&words[FT_W_FAILS], 0u) == 0u ? FT_CERTIFIED : 0u;
    }
  }
}

// Stage grid and rows into LDS (once per workgroup: the table does not depend on the slice)
__device__ __forceinline__ void ft_stage(float* dst, const float* __restrict__ ft, int tid, int nthreads) {
  const f4* src = reinterpret_cast<const f4*>(ft + FT_WORDS);
  f4* d = reinterpret_cast<f4*>(dst);
  for (int i = tid; i < FT_LDS_FLOATS / 4; i += nthreads) d[i] = src[i];
}

// What the lookup needs beside the table: cell = (int)(v cs + c0), as wave-uniform scalars
struct FtConsts { float cs, c0; uint32_t grid, rows; };
__device__ __forceinline__ FtConsts ft_consts(const float* ftl, const SplineConsts sc) {
  FtConsts f;
  f.cs = (float)FT_CELLS / (sc.hi - sc.lo);
  f.c0 = -sc.lo * f.cs;
  f.grid = (uint32_t)(uintptr_t)ftl;              // low 32 bits of a flat LDS address = LDS offset
  f.rows = f.grid + FT_GRID_FLOATS * 4;
  return f;
}

typedef const f4 __attribute__((address_space(3))) * ft_f4_ptr;

// A sample's grid entry: cell index (one FMA, convert, clamp), one ds_read_b128
__device__ __forceinline__ f4 ft_cell(const FtConsts f, float v) {
  // v_cvt_u32_f32 saturates: a negative value or a NaN gives cell 0, and the upper clamp is one v_min_u32 with a
  // literal (a v_med3_i32 would hold 1023 in a register of its own).  The operand comes from an FMA, not from a
  // transcendental: no wait state is needed (mul_clip01).
  uint32_t cell;
  asm("v_cvt_u32_f32 %0, %1" : "=v"(cell) : "v"(fmaf(v, f.cs, f.c0)));
  cell = cell > (uint32_t)(FT_CELLS - 1) ? (uint32_t)(FT_CELLS - 1) : cell;
  return *(ft_f4_ptr)(uintptr_t)(f.grid + (cell << 4));
}
// ... its row: one comparison against the breakpoint where a knot splits the cell
__device__ __forceinline__ uint32_t ft_row(const FtConsts f, float v, f4 g) {
  return f.rows + __float_as_uint(g.z) + (v >= g.y ? (uint32_t)(FT_ROW * 4) : 0u);
}
// ... and the row's two quintics at dv: three 16-byte reads at immediate offsets, Horner on (out, ld) as a pair
__device__ __forceinline__ v2f ft_horner(uint32_t ra, float dv) {
  const ft_f4_ptr row = (ft_f4_ptr)(uintptr_t)ra;
  const f4 r0 = row[0], r1 = row[1], r2 = row[2];
  const v2f d2 = v2f{dv, dv};
  v2f acc = __builtin_elementwise_fma(v2f{r2.z, r2.w}, d2, v2f{r2.x, r2.y});
  acc = __builtin_elementwise_fma(acc, d2, v2f{r1.z, r1.w});
  acc = __builtin_elementwise_fma(acc, d2, v2f{r1.x, r1.y});
  acc = __builtin_elementwise_fma(acc, d2, v2f{r0.z, r0.w});
  return __builtin_elementwise_fma(acc, d2, v2f{r0.x, r0.y});
}
// A sample pair
__device__ __forceinline__ void ft_eval(const FtConsts f, v2f v, v2f& out, v2f& ld) {
  const f4 gx = ft_cell(f, v.x), gy = ft_cell(f, v.y);
  const v2f px = ft_horner(ft_row(f, v.x, gx), v.x - gx.x);
  const v2f py = ft_horner(ft_row(f, v.y, gy), v.y - gy.x);
  out = v2f{px.x, py.x};
  ld = v2f{px.y, py.y};
}

}  // namespace cnf
