// cnf_fp_stats.h -- what the particle references share (cnf_fp_particles.hip: the Euler-Maruyama ensemble and
// cnf_point_stats; cnf_mv_particles.hip: the interacting ensemble): the per-snapshot statistics of a chunk of particles
// -- raw sums over a fixed partition, a histogram by no-return integer adds -- the sum over the chunks, the host side
// that fills FpStats from the C ABI's arguments, and a lane's walk through its Philox blocks.  One definition each.
#pragma once
#include "cnf_terms.h"

#include <math.h>

#include <cmath>

namespace cnf {
namespace {

constexpr int FP_CHUNK = 256;      // particles per chunk = lanes per workgroup: the unit of the sums' fixed partition
constexpr int FP_WAVES = FP_CHUNK / 64;
constexpr int FP_MAX_S = 64;
constexpr int FP_MAX_D = 14;
constexpr int64_t FP_MAX_STEPS = int64_t(1) << 30;
constexpr int64_t FP_MAX_CELLS = int64_t(1) << 24;

__host__ __device__ constexpr int fp_terms(int D) { return 2 + D + D * D; }

// Where the statistics of a snapshot go: partial [slabs][K][n_chunks] (K = fp_terms(D) + EXTRA), hist [S][ny][nx]
struct FpStats {
  double* partial;
  uint32_t* hist;
  int64_t n_chunks;
  double edge_x, edge_y, step_x, step_y;     // edge = lo - step / 2: cell j is centred on lo + j step
  int32_t nx, ny, axis_x, axis_y;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One chunk's contribution to a snapshot: the particle of this lane is x (live: the lane holds one); its counts go to
// histogram s, its sums to slab `slab` of the partials (cnf_fp_particles: the snapshot; cnf_mv_particles: snapshot and
// replica).  Every lane of the workgroup calls this (it synchronises).  A non-finite particle counts as such and
// enters neither sums nor histogram.  EXTRA = 1: one more per-particle term, `extra`, summed after the moments.
template <int D, int EXTRA = 0>
__device__ __forceinline__ void fp_accumulate(const double (&x)[D], bool live, int s, int64_t slab, int64_t chunk,
                                              const FpStats& o, double* s_part, double extra = 0.0) {
  constexpr int K = fp_terms(D) + EXTRA;
  bool finite = live;
#pragma unroll
  for (int d = 0; d < D; ++d) finite = finite && isfinite(x[d]);
  if (o.hist && finite) {
    double cx = 0.0, cy = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (d == o.axis_x) cx = x[d];
      if (d == o.axis_y) cy = x[d];
    }
    // IEEE float64 division (no reciprocal): the same cell as the float64 restatement
    const double qx = floor((cx - o.edge_x) / o.step_x), qy = floor((cy - o.edge_y) / o.step_y);
    if (qx >= 0.0 && qx < (double)o.nx && qy >= 0.0 && qy < (double)o.ny) {
      const int64_t cell = ((int64_t)s * o.ny + (int64_t)qy) * o.nx + (int64_t)qx;
      (void)__hip_atomic_fetch_add(o.hist + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (!o.partial) return;
  const int wave = (int)threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  double* mine = s_part + wave * K;
  double y[D];
#pragma unroll
  for (int d = 0; d < D; ++d) y[d] = finite ? x[d] : 0.0;
  const double n_ok = wave_sum(finite ? 1.0 : 0.0), n_bad = wave_sum(live && !finite ? 1.0 : 0.0);
  if (lead) { mine[0] = n_ok; mine[1] = n_bad; }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double v = wave_sum(y[d]);
    if (lead) mine[2 + d] = v;
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int e = 0; e < D; ++e) {
      const double v = wave_sum(y[d] * y[e]);
      if (lead) mine[2 + D + d * D + e] = v;
    }
  if constexpr (EXTRA == 1) {
    const double v = wave_sum(finite ? extra : 0.0);
    if (lead) mine[K - 1] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    double v = s_part[threadIdx.x];
#pragma unroll
    for (int w = 1; w < FP_WAVES; ++w) v += s_part[w * K + threadIdx.x];
    o.partial[(slab * K + threadIdx.x) * o.n_chunks + chunk] = v;
  }
  __syncthreads();
}

// sums[i] = the chunks' partials of (slab, term) i in ascending order, one thread each
__global__ __launch_bounds__(64) void fp_sum_chunks_kernel(const double* partial, int64_t n_chunks, int n_out,
                                                           double* sums) {
  const int i = blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_out) return;
  const double* p = partial + (int64_t)i * n_chunks;
  double v = 0.0;
  for (int64_t c = 0; c < n_chunks; ++c) v += p[c];
  sums[i] = v;
}

// The lane's walk through its Philox blocks.  The position is the same in every lane of the launch (all particles are
// at the same step), so the refill branch and the selects are wave-uniform.
struct NormalWalk {
  uint64_t seed, blk;
  float z[4];
  int e;
  __device__ __forceinline__ double next() {
    const int r = e & 3;
    if (r == 0) philox_normals4(seed, blk++, z);
    ++e;
    return (double)(r == 0 ? z[0] : r == 1 ? z[1] : r == 2 ? z[2] : z[3]);
  }
  // The walk of a particle whose elements start at block `first_blk`, standing at its element `off`: what `off` calls
  // of next() from the block boundary leave behind, computed from (first_blk, off) alone
  __device__ __forceinline__ static NormalWalk at(uint64_t seed, uint64_t first_blk, int64_t off) {
    NormalWalk w{seed, first_blk + (uint64_t)(off >> 2), {0.0f, 0.0f, 0.0f, 0.0f}, (int)(off & 3)};
    if (w.e != 0) philox_normals4(seed, w.blk++, w.z);
    return w;
  }
};

int64_t fp_chunks(int64_t N) { return (N + FP_CHUNK - 1) / FP_CHUNK; }

// The histogram side of FpStats from the C ABI's grid; false: refuse
bool fp_hist_of(int32_t D, const CnfFieldGrid* grid, uint32_t* hist, FpStats* o) {
  if (!hist) return true;
  if (!grid) return false;
  const CnfFieldGrid& g = *grid;
  if (g.nx < 1 || g.ny < 1 || (int64_t)g.nx * g.ny > FP_MAX_CELLS) return false;
  if (!(g.step_x > 0.0) || !(g.step_y > 0.0) || !std::isfinite(g.step_x) || !std::isfinite(g.step_y) ||
      !std::isfinite(g.lo_x) || !std::isfinite(g.lo_y))
    return false;
  if (g.axis_x < 0 || g.axis_x >= D || g.axis_y < 0 || g.axis_y >= D || g.axis_x == g.axis_y) return false;
  o->hist = hist;
  o->edge_x = g.lo_x - g.step_x / 2;
  o->edge_y = g.lo_y - g.step_y / 2;
  o->step_x = g.step_x;
  o->step_y = g.step_y;
  o->nx = g.nx; o->ny = g.ny; o->axis_x = g.axis_x; o->axis_y = g.axis_y;
  return true;
}

int fp_clear_hist(const FpStats& o, int32_t S, hipStream_t st) {
  if (!o.hist) return CNF_OK;
  return hipMemsetAsync(o.hist, 0, (size_t)S * o.nx * o.ny * sizeof(uint32_t), st) == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// sums [n_out] from the partials [n_out][n_chunks]
int fp_finish_sums(const FpStats& o, int n_out, double* sums, hipStream_t st) {
  if (!sums) return CNF_OK;
  hipLaunchKernelGGL(fp_sum_chunks_kernel, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, st, o.partial, o.n_chunks,
                     n_out, sums);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// The checks on step, start and stream that both ensembles make: h, var0 > 0 and finite, sigma >= 0, a finite,
// n_steps in [0, 2^30], first_particle >= 0, ascending snapshot steps in [0, n_steps], and an element index that fits
// for `particles` particles from first_particle on.  *blocks_per_particle: R / 4.
bool fp_run_ok(int32_t D, float a, double sigma, double h, int64_t n_steps, double var0, int64_t first_particle,
               int64_t particles, const int64_t* snap_step, int32_t S, int64_t* blocks_per_particle) {
  if (!(h > 0.0) || !std::isfinite(h) || !(var0 > 0.0) || !std::isfinite(var0) || !(sigma >= 0.0) ||
      !std::isfinite(sigma) || !std::isfinite(a) || n_steps < 0 || n_steps > FP_MAX_STEPS || first_particle < 0)
    return false;
  if (!snap_step) return false;
  for (int32_t s = 0; s < S; ++s)
    if (snap_step[s] < 0 || snap_step[s] > n_steps || (s > 0 && snap_step[s] <= snap_step[s - 1])) return false;
  const int64_t per_particle = ((n_steps + 1) * D + 3) / 4;        // R / 4
  if (first_particle > INT64_MAX - particles || (first_particle + particles) > (INT64_MAX / 4) / per_particle)
    return false;                                                   // the element index fits
  *blocks_per_particle = per_particle;
  return true;
}

}  // namespace
}  // namespace cnf
