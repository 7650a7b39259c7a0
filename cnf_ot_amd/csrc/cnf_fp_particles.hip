// cnf_fp_particles.hip -- a particle reference for the Fokker-Planck problems: an Euler-Maruyama ensemble of the SDE
// behind flow_matching_loss_fn (applications.py:279-374; the reference's authors sketch it in tests/test_lorenz.py).
// The loss fits v_flow + sigma grad log rho = drift, the continuity form of d rho / dt = -div(rho drift) + sigma lap rho,
// so the density is the law of
//   dX = drift(X) dt + sqrt(2 sigma) dW,   X_0 ~ N(0, var0 I),
// stepped as x <- x + h drift(x) + sqrt(2 sigma h) z.  State and drift are float64 (drift_field<double>, cnf_terms.h:
// the one definition); the normals are the float32 Philox / Box-Muller stream of cnf_fill_normal, widened exactly.
//
// One particle per lane, the state in registers.  Global particle p owns elements [p R, p R + (n_steps + 1) D) of the
// stream, R = (n_steps + 1) D rounded up to a multiple of 4, so a lane walks its own Philox blocks from a block
// boundary and consumes their 4 normals in order: D for the start, then D per step.
//
// At a snapshot a chunk of FP_CHUNK consecutive particles (one workgroup) reduces its 2 + D + D D raw sums over each
// wave by a fixed butterfly, adds the waves in order and writes ONE partial; fp_sum_chunks_kernel then adds the chunks'
// partials in ascending order.  The partition is by particle index, not by launch geometry: repeated calls are
// bit-identical.  Histogram counts go to global memory by no-return integer atomics (order-free).  A workgroup brings
// FP_CHUNK particles to a snapshot: an LDS-private histogram of nx ny cells would be cleared and flushed for 256
// increments, so it is not used.
#include "cnf_fp_stats.h"

#include <algorithm>

namespace cnf {
namespace {

constexpr int64_t FP_MAX_N = int64_t(1) << 31;

struct FpArgs {
  uint64_t seed;
  int64_t first, N, blocks_per_particle;     // R / 4
  const double* x0;
  double* pos;
  double h, sd0, sdn;                        // sqrt(var0), sqrt(2 sigma h)
  float a;
  int32_t S;
  FpStats st;
  int32_t snap[FP_MAX_S];
};

template <int D, int DRIFT>
__global__ __launch_bounds__(FP_CHUNK) void fp_particles_kernel(const FpArgs p) {
  __shared__ double s_part[FP_WAVES * fp_terms(D)];
  const int last = p.snap[p.S - 1];
  for (int64_t chunk = blockIdx.x; chunk < p.st.n_chunks; chunk += gridDim.x) {
    const int64_t i = chunk * FP_CHUNK + (int64_t)threadIdx.x;
    const bool live = i < p.N;
    NormalWalk w{p.seed, (uint64_t)(p.first + i) * (uint64_t)p.blocks_per_particle, {0.0f, 0.0f, 0.0f, 0.0f}, 0};
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = p.sd0 * w.next();
    if (p.x0 && live) {
#pragma unroll
      for (int d = 0; d < D; ++d) x[d] = p.x0[i * D + d];
    }
    int si = 0;
    for (int k = 0;; ++k) {
      if (p.snap[si] == k) {
        if (p.pos && live) {
#pragma unroll
          for (int d = 0; d < D; ++d) p.pos[((int64_t)si * p.N + i) * D + d] = x[d];
        }
        fp_accumulate<D>(x, live, si, si, chunk, p.st, s_part);
        ++si;
      }
      if (k == last) break;
      double xn[D];
      const auto at = [&](int d) { return x[d]; };
#pragma unroll
      for (int d = 0; d < D; ++d) xn[d] = fma(p.h, drift_field<double>(at, d, DRIFT, p.a), x[d]);
#pragma unroll
      for (int d = 0; d < D; ++d) x[d] = fma(p.sdn, w.next(), xn[d]);
    }
  }
}

struct PsArgs {
  const float* pts;
  int64_t N;
  int32_t S;
  FpStats st;
};

// The same statistics over given points pts [S][N][D] (float32, widened): chunk c of slab s is one workgroup's turn
template <int D>
__global__ __launch_bounds__(FP_CHUNK) void point_stats_kernel(const PsArgs p) {
  __shared__ double s_part[FP_WAVES * fp_terms(D)];
  const int64_t total = p.st.n_chunks * p.S;
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int s = (int)(t / p.st.n_chunks);
    const int64_t chunk = t % p.st.n_chunks;
    const int64_t i = chunk * FP_CHUNK + (int64_t)threadIdx.x;
    const bool live = i < p.N;
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = live ? (double)p.pts[((int64_t)s * p.N + i) * D + d] : 0.0;
    fp_accumulate<D>(x, live, s, s, chunk, p.st, s_part);
  }
}

template <int D> void fp_launch_drift(int drift, unsigned grid, hipStream_t st, const FpArgs& a) {
  if (drift == CNF_DRIFT_OU) hipLaunchKernelGGL((fp_particles_kernel<D, CNF_DRIFT_OU>), dim3(grid), dim3(FP_CHUNK), 0, st, a);
  if constexpr (D == 2) {
    if (drift == CNF_DRIFT_SMILE)
      hipLaunchKernelGGL((fp_particles_kernel<2, CNF_DRIFT_SMILE>), dim3(grid), dim3(FP_CHUNK), 0, st, a);
    if (drift == CNF_DRIFT_NONGRADIENT)
      hipLaunchKernelGGL((fp_particles_kernel<2, CNF_DRIFT_NONGRADIENT>), dim3(grid), dim3(FP_CHUNK), 0, st, a);
  }
  if constexpr (D == 3) {
    if (drift == CNF_DRIFT_LORENZ)
      hipLaunchKernelGGL((fp_particles_kernel<3, CNF_DRIFT_LORENZ>), dim3(grid), dim3(FP_CHUNK), 0, st, a);
  }
}

// f.template operator()<D>() for the runtime D in [1, FP_MAX_D]
template <int D = 1, class F> void fp_with_dim(int dim, F f) {
  if (dim == D) f.template operator()<D>();
  else if constexpr (D < FP_MAX_D) fp_with_dim<D + 1>(dim, f);
}

struct LaunchParticles {
  int drift;
  unsigned grid;
  hipStream_t st;
  const FpArgs* a;
  template <int D> void operator()() const { fp_launch_drift<D>(drift, grid, st, *a); }
};
struct LaunchStats {
  unsigned grid;
  hipStream_t st;
  const PsArgs* a;
  template <int D> void operator()() const {
    hipLaunchKernelGGL((point_stats_kernel<D>), dim3(grid), dim3(FP_CHUNK), 0, st, *a);
  }
};

bool fp_shape_ok(int64_t N, int32_t D, int32_t S) { return N >= 1 && N <= FP_MAX_N && D >= 1 && D <= FP_MAX_D && S >= 1 && S <= FP_MAX_S; }
int64_t fp_workspace_bytes(int64_t N, int32_t D, int32_t S) {
  return (int64_t)S * fp_terms(D) * fp_chunks(N) * (int64_t)sizeof(double);
}

// The output side shared by both entry points; false: refuse
bool fp_stats_of(int64_t N, int32_t D, int32_t S, const CnfFieldGrid* grid, double* sums, uint32_t* hist,
                 void* workspace, int64_t workspace_bytes, FpStats* o) {
  *o = FpStats{};
  o->n_chunks = fp_chunks(N);
  if (sums) {
    if (!workspace || workspace_bytes < fp_workspace_bytes(N, D, S)) return false;
    o->partial = (double*)workspace;
  }
  return fp_hist_of(D, grid, hist, o);
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_fp_particles_workspace(int64_t N, int32_t D, int32_t S, int64_t* bytes) {
  if (!bytes || !fp_shape_ok(N, D, S)) return CNF_ERR_INVALID;
  *bytes = fp_workspace_bytes(N, D, S);
  return CNF_OK;
}

extern "C" int cnf_fp_particles(int32_t drift, int32_t D, float a, double sigma, double h, int64_t n_steps,
                                double var0, uint64_t seed, int64_t first_particle, int64_t N, const double* x0,
                                const int64_t* snap_step, int32_t S, const CnfFieldGrid* grid, double* pos,
                                double* sums, uint32_t* hist, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!fp_shape_ok(N, D, S) || drift < CNF_DRIFT_OU || drift > CNF_DRIFT_LORENZ) return CNF_ERR_INVALID;
  if (((drift == CNF_DRIFT_SMILE || drift == CNF_DRIFT_NONGRADIENT) && D != 2) || (drift == CNF_DRIFT_LORENZ && D != 3))
    return CNF_ERR_INVALID;
  if (!pos && !sums && !hist) return CNF_ERR_INVALID;
  int64_t per_particle = 0;
  if (!fp_run_ok(D, a, sigma, h, n_steps, var0, first_particle, N, snap_step, S, &per_particle)) return CNF_ERR_INVALID;
  FpArgs args{};
  if (!fp_stats_of(N, D, S, grid, sums, hist, workspace, workspace_bytes, &args.st)) return CNF_ERR_INVALID;
  args.seed = seed;
  args.first = first_particle;
  args.N = N;
  args.blocks_per_particle = per_particle;
  args.x0 = x0;
  args.pos = pos;
  args.h = h;
  args.sd0 = std::sqrt(var0);
  args.sdn = std::sqrt(2.0 * sigma * h);
  args.a = a;
  args.S = S;
  for (int32_t s = 0; s < S; ++s) args.snap[s] = (int32_t)snap_step[s];
  hipStream_t st = (hipStream_t)stream;
  int rc = fp_clear_hist(args.st, S, st);
  if (rc != CNF_OK) return rc;
  const unsigned grid_blocks = (unsigned)std::min<int64_t>(args.st.n_chunks, int64_t(1) << 20);
  fp_with_dim(D, LaunchParticles{drift, grid_blocks, st, &args});
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  return fp_finish_sums(args.st, S * fp_terms(D), sums, st);
}

extern "C" int cnf_point_stats(const float* pts, int64_t N, int32_t D, int32_t S, const CnfFieldGrid* grid,
                               double* sums, uint32_t* hist, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!fp_shape_ok(N, D, S) || !pts || (!sums && !hist)) return CNF_ERR_INVALID;
  PsArgs args{};
  if (!fp_stats_of(N, D, S, grid, sums, hist, workspace, workspace_bytes, &args.st)) return CNF_ERR_INVALID;
  args.pts = pts;
  args.N = N;
  args.S = S;
  hipStream_t st = (hipStream_t)stream;
  int rc = fp_clear_hist(args.st, S, st);
  if (rc != CNF_OK) return rc;
  const unsigned grid_blocks = (unsigned)std::min<int64_t>(args.st.n_chunks * S, int64_t(1) << 20);
  fp_with_dim(D, LaunchStats{grid_blocks, st, &args});
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  return fp_finish_sums(args.st, S * fp_terms(D), sums, st);
}
