// cnf_mv_particles.hip -- a particle reference for the interacting (McKean-Vlasov) Fokker-Planck equation
//   d rho / dt = -div(rho (drift - kappa grad (W * rho))) + sigma lap rho:
// R independent replicas of N particles whose empirical law converges to it,
//   x_i <- x_i + h (drift(x_i) - kappa G_i) + sqrt(2 sigma h) z,   G_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j).
// Built from two pieces: the pair loop of cnf_interaction.hip -- ia_kernel itself, enqueued through
// interaction_pairs (cnf_host.h), a replica being one of its sets -- and the step, stream and statistics of
// cnf_fp_particles.hip (cnf_fp_stats.h).
//
// A step is two launches on the caller's stream, ordered by the stream alone: the pair pass over the float32 mirror
// of the positions, which leaves per (split, particle) one double of W and D doubles of grad W in the workspace; then
// mv_step_kernel, one particle per lane in workgroups of FP_CHUNK = one chunk of the sums' partition, which adds a
// particle's splits in ascending order, G_d = (cf sum) / (N - 1) in double (no float32 rounding of the force), takes
// the snapshot if step k is one -- positions, raw sums with the particle's W row sum as one more term, histogram --
// advances the float64 state in place and writes the float32 mirror for the next pair pass.  The update is
//   v = fma(-kappa, G_d, drift_d);  xn_d = fma(h, v, x_d)  for every d from the OLD x;  x_d = fma(sdn, z, xn_d),
// so kappa = 0 is cnf_fp_particles' step bit for bit (fma(-0.0, G, drift) == drift for finite G).  The step kernel
// keeps nothing across launches: its normals' Philox block comes from (particle, k).  The last snapshot's pair pass
// runs without the force and its step launch does not advance; after it only the chunks' partials are added.
//
// A non-finite particle is counted as such at snapshots and is NOT masked out of the pair pass: its differences are
// not finite, so every force of its own replica is non-finite one step later.  Replicas never interact.
#include "cnf_fp_stats.h"
#include "cnf_host.h"

#include <algorithm>

namespace cnf {
namespace {

constexpr int MV_MAX_R = 64;
constexpr int64_t MV_MAX_N = int64_t(1) << 20;

__host__ __device__ constexpr int mv_terms(int D) { return fp_terms(D) + 1; }

struct MvArgs {
  uint64_t seed;
  int64_t first, N, blocks_per_particle;     // R / 4 of the stream's stride
  double* state;                             // [R][N][D]
  float* mirror;                             // [R][N][D]: the state rounded, what the pair pass reads
  const double* pairs;                       // the pair pass's workspace (IaPairLayout)
  double* pos;                               // [S][R][N][D] or null
  int64_t force_off;
  int32_t P, R;
  double h, sdn, kappa, cv, cf, inv_nm1;
  float a;
  FpStats st;
};

// The start: x = sqrt(var0) z from the first D elements of the particle's stream, or the given x0; state and mirror
template <int D>
__global__ __launch_bounds__(FP_CHUNK) void mv_init_kernel(const MvArgs p, const double* __restrict__ x0, double sd0) {
  const int r = (int)blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * FP_CHUNK + (int64_t)threadIdx.x;
  if (i >= p.N) return;
  const int64_t g = (int64_t)r * p.N + i;
  NormalWalk w = NormalWalk::at(p.seed, (uint64_t)(p.first + g) * (uint64_t)p.blocks_per_particle, 0);
  double x[D];
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = sd0 * w.next();
  if (x0) {
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = x0[g * D + d];
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    p.state[g * D + d] = x[d];
    p.mirror[g * D + d] = (float)x[d];
  }
}

// Step k of replica blockIdx.y, chunk blockIdx.x, after the pair pass over the mirror of step k's positions.
// si >= 0: step k is snapshot si; advance: step k is not the last snapshot.
template <int D, int DRIFT>
__global__ __launch_bounds__(FP_CHUNK) void mv_step_kernel(const MvArgs p, int64_t k, int si, bool advance) {
  __shared__ double s_part[FP_WAVES * mv_terms(D)];
  const int r = (int)blockIdx.y;
  const int64_t chunk = blockIdx.x;
  const int64_t i = chunk * FP_CHUNK + (int64_t)threadIdx.x;
  const bool live = i < p.N;
  const int64_t g = (int64_t)r * p.N + i;
  double x[D];
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = live ? p.state[g * D + d] : 0.0;
  if (si >= 0) {
    double wsum = 0.0;
    if (live) {
      const double* part = p.pairs + (int64_t)r * p.P * p.N + i;
      wsum = part[0];
      for (int s = 1; s < p.P; ++s) wsum += part[(int64_t)s * p.N];
      if (p.pos) {
#pragma unroll
        for (int d = 0; d < D; ++d) p.pos[(((int64_t)si * p.R + r) * p.N + i) * D + d] = x[d];
      }
    }
    fp_accumulate<D, 1>(x, live, si, (int64_t)si * p.R + r, chunk, p.st, s_part, p.cv * wsum);
  }
  if (!advance || !live) return;
  double G[D];
  const double* gpart = p.pairs + p.force_off + ((int64_t)r * p.P * p.N + i) * D;
#pragma unroll
  for (int d = 0; d < D; ++d) G[d] = gpart[d];
  for (int s = 1; s < p.P; ++s) {
#pragma unroll
    for (int d = 0; d < D; ++d) G[d] += gpart[(int64_t)s * p.N * D + d];
  }
  NormalWalk w = NormalWalk::at(p.seed, (uint64_t)(p.first + g) * (uint64_t)p.blocks_per_particle, (k + 1) * D);
  double xn[D];
  const auto at = [&](int d) { return x[d]; };
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double v = fma(-p.kappa, (p.cf * G[d]) * p.inv_nm1, drift_field<double>(at, d, DRIFT, p.a));
    xn[d] = fma(p.h, v, x[d]);
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double xd = fma(p.sdn, w.next(), xn[d]);
    p.state[g * D + d] = xd;
    p.mirror[g * D + d] = (float)xd;
  }
}

struct MvStep {
  int64_t k;
  int si;
  bool advance;
};

template <int D, int DRIFT> void mv_launch(dim3 grid, hipStream_t st, const MvArgs& a, const MvStep& s) {
  hipLaunchKernelGGL((mv_step_kernel<D, DRIFT>), grid, dim3(FP_CHUNK), 0, st, a, s.k, s.si, s.advance);
}
template <int D> void mv_launch_drift(int drift, dim3 grid, hipStream_t st, const MvArgs& a, const MvStep& s) {
  if (drift == CNF_DRIFT_OU) mv_launch<D, CNF_DRIFT_OU>(grid, st, a, s);
  if constexpr (D == 2) {
    if (drift == CNF_DRIFT_SMILE) mv_launch<2, CNF_DRIFT_SMILE>(grid, st, a, s);
    if (drift == CNF_DRIFT_NONGRADIENT) mv_launch<2, CNF_DRIFT_NONGRADIENT>(grid, st, a, s);
  }
  if constexpr (D == 3) {
    if (drift == CNF_DRIFT_LORENZ) mv_launch<3, CNF_DRIFT_LORENZ>(grid, st, a, s);
  }
}
template <int D = 1> void mv_step_dim(int dim, int drift, dim3 grid, hipStream_t st, const MvArgs& a, const MvStep& s) {
  if (dim == D) mv_launch_drift<D>(drift, grid, st, a, s);
  else if constexpr (D < FP_MAX_D) mv_step_dim<D + 1>(dim, drift, grid, st, a, s);
}
template <int D = 1> void mv_init_dim(int dim, dim3 grid, hipStream_t st, const MvArgs& a, const double* x0, double sd0) {
  if (dim == D) hipLaunchKernelGGL((mv_init_kernel<D>), grid, dim3(FP_CHUNK), 0, st, a, x0, sd0);
  else if constexpr (D < FP_MAX_D) mv_init_dim<D + 1>(dim, grid, st, a, x0, sd0);
}

bool mv_shape_ok(int32_t R, int64_t N, int32_t D, int32_t S) {
  return R >= 1 && R <= MV_MAX_R && N >= 2 && N <= MV_MAX_N && D >= 1 && D <= FP_MAX_D && S >= 1 && S <= FP_MAX_S;
}

// Workspace, in bytes: the pair pass's partials, then the chunks' partials [S R][K][chunks] (doubles), then the mirror
struct MvLayout {
  int64_t pair_bytes, partial_bytes, mirror_bytes;
  int64_t total() const { return pair_bytes + partial_bytes + mirror_bytes; }
};
bool mv_layout(int32_t R, int64_t N, int32_t D, int32_t S, MvLayout* l) {
  if (cnf_interaction_workspace(R, N, 0, D, 1, &l->pair_bytes) != CNF_OK) return false;
  l->partial_bytes = (int64_t)S * R * mv_terms(D) * fp_chunks(N) * (int64_t)sizeof(double);
  l->mirror_bytes = (R * N * D * (int64_t)sizeof(float) + 7) / 8 * 8;
  return true;
}

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_mv_particles_workspace(int32_t R, int64_t N, int32_t D, int32_t S, int64_t* bytes) {
  MvLayout l{};
  if (!bytes || !mv_shape_ok(R, N, D, S) || !mv_layout(R, N, D, S, &l)) return CNF_ERR_INVALID;
  *bytes = l.total();
  return CNF_OK;
}

extern "C" int cnf_mv_particles(const CnfInteractionSpec* spec, double kappa, int32_t drift, int32_t D, float a,
                                double sigma, double h, int64_t n_steps, double var0, uint64_t seed,
                                int64_t first_particle, int32_t R, int64_t N, const double* x0,
                                const int64_t* snap_step, int32_t S, const CnfFieldGrid* grid, double* state,
                                double* pos, double* sums, uint32_t* hist, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  if (!spec || !state || !sums || !workspace || !mv_shape_ok(R, N, D, S) || !std::isfinite(kappa))
    return CNF_ERR_INVALID;
  if (!drift_ok(drift, D)) return CNF_ERR_INVALID;
  MvArgs args{};
  if (!fp_run_ok(D, a, sigma, h, n_steps, var0, first_particle, (int64_t)R * N, snap_step, S, &args.blocks_per_particle))
    return CNF_ERR_INVALID;
  MvLayout l{};
  if (!mv_layout(R, N, D, S, &l) || workspace_bytes < l.total()) return CNF_ERR_INVALID;
  IaPairLayout lay{};
  hipStream_t st = (hipStream_t)stream;
  if (interaction_pairs(spec, R, nullptr, N, nullptr, 0, D, true, nullptr, 0, st, &lay) != CNF_OK) return CNF_ERR_INVALID;
  args.st.n_chunks = fp_chunks(N);
  args.st.partial = (double*)((char*)workspace + l.pair_bytes);
  if (!fp_hist_of(D, grid, hist, &args.st)) return CNF_ERR_INVALID;
  args.seed = seed;
  args.first = first_particle;
  args.N = N;
  args.state = state;
  args.mirror = (float*)((char*)workspace + l.pair_bytes + l.partial_bytes);
  args.pairs = (const double*)workspace;
  args.pos = pos;
  args.force_off = lay.force_off;
  args.P = lay.P;
  args.R = R;
  args.h = h;
  args.sdn = std::sqrt(2.0 * sigma * h);
  args.kappa = kappa;
  args.cv = lay.cv;
  args.cf = lay.cf;
  args.inv_nm1 = 1.0 / (double)(N - 1);
  args.a = a;
  int rc = fp_clear_hist(args.st, S, st);
  if (rc != CNF_OK) return rc;
  const dim3 chunks((unsigned)args.st.n_chunks, (unsigned)R);
  mv_init_dim(D, chunks, st, args, x0, std::sqrt(var0));
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  const int64_t last = snap_step[S - 1];
  int si = 0;
  for (int64_t k = 0; k <= last; ++k) {
    const bool advance = k < last;
    rc = interaction_pairs(spec, R, args.mirror, N, nullptr, 0, D, advance, workspace, l.pair_bytes, st, &lay);
    if (rc != CNF_OK) return rc;
    const bool snap = snap_step[si] == k;
    mv_step_dim(D, drift, chunks, st, args, MvStep{k, snap ? si : -1, advance});
    if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
    if (snap) ++si;
  }
  return fp_finish_sums(args.st, S * R * mv_terms(D), sums, st);
}
