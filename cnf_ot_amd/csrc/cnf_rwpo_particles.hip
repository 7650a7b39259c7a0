// cnf_rwpo_particles.hip -- a particle reference for the rwpo problems at any dimension: the Hopf-Cole formula read as
// an expectation (the reference's cost_rwpo, cnf_ot/mfc/solvers.py:190-220, is its nested Monte-Carlo at dim 2).
// With eps = 1 / beta the optimal path measure is Brownian motion of variance 2 eps t started from rho0 = N(0, var0 I),
// reweighted by exp(-g(X_T) / (2 eps)) / h(X_0), h(y) = E exp(-g(y + sqrt(2 eps T) xi) / (2 eps)):
//   the optimal energy is -2 eps E log h;  X_T given X_0 = y is the weighted inner ensemble;  the path between the two
//   endpoints is a Brownian bridge;  the control at time 0 is (E[X_T | y] - y) / T.
// Everything is float64; g is potential<false, double> (cnf_terms.h: the one definition).  The inner draws come from a
// symmetric two-centre Gaussian proposal  z = shrink y +- m + sqrt(prop_var) xi  and are weighted by target / proposal,
// so that wells far from y keep an effective sample at dim > 3.  No draw reaches memory.
//
// Global particle p owns R = 4 (BY + K BD + ceil(S D / 4)) elements of the cnf_fill_normal stream from p R:
// BY = ceil(D / 4) blocks for y, BD = ceil((D + 1) / 4) blocks per inner draw (xi [D], then the sign normal), then
// S D elements for the bridges.  Every draw starts on a Philox block boundary and is a function of (seed, p, k) alone.
//
// rwpo_inner_kernel: one wave per outer particle, draw k on lane k mod 64.  Pass 1 keeps an online (max, sum, sum of
// squares, sum of w z) per lane, brings the lanes to the wave's maximum and adds them by the fixed butterfly.  Pass 2
// (with u) regenerates the draws by counter, scans exp(l - max) over the lanes of a round in ascending k, carries the
// rounds' running sum and takes the first k whose cumulative sum exceeds u times pass 1's total; the lane that holds it
// writes z* to the workspace.  Both loops run ceil(K / 64) rounds whatever the data.
// rwpo_bridge_kernel: one particle per lane, chunks of FP_CHUNK as cnf_fp_particles: y again from the stream, the
// bridge to z* through the snapshot times, the statistics through fp_accumulate.  The partition is by particle index
// and every per-particle output depends on (seed, p) alone: repeats and splits reproduce it bit for bit.
#include "cnf_fp_stats.h"

#include <algorithm>

namespace cnf {
namespace {

constexpr int64_t RW_MAX_N = int64_t(1) << 31;
constexpr int64_t RW_MAX_K = int64_t(1) << 20;
constexpr int RW_WAVES = 4;                   // outer particles per workgroup of the inner kernel

struct RwArgs {
  uint64_t seed;
  int64_t first, N, K;
  int64_t blocks_per_particle;                // R / 4
  const double* u;
  double *log_h, *ess, *mean_T, *zsel, *pos;
  int32_t* sel;
  double sd0, shrink, sdp;                    // sqrt(var0), sqrt(prop_var)
  double half_beta, inv_2s2, inv_2pv, const0; // beta / 2, 1 / (2 s^2), 1 / (2 prop_var), (D / 2) log(prop_var / s^2) + log 2
  double log_K;
  double centre[FP_MAX_D];
  float a;
  int32_t subtype, S, last_is_T;
  double bridge_c[FP_MAX_S], bridge_sd[FP_MAX_S];
  FpStats st;
};

__host__ __device__ constexpr int rw_blocks_y(int D) { return (D + 3) / 4; }
__host__ __device__ constexpr int rw_blocks_draw(int D) { return (D + 4) / 4; }

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// y = sqrt(var0) z from the particle's first BY blocks
template <int D>
__device__ __forceinline__ void rw_start(const RwArgs& p, uint64_t blk0, double (&y)[D]) {
  NormalWalk w{p.seed, blk0, {0.0f, 0.0f, 0.0f, 0.0f}, 0};
#pragma unroll
  for (int d = 0; d < D; ++d) y[d] = p.sd0 * w.next();
}

// Inner draw at block `blk`: z and its log-weight l = log(target / proposal) up to the constant log h's normalisation
// carries.  CENTRE = false: m = 0, the two proposal components coincide and their log-mean is the one Gaussian's.
template <int D, bool CENTRE>
__device__ __forceinline__ double rw_draw(const RwArgs& p, uint64_t blk, const double (&y)[D], const double (&mu)[D],
                                          double (&z)[D]) {
  constexpr int BD = rw_blocks_draw(D);
  float xi[4 * BD];
#pragma unroll
  for (int b = 0; b < BD; ++b) {
    float q[4];
    philox_normals4(p.seed, blk + b, q);
#pragma unroll
    for (int j = 0; j < 4; ++j) xi[4 * b + j] = q[j];
  }
  const double sg = xi[D] >= 0.0f ? 1.0 : -1.0;
  double dy2 = 0.0, qm = 0.0, qp = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double c = CENTRE ? fma(sg, p.centre[d], mu[d]) : mu[d];
    z[d] = fma(p.sdp, (double)xi[d], c);
    const double dy = z[d] - y[d], r = z[d] - mu[d];
    dy2 = fma(dy, dy, dy2);
    if constexpr (CENTRE) {
      const double rm = r - p.centre[d], rp = r + p.centre[d];
      qm = fma(rm, rm, qm);
      qp = fma(rp, rp, qp);
    } else {
      qm = fma(r, r, qm);
    }
  }
  const auto at = [&](int d) { return z[d]; };
  const double g = potential<false, double>(at, D, p.subtype, p.a).v;
  double lae;                                 // logaddexp of the two components' exponents, less log 2 when they coincide
  if constexpr (CENTRE) {
    const double A = -qm * p.inv_2pv, B = -qp * p.inv_2pv;
    lae = fmax(A, B) + log1p(exp(-fabs(A - B)));
    return ((p.const0 - p.half_beta * g) - p.inv_2s2 * dy2) - lae;
  } else {
    lae = -qm * p.inv_2pv;                    // (log 2 cancels: const0 carries it, so it is taken out again)
    return (((p.const0 - 0.6931471805599453094) - p.half_beta * g) - p.inv_2s2 * dy2) - lae;
  }
}

template <int D, bool CENTRE>
__global__ __launch_bounds__(64 * RW_WAVES) void rwpo_inner_kernel(const RwArgs p) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  constexpr int BY = rw_blocks_y(D), BD = rw_blocks_draw(D);
  const int64_t rounds = (p.K + 63) >> 6;
  for (int64_t i = (int64_t)blockIdx.x * RW_WAVES + wave; i < p.N; i += (int64_t)gridDim.x * RW_WAVES) {
    const uint64_t blk0 = (uint64_t)(p.first + i) * (uint64_t)p.blocks_per_particle;
    const uint64_t blkd = blk0 + BY;
    double y[D], mu[D], z[D];
    rw_start<D>(p, blk0, y);
#pragma unroll
    for (int d = 0; d < D; ++d) mu[d] = p.shrink * y[d];
    // pass 1: this lane's draws as (m, sum exp(l - m), sum exp(2 (l - m)), sum exp(l - m) z)
    double m = -INFINITY, s = 0.0, s2 = 0.0, sz[D];
#pragma unroll
    for (int d = 0; d < D; ++d) sz[d] = 0.0;
    for (int64_t r = 0; r < rounds; ++r) {
      const int64_t k = (r << 6) + lane;
      if (k < p.K) {
        const double l = rw_draw<D, CENTRE>(p, blkd + (uint64_t)k * BD, y, mu, z);
        const double dl = l - m, e = exp(-fabs(dl));
        const bool up = dl > 0.0;
        const double scale = up ? e : 1.0, w = up ? 1.0 : e;
        s = fma(s, scale, w);
        s2 = fma(s2, scale * scale, w * w);
#pragma unroll
        for (int d = 0; d < D; ++d) sz[d] = fma(sz[d], scale, w * z[d]);
        m = up ? l : m;
      }
    }
    const double M = wave_max(m);
    const double f = exp(m - M);              // (a lane without a draw: m = -inf, f = 0, its sums are 0)
    const double tot = wave_sum(s * f), tot2 = wave_sum(s2 * (f * f));
    if (p.mean_T) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double v = wave_sum(sz[d] * f);
        if (lane == 0) p.mean_T[i * D + d] = v / tot;
      }
    }
    if (lane == 0) {
      if (p.log_h) p.log_h[i] = (M + log(tot)) - p.log_K;
      if (p.ess) p.ess[i] = tot * tot / tot2;
    }
    if (!p.u) continue;
    // pass 2: the first k whose cumulative sum of exp(l - M), ascending, exceeds u tot
    const double thr = p.u[i] * tot;
    double run = 0.0;
    bool found = false;
    int32_t pick = (int32_t)(p.K - 1);
    for (int64_t r = 0; r < rounds; ++r) {
      const int64_t k = (r << 6) + lane;
      const bool valid = k < p.K;
      double v = 0.0;
      if (valid) v = exp(rw_draw<D, CENTRE>(p, blkd + (uint64_t)k * BD, y, mu, z) - M);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o);
        if (lane >= o) v += t;
      }
      const uint64_t hit = __ballot(valid && run + v > thr);
      if (!found && hit != 0) {
        const int who = __builtin_ctzll(hit);
        pick = (int32_t)((r << 6) + who);
        found = true;
        if (lane == who && p.zsel) {
#pragma unroll
          for (int d = 0; d < D; ++d) p.zsel[i * D + d] = z[d];
        }
      }
      run += __shfl(v, 63);
    }
    if (!found) {                             // (rounding left the last cumulative sum at or under u tot: the last draw)
      (void)rw_draw<D, CENTRE>(p, blkd + (uint64_t)(p.K - 1) * BD, y, mu, z);
      if (lane == 0 && p.zsel) {
#pragma unroll
        for (int d = 0; d < D; ++d) p.zsel[i * D + d] = z[d];
      }
    }
    if (lane == 0 && p.sel) p.sel[i] = pick;
  }
}

// The Brownian bridge from (0, y) to (T, z*) through the snapshot times: snapshot s draws its own D normals
template <int D>
__global__ __launch_bounds__(FP_CHUNK) void rwpo_bridge_kernel(const RwArgs p) {
  __shared__ double s_part[FP_WAVES * fp_terms(D)];
  constexpr int BY = rw_blocks_y(D), BD = rw_blocks_draw(D);
  for (int64_t chunk = blockIdx.x; chunk < p.st.n_chunks; chunk += gridDim.x) {
    const int64_t i = chunk * FP_CHUNK + (int64_t)threadIdx.x;
    const bool live = i < p.N;
    const uint64_t blk0 = (uint64_t)(p.first + i) * (uint64_t)p.blocks_per_particle;
    double x[D], zs[D];
    rw_start<D>(p, blk0, x);
#pragma unroll
    for (int d = 0; d < D; ++d) zs[d] = live ? p.zsel[i * D + d] : 0.0;
    NormalWalk w = NormalWalk::at(p.seed, blk0 + BY + (uint64_t)p.K * BD, 0);
    for (int s = 0; s < p.S; ++s) {
      const double c = p.bridge_c[s], sd = p.bridge_sd[s];
      const bool exact = p.last_is_T && s == p.S - 1;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double zeta = w.next();
        const double v = fma(sd, zeta, fma(c, zs[d] - x[d], x[d]));
        x[d] = exact ? zs[d] : v;
      }
      if (p.pos && live) {
#pragma unroll
        for (int d = 0; d < D; ++d) p.pos[((int64_t)s * p.N + i) * D + d] = x[d];
      }
      fp_accumulate<D>(x, live, s, s, chunk, p.st, s_part);
    }
  }
}

template <int D> void rw_launch(bool centre, bool bridge, unsigned grid, hipStream_t st, const RwArgs& a) {
  if (bridge) hipLaunchKernelGGL((rwpo_bridge_kernel<D>), dim3(grid), dim3(FP_CHUNK), 0, st, a);
  else if (centre) hipLaunchKernelGGL((rwpo_inner_kernel<D, true>), dim3(grid), dim3(64 * RW_WAVES), 0, st, a);
  else hipLaunchKernelGGL((rwpo_inner_kernel<D, false>), dim3(grid), dim3(64 * RW_WAVES), 0, st, a);
}

template <int D = 1> void rw_with_dim(int dim, bool centre, bool bridge, unsigned grid, hipStream_t st, const RwArgs& a) {
  if (dim == D) rw_launch<D>(centre, bridge, grid, st, a);
  else if constexpr (D < FP_MAX_D) rw_with_dim<D + 1>(dim, centre, bridge, grid, st, a);
}

bool rw_shape_ok(int64_t N, int32_t D, int32_t S) {
  return N >= 1 && N <= RW_MAX_N && D >= 1 && D <= FP_MAX_D && S >= 0 && S <= FP_MAX_S;
}
int64_t rw_partial_bytes(int64_t N, int32_t D, int32_t S) {
  return (int64_t)S * fp_terms(D) * fp_chunks(N) * (int64_t)sizeof(double);
}
int64_t rw_workspace_bytes(int64_t N, int32_t D, int32_t S) {
  return rw_partial_bytes(N, D, S) + N * D * (int64_t)sizeof(double);
}
bool rw_pos_finite(double v) { return v > 0.0 && std::isfinite(v); }

}  // namespace
}  // namespace cnf

using namespace cnf;

extern "C" int cnf_rwpo_particles_workspace(int64_t N, int32_t D, int32_t S, int64_t* bytes) {
  if (!bytes || !rw_shape_ok(N, D, S)) return CNF_ERR_INVALID;
  *bytes = rw_workspace_bytes(N, D, S);
  return CNF_OK;
}

extern "C" int cnf_rwpo_particles(int32_t subtype, int32_t D, float a, double T, double beta, double var0, double shrink,
                                  double prop_var, const double* centre, int64_t K, uint64_t seed, int64_t first_particle,
                                  int64_t N, const double* u, const double* times, int32_t S, const CnfFieldGrid* grid,
                                  double* log_h, double* ess, double* mean_T, int32_t* sel, double* pos, double* sums,
                                  uint32_t* hist, void* workspace, int64_t workspace_bytes, void* stream) {
  if (subtype < CNF_POT_QUADRATIC || subtype > CNF_POT_OBSTACLE || !rw_shape_ok(N, D, S)) return CNF_ERR_INVALID;
  if (!rw_pos_finite(T) || !rw_pos_finite(beta) || !rw_pos_finite(var0) || !rw_pos_finite(prop_var) ||
      !std::isfinite(shrink) || !std::isfinite(a))
    return CNF_ERR_INVALID;
  if (K < 1 || K > RW_MAX_K || first_particle < 0) return CNF_ERR_INVALID;
  const bool path = pos || sums || hist;
  if (!path && !log_h && !ess && !mean_T && !sel) return CNF_ERR_INVALID;
  if ((path && S < 1) || ((path || sel) && !u)) return CNF_ERR_INVALID;
  if (S > 0 && !times) return CNF_ERR_INVALID;
  for (int32_t s = 0; s < S; ++s)
    if (!std::isfinite(times[s]) || times[s] < 0.0 || times[s] > T || (s > 0 && times[s] <= times[s - 1]))
      return CNF_ERR_INVALID;
  bool has_centre = false;
  if (centre)
    for (int32_t d = 0; d < D; ++d) {
      if (!std::isfinite(centre[d])) return CNF_ERR_INVALID;
      has_centre = has_centre || centre[d] != 0.0;
    }
  const int64_t per_particle = rw_blocks_y(D) + K * rw_blocks_draw(D) + ((int64_t)S * D + 3) / 4;      // R / 4
  if (first_particle > INT64_MAX - N || (first_particle + N) > (INT64_MAX / 4) / per_particle)
    return CNF_ERR_INVALID;                                         // the element index fits
  RwArgs args{};
  args.st.n_chunks = fp_chunks(N);
  if (path) {
    if (!workspace || workspace_bytes < rw_workspace_bytes(N, D, S)) return CNF_ERR_INVALID;
    if (sums) args.st.partial = (double*)workspace;
    args.zsel = (double*)((char*)workspace + rw_partial_bytes(N, D, S));
    if (!fp_hist_of(D, grid, hist, &args.st)) return CNF_ERR_INVALID;
  }
  const double s2 = 2.0 * T / beta;
  args.seed = seed;
  args.first = first_particle;
  args.N = N;
  args.K = K;
  args.blocks_per_particle = per_particle;
  args.u = u;
  args.log_h = log_h;
  args.ess = ess;
  args.mean_T = mean_T;
  args.sel = sel;
  args.pos = pos;
  args.sd0 = std::sqrt(var0);
  args.shrink = shrink;
  args.sdp = std::sqrt(prop_var);
  args.half_beta = beta / 2.0;
  args.inv_2s2 = 1.0 / (2.0 * s2);
  args.inv_2pv = 1.0 / (2.0 * prop_var);
  args.const0 = 0.5 * D * std::log(prop_var / s2) + 0.6931471805599453094;
  args.log_K = std::log((double)K);
  for (int32_t d = 0; d < D; ++d) args.centre[d] = centre ? centre[d] : 0.0;
  args.a = a;
  args.subtype = subtype;
  args.S = S;
  if (path) {
    double prev = 0.0;
    for (int32_t s = 0; s < S; ++s) {
      const double t = times[s];
      if (t == T) {                           // (the last snapshot: z* itself)
        args.bridge_c[s] = 1.0;
        args.bridge_sd[s] = 0.0;
        args.last_is_T = 1;
      } else {
        args.bridge_c[s] = (t - prev) / (T - prev);
        args.bridge_sd[s] = std::sqrt(2.0 / beta * (t - prev) * (T - t) / (T - prev));
      }
      prev = t;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  int rc = fp_clear_hist(args.st, S, st);
  if (rc != CNF_OK) return rc;
  const unsigned inner_grid = (unsigned)std::min<int64_t>((N + RW_WAVES - 1) / RW_WAVES, int64_t(1) << 20);
  rw_with_dim(D, has_centre, false, inner_grid, st, args);
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  if (!path) return CNF_OK;
  const unsigned bridge_grid = (unsigned)std::min<int64_t>(args.st.n_chunks, int64_t(1) << 20);
  rw_with_dim(D, has_centre, true, bridge_grid, st, args);
  if (hipGetLastError() != hipSuccess) return CNF_ERR_HIP;
  return fp_finish_sums(args.st, S * fp_terms(D), sums, st);
}
