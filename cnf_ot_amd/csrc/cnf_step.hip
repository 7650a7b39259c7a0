// cnf_step.hip -- the training step's model-free kernels: the Adam update (`optax.adam` in
// cnf_ot/mfc/solvers.py:90-97), the weighted sum of a composite loss's term sums, and the residual
// kernels of the loss terms that are composed from separate flow launches (score, kinetic / potential / -log_prob,
// reverse KL): what `jax.value_and_grad` differentiates around the flow in the reference's loss functions.
// No entry point here takes a CnfModel; every one rejects bad arguments before it touches a device.
#include "cnf_host.h"

#include <math.h>

namespace cnf {

// optax.adam(lr): mu = b1 mu + (1-b1) g; nu = b2 nu + (1-b2) g^2;
// update = -lr * (mu / (1-b1^t)) / (sqrt(nu / (1-b2^t)) + eps)   (eps_root = 0)
__global__ void adam_kernel(float* __restrict__ params, const float* __restrict__ grad, float* __restrict__ mu,
                            float* __restrict__ nu, int64_t n, float lr, float b1, float b2, float eps,
                            float bc1, float bc2) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float g = grad[i];
  const float m = b1 * mu[i] + (1.0f - b1) * g;
  const float v = b2 * nu[i] + (1.0f - b2) * g * g;
  mu[i] = m; nu[i] = v;
  params[i] -= lr * (m / bc1) / (sqrtf(v / bc2) + eps);
}

// The same update with the step count read from device memory (state[0] of cnf_step_begin, already incremented for
// this step): the bias corrections cannot be kernel arguments of a step that is captured once and replayed
__global__ void adam_dev_kernel(float* __restrict__ params, const float* __restrict__ grad, float* __restrict__ mu,
                                float* __restrict__ nu, int64_t n, float lr, float b1, float b2, float eps,
                                const uint64_t* __restrict__ state) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float step = (float)state[0];
  const float bc1 = 1.0f - powf(b1, step), bc2 = 1.0f - powf(b2, step);
  const float g = grad[i];
  const float m = b1 * mu[i] + (1.0f - b1) * g;
  const float v = b2 * nu[i] + (1.0f - b2) * g * g;
  mu[i] = m; nu[i] = v;
  params[i] -= lr * (m / bc1) / (sqrtf(v / bc2) + eps);
}

// out[0] = sum_i v[i] w[i]: the composite loss from the terms' per-slice sums and their coefficients, in a fixed order
__global__ __launch_bounds__(256) void weighted_sum_kernel(const double* __restrict__ v, const double* __restrict__ w,
                                                           int64_t n, double* __restrict__ out) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += v[i] * w[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) part[threadIdx.x] += part[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = part[0];
}

// ---------------------------------------------------------------------------
// Epilogues of the UNFUSED loss terms (dim >= applications.UNFUSED_SCORE_MIN_DIM: the flow passes are separate,
// chip-filling launches; these turn their outputs into per-slice sums and, for value_and_grad, into the adjoints
// the backward launches start from).  One thread per sample.
// ---------------------------------------------------------------------------
struct ResidArgs {
  const float* r;        // [3 n, D]: r1 (t - dt/2) | r2 (t + dt/2) | r3 (t)
  const float* score;    // [n, D] central-difference score of log_prob at r3
  float* rbar;           // [3 n, D] or null
  float* sbar;           // [n, D] or null
  double* sums;          // [n / count]
  int64_t n, count;
  int32_t D, subtype;    // subtype < 0: no drift (kinetic_with_score), else CnfDrift
  float inv_dt, coef, a, loss_coef;
  const float* force;    // [n, D]: an interaction force at r3, or null (FORCE instantiation alone reads the three)
  float* fbar;           // [n, D] or null
  float strength;
};

// sum_d ((r2 - r1)/dt + coef score_d - drift_d(r3))^2 per slice (applications.py:245-374) and its adjoints.  FORCE:
// u gains strength * force_d (the interacting Fokker-Planck residual) and fbar = strength * u_bar leaves with the rest
template <bool FORCE>
__global__ __launch_bounds__(256) void score_residual_kernel(const ResidArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int D = a.D;
  float acc = 0.0f;
  const bool valid = i < a.n;
  if (valid) {
    const float* r1 = a.r + i * D;
    const float* r2 = a.r + (a.n + i) * D;
    const float* r3 = a.r + (2 * a.n + i) * D;
    const float* sc = a.score + i * D;
    float* r3b = a.rbar + (2 * a.n + i) * D;
    const bool ou = a.subtype == CNF_DRIFT_OU;
    // the coupled 2-D / 3-D fields' coordinates and u_bar, in registers (read before any store: rbar may alias r)
    const float x = r3[0], y = D > 1 ? r3[1] : 0.0f, z = D > 2 ? r3[2] : 0.0f;
    const auto r = [&](int e) { return e == 0 ? x : (e == 1 ? y : z); };
    float ub0 = 0.f, ub1 = 0.f, ub2 = 0.f;
    for (int d = 0; d < D; ++d) {
      const float drift = ou ? ou_drift(r3[d], a.a) : drift_field<float>(r, d, a.subtype, a.a);
      float u = score_residual((r2[d] - r1[d]) * a.inv_dt, sc[d], a.coef, drift);
      if constexpr (FORCE) u = fmaf(a.strength, a.force[i * D + d], u);
      acc = fmaf(u, u, acc);
      if (a.rbar) {
        const float ub = score_residual_bar(u, a.loss_coef);
        if constexpr (FORCE) a.fbar[i * D + d] = a.strength * ub;
        a.rbar[i * D + d] = -ub * a.inv_dt;
        a.rbar[(a.n + i) * D + d] = ub * a.inv_dt;
        a.sbar[i * D + d] = a.coef * ub;
        if (d == 0) ub0 = ub; else if (d == 1) ub1 = ub; else if (d == 2) ub2 = ub;
        r3b[d] = ou ? ou_drift_adjoint(ub, a.a) : 0.0f;      // complete for OU and no drift; the coupled fields below
      }
    }
    if (a.rbar && a.subtype > CNF_DRIFT_OU)
      drift_adjoint(r, [&](int e) { return e == 0 ? ub0 : (e == 1 ? ub1 : ub2); }, D, a.subtype, a.a,
                    [&](int e, float b) { r3b[e] = b; });
  }
  // a wave whose samples share a slice: shuffle reduce, one double atomic; otherwise one atomic per sample
  const int64_t slice = valid ? i / a.count : -1;
  const int64_t s0 = __shfl(slice, 0, 64), s63 = __shfl(slice, 63, 64);
  if (s0 == s63 && s0 >= 0) {
    float part = acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(a.sums + s0, (double)part);
  } else if (valid) {
    atomicAdd(a.sums + slice, (double)acc);
  }
}

// Value and adjoints of the terms cnf_ot_amd.applications composes from table launches at dim 2 (5.4b): one thread
// per sample, per-slice sums like score_residual_kernel.
//   CNF_TERM_KINETIC:      r = [r1 | r2] (2 n points), sums[s] = sum |(r2 - r1) / dt|^2, rbar = -+ 2 c (r2 - r1) / dt^2
//   CNF_TERM_POTENTIAL:    r (n points), sums[s] = sum V(r), rbar = c grad V(r)            (CnfPotential subtype, a)
//   CNF_TERM_NEG_LOGPROB:  r = recovered base points x, aux = ildj: sums[s] = -sum (base(x) + ildj), rbar = c x,
//                          auxbar = -c
struct TermResidArgs {
  const float* r; const float* aux; float* rbar; float* auxbar; double* sums;
  int64_t n, count;
  int32_t kind, D, subtype;
  float p0, loss_coef;
  uint32_t* amax;      // non-null (DFIX = 2, rbar written): [0] max |rbar| as bits, [1] non-finite flag -- what adjoint_max_kernel
};                     // would find in rbar afterwards (cnf_kinetic_potential_vjp)

// DFIX = 2: the points are float2 -- one 8-byte load / store per point instead of a strided loop.
// The kernel is a stream of independent 8-byte accesses: 1 024-thread workgroups, RESID_PER points per thread a
// workgroup-width apart (one point per thread left the chip waiting on workgroup launches: 49 us for 4.2 M points,
// twice the time of the memory traffic).  The sums: a lane adds up its points of the wave's current slice; when the
// slice changes the wave flushes (shuffles + one double atomic); at the end lanes -> wave -> workgroup (LDS) -> ONE
// atomic per run of equal slices in the workgroup.  (One atomic per wave put 65 536 of them on the single address of
// a 4.2 M-sample slice and took longer than the flow kernels around it.)
constexpr int RESID_PER = 4;
template <int DFIX>
__global__ __launch_bounds__(1024) void term_residual_kernel(const TermResidArgs a) {
  const int D = DFIX ? DFIX : a.D;
  __shared__ double wsum[16];
  __shared__ long long wslice[16];
  uint32_t amx = 0, abad = 0;
  auto seen = [&](v2f gbar) {
    const uint32_t bx = __float_as_uint(gbar.x) & 0x7fffffffu, by = __float_as_uint(gbar.y) & 0x7fffffffu;
    const uint32_t b = bx > by ? bx : by;
    abad |= b >= 0x7f800000u ? 1u : 0u;
    amx = (b > amx && b < 0x7f800000u) ? b : amx;
  };
  auto term = [&](int64_t i) -> float {      // the term's value at point i; writes the adjoints
    float v = 0.0f;
    const auto pt = [&](int d) { return a.r[i * D + d]; };
    if (DFIX == 2) {
      const v2f* r2p = reinterpret_cast<const v2f*>(a.r);
      v2f* rb2 = reinterpret_cast<v2f*>(a.rbar);
      if (a.kind == CNF_TERM_KINETIC) {
        const float inv_dt = 1.0f / a.p0, g = 2.0f * a.loss_coef * inv_dt * inv_dt;
        const v2f dr = r2p[a.n + i] - r2p[i];
        const v2f w = dr * inv_dt;
        v = fmaf(w.x, w.x, w.y * w.y);
        if (a.rbar) { rb2[i] = dr * -g; rb2[a.n + i] = dr * g; if (a.amax) seen(dr * g); }
      } else if (a.kind == CNF_TERM_POTENTIAL) {
        const v2f x = r2p[i];
        const Potential<float> p = potential<false>(x, a.subtype, a.p0);
        const v2f gr = p.grad(x) * a.loss_coef;      // (formed beside the value: one branch on the subtype)
        v = p.v;
        if (a.rbar) { rb2[i] = gr; if (a.amax) seen(gr); }
      } else {      // CNF_TERM_NEG_LOGPROB
        const v2f x = r2p[i];
        if (a.rbar) rb2[i] = x * a.loss_coef;
        v = -base_logprob<float>([&](int e) { return e == 0 ? x.x : x.y; }, 2) - a.aux[i];
        if (a.auxbar) a.auxbar[i] = -a.loss_coef;
      }
    } else {
      if (a.kind == CNF_TERM_KINETIC) {
        const float inv_dt = 1.0f / a.p0, g = 2.0f * a.loss_coef * inv_dt * inv_dt;
        for (int d = 0; d < D; ++d) {
          const float dr = a.r[(a.n + i) * D + d] - a.r[i * D + d];
          const float w = dr * inv_dt;
          v = fmaf(w, w, v);
          if (a.rbar) { a.rbar[i * D + d] = -g * dr; a.rbar[(a.n + i) * D + d] = g * dr; }
        }
      } else if (a.kind == CNF_TERM_POTENTIAL) {
        const Potential<float> p = potential<false, float>(pt, D, a.subtype, a.p0);
        v = p.v;
        if (a.rbar)
          for (int d = 0; d < D; ++d) a.rbar[i * D + d] = a.loss_coef * p.grad(pt(d));
      } else {
        // (one read per coordinate: the accessor also writes its adjoint)
        v = -base_logprob<float>([&](int d) {
              const float x = pt(d);
              if (a.rbar) a.rbar[i * D + d] = a.loss_coef * x;
              return x;
            }, D) - a.aux[i];
        if (a.auxbar) a.auxbar[i] = -a.loss_coef;
      }
    }
    return v;
  };
  auto wave_sum = [](float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
  };
  const bool small = a.n < ((int64_t)1 << 31) && a.count < ((int64_t)1 << 31);      // 32-bit slice arithmetic
  const int64_t base = blockIdx.x * (int64_t)(blockDim.x * RESID_PER) + threadIdx.x;
  float acc = 0.0f;              // this lane's points of slice `cur`
  long long cur = -1;            // wave-uniform
#pragma unroll
  for (int it = 0; it < RESID_PER; ++it) {
    const int64_t i = base + (int64_t)it * blockDim.x;
    const bool valid = i < a.n;
    const float v = valid ? term(i) : 0.0f;
    const long long slice = !valid ? -1 : small ? (long long)((uint32_t)i / (uint32_t)a.count) : (long long)(i / a.count);
    const long long sl0 = __shfl(slice, 0, 64), sl63 = __shfl(slice, 63, 64);
    if (sl0 == sl63) {                      // (-1 == -1: a wave past the end, contributing nothing)
      if (sl0 != cur) {
        const float part = wave_sum(acc);
        if (cur >= 0 && (threadIdx.x & 63) == 0) unsafeAtomicAdd(a.sums + cur, (double)part);
        cur = sl0; acc = 0.0f;
      }
      acc += v;
    } else if (valid) {
      unsafeAtomicAdd(a.sums + slice, (double)v);      // a wave across a slice border: per lane
    }
  }
  __shared__ uint32_t wmax[16];
  if (DFIX == 2 && a.amax) {      // adjoint_max_kernel's result, without its pass over rbar
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(amx, off, 64); amx = o > amx ? o : amx; }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amx;
    if (__builtin_amdgcn_ballot_w64(abad != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(a.amax + 1, 1u);
  }
  const float part = wave_sum(acc);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wsum[wv] = (double)part; wslice[wv] = cur; }
  __syncthreads();
  if (DFIX == 2 && a.amax && threadIdx.x == 64) {
    // one atomic per workgroup, and none where the maximum on record is already as large (a wave's atomic each put
    // 130 000 of them on one address: +0.25 ms for config 5's kinetic + obstacle term)
    uint32_t mm = 0;
    for (int w2 = 0; w2 < (int)(blockDim.x >> 6); ++w2) mm = wmax[w2] > mm ? wmax[w2] : mm;
    if (mm > __hip_atomic_load(a.amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.amax, mm);
  }
  if (threadIdx.x == 0) {
    const int nw = blockDim.x >> 6;
    double run = 0.0;
    long long c2 = -1;
    for (int w2 = 0; w2 < nw; ++w2) {
      if (wslice[w2] != c2) { if (c2 >= 0) unsafeAtomicAdd(a.sums + c2, run); c2 = wslice[w2]; run = 0.0; }
      run += wsum[w2];
    }
    if (c2 >= 0) unsafeAtomicAdd(a.sums + c2, run);
  }
}

struct RklArgs {
  const float* y;        // [n, D] samples
  const float* lp;       // [n] their log_prob
  float* ybar;           // [n, D] or null
  float* lpbar;          // [n] or null
  double* sums;          // [1]
  int64_t n;
  int32_t D;
  float t, T, beta, loss_coef;
};

// sum_i log_prob_i - log(N(y_i; 0, vs I) ws + N(y_i; 0, vt I) wt)  (reverse_kl_loss_fn, applications.py:129-163)
__global__ __launch_bounds__(256) void rkl_residual_kernel(const RklArgs a) {
  // grid-stride with a running per-lane sum: one double atomic per wave at the END (one per 64 samples put 65 536
  // atomics on the single address of a 4 M-sample batch)
  float acc = 0.0f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int D = a.D;
    const RklMix<float> mix = rkl_mixture<false, float>([&](int d) { return a.y[i * D + d]; }, D, a.t, a.T, a.beta);
    acc += a.lp[i] - mix.logmix;
    if (a.ybar) {
      for (int d = 0; d < D; ++d) a.ybar[i * D + d] = a.loss_coef * mix.g * a.y[i * D + d];
      a.lpbar[i] = a.loss_coef;
    }
  }
  float part = acc;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(a.sums, (double)part);
}

}  // namespace cnf

using namespace cnf;

extern "C" int cnf_adam_step(float* params, const float* grad, float* mu, float* nu, int64_t n, float lr, float b1,
                             float b2, float eps, int64_t step, void* stream) {
  if (!params || !grad || !mu || !nu || n < 0 || step < 1) return CNF_ERR_INVALID;
  if (n == 0) return CNF_OK;
  const float bc1 = 1.0f - powf(b1, (float)step), bc2 = 1.0f - powf(b2, (float)step);
  return launch_plain(adam_kernel, (n + 255) / 256, 256, 0, (hipStream_t)stream, params, grad, mu, nu, n, lr, b1, b2,
                      eps, bc1, bc2);
}

extern "C" int cnf_adam_step_dev(float* params, const float* grad, float* mu, float* nu, int64_t n, float lr, float b1,
                                 float b2, float eps, const uint64_t* state, void* stream) {
  if (!params || !grad || !mu || !nu || !state || n < 0) return CNF_ERR_INVALID;
  if (n == 0) return CNF_OK;
  return launch_plain(adam_dev_kernel, (n + 255) / 256, 256, 0, (hipStream_t)stream, params, grad, mu, nu, n, lr, b1,
                      b2, eps, state);
}

extern "C" int cnf_weighted_sum(const double* v, const double* w, int64_t n, double* out, void* stream) {
  if (!v || !w || !out || n < 0) return CNF_ERR_INVALID;
  return launch_plain(weighted_sum_kernel, 1, 256, 0, (hipStream_t)stream, v, w, n, out);
}

extern "C" int cnf_score_residual(const float* r, const float* score, int64_t n, int64_t count, int32_t D, float dt,
                                  float coef, int32_t drift, float a_, float loss_coef, double* sums, float* rbar,
                                  float* sbar, void* stream_) {
  if (!r || !score || !sums || n < 0 || count < 1 || D < 1 || !(dt > 0.f) || (rbar == nullptr) != (sbar == nullptr))
    return CNF_ERR_INVALID;
  if (drift != -1 && !drift_ok(drift, D)) return CNF_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int todo = zero_sums(sums, (n + count - 1) / count, n, stream); todo <= 0) return todo;
  ResidArgs a;
  a.r = r; a.score = score; a.rbar = rbar; a.sbar = sbar; a.sums = sums; a.n = n; a.count = count;
  a.D = D; a.subtype = drift; a.inv_dt = 1.0f / dt; a.coef = coef; a.a = a_; a.loss_coef = loss_coef;
  a.force = nullptr; a.fbar = nullptr; a.strength = 0.0f;
  return launch_plain(score_residual_kernel<false>, (n + 255) / 256, 256, 0, stream, a);
}

extern "C" int cnf_score_residual_force(const float* r, const float* score, const float* force, float strength, int64_t n,
                                        int64_t count, int32_t D, float dt, float coef, int32_t drift, float a_,
                                        float loss_coef, double* sums, float* rbar, float* sbar, float* fbar,
                                        void* stream_) {
  if (!r || !score || !force || !sums || n < 0 || count < 1 || D < 1 || !(dt > 0.f) ||
      (rbar == nullptr) != (sbar == nullptr) || (rbar == nullptr) != (fbar == nullptr))
    return CNF_ERR_INVALID;
  if (drift != -1 && !drift_ok(drift, D)) return CNF_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int todo = zero_sums(sums, (n + count - 1) / count, n, stream); todo <= 0) return todo;
  ResidArgs a;
  a.r = r; a.score = score; a.rbar = rbar; a.sbar = sbar; a.sums = sums; a.n = n; a.count = count;
  a.D = D; a.subtype = drift; a.inv_dt = 1.0f / dt; a.coef = coef; a.a = a_; a.loss_coef = loss_coef;
  a.force = force; a.fbar = fbar; a.strength = strength;
  return launch_plain(score_residual_kernel<true>, (n + 255) / 256, 256, 0, stream, a);
}

// (cnf_host.h.  The float2 kernel where the points allow it: cnf_kinetic_potential_vjp's, 16-byte aligned, always do.)
int term_residual_launch(int32_t kind, const float* r, const float* aux, int64_t n, int64_t count, int32_t D,
                         int32_t subtype, float p0, float loss_coef, double* sums, float* rbar, float* auxbar,
                         uint32_t* amax, hipStream_t stream) {
  TermResidArgs a;
  a.r = r; a.aux = aux; a.rbar = rbar; a.auxbar = auxbar; a.sums = sums; a.n = n; a.count = count;
  a.kind = kind; a.D = D; a.subtype = subtype; a.p0 = p0; a.loss_coef = loss_coef; a.amax = amax;
  const int64_t blocks = (n + 1024 * RESID_PER - 1) / (1024 * RESID_PER);
  const bool vec2 = D == 2 && (reinterpret_cast<uintptr_t>(r) & 7) == 0 && (reinterpret_cast<uintptr_t>(rbar) & 7) == 0;
  if (amax && !vec2) return CNF_ERR_INVALID;      // (only the float2 kernel leaves the adjoint maximum)
  return launch_plain(vec2 ? term_residual_kernel<2> : term_residual_kernel<0>, blocks, 1024, 0, stream, a);
}

extern "C" int cnf_term_residual(int32_t kind, const float* r, const float* aux, int64_t n, int64_t count, int32_t D,
                                 int32_t subtype, float p0, float loss_coef, double* sums, float* rbar,
                                 float* auxbar, void* stream_) {
  if (!r || !sums || n < 0 || count < 1 || D < 1) return CNF_ERR_INVALID;
  if (kind != CNF_TERM_KINETIC && kind != CNF_TERM_POTENTIAL && kind != CNF_TERM_NEG_LOGPROB) return CNF_ERR_INVALID;
  if (kind == CNF_TERM_KINETIC && !(p0 > 0.f)) return CNF_ERR_INVALID;
  if (kind == CNF_TERM_POTENTIAL && !potential_ok(subtype)) return CNF_ERR_INVALID;
  if (kind == CNF_TERM_NEG_LOGPROB && !aux) return CNF_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int todo = zero_sums(sums, (n + count - 1) / count, n, stream); todo <= 0) return todo;
  return term_residual_launch(kind, r, aux, n, count, D, subtype, p0, loss_coef, sums, rbar, auxbar, nullptr, stream);
}

extern "C" int cnf_rkl_residual(const float* y, const float* lp, int64_t n, int32_t D, float t, float T, float beta,
                                float loss_coef, double* sum, float* ybar, float* lpbar, void* stream_) {
  if (!y || !lp || !sum || n < 0 || D < 1 || !(T > 0.f) || !(beta > 0.f) || (ybar == nullptr) != (lpbar == nullptr))
    return CNF_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  if (const int todo = zero_sums(sum, 1, n, stream); todo <= 0) return todo;
  RklArgs a;
  a.y = y; a.lp = lp; a.ybar = ybar; a.lpbar = lpbar; a.sums = sum; a.n = n; a.D = D;
  a.t = t; a.T = T; a.beta = beta; a.loss_coef = loss_coef;
  const int64_t blocks = (n + 255) / 256;
  return launch_plain(rkl_residual_kernel, blocks > 1024 ? 1024 : blocks, 256, 0, stream, a);
}
