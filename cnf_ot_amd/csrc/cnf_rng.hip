// cnf_rng.hip -- the random streams of libcnf_ot_amd.so as stand-alone fills: the Philox normal stream that the
// flow and loss kernels also draw in place (cnf_fill_normal), the JAX-compatible threefry draw, and the random inputs
// of a captured training step drawn from a key in device memory.  Declarations: include/cnf_ot_amd.h.
#include "cnf_common.h"

#include <math.h>

namespace cnf {

// ---------------------------------------------------------------------------
// Base noise: Philox4x32-10 + Box-Muller; one counter block (4 normals) per
// thread.  Element e of the stream uses block e>>2, word pair (e&3)>>1.
// ---------------------------------------------------------------------------
// seed_dev (optional): the key is read from device memory -- state[1] of a training step's device-side state
// (cnf_step_begin) -- so that a captured step draws new noise on every replay
__global__ void fill_normal_kernel(uint64_t seed, uint64_t first_element, int64_t n,
                                   float* __restrict__ out, const uint64_t* __restrict__ seed_dev) {
  if (seed_dev) seed = seed_dev[1];
  const uint64_t first_blk = first_element >> 2;
  const uint64_t last_blk = (first_element + (uint64_t)n - 1) >> 2;
  for (uint64_t blk = first_blk + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; blk <= last_blk;
       blk += (uint64_t)gridDim.x * blockDim.x) {
    float z[4];
    philox_normals4(seed, blk, z);
    const uint64_t e0 = blk << 2;
    if (e0 >= first_element && e0 + 3 < first_element + (uint64_t)n && (((e0 - first_element) & 3) == 0) &&
        ((reinterpret_cast<uintptr_t>(out) & 15) == 0)) {
      *reinterpret_cast<float4*>(out + (e0 - first_element)) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint64_t e = e0 + r;
        if (e >= first_element && e < first_element + (uint64_t)n) out[e - first_element] = z[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// JAX-compatible base draw: jax.random.normal(key, (n, D), float64) as the reference makes it
// (conditional.py:378,399 -> distrax Normal -> jax.random.normal; float64 because solvers.py:23 enables x64), for the
// classic (non-"partitionable") threefry bit generation: element j of the flattened [size] draw takes the 64 bits
// (o0 << 32) | o1 of the Threefry-2x32-20 block with counter (j, size + j) and key (k0, k1)
// [threefry_2x32 splits the iota of 2 size counters in halves; the 64-bit combine takes the halves of the output],
// maps them to a uniform in [nextafter(-1, 0), 1) through the mantissa of a double in [1, 2), and returns
// sqrt(2) erfinv(u).  The Threefry function is pinned by the Random123 known-answer vectors (tests); the bit ->
// normal mapping restates jax._src.random (un-pinned JAX version, not installable here: cannot be compared with
// JAX itself -- "parity unpinned" for this entry point).
// ---------------------------------------------------------------------------
__host__ __device__ inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__host__ __device__ inline void threefry2x32_20(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t& o0,
                                                uint32_t& o1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  const int rot[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  uint32_t x0 = c0 + ks[0], x1 = c1 + ks[1];
  for (int g = 0; g < 5; ++g) {
    for (int r = 0; r < 4; ++r) { x0 += x1; x1 = rotl32(x1, rot[g & 1][r]); x1 ^= x0; }
    x0 += ks[(g + 1) % 3];
    x1 += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
  o0 = x0; o1 = x1;
}

__global__ __launch_bounds__(256) void fill_normal_threefry_kernel(uint32_t k0, uint32_t k1, uint64_t size, uint64_t first, int64_t n,
                                            float* __restrict__ out32, double* __restrict__ out64) {
  const double lo = -0.99999999999999988897769753748;        // nextafter(-1, 0)
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t j = first + (uint64_t)i;
    uint32_t o0, o1;
    threefry2x32_20(k0, k1, (uint32_t)j, (uint32_t)(size + j), o0, o1);
    const uint64_t bits = ((uint64_t)o0 << 32) | (uint64_t)o1;
    const double f = __longlong_as_double((long long)((bits >> 12) | 0x3FF0000000000000ull)) - 1.0;
    const double u = fmax(lo, f * (1.0 - lo) + lo);
    const double z = 1.41421356237309504880 * erfinv(u);
    if (out64) out64[i] = z;
    if (out32) out32[i] = (float)z;
  }
}

}  // namespace cnf

// ===========================================================================
// C ABI
// ===========================================================================
using namespace cnf;

extern "C" int cnf_fill_normal_threefry(uint32_t key0, uint32_t key1, uint64_t size, uint64_t first_element, int64_t n,
                                        float* out_f32, double* out_f64, void* stream) {
  if (n < 0 || (n > 0 && !out_f32 && !out_f64) || first_element + (uint64_t)n > size || size > 0x7fffffffull)
    return CNF_ERR_INVALID;        // (2 size 32-bit counters: jax's single-block case)
  if (n == 0) return CNF_OK;
  int64_t grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(fill_normal_threefry_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, key0, key1,
                     size, first_element, n, out_f32, out_f64);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_fill_normal(uint64_t seed, uint64_t first_element, int64_t n, float* out,
                               void* stream) {
  if (n < 0 || (n > 0 && !out)) return CNF_ERR_INVALID;
  if (n == 0) return CNF_OK;
  const uint64_t n_blk = ((first_element + (uint64_t)n - 1) >> 2) - (first_element >> 2) + 1;
  uint64_t grid = (n_blk + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, seed,
                     first_element, n, out, (const uint64_t*)nullptr);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// ---- the random inputs of a training step drawn from a key in DEVICE memory ---------------------------------------
// state: uint64[2] on the device = { step count, key }.  The caller writes the key (one 8-byte copy) before a step;
// every draw below reads it on the device, so the whole step -- draws, loss, gradient, Adam -- can be captured into
// a HIP graph once and replayed with a new key each time.  Streams of one key: the normal stream of
// cnf_fill_normal (Philox counter words 2, 3 = 0, 0), uniforms (word 2 = 1) and 3-bit integers (word 2 = 2).
namespace cnf {
__global__ void step_begin_kernel(uint64_t* state) { if (threadIdx.x == 0 && blockIdx.x == 0) state[0] += 1; }

// out[i] = scale * u, u = 24-bit uniform in [0, 1) from word (first + i) & 3 of block (first + i) >> 2 of stream 1
__global__ void fill_uniform_kernel(const uint64_t* __restrict__ state, uint64_t first, int64_t n, float scale,
                                    float* __restrict__ out) {
  const uint64_t key = state[1];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = first + (uint64_t)i;
    uint32_t u[4];
    philox4x32((uint32_t)(e >> 2), (uint32_t)(e >> 34), 1u, 0u, (uint32_t)key, (uint32_t)(key >> 32), u);
    out[i] = scale * ((float)(u[e & 3] >> 8) * (1.0f / 16777216.0f));
  }
}

// The 8-mode mixture source of kl_loss_fn (applications.py:34-71) for n samples of dim 2: out[i] = z[i] + centre of
// component (first_sample + i), the component = the top 3 bits of word e & 3 of block e >> 2 of stream 2
__global__ void mixture_source_kernel(const uint64_t* __restrict__ state, uint64_t first_sample, int64_t n,
                                      const float* __restrict__ z, float* __restrict__ out, int32_t* __restrict__ comp_out) {
  constexpr float R = 5.0f;
  const float cx[8] = {0.0f, 1.0f, 0.0f, -1.0f, 0.6f, 0.6f, -0.6f, -0.6f};
  const float cy[8] = {1.0f, 0.0f, -1.0f, 0.0f, 0.8f, -0.8f, -0.8f, 0.8f};
  const uint64_t key = state[1];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = first_sample + (uint64_t)i;
    uint32_t u[4];
    philox4x32((uint32_t)(e >> 2), (uint32_t)(e >> 34), 2u, 0u, (uint32_t)key, (uint32_t)(key >> 32), u);
    const int k = (int)(u[e & 3] >> 29);
    float mx = 0.0f, my = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { mx = k == j ? cx[j] : mx; my = k == j ? cy[j] : my; }
    if (out) { out[2 * i] = z[2 * i] + R * mx; out[2 * i + 1] = z[2 * i + 1] + R * my; }
    if (comp_out) comp_out[i] = k;
  }
}
}  // namespace cnf

extern "C" int cnf_step_begin(uint64_t* state, void* stream) {
  if (!state) return CNF_ERR_INVALID;
  hipLaunchKernelGGL(cnf::step_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_fill_normal_dev(const uint64_t* state, uint64_t first_element, int64_t n, float* out, void* stream) {
  if (!state || n < 0 || (n > 0 && !out)) return CNF_ERR_INVALID;
  if (n == 0) return CNF_OK;
  const uint64_t n_blk = ((first_element + (uint64_t)n - 1) >> 2) - (first_element >> 2) + 1;
  uint64_t grid = (n_blk + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (uint64_t)0,
                     first_element, n, out, state);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_fill_uniform_dev(const uint64_t* state, uint64_t first, int64_t n, float scale, float* out, void* stream) {
  if (!state || n < 0 || (n > 0 && !out)) return CNF_ERR_INVALID;
  if (n == 0) return CNF_OK;
  int64_t grid = (n + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(cnf::fill_uniform_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, state, first, n, scale, out);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

extern "C" int cnf_mixture_source_dev(const uint64_t* state, uint64_t first_sample, int64_t n, const float* z, float* out,
                                      int32_t* comp, void* stream) {
  if (!state || n < 0 || (n > 0 && !out && !comp) || (out && !z)) return CNF_ERR_INVALID;
  if (n == 0) return CNF_OK;
  int64_t grid = (n + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(cnf::mixture_source_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, state, first_sample,
                     n, z, out, comp);
  return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
