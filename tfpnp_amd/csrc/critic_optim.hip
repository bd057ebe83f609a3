// Optimiser step of the value network on its live parameter vector: clip_grad_norm_ + torch's single-tensor Adam
// (trainer/mddpg/trainer.py:208-209), three launches (driver: critic.hip::critic_adam_step).
//
//   critic_sumsq_kernel        sum of squares of the gradient: a fixed grid, each thread owns the 16-byte chunks
//                              tid, tid + T, tid + 2 T, ... (T = threads of the grid) and adds them in that order in double;
//                              the block is reduced by a fixed tree; one double per block, no atomics
//   critic_norm_finish_kernel  one block adds the partials in index order; norm and clip coefficient go to a device slot
//   critic_adam_kernel         g = grad * c;  m += (g - m) (1 - b1);  v = v b2 + (1 - b2) g g;
//                              p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)        -- one read of grad, p, m, v and one
//                              write of p, m, v per element; the coefficient comes from the slot (no host read in between)
//
// A chunk is four consecutive floats from the start of the vector.  The parameter count is 2 mod 4 for every num_inputs, so
// last n % 4 elements always take the 4-byte path; a gradient that is not 16-byte aligned takes the 4-byte
// path throughout, with the same ownership and the same order of additions: the result does not depend on the alignment.
// Everything is fp32 element by element with no contraction, so it does not depend on the path or the grid either.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace pnpx {
namespace {

constexpr int OPT_THREADS = 256;
constexpr int ADAM_BLOCKS = 2048;   // HBM-bound streaming: 8 blocks of 256 on each of the 256 CUs, grid-stride over the rest

template <bool VEC>
__device__ inline float4 load_chunk(const float* __restrict__ g, size_t c) {
  if (VEC) return reinterpret_cast<const float4*>(g)[c];
  return make_float4(g[4 * c], g[4 * c + 1], g[4 * c + 2], g[4 * c + 3]);
}

template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void critic_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double part[OPT_THREADS];
  const size_t T = (size_t)gridDim.x * OPT_THREADS, t = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  const size_t n4 = n / 4;
  double acc = 0.0;
  for (size_t c = t; c < n4; c += T) {
    const float4 x = load_chunk<VEC>(g, c);
    acc += (double)x.x * (double)x.x;
    acc += (double)x.y * (double)x.y;
    acc += (double)x.z * (double)x.z;
    acc += (double)x.w * (double)x.w;
  }
  if (4 * n4 + t < n) {   // the tail: element 4 n4 + t belongs to thread t
    const float x = g[4 * n4 + t];
    acc += (double)x * (double)x;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int st = OPT_THREADS / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = part[0];
}

// slot[0] = ||grad||_2 (float), slot[1] = min(1, max_norm / (norm + 1e-6)) as clip_grad_norm_ computes it on an fp32 norm
__global__ __launch_bounds__(OPT_THREADS) void critic_norm_finish_kernel(const double* __restrict__ partials, float max_norm,
                                                                         float* __restrict__ slot, float* __restrict__ norm_out) {
#pragma clang fp contract(off)
  __shared__ double part[CRITIC_OPTIM_PARTIALS];
  for (int i = threadIdx.x; i < CRITIC_OPTIM_PARTIALS; i += OPT_THREADS) part[i] = partials[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int i = 0; i < CRITIC_OPTIM_PARTIALS; ++i) sum += part[i];
  const float norm = (float)sqrt(sum);
  const float c = max_norm / (norm + 1e-6f);
  slot[0] = norm;
  slot[1] = c > 1.0f ? 1.0f : c;   // (a NaN stays a NaN: the step kernel looks at the norm first)
  if (norm_out) norm_out[0] = norm;
}

struct AdamArgs {
  float one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps;
};

__device__ inline void adam_element(float g, float& p, float& m, float& v, float c, const AdamArgs& a) {
#pragma clang fp contract(off)
  g = g * c;
  m = m + (g - m) * a.one_minus_b1;
  v = v * a.b2 + (a.one_minus_b2 * g) * g;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p - a.step_size * (m / denom);
}

template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void critic_adam_kernel(const float* __restrict__ g, float* __restrict__ p, float* __restrict__ m,
                                                                  float* __restrict__ v, size_t n, const float* __restrict__ slot, AdamArgs a) {
  const float norm = slot[0], c = slot[1];
  if (!(fabsf(norm) <= 3.402823466e+38f)) return;   // gradient norm not finite: nothing is touched
  const size_t T = (size_t)gridDim.x * OPT_THREADS, t = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  if (VEC) {   // p, m, v are 16-byte aligned allocations of the context; g was checked by the launcher
    const size_t n4 = n / 4;
    for (size_t ch = t; ch < n4; ch += T) {
      const float4 gg = reinterpret_cast<const float4*>(g)[ch];
      float4 pp = reinterpret_cast<float4*>(p)[ch], mm = reinterpret_cast<float4*>(m)[ch], vv = reinterpret_cast<float4*>(v)[ch];
      adam_element(gg.x, pp.x, mm.x, vv.x, c, a);
      adam_element(gg.y, pp.y, mm.y, vv.y, c, a);
      adam_element(gg.z, pp.z, mm.z, vv.z, c, a);
      adam_element(gg.w, pp.w, mm.w, vv.w, c, a);
      reinterpret_cast<float4*>(p)[ch] = pp;
      reinterpret_cast<float4*>(m)[ch] = mm;
      reinterpret_cast<float4*>(v)[ch] = vv;
    }
    const size_t i = 4 * n4 + t;   // the tail, 4 bytes at a time
    if (i < n) adam_element(g[i], p[i], m[i], v[i], c, a);
  } else {
    for (size_t i = t; i < n; i += T) adam_element(g[i], p[i], m[i], v[i], c, a);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int launch_critic_sumsq(const float* grad, size_t n, double* partials, hipStream_t s) {
  if (aligned16(grad))
    hipLaunchKernelGGL(critic_sumsq_kernel<true>, dim3(CRITIC_OPTIM_PARTIALS), dim3(OPT_THREADS), 0, s, grad, n, partials);
  else
    hipLaunchKernelGGL(critic_sumsq_kernel<false>, dim3(CRITIC_OPTIM_PARTIALS), dim3(OPT_THREADS), 0, s, grad, n, partials);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_critic_norm_finish(const double* partials, float max_norm, float* slot, float* norm_out, hipStream_t s) {
  hipLaunchKernelGGL(critic_norm_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, s, partials, max_norm, slot, norm_out);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_critic_adam(const float* grad, float* p, float* m, float* v, size_t n, const float* slot, float one_minus_b1, float b2,
                       float one_minus_b2, float step_size, float bc2_sqrt, float eps, hipStream_t s) {
  const AdamArgs a{one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps};
  const size_t work = (n / 4 + OPT_THREADS - 1) / OPT_THREADS;
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(work, ADAM_BLOCKS));
  if (aligned16(grad) && aligned16(p) && aligned16(m) && aligned16(v))
    hipLaunchKernelGGL(critic_adam_kernel<true>, dim3(blocks), dim3(OPT_THREADS), 0, s, grad, p, m, v, n, slot, a);
  else
    hipLaunchKernelGGL(critic_adam_kernel<false>, dim3(blocks), dim3(OPT_THREADS), 0, s, grad, p, m, v, n, slot, a);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

}  // namespace pnpx
