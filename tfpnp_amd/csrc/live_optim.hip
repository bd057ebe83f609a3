// Optimiser step on a live parameter vector (live_params.h: LiveOptim): clip_grad_norm_ + torch's single-tensor Adam
// (trainer/mddpg/trainer.py:201-204 for the actor, :208-209 for the critic), three launches.  Nothing here knows which network the
// vector belongs to; the drivers (critic.hip::critic_adam_step, policy_pack.hip::policy_adam_step) keep their own checks, their
// re-packing and the read-back slot the norm travels in.
//
//   live_sumsq_kernel        sum of squares of the gradient: a fixed grid, each thread owns the 16-byte chunks
//                            tid, tid + T, tid + 2 T, ... (T = threads of the grid) and adds them in that order in double;
//                            the block is reduced by a fixed tree; one double per block, no atomics
//   live_norm_finish_kernel  one block adds the partials in index order; norm and clip coefficient go to a device slot
//   live_adam_kernel         g = grad * c;  m += (g - m) (1 - b1);  v = v b2 + (1 - b2) g g;
//                            p -= step_size * m / (sqrt(v) / bc2_sqrt + eps)        -- one read of grad, p, m, v and one
//                            write of p, m, v per element; the coefficient comes from the slot (no host read in between)
//
// A chunk is four consecutive floats from the start of the vector.  The last n % 4 elements always take the 4-byte path; a
// gradient that is not 16-byte aligned takes the 4-byte path throughout, with the same ownership and the same order of additions:
// the result does not depend on the alignment.  Everything is fp32 element by element with no contraction, so it does not depend
// on the path or the grid either.
//
// FROZEN RANGES.  Both kernels take a sorted table of disjoint [first, first + count) ranges of the vector (LiveOptim::frozen,
// uploaded once with the network; the actor's running statistics, which are buffers and not parameters: neither clip_grad_norm_ nor
// the optimiser of the reference sees them).  An element inside a range adds nothing to the norm -- whatever the gradient holds
// there, a NaN included -- and its p, m and v are not written.  Ownership and order of everything outside the ranges are as above:
// a chunk that no range touches takes the path it always took, a chunk inside a range is skipped, a chunk that straddles a boundary
// is handled element by element (4-byte loads and stores of exactly the elements outside).  Without a table (the critic) the
// instances compiled are the ones without any of this.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace pnpx {
namespace {

constexpr int OPT_THREADS = 256;
constexpr int ADAM_BLOCKS = 2048;   // HBM-bound streaming: 8 blocks of 256 on each of the 256 CUs, grid-stride over the rest

// the table in LDS (nf <= LIVE_OPTIM_MAX_FROZEN entries; every thread of the block calls this)
struct Frozen {
  const FrozenRange* r;
  int n;
  // first range that ends behind element i (n: none)
  __device__ int find(size_t i) const {
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (r[mid].first + r[mid].count > i) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  }
  __device__ bool holds(size_t i) const {
    const int k = find(i);
    return k < n && r[k].first <= i;
  }
  // chunk [i0, i0 + 4): 0 = no range touches it, 1 = inside one range, 2 = mixed; k = find(i0)
  __device__ int chunk(size_t i0, int& k) const {
    k = find(i0);
    if (k == n || r[k].first >= i0 + 4) return 0;
    if (r[k].first <= i0 && r[k].first + r[k].count >= i0 + 4) return 1;
    return 2;
  }
  // element i >= the one k was found for; k moves along
  __device__ bool holds_from(size_t i, int& k) const {
    while (k < n && r[k].first + r[k].count <= i) ++k;
    return k < n && r[k].first <= i;
  }
};
__device__ inline Frozen frozen_to_lds(const FrozenRange* __restrict__ tab, int nf, FrozenRange* lds) {
  for (int i = threadIdx.x; i < nf; i += OPT_THREADS) lds[i] = tab[i];
  __syncthreads();
  return Frozen{lds, nf};
}

template <bool VEC>
__device__ inline float4 load_chunk(const float* __restrict__ g, size_t c) {
  if (VEC) return reinterpret_cast<const float4*>(g)[c];
  return make_float4(g[4 * c], g[4 * c + 1], g[4 * c + 2], g[4 * c + 3]);
}

template <bool VEC, bool FROZEN>
__global__ __launch_bounds__(OPT_THREADS) void live_sumsq_kernel(const float* __restrict__ g, size_t n, const FrozenRange* __restrict__ tab,
                                                                 int nf, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double part[OPT_THREADS];
  __shared__ FrozenRange ftab[FROZEN ? LIVE_OPTIM_MAX_FROZEN : 1];
  Frozen F{nullptr, 0};
  if (FROZEN) F = frozen_to_lds(tab, nf, ftab);
  const size_t T = (size_t)gridDim.x * OPT_THREADS, t = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  const size_t n4 = n / 4;
  double acc = 0.0;
  for (size_t c = t; c < n4; c += T) {
    int k = 0;
    const int kind = FROZEN ? F.chunk(4 * c, k) : 0;
    if (kind == 0) {
      const float4 x = load_chunk<VEC>(g, c);
      acc += (double)x.x * (double)x.x;
      acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z;
      acc += (double)x.w * (double)x.w;
    } else if (kind == 2) {
      for (int e = 0; e < 4; ++e) {
        const size_t i = 4 * c + e;
        if (F.holds_from(i, k)) continue;
        const float x = g[i];
        acc += (double)x * (double)x;
      }
    }
  }
  if (4 * n4 + t < n && !(FROZEN && F.holds(4 * n4 + t))) {   // the tail: element 4 n4 + t belongs to thread t
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
__global__ __launch_bounds__(OPT_THREADS) void live_norm_finish_kernel(const double* __restrict__ partials, float max_norm,
                                                                       float* __restrict__ slot, float* __restrict__ norm_out) {
#pragma clang fp contract(off)
  __shared__ double part[LIVE_OPTIM_PARTIALS];
  for (int i = threadIdx.x; i < LIVE_OPTIM_PARTIALS; i += OPT_THREADS) part[i] = partials[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int i = 0; i < LIVE_OPTIM_PARTIALS; ++i) sum += part[i];
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

template <bool VEC, bool FROZEN>
__global__ __launch_bounds__(OPT_THREADS) void live_adam_kernel(const float* __restrict__ g, float* __restrict__ p, float* __restrict__ m,
                                                                float* __restrict__ v, size_t n, const FrozenRange* __restrict__ tab, int nf,
                                                                const float* __restrict__ slot, AdamArgs a) {
  __shared__ FrozenRange ftab[FROZEN ? LIVE_OPTIM_MAX_FROZEN : 1];
  const float norm = slot[0], c = slot[1];
  if (!(fabsf(norm) <= 3.402823466e+38f)) return;   // gradient norm not finite: nothing is touched (uniform over the grid)
  Frozen F{nullptr, 0};
  if (FROZEN) F = frozen_to_lds(tab, nf, ftab);
  const size_t T = (size_t)gridDim.x * OPT_THREADS, t = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  if (VEC) {   // p, m, v are 16-byte aligned allocations of the context; g was checked by the launcher
    const size_t n4 = n / 4;
    for (size_t ch = t; ch < n4; ch += T) {
      int k = 0;
      const int kind = FROZEN ? F.chunk(4 * ch, k) : 0;
      if (kind == 0) {
        const float4 gg = reinterpret_cast<const float4*>(g)[ch];
        float4 pp = reinterpret_cast<float4*>(p)[ch], mm = reinterpret_cast<float4*>(m)[ch], vv = reinterpret_cast<float4*>(v)[ch];
        adam_element(gg.x, pp.x, mm.x, vv.x, c, a);
        adam_element(gg.y, pp.y, mm.y, vv.y, c, a);
        adam_element(gg.z, pp.z, mm.z, vv.z, c, a);
        adam_element(gg.w, pp.w, mm.w, vv.w, c, a);
        reinterpret_cast<float4*>(p)[ch] = pp;
        reinterpret_cast<float4*>(m)[ch] = mm;
        reinterpret_cast<float4*>(v)[ch] = vv;
      } else if (kind == 2) {
        for (int e = 0; e < 4; ++e) {
          const size_t i = 4 * ch + e;
          if (!F.holds_from(i, k)) adam_element(g[i], p[i], m[i], v[i], c, a);
        }
      }
    }
    const size_t i = 4 * n4 + t;   // the tail, 4 bytes at a time
    if (i < n && !(FROZEN && F.holds(i))) adam_element(g[i], p[i], m[i], v[i], c, a);
  } else {
    for (size_t i = t; i < n; i += T)
      if (!(FROZEN && F.holds(i))) adam_element(g[i], p[i], m[i], v[i], c, a);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline size_t optim_stride(size_t n) { return (n + 3) & ~(size_t)3; }   // floats: exp_avg_sq starts 16-byte aligned

int launch_sumsq(const float* grad, size_t n, const FrozenRange* tab, int nf, double* partials, hipStream_t s) {
  const dim3 grid(LIVE_OPTIM_PARTIALS), block(OPT_THREADS);
  const bool vec = aligned16(grad);
  if (nf) {
    if (vec) hipLaunchKernelGGL((live_sumsq_kernel<true, true>), grid, block, 0, s, grad, n, tab, nf, partials);
    else hipLaunchKernelGGL((live_sumsq_kernel<false, true>), grid, block, 0, s, grad, n, tab, nf, partials);
  } else {
    if (vec) hipLaunchKernelGGL((live_sumsq_kernel<true, false>), grid, block, 0, s, grad, n, tab, nf, partials);
    else hipLaunchKernelGGL((live_sumsq_kernel<false, false>), grid, block, 0, s, grad, n, tab, nf, partials);
  }
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_adam(const float* grad, float* p, float* m, float* v, size_t n, const FrozenRange* tab, int nf, const float* slot,
                const AdamArgs& a, hipStream_t s) {
  const size_t work = (n / 4 + OPT_THREADS - 1) / OPT_THREADS;
  const dim3 grid((unsigned)std::max<size_t>(1, std::min<size_t>(work, ADAM_BLOCKS))), block(OPT_THREADS);
  const bool vec = aligned16(grad) && aligned16(p) && aligned16(m) && aligned16(v);
  if (nf) {
    if (vec) hipLaunchKernelGGL((live_adam_kernel<true, true>), grid, block, 0, s, grad, p, m, v, n, tab, nf, slot, a);
    else hipLaunchKernelGGL((live_adam_kernel<false, true>), grid, block, 0, s, grad, p, m, v, n, tab, nf, slot, a);
  } else {
    if (vec) hipLaunchKernelGGL((live_adam_kernel<true, false>), grid, block, 0, s, grad, p, m, v, n, tab, nf, slot, a);
    else hipLaunchKernelGGL((live_adam_kernel<false, false>), grid, block, 0, s, grad, p, m, v, n, tab, nf, slot, a);
  }
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

}  // namespace

int live_merge_frozen(const FrozenRange* in, int n, size_t vec_n, FrozenRange* out, int* n_out) {
  int k = 0;
  size_t end = 0;
  for (int i = 0; i < n; ++i) {
    if (in[i].count == 0) continue;
    if (in[i].first < end || in[i].first + in[i].count > vec_n) return PNPX_ERR_SHAPE;   // unsorted, overlapping or outside the vector
    if (k && in[i].first == end) {
      out[k - 1].count += in[i].count;
    } else {
      if (k == LIVE_OPTIM_MAX_FROZEN) return PNPX_ERR_SHAPE;
      out[k++] = in[i];
    }
    end = in[i].first + in[i].count;
  }
  *n_out = k;
  return PNPX_OK;
}

int LiveOptim::set_frozen(const FrozenRange* ranges, int n, size_t vec_n, const char* what) {
  FrozenRange merged[LIVE_OPTIM_MAX_FROZEN];
  int k = 0;
  if (live_merge_frozen(ranges, n, vec_n, merged, &k) != PNPX_OK) {
    set_error("%s: internal error: the frozen ranges are not sorted, disjoint, inside the vector and at most %d", what, LIVE_OPTIM_MAX_FROZEN);
    return PNPX_ERR_SHAPE;
  }
  if (frozen.p) (void)hipFree(frozen.p);
  frozen = DeviceBuf();
  nfrozen = 0;
  if (!k) return PNPX_OK;
  PNPX_TRY(alloc_dev(frozen, k * sizeof(FrozenRange), what));
  PNPX_HIP(hipMemcpy(frozen.p, merged, k * sizeof(FrozenRange), hipMemcpyHostToDevice));
  nfrozen = k;
  return PNPX_OK;
}

int LiveOptim::launch_step(const LiveParams& live, const float* grad, float lr, float beta1, float beta2, float eps, float max_norm,
                           float* slot, float* norm_out, const char* what, hipStream_t s) {
  const size_t n = live.n;
  if (!state.p) {   // first step: zero-filled moments (the only place the call allocates or synchronises the device)
    PNPX_HIP(hipDeviceSynchronize());
    PNPX_TRY(alloc_dev(state, 2 * optim_stride(n) * sizeof(float) + LIVE_OPTIM_PARTIALS * sizeof(double), what));
    PNPX_HIP(hipMemset(state.p, 0, state.bytes));
    PNPX_HIP(hipDeviceSynchronize());
    step = 0;
  }
  float* m = static_cast<float*>(state.p);
  float* v = m + optim_stride(n);
  double* partials = reinterpret_cast<double*>(v + optim_stride(n));
  const FrozenRange* tab = static_cast<const FrozenRange*>(frozen.p);
  const double t = (double)(step + 1);
  const double step_size = (double)lr / (1.0 - std::pow((double)beta1, t));
  const double bc2_sqrt = std::sqrt(1.0 - std::pow((double)beta2, t));
  const AdamArgs a{(float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2), (float)step_size, (float)bc2_sqrt, eps};
  PNPX_TRY(launch_sumsq(grad, n, tab, nfrozen, partials, s));
  hipLaunchKernelGGL(live_norm_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, s, partials, max_norm, slot, norm_out);
  PNPX_LAUNCH_CHECK();
  return launch_adam(grad, live.p(), m, v, n, tab, nfrozen, slot, a, s);
}

int LiveOptim::copy_state(size_t n, float* exp_avg_dst, float* exp_avg_sq_dst, long long* step_host, hipStream_t s) const {
  if (state.p) {
    const float* m = static_cast<const float*>(state.p);
    PNPX_HIP(hipMemcpyAsync(exp_avg_dst, m, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    PNPX_HIP(hipMemcpyAsync(exp_avg_sq_dst, m + optim_stride(n), n * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {   // before the first step
    PNPX_HIP(hipMemsetAsync(exp_avg_dst, 0, n * sizeof(float), s));
    PNPX_HIP(hipMemsetAsync(exp_avg_sq_dst, 0, n * sizeof(float), s));
  }
  if (step_host) *step_host = state.p ? step : 0;
  return PNPX_OK;
}

int LiveOptim::reset() {
  if (state.p) {
    PNPX_HIP(hipDeviceSynchronize());
    PNPX_HIP(hipFree(state.p));
  }
  state = DeviceBuf();
  step = 0;
  return PNPX_OK;
}

void LiveOptim::free() {
  if (state.p) (void)hipFree(state.p);
  if (frozen.p) (void)hipFree(frozen.p);
  *this = LiveOptim();
}

}  // namespace pnpx
