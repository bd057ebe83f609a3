// The 32-byte record of the half-split (HS8) activation layout: 8 channels of one pixel as hi[8] | lo[8] f16, the value
// (times HS_ASCALE) being hi + lo.  Tensors are [B][C/8][H+2][W+2] records with a zero border (conv_hs.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pnpx {

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
struct HsRec {
  h8v hi, lo;
};
__device__ __forceinline__ void hs_unpack(const HsRec& r, float v[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)r.hi[e] + (float)r.lo[e];
}
__device__ __forceinline__ HsRec hs_pack(const float v[8]) {
  HsRec r;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    r.hi[e] = (_Float16)v[e];
    r.lo[e] = (_Float16)(v[e] - (float)r.hi[e]);
  }
  return r;
}
// A product that is the LAST operation before hs_pack goes through this: left to the compiler it is fused into hs_pack's two conversions
// separately (hi = f16(fp32(a * b)), lo = f16(a * b - f16(a * b)) from the unrounded product, v_fma_mixlo_f16), and where fp32(a * b)
// falls on an f16 tie the record comes out one hi-ulp off (unet_bwd.hip, policy_grad.hip::pol_grad_seed_kernel).  A product with a power
// of two is exact and needs none.
__device__ __forceinline__ float rounded_f32(float x) {
  asm("" : "+v"(x));      // the fp32 value itself, in a register: nothing upstream can be fused into what is computed from it
  return x;
}
// global average pool: the sum of channel c of image b over the h x w interior of an HS8 tensor of G groups, times inv.
// Fixed summation order (a result does not depend on the batch it arrives in).
__device__ __forceinline__ float hs_pooled(const HsRec* __restrict__ feat, int b, int G, int c, int h, int w, float inv) {
  const HsRec* p = feat + ((size_t)b * G + (c >> 3)) * (h + 2) * (w + 2);
  float s = 0.f;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const HsRec& r = p[(y + 1) * (w + 2) + x + 1];
      s += (float)r.hi[c & 7] + (float)r.lo[c & 7];
    }
  return s * inv;
}

}  // namespace pnpx
