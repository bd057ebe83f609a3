// Kernels shared by the denoiser VJPs (unet_bwd.hip, drunet.hip) and pieces shared by the finishing kernels of the weight gradients
// (critic_grad.hip, policy_grad.hip); `static`: one copy per translation unit.
#pragma once
#include "conv_hs.h"
#include "hs_rec.h"
#include "pack_desc.h"

namespace pnpx {

constexpr int SIG_CHUNKS = 64;

static __global__ void sigma_grad_final_kernel(const float* __restrict__ part, float* __restrict__ gsigma, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int c = 0; c < SIG_CHUNKS; ++c) s += part[b * SIG_CHUNKS + c];
  gsigma[b] = s;
}

static __global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ g, size_t n, unsigned* __restrict__ bits) {
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(g[i]));
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(bits, __float_as_uint(m));   // non-negative floats order like their bits
}
static __global__ void grad_scale_kernel(const unsigned* __restrict__ bits, float2* __restrict__ sc) {
  const float m = __uint_as_float(*bits);
  if (!(m > 0.f) || !isfinite(m)) {
    *sc = make_float2(m > 0.f ? 1.f : 0.f, m > 0.f ? 1.f : 0.f);   // all-zero gradient -> zeros; inf/nan -> pass through
    return;
  }
  int e;
  (void)frexpf(m, &e);                    // m = f * 2^e, f in [0.5, 1)
  if (e < -126) e = -126;                 // a denormal maximum: 2^-e would be inf.  2^126 is the largest scale; the scaled gradients stay below 1
  *sc = make_float2(ldexpf(1.f, -e), ldexpf(1.f, e));
}

static __global__ __launch_bounds__(256) void input_grad_hs_kernel(const HsRec* __restrict__ g_in0, const float* __restrict__ g_res,
                                                            float* __restrict__ gx, float* __restrict__ part,
                                                            const float2* __restrict__ sc, int H, int W) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int n = H * W, per = (n + SIG_CHUNKS - 1) / SIG_CHUNKS;
  const int lo = chunk * per, hi = min(n, lo + per);
  const HsRec* g0 = g_in0 + (size_t)b * 4 * (H + 2) * (W + 2);     // group 0 of 4: channels 0 (image) and 1 (noise map)
  const float m = sc->y, inv = 1.f / HS_ASCALE;
  float acc = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int y = i / W, x = i - y * W;
    float v[8];
    hs_unpack(g0[(size_t)(y + 1) * (W + 2) + x + 1], v);
    gx[(size_t)b * n + i] = (v[0] * inv + g_res[(size_t)b * n + i]) * m;
    acc += v[1] * inv;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ float w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[b * SIG_CHUNKS + chunk] = ((w[0] + w[1]) + (w[2] + w[3])) * m;
}

// ---- the launches between the UNet VJP's 27 adjoint convolutions (kernels and launchers: unet_bwd.hip).  unet_denoise_backward and the test
// probe (vjp_glue_probe.hip) both go through these launchers, so a form decision, a grid formula and sy / sx exist once.  The form
// decisions are host-only and need no device.  Form ids are those of include/pnpx.h (pnpx_vjp_glue_probe_desc.form); 0 = decide here.
enum VjpGlueForm {
  VG_AUTO = 0,
  VG_UPS_PLAIN = 1, VG_UPS_LDS16 = 2, VG_UPS_LDS64 = 3,     // fp32 up-sampling adjoint
  VG_SPM_PIXEL = 1, VG_SPM_BLOCK = 2,                       // fp32 skip / pool merge
  VG_ONLY = 1                                               // every other launch has one form
};
constexpr size_t VG_GRID_Z_MAX = 65535;                     // gridDim.z of one launch
// fp32 up-sampling adjoint: the LDS-window forms put one (image, channel) plane on gridDim.z; w = the SOURCE width
inline int upsample_bwd_form_f32(size_t B, int C, int w) {
  if (B * (size_t)C > VG_GRID_Z_MAX) return VG_UPS_PLAIN;
  return w >= 64 ? VG_UPS_LDS64 : VG_UPS_LDS16;
}
inline bool upsample_bwd_form_runs(int form, size_t B, int C) {
  return form == VG_UPS_PLAIN || ((form == VG_UPS_LDS16 || form == VG_UPS_LDS64) && B * (size_t)C <= VG_GRID_Z_MAX);
}
inline int skip_pool_merge_form_f32(int H, int W) { return (H % 2 == 0 && W % 2 == 0) ? VG_SPM_BLOCK : VG_SPM_PIXEL; }
inline bool skip_pool_merge_form_runs(int form, int H, int W) {
  return form == VG_SPM_PIXEL || (form == VG_SPM_BLOCK && H % 2 == 0 && W % 2 == 0);
}
// HS8 up-sampling adjoint: one (image, group) per gridDim.z.  B * Gs above the limit runs as consecutive launches over whole images,
// each of at most VG_GRID_Z_MAX / Gs images (0: a single image is over the limit, the launcher refuses with PNPX_ERR_SHAPE).
inline int upsample_bwd_hs_images_per_launch(int Gs) { return Gs > 0 ? (int)(VG_GRID_Z_MAX / (size_t)Gs) : 0; }
inline int upsample_bwd_hs_launches(int B, int Gs) {
  const int per = upsample_bwd_hs_images_per_launch(Gs);
  return per > 0 ? (B + per - 1) / per : 0;
}
// align_corners scale of the x2 bilinear up-sampling from n source rows / columns
inline float upsample2x_scale(int n) { return (2 * n > 1) ? (float)(n - 1) / (float)(2 * n - 1) : 0.f; }

// Every launcher checks its launch and returns a PNPX status.  fp32 tensors: padded planar; HS8: records (hs_rec.h).
int launch_outc_bwd_f32(const float* g_out, const float* pre, const float* w, const float* feat, float* g_feat, float* g_res, int B, int H,
                        int W, hipStream_t s);
int launch_outc_bwd_hs(const float* g_out, const float* pre, const float* w, const HsRec* feat, HsRec* g_feat, float* g_res, const float2* sc,
                       int B, int H, int W, hipStream_t s);
// gcat [B][Ccat][Ht][Wt], channels [c_off, c_off + C) -> g_src [B][C][h][w] (HS8: groups of 8 channels)
int launch_upsample_bwd_f32(int form, const float* gcat, int Ccat, int c_off, const float* src_act, float* g_src, int B, int C, int h, int w,
                            int Ht, int Wt, hipStream_t s);
int launch_upsample_bwd_hs(const HsRec* gcat, int Gcat, int g_off, const HsRec* src_act, HsRec* g_src, int B, int Gs, int h, int w, int Ht,
                           int Wt, hipStream_t s);
// gcat [B][Ccat][H][W] (channels [0, C)), g_pool [B][C][H/2][W/2] or null -> g_x [B][C][H][W]
int launch_skip_pool_merge_f32(int form, const float* gcat, int Ccat, const float* g_pool, const float* xact, float* g_x, int B, int C, int H,
                               int W, hipStream_t s);
int launch_skip_pool_merge_hs(const HsRec* gcat, int Gcat, const HsRec* g_pool, const HsRec* xact, HsRec* g_x, int B, int G, int H, int W,
                              hipStream_t s);
// gx [B][H][W], part [B][SIG_CHUNKS], gsigma [B]: the input-gradient kernel, then sigma_grad_final_kernel
int launch_input_grad_f32(const float* g_in0, int Cg, const float* g_res, float* gx, float* part, float* gsigma, int B, int H, int W,
                          hipStream_t s);
int launch_input_grad_hs(const HsRec* g_in0, const float* g_res, float* gx, float* part, const float2* sc, float* gsigma, int B, int H, int W,
                         hipStream_t s);
// bits <- 0, absmax_kernel over g [n], grad_scale_kernel: sc = {1 / m, m}, m the power of two above max |g|
int launch_grad_scale(const float* g, size_t n, unsigned* bits, float2* sc, hipStream_t s);

// ---- finishing kernels of the K-split weight-gradient GEMM (critic_grad.hip::critic_wgrad_kernel): slab[piece][co][tap index][k]
// tap -> its index in the window of packing D (-1: absent).  Threads 0..8 fill sTi[9]; the caller synchronises.
__device__ inline void wgrad_tap_index(const PackDesc& D, int* sTi) {
  const int tid = threadIdx.x;
  if (tid < 9) {
    int ti = -1;
    for (int i = 0; i < D.nt; ++i)
      if (D.tap[i] == tid) ti = i;
    sTi[tid] = ti;
  }
}
// Raw element i of output channel co's fan: its one effective position (eff_pos_of_src), the pieces added in piece order in double.
__device__ inline double wgrad_gather(const PackDesc& D, const int* sTi, const float* __restrict__ slab, size_t stride, int pieces,
                                      int co, int i) {
  int k, tap;
  eff_pos_of_src(D, i, k, tap);
  const int ti = sTi[tap];
  double sum = 0.0;
  if (ti >= 0) {
    const float* src = slab + ((size_t)co * D.nt + ti) * D.K + k;
    for (int pc = 0; pc < pieces; ++pc) sum += (double)src[(size_t)pc * stride];
  }
  return sum;
}

}  // namespace pnpx
