// Parameter gradients of the actor through its train-mode forward: launch interface of policy_grad.hip (driver:
// policy_bn.hip::policy_param_grad; the weight-gradient GEMM is the critic's, critic_grad.h).
#pragma once
#include "common.h"
#include "hs_rec.h"
#include "pack_desc.h"

namespace pnpx {

// the forward (fold-free) packing descriptors of the 21 convolutions, in the trunk's layer numbering (policy_pack.hip)
int policy_pack_descs(const PolicyNet& N, PackDesc* out21);

// ------------------------------------------------------------------------------------------- heads
// Per-image scratch of the head backward, POL_HEAD_STRIDE floats: the pooled feature f[512]; gl[2] (softmax logits' gradient);
// g1[64] (gradient at the rows of the first deterministic Linear: n_det of them, 64 with the SPI head); hid[64] and g2[64]
// (SPI head: the hidden activation and the gradient at the n_det rows of the second Linear)
constexpr int POL_HEAD_STRIDE = 768;
constexpr int POL_HEAD_GL = 512, POL_HEAD_G1 = 576, POL_HEAD_HID = 640, POL_HEAD_G2 = 704;
struct PolHeadGradJob {
  const HsRec* feat = nullptr;     // the last activation, HS8 [B][64][h+2][w+2]
  int h = 0, w = 0, B = 0, n_det = 0, spi = 0;
  const float *sm_w = nullptr, *sm_b = nullptr, *d_w = nullptr, *d_b = nullptr, *d2_w = nullptr, *d2_b = nullptr;
  const float *gp = nullptr, *gd = nullptr;   // upstream gradients [B][2], [B][n_det]
  float* gf = nullptr;             // [B][512]: gradient of the pooled feature, unscaled fp32
  float* rows = nullptr;           // [B][POL_HEAD_STRIDE]
  float* grad = nullptr;           // grad_params
  size_t head_src = 0;             // floats into the parameter vector: fc_softmax.0.weight (the head tensors follow in order)
};
// pol_head_grad_kernel (one workgroup per observation) and the fixed-order sums over the batch of the 4 / 6 head tensors
int launch_pol_head_grad(const PolHeadGradJob& J, hipStream_t s);

// ------------------------------------------------------------------------------------------- gradient range
// Gradients travel as HS8 tensors of  s * boost * g  (times HS_ASCALE as every record).  s: the power of two that brings max |g_f|
// into [0.5, 1), found on the device (slot: float2 (s, 1 / s); (0, 0) for an all-zero gradient); boost: a host-side power of two.
//   bits / slot     one word (zeroed by the launcher) and the float2
//   ga              gradient of the last activation, HS8 [B][64][h+2][w+2]: every interior pixel  (g_f * s) * (boost / (h w))
//   gv[b]           1 / (s * boost): the per-image factor of the weight-gradient GEMM, which so undoes the scale
int launch_pol_grad_seed(const float* gf, unsigned* bits, float2* slot, HsRec* ga, float* gv, float boost, int B, int h, int w, hipStream_t s);

// ------------------------------------------------------------------------------------------- BatchNorm forward (train mode)
// Kernels: policy_bn.hip.  The train-mode walk and the test probe (net_train_probe.hip) both go through these two launchers.
constexpr int BN_FWD_PIECE = 2048;   // pixels per partial sum: 256 threads x 8
inline size_t bn_fwd_pieces(long long npix) { return (size_t)((npix + BN_FWD_PIECE - 1) / BN_FWD_PIECE); }
struct BnStatsJob {
  const HsRec* z = nullptr;         // the layer's raw convolution output, HS8 [B][G][h+2][w+2]
  int G = 0, B = 0, h = 0, w = 0;
  double* part = nullptr;           // [pieces][8 G][2]: sum, sum of squares
  float* params = nullptr;          // the live parameter vector
  size_t bn = 0;                    // floats into it: weight, bias, running_mean, running_var (8 G each)
  float *mean = nullptr, *var = nullptr, *scale = nullptr, *shift = nullptr;   // out, at the layer's first channel
  float momentum = 0.f;
  int update = 0;                   // move the running statistics
};
// bn_partial_kernel, bn_finish_kernel
int launch_bn_stats(const BnStatsJob& J, hipStream_t s);
struct BnSrc {
  const HsRec* z;      // the layer's raw output, HS8 [B][G][h+2][w+2]; null: absent
  const float *mean, *scale, *beta;   // at the layer's first channel
};
struct BnApplyJob {
  BnSrc a{nullptr, nullptr, nullptr, nullptr}, b{nullptr, nullptr, nullptr, nullptr};   // b: the second normalised summand (block 0: the shortcut)
  const HsRec* res = nullptr;       // identity residual, HS8 [B][G][h+2][w+2], or null
  HsRec* out = nullptr;             // HS8 [B][G][h+2][w+2] or null
  HsRec* s2d_hs = nullptr;          // HS8 [B][4G][h/2+2][w/2+2] (phase-major groups, hs_relayout.h) or null
  int G = 0, B = 0, h = 0, w = 0;
};
// bn_apply_kernel
int launch_bn_apply(const BnApplyJob& J, hipStream_t s);

// ------------------------------------------------------------------------------------------- BatchNorm backward
constexpr int BN_BWD_PIECE = 2048;   // pixels per partial sum (the forward's BN_PIECE)
inline size_t bn_bwd_pieces(long long npix) { return (size_t)((npix + BN_BWD_PIECE - 1) / BN_BWD_PIECE); }
struct BnBwdLayer {     // one BatchNorm layer fed by the tensor of dy
  const HsRec* z = nullptr;         // its raw convolution output, HS8 [B][G][h+2][w+2]; null: absent
  const float *mean = nullptr, *var = nullptr;   // batch statistics at the layer's first channel
  size_t bn = 0;                    // floats into the parameter vector: weight, bias, running_mean, running_var (cout each)
  float* coef = nullptr;            // [3][cout] at the layer's first channel: A = weight * rstd, c1 = A * S1 / n, c2 = A * rstd^2 * S2 / n
  HsRec* dz = nullptr;              // out: HS8 [B][G][h+2][w+2]
};
struct BnBwdJob {
  const HsRec* g = nullptr;         // gradient of the activation, HS8 [B][G][h+2][w+2]
  const HsRec* act = nullptr;       // the saved activation (mask: dy = g * [act > 0])
  BnBwdLayer l0, l1;                // l1: the second BatchNorm the same dy feeds (block 0: the shortcut's), or absent
  HsRec* dy_out = nullptr;          // the masked dy itself as a tensor (block 1: the identity branch), or null
  int G = 0, B = 0, h = 0, w = 0;
  double* part = nullptr;           // [pieces][8 G][3]: S1, S2 of l0, S2 of l1
  const float* params = nullptr;    // the live parameter vector
  float* grad = nullptr;            // grad_params
  const float2* slot = nullptr;
  float inv_boost = 1.f;
  unsigned* range_flag = nullptr;
};
// bn_bwd_partial_kernel, bn_bwd_finish_kernel (per layer), bn_bwd_apply_kernel
int launch_bn_bwd(const BnBwdJob& J, hipStream_t s);

// ------------------------------------------------------------------------------------------- weight gradients
// pol_wgrad_finish_kernel: adds the K-split pieces of launch_critic_wgrad in piece order in double, gathers each raw
// [cout][cin][kh][kw] element from its effective position, times inv_w; writes the convolution's gradient (no weight-norm, no bias)
int launch_pol_wgrad_finish(const PackDesc& D, int fan, int pieces, float inv_w, const float* slab, float* grad, hipStream_t s);

}  // namespace pnpx
