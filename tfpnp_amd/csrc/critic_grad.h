// Parameter gradients of the value network: launch interface of critic_grad.hip (driver: critic.hip::critic_param_grad).
#pragma once
#include "common.h"
#include "hs_rec.h"
#include "pack_desc.h"

namespace pnpx {

// One weight-gradient GEMM: slab[piece][co][tap][k] = sum over the piece's pixels of  gv[b] * G[b,co,y,x] * X[b,k,y+dy,x+dx]
// (both operands as stored: G carries s * 16, X carries 16 -- the finishing kernel undoes the scales), and behind every
// piece's tile block the same sum without X (bias gradient), cout floats.
struct WgradJob {
  const HsRec* G = nullptr;   // HS8 [B][Gg][h+2][w+2]: gradient with respect to the convolution's output
  const HsRec* X = nullptr;   // HS8 [B][Xg][h+2][w+2]: the tensor the forward launch read (its first K/8 groups are used)
  const float* gv = nullptr;  // [B]
  int Gg = 0, Xg = 0;
  int cout = 0, K = 0;        // multiples of 32
  int nt = 0, tap[9] = {};    // the launch's window (ascending taps of its mask)
  int B = 0, h = 0, w = 0;
};
// K-split: pieces the pixel axis of a layer is cut into -- a function of (cout, K, B, h, w) only
int critic_wgrad_pieces(int cout, int K, int B, int h, int w);
// chunks of 32 pixels each piece but the last takes (the last takes what is left)
int critic_wgrad_chunks_per_piece(int cout, int K, int B, int h, int w);
inline size_t critic_wgrad_piece_floats(int cout, int K, int nt) { return (size_t)cout * nt * K + cout; }
int launch_critic_wgrad(const WgradJob& J, float* slab, hipStream_t s);

// Finishing kernel of one convolution: adds the pieces in piece order, gathers each raw weight element from its effective
// position (the inverse of eff_src_offset), and takes the gradient through weight-norm; writes bias, weight_g, weight_v.
struct WnGradJob {
  PackDesc D;                 // the convolution's FORWARD packing descriptor
  unsigned src_b = 0, src_g = 0;   // floats into the parameter vector (src_v: D.src_v)
  int fan = 0, pieces = 0;
  float inv_w = 1.f, inv_b = 1.f;  // 1 / (s * 256), 1 / (s * 16)
};
int launch_critic_wn_grad(const WnGradJob& J, const float* slab, const float* params, float* grad, hipStream_t s);

// Threshold gradient, the identity  sum [clipped] * (W^T g + res) = <g, W m> + <res, m>  with m the clip indicator:
// m = 16 where the saved activation does not exceed thr, else 0, zero border (the whole padded tensor is written)
int launch_critic_clip_mask(const HsRec* act, HsRec* m, float thr, int B, int groups, int h, int w, hipStream_t s);
// out[b] = sum over the interior of image b of  g * wm  (G groups)  +  res * m  (the first resG groups; res may be null)
int launch_critic_alpha_dot(const HsRec* g, const HsRec* wm, int G, const HsRec* res, int resG, const HsRec* m, int mG, int B, int h, int w,
                            double* out, hipStream_t s);
// fc.weight, and per channel the head threshold's closed-form share: a20[c] = sum_b gv[b] * fc_w[c] / (h w) * #clipped(b, c)
int launch_critic_fc_grad(const HsRec* feat, const float* gv, const float* fc_w, float thr, int B, int h, int w, float* grad_fcw, double* a20,
                          hipStream_t s);
// the 17 thresholds and fc.bias: alpha_src[i] >= 0 names the parameter of chain threshold i (dots[i][B], times gv[b] * inv);
// the head's threshold is the sum of a20[512]
struct AlphaFinishJob {
  int alpha_src[21];
  int head_src = 0, fcb_src = 0;
  int B = 0;
  float inv = 1.f;            // 1 / (s * 256)
};
int launch_critic_alpha_finish(const AlphaFinishJob& J, const double* dots, const double* a20, const float* gv, float* grad, hipStream_t s);

}  // namespace pnpx
