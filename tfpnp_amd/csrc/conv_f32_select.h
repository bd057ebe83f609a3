// Which kernel runs a 3x3 layer of the exact-fp32 family (conv_mode 0), decided in one place: pure host functions over the options and the
// layer's geometry (no launches, no device state), and the one helper that turns a decision into its launch.  DESIGN.md "fp32 kernel
// selection" states the rule as a table.  The kernels, their packers and their *_ok predicates stay in their own files (conv3x3.h).
#pragma once
#include "conv3x3.h"

namespace pnpx {

enum class ConvF32Kernel { Direct, Wino4, Wino8, WinoF4, WinoF4C32 };   // conv3x3.hip, conv3x3_wino.hip, conv3x3_wino8.hip, conv3x3_winof4.hip (the last two)

struct ConvF32Choice {
  ConvF32Kernel kernel = ConvF32Kernel::Direct;
  int pieces = 1;       // K-split pieces of the 8-wave kernel (1 = no split)
  bool fused = false;   // the fused form the caller asked about is available: forward layer = the 2x2 max-pool epilogue, decoder entry =
                        // the up-sampling instance, last layer = the out-conv epilogue
  bool wino() const { return kernel != ConvF32Kernel::Direct; }
};

// The options as they apply to ONE layer, and that layer's packed weights (null = not packed)
struct ConvF32Sel {
  bool winograd = false;   // fp32_winograd
  bool wino8 = false;      // the layer's fp32_wino8_layers bit (DRUNet: any bit)
  bool winof4 = false;     // the layer's fp32_winof4_layers bit (DRUNet: never)
  bool winof4_entry = false;   // the layer's fp32_winof4_entries bit (decoder entries 15, 18, 21; DRUNet: never)
  bool winof4_fuse_up = false; // the layer's fp32_winof4_fuse_up bit (the same entries)
  bool winof4_c32 = false;     // the layer's fp32_winof4_c32 bit (layers 1, 2, 25; DRUNet: never)
  int ksplit = 0;          // fp32_ksplit (DRUNet: 0)
  int ksplit_rule = 1;     // fp32_ksplit_rule
  bool fuse_up = false;    // fp32_fuse_up
  const float* u = nullptr;      // F(2x2,3x3) weights (both Winograd kernels)
  const float* u_f4 = nullptr;   // F(4x4,3x3) weights
  const float* u_f4c32 = nullptr;   // F(4x4,3x3) weights in the 32-cout instance's layout
  const float* u_bwd = nullptr;  // F(2x2,3x3) weights of the adjoint layer
};
ConvF32Sel conv_f32_sel(const pnpx_ctx* ctx, int li);                                      // layer li of the UNet
ConvF32Sel conv_f32_sel_drunet(const pnpx_ctx* ctx, const float* u, const float* u_bwd);   // a DRUNet layer (weights in its own tables)

// B_call: the batch of the whole call (launch chains beside each other count as one call), which the fp32_ksplit = 1 rule reads
ConvF32Choice conv_f32_forward(const ConvF32Sel& v, int C0, int C1, int cout, int H, int W, int B_call);
// decoder entry (second source at H/2 x W/2): fused = the instance that up-samples it in the kernel runs; else the forward decision, or
// WinoF4 where fp32_winof4_entries puts the entry (fused where fp32_winof4_fuse_up and the geometry allow, else the two-source instance
// on the up-sampled tensor)
ConvF32Choice conv_f32_entry(const ConvF32Sel& v, int C0, int C1, int cout, int H, int W, int B_call);
// the UNet's last 3x3 layer: fused = the 1x1 out-conv + residual + clamp ride on `kernel`'s epilogue; else the forward decision
ConvF32Choice conv_f32_last(const ConvF32Sel& v, int cin, int cout, int H, int W, int B_call);
// input-gradient convolution cin -> cout gradient channels: Wino8 or Direct
ConvF32Choice conv_f32_adjoint(const ConvF32Sel& v, int cin, int cout, int H, int W);
// bottom level (layers 12..14 at H x W) as two launch chains of 8-wave launches: true when all three run on that kernel; c = their decisions
bool conv_f32_bottom_all8(const pnpx_ctx* ctx, int H, int W, int B_call, ConvF32Sel v[3], ConvF32Choice c[3]);

struct ConvF32Operands {
  const float* in0;
  int C0;
  const float* in1;   // second source (C1 channels) or null
  int C1;
  float* out;
  int B, H, W;
  float slope = 0.2f;
  const float* res = nullptr;
  float* pool_out = nullptr;   // MaxPool2d(2) of the output too (Winograd kernels only: ConvF32Choice::fused)
  float* ks_part = nullptr;    // K-split scratch of these B images (used when c.pieces > 1)
  bool in1_lowres = false;     // decoder entry whose choice is fused on the F(4x4,3x3) kernel: in1 is the second source at H/2 x W/2
};
int launch_conv_f32(const ConvF32Choice& c, const ConvF32Sel& v, const ConvLayer& L, const ConvF32Operands& a, hipStream_t s);

}  // namespace pnpx
