// Kernel selection of the exact-fp32 convolution family (conv_f32_select.h).  Host code only.
#include "conv_f32_select.h"

namespace pnpx {

ConvF32Sel conv_f32_sel(const pnpx_ctx* ctx, int li) {
  ConvF32Sel v;
  v.winograd = ctx->opt_fp32_winograd != 0;
  v.wino8 = (ctx->opt_fp32_wino8 >> li) & 1;
  v.winof4 = (ctx->opt_fp32_winof4 >> li) & 1;
  v.winof4_entry = (ctx->opt_fp32_winof4_entries >> li) & 1;
  v.winof4_fuse_up = (ctx->opt_fp32_winof4_fuse_up >> li) & 1;
  v.winof4_c32 = (ctx->opt_fp32_winof4_c32 >> li) & 1;
  v.ksplit = ctx->opt_fp32_ksplit;
  v.ksplit_rule = ctx->opt_ksplit_rule;
  v.fuse_up = ctx->opt_fp32_fuse_up != 0;
  v.u = ctx->conv_wino_u[li];
  v.u_f4 = ctx->conv_winof4_u[li];
  v.u_f4c32 = ctx->conv_winof4_c32_u[li];
  v.u_bwd = ctx->conv_wino_u_bwd[li];
  return v;
}

// The DRUNet's layers are not numbered like the UNet's: any fp32_wino8_layers bit switches the 8-wave kernel on for all of them, and they
// run neither F(4x4,3x3) nor the K-split.
ConvF32Sel conv_f32_sel_drunet(const pnpx_ctx* ctx, const float* u, const float* u_bwd) {
  ConvF32Sel v;
  v.winograd = ctx->opt_fp32_winograd != 0;
  v.wino8 = ctx->opt_fp32_wino8 != 0;
  v.u = u;
  v.u_bwd = u_bwd;
  return v;
}

// Option fp32_ksplit: 0 = never; 1 (default) = the layers whose unsplit tiles cannot fill the chip for THIS call's batch (tiles per image x
// B_call < 256); 2 = every layer the geometry rule names, at every batch size (per-image results then bit-identical across ALL batch
// sizes; costs 4 % at 48 x 256^2, where the extra epilogues and the slab round trip buy nothing: profiles/r6_ksplit.txt)
static bool ksplit_on(const ConvF32Sel& v, int cout, int H, int W, int B_call) {
  if (v.ksplit == 2) return true;
  return v.ksplit == 1 && (long long)(H / 16) * (W / 16) * (cout / 64) * B_call < 256;
}

ConvF32Choice conv_f32_forward(const ConvF32Sel& v, int C0, int C1, int cout, int H, int W, int B_call) {
  ConvF32Choice c;
  if (!v.winograd || !v.u || !conv3x3_wino_ok(C0, C1, cout, H, W)) return c;
  c.fused = true;      // all three Winograd kernels write the pooled tensor too (one 2x2 output tile = one lane's four values)
  c.kernel = ConvF32Kernel::Wino4;
  if (!v.wino8 || !conv3x3_wino8_ok(C0, C1, cout, H, W)) return c;
  c.kernel = ConvF32Kernel::Wino8;
  if (ksplit_on(v, cout, H, W, B_call)) c.pieces = conv3x3_wino8_ksplit(C0, C1, cout, H, W, v.ksplit_rule);
  // F(4x4,3x3): plain single-source layers whose bit is set in both masks and that the K-split does not claim in this call.  Training
  // forwards take the same kernel as inference forwards: a solver's composed (differentiable) forward and its fused one then agree as
  // closely as before (tests/test_gpu_amp.py holds them to 1e-5 through the Onsager term, which amplifies a layer-level 7e-7 difference
  // past that bar); the backward pass keeps the F(2x2) adjoint kernels.
  if (c.pieces == 1 && v.winof4 && v.u_f4 && C1 == 0 && conv3x3_winof4_ok(C0, 0, cout, H, W)) c.kernel = ConvF32Kernel::WinoF4;
  // ... and its 32-cout instance under its own mask (the full-resolution 32 -> 32 layers; the K-split never names a 32-cout layer)
  else if (c.pieces == 1 && v.winof4_c32 && v.u_f4c32 && C1 == 0 && conv3x3_winof4_c32_ok(C0, 0, cout, H, W)) c.kernel = ConvF32Kernel::WinoF4C32;
  return c;
}

// A decoder entry that the K-split takes in this call (the 32 x 32 level's 768 -> 256 entry when the call cannot fill the chip: its
// 48-chunk tiles are the longest of the forward) runs UNFUSED -- the separate up-sampling kernel + the plain two-source instance, which
// splits; the fused instance's interpolation pipeline assumes a tile starts in its first, full-resolution source.  (The two forms agree to
// 2-5e-7; like the K-split itself this is a property of the call's class, not of the batch.)
// An entry that the 8-wave kernel would run in one piece goes to the F(4x4,3x3) kernel's two-source instance instead when its
// fp32_winof4_entries bit is set and its weights are packed (levels 1-3).  There the instance that up-samples the low-resolution second
// source itself runs (fused = true) when the entry's fp32_winof4_fuse_up bit is set and the geometry gives it two chunks of the first source
// (conv3x3_winof4_ups_ok); otherwise the entry runs behind the separate up-sampling kernel (fused = false).  Both forms write the same bits,
// and fp32_fuse_up has no say in either.  fp32_winof4_layers is not read here.
ConvF32Choice conv_f32_entry(const ConvF32Sel& v, int C0, int C1, int cout, int H, int W, int B_call) {
  ConvF32Choice c = conv_f32_forward(v, C0, C1, cout, H, W, B_call);
  if (c.kernel == ConvF32Kernel::Wino8 && c.pieces == 1 && v.winof4_entry && v.u_f4 && conv3x3_winof4_entry_ok(C0, C1, cout, H, W)) {
    c.kernel = ConvF32Kernel::WinoF4;
    c.fused = v.winof4_fuse_up && conv3x3_winof4_ups_ok(C0, C1, cout, H, W);
    return c;
  }
  c.fused = c.kernel == ConvF32Kernel::Wino8 && c.pieces == 1 && v.fuse_up && conv3x3_wino8_ups_ok(C0, C1, cout, H, W);
  return c;
}

ConvF32Choice conv_f32_last(const ConvF32Sel& v, int cin, int cout, int H, int W, int B_call) {
  ConvF32Choice c = conv_f32_forward(v, cin, 0, cout, H, W, B_call);
  c.fused = false;
  if (v.winograd && v.u && conv3x3_wino_outc_ok(cin, cout, H, W)) {      // 32 output channels: no K-split, no F(4x4,3x3)
    c.fused = true;
    c.kernel = v.wino8 && conv3x3_wino8_ok(cin, 0, cout, H, W) ? ConvF32Kernel::Wino8 : ConvF32Kernel::Wino4;
  }
  return c;
}

ConvF32Choice conv_f32_adjoint(const ConvF32Sel& v, int cin, int cout, int H, int W) {
  ConvF32Choice c;
  if (v.winograd && v.wino8 && v.u_bwd && conv3x3_wino8_ok(cin, 0, cout, H, W)) c.kernel = ConvF32Kernel::Wino8;
  return c;
}

// The fork's slices are 8-wave launches, so the three layers are decided with their F(4x4,3x3) weights withheld.
bool conv_f32_bottom_all8(const pnpx_ctx* ctx, int H, int W, int B_call, ConvF32Sel v[3], ConvF32Choice c[3]) {
  bool all8 = true;
  for (int k = 0; k < 3; ++k) {
    const ConvLayer& L = ctx->conv[12 + k];
    v[k] = conv_f32_sel(ctx, 12 + k);
    v[k].u_f4 = nullptr;
    c[k] = conv_f32_forward(v[k], L.cin, 0, L.cout, H, W, B_call);
    all8 = all8 && c[k].kernel == ConvF32Kernel::Wino8;
  }
  return all8;
}

int launch_conv_f32(const ConvF32Choice& c, const ConvF32Sel& v, const ConvLayer& L, const ConvF32Operands& a, hipStream_t s) {
  switch (c.kernel) {
    case ConvF32Kernel::WinoF4:      // no residual operand
      if (a.in1_lowres) return launch_conv3x3_winof4_ups(v.u_f4, L.b, L.cout, a.in0, a.C0, a.in1, a.C1, a.out, a.B, a.H, a.W, s, a.slope);
      return launch_conv3x3_winof4(v.u_f4, L.b, L.cout, a.in0, a.C0, a.in1, a.C1, a.out, a.B, a.H, a.W, s, a.slope, a.pool_out);
    case ConvF32Kernel::WinoF4C32:   // single source, no residual operand
      return launch_conv3x3_winof4_c32(v.u_f4c32, L.b, L.cout, a.in0, a.C0, a.out, a.B, a.H, a.W, s, a.slope, a.pool_out);
    case ConvF32Kernel::Wino8:
      return launch_conv3x3_wino8(v.u, L.b, L.cout, a.in0, a.C0, a.in1, a.C1, a.out, a.B, a.H, a.W, s, a.slope, a.res, a.pool_out,
                                  c.pieces > 1 ? a.ks_part : nullptr, v.ksplit_rule);
    case ConvF32Kernel::Wino4:
      return launch_conv3x3_wino(v.u, L.b, L.cout, a.in0, a.C0, a.in1, a.C1, a.out, a.B, a.H, a.W, s, a.slope, a.res, a.pool_out);
    case ConvF32Kernel::Direct:
      break;
  }
  return launch_conv3x3_act(L, a.in0, a.C0, a.in1, a.C1, a.out, a.B, a.H, a.W, a.slope, a.res, s);
}

}  // namespace pnpx

// conv_f32_entry as a host-only C entry, for tests (include/pnpx.h)
extern "C" int pnpx_conv_f32_entry_plan(int opts, int ksplit, int ksplit_rule, int C0, int C1, int cout, int H, int W, int B_call) {
  static const float packed = 0.f;      // stands for a layer's packed weights: the selector only asks whether they exist
  pnpx::ConvF32Sel v;
  v.winograd = opts & 1;
  v.wino8 = opts & 2;
  v.winof4 = opts & 4;
  v.winof4_entry = opts & 8;
  v.fuse_up = opts & 16;
  v.u = (opts & 32) ? &packed : nullptr;
  v.u_f4 = (opts & 64) ? &packed : nullptr;
  v.winof4_fuse_up = opts & 128;
  v.ksplit = ksplit;
  v.ksplit_rule = ksplit_rule;
  if (C0 <= 0 || C1 <= 0 || cout <= 0 || H <= 0 || W <= 0 || B_call <= 0) return -1;
  const pnpx::ConvF32Choice c = pnpx::conv_f32_entry(v, C0, C1, cout, H, W, B_call);
  return static_cast<int>(c.kernel) + 16 * c.pieces + 256 * (c.fused ? 1 : 0);
}

// conv_f32_forward and conv_f32_last likewise.  opts: bit 0 fp32_winograd, bit 1 the layer's fp32_wino8_layers bit, bit 2 its
// fp32_winof4_layers bit, bit 3 its fp32_winof4_c32 bit, bit 4 its F(2x2) weights are packed, bit 5 its F(4x4) weights, bit 6 its F(4x4)
// weights in the 32-cout instance's layout, bit 7 the layer is the network's last (conv_f32_last; C1 must be 0)
extern "C" int pnpx_conv_f32_forward_plan(int opts, int ksplit, int ksplit_rule, int C0, int C1, int cout, int H, int W, int B_call) {
  static const float packed = 0.f;
  pnpx::ConvF32Sel v;
  v.winograd = opts & 1;
  v.wino8 = opts & 2;
  v.winof4 = opts & 4;
  v.winof4_c32 = opts & 8;
  v.u = (opts & 16) ? &packed : nullptr;
  v.u_f4 = (opts & 32) ? &packed : nullptr;
  v.u_f4c32 = (opts & 64) ? &packed : nullptr;
  v.ksplit = ksplit;
  v.ksplit_rule = ksplit_rule;
  if (C0 <= 0 || C1 < 0 || cout <= 0 || H <= 0 || W <= 0 || B_call <= 0 || ((opts & 128) && C1 != 0)) return -1;
  const pnpx::ConvF32Choice c = (opts & 128) ? pnpx::conv_f32_last(v, C0, cout, H, W, B_call) : pnpx::conv_f32_forward(v, C0, C1, cout, H, W, B_call);
  return static_cast<int>(c.kernel) + 16 * c.pieces + 256 * (c.fused ? 1 : 0);
}
