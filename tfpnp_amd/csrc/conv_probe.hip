// Single-layer probe of the fp32 3x3 convolution kernels (conv_mode 0), for tests (tests/test_gpu_conv_layers.py): packs one layer's
// weights with the packers pnpx_unet_load uses, launches ONE of the kernels on tensors the caller laid out, and returns.  Nothing in the
// library calls it; it adds no option and reads no state of the context beyond its device.
#include "common.h"
#include "conv3x3.h"
#include "fwd_glue.h"

using namespace pnpx;

namespace {

bool is_grad(int kind) { return kind == PNPX_PROBE_DIRECT_GRAD || kind == PNPX_PROBE_WINO8_GRAD; }

// cout tile of the direct kernel for a forward layer (conv_pack_mt / conv_pack_cc, as pnpx_unet_load packs it); 0 = no instance
int direct_ct(int C0, int C1, int cout) {
  if (C0 <= 0 || C1 < 0 || cout <= 0) return 0;
  const int mt = conv_pack_mt(cout), cc = conv_pack_cc(C0 + C1);
  if (C0 % cc != 0 || C1 % cc != 0 || cout % mt != 0 || (mt == 64 && cc != 8)) return 0;
  return mt;
}
// ... and for an adjoint layer (pnpx_unet_load: 64 where it divides the zero-padded channel count, else 32; chunks of 8)
int direct_grad_ct(int C0, int cout) {
  if (C0 <= 0 || C0 % 8 != 0 || cout <= 0 || cout % 32 != 0) return 0;
  return cout % 64 == 0 ? 64 : 32;
}

}  // namespace

extern "C" int pnpx_conv3x3_probe_plan(int kind, int C0, int C1, int cout, int H, int W, int ks_rule) {
  if (C0 <= 0 || C1 < 0 || cout <= 0 || H <= 0 || W <= 0) return 0;
  const int wct = cout % 64 == 0 ? 64 : 32;   // the Winograd kernels' tile follows cout alone
  switch (kind) {
    case PNPX_PROBE_DIRECT: return direct_ct(C0, C1, cout);
    case PNPX_PROBE_WINO4: return conv3x3_wino_ok(C0, C1, cout, H, W) ? wct : 0;
    case PNPX_PROBE_WINO8: return conv3x3_wino8_ok(C0, C1, cout, H, W) ? wct : 0;
    case PNPX_PROBE_WINO8_KSPLIT:
      return conv3x3_wino8_ok(C0, C1, cout, H, W) ? wct + 256 * conv3x3_wino8_ksplit(C0, C1, cout, H, W, ks_rule) : 0;
    case PNPX_PROBE_WINOF4: return conv3x3_winof4_ok(C0, C1, cout, H, W) ? 64 : 0;
    case PNPX_PROBE_WINO8_UPS: return conv3x3_wino8_ups_ok(C0, C1, cout, H, W) ? wct : 0;
    case PNPX_PROBE_DIRECT_GRAD: return C1 == 0 ? direct_grad_ct(C0, cout) : 0;
    case PNPX_PROBE_WINO8_GRAD: return C1 == 0 && conv3x3_wino8_ok(C0, 0, cout, H, W) ? wct : 0;
    case PNPX_PROBE_WINOF4_2SRC: return C1 > 0 && conv3x3_winof4_entry_ok(C0, C1, cout, H, W) ? 64 : 0;
    case PNPX_PROBE_WINOF4_UPS: return 0;      // reserved before the up-sampling instance existed: still refuses every geometry
    case PNPX_PROBE_WINOF4_FUSE_UP: return C1 > 0 && conv3x3_winof4_ups_ok(C0, C1, cout, H, W) ? 64 : 0;
    case PNPX_PROBE_WINOF4_C32: return conv3x3_winof4_c32_ok(C0, C1, cout, H, W) ? 32 : 0;
  }
  return 0;
}

extern "C" int pnpx_conv3x3_probe(pnpx_ctx* ctx, int kind, const float* w_host, const float* bias_host, int cout, const float* in0, int C0,
                                  const float* in1, int C1, float* out, const float* res, const float* mask, float slope, float* pool_out,
                                  int ks_rule, int B, int H, int W, void* stream) {
  if (!ctx) {
    set_error("null context");
    return PNPX_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  PNPX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool grad = is_grad(kind);
  if (kind < PNPX_PROBE_DIRECT || (kind > PNPX_PROBE_WINOF4_UPS && kind != PNPX_PROBE_WINOF4_FUSE_UP && kind != PNPX_PROBE_WINOF4_C32)) {      // (10 is no kind)
    set_error("pnpx_conv3x3_probe: unknown kind %d", kind);
    return PNPX_ERR_ARG;
  }
  if (!w_host || (!grad && !bias_host) || !in0 || !out || B <= 0 || H <= 0 || W <= 0 || cout <= 0 || C0 <= 0 || C1 < 0 || (C1 > 0 && !in1)) {
    set_error("pnpx_conv3x3_probe: null pointer or non-positive size");
    return PNPX_ERR_ARG;
  }
  // operands a kind has no place for are refused, never dropped
  const bool takes_res = kind == PNPX_PROBE_DIRECT || kind == PNPX_PROBE_WINO4 || kind == PNPX_PROBE_WINO8;
  const bool takes_pool = kind == PNPX_PROBE_WINO4 || kind == PNPX_PROBE_WINO8 || kind == PNPX_PROBE_WINOF4 || kind == PNPX_PROBE_WINOF4_2SRC ||
                          kind == PNPX_PROBE_WINOF4_C32;
  if ((res && !takes_res) || (pool_out && !takes_pool) || (mask && !grad) || (res && pool_out)) {
    set_error("pnpx_conv3x3_probe: kind %d takes no %s operand", kind, res && !takes_res ? "res" : (mask && !grad ? "mask" : "pool_out"));
    return PNPX_ERR_ARG;
  }
  if ((grad || kind == PNPX_PROBE_WINOF4 || kind == PNPX_PROBE_WINOF4_C32) && C1 != 0) {
    set_error("pnpx_conv3x3_probe: kind %d is single-source (C1 = %d)", kind, C1);
    return PNPX_ERR_SHAPE;
  }
  if (kind == PNPX_PROBE_WINOF4_UPS || ((kind == PNPX_PROBE_WINOF4_2SRC || kind == PNPX_PROBE_WINOF4_FUSE_UP) && C1 == 0)) {
    set_error(kind == PNPX_PROBE_WINOF4_UPS ? "pnpx_conv3x3_probe: unsupported geometry (kind %d has no instance)"
                                            : "pnpx_conv3x3_probe: unsupported geometry (kind %d needs a second source)", kind);
    return PNPX_ERR_SHAPE;
  }
  const int cin = C0 + C1;
  const int plan = pnpx_conv3x3_probe_plan(kind, C0, C1, cout, H, W, ks_rule);

  // one launch of the kind on packed weights `pk` (ConvLayer::w / u), bias `b` and the K-split scratch `ks`
  auto launch = [&](const float* pk, const float* b, float* ks) -> int {
    ConvLayer L;
    L.cin = grad ? C0 : cin;
    L.cout = cout;
    L.w = const_cast<float*>(pk);
    L.b = const_cast<float*>(b);
    switch (kind) {
      case PNPX_PROBE_DIRECT:
        L.mt = conv_pack_mt(cout);
        L.cc = conv_pack_cc(cin);
        return launch_conv3x3_act(L, in0, C0, in1, C1, out, B, H, W, slope, res, s);
      case PNPX_PROBE_WINO4: return launch_conv3x3_wino(pk, b, cout, in0, C0, in1, C1, out, B, H, W, s, slope, res, pool_out);
      case PNPX_PROBE_WINO8: return launch_conv3x3_wino8(pk, b, cout, in0, C0, in1, C1, out, B, H, W, s, slope, res, pool_out, nullptr, ks_rule);
      case PNPX_PROBE_WINO8_KSPLIT: return launch_conv3x3_wino8(pk, b, cout, in0, C0, in1, C1, out, B, H, W, s, slope, nullptr, nullptr, ks, ks_rule);
      case PNPX_PROBE_WINOF4: return launch_conv3x3_winof4(pk, b, cout, in0, C0, nullptr, 0, out, B, H, W, s, slope, pool_out);
      case PNPX_PROBE_WINOF4_2SRC: return launch_conv3x3_winof4(pk, b, cout, in0, C0, in1, C1, out, B, H, W, s, slope, pool_out);
      case PNPX_PROBE_WINO8_UPS: return launch_conv3x3_wino8_ups(pk, b, cout, in0, C0, in1, C1, out, B, H, W, s, slope);
      case PNPX_PROBE_WINOF4_FUSE_UP: return launch_conv3x3_winof4_ups(pk, b, cout, in0, C0, in1, C1, out, B, H, W, s, slope);
      case PNPX_PROBE_WINOF4_C32: return launch_conv3x3_winof4_c32(pk, b, cout, in0, C0, out, B, H, W, s, slope, pool_out);
      case PNPX_PROBE_DIRECT_GRAD:
        L.mt = cout % 64 == 0 ? 64 : 32;
        L.cc = 8;
        return launch_conv3x3_grad(L, in0, out, mask, B, H, W, s, nullptr, slope);
      case PNPX_PROBE_WINO8_GRAD: return launch_conv3x3_wino8_grad(pk, b, cout, in0, C0, out, mask, slope, B, H, W, s);
    }
    return PNPX_ERR_ARG;
  };
  if (!plan) {   // the launcher refuses the geometry before it touches a pointer: its own message, nothing packed, nothing launched
    const int rc = launch(nullptr, nullptr, nullptr);
    if (rc == PNPX_OK) {
      set_error("pnpx_conv3x3_probe: the plan refuses a geometry kind %d's launcher accepts (%d + %d -> %d channels, %d x %d)", kind, C0, C1, cout, H, W);
      return PNPX_ERR_SHAPE;
    }
    return rc;
  }

  // host blob like pnpx_unet_load's: packed weights, bias (zeros for the adjoint kinds), slack for the last weight block's DMA over-read
  std::vector<float> host, wt;
  switch (kind) {
    case PNPX_PROBE_DIRECT:
      host.resize((size_t)cout * cin * 9);
      pack_conv_weights(w_host, cout, cin, conv_pack_mt(cout), conv_pack_cc(cin), host.data());
      break;
    case PNPX_PROBE_WINOF4:
    case PNPX_PROBE_WINOF4_2SRC:
    case PNPX_PROBE_WINOF4_FUSE_UP:
      host.resize(conv3x3_winof4_floats(cout, cin));
      pack_conv_weights_winof4(w_host, cout, cin, host.data());
      break;
    case PNPX_PROBE_WINOF4_C32:
      host.resize(conv3x3_winof4_floats(cout, cin));
      pack_conv_weights_winof4_c32(w_host, cout, cin, host.data());
      break;
    case PNPX_PROBE_DIRECT_GRAD:   // w_host: the forward layer's [C0][cout][3][3]
      host.resize((size_t)cout * C0 * 9);
      pack_conv_weights_transposed(w_host, C0, cout, cout, cout % 64 == 0 ? 64 : 32, 8, host.data());
      break;
    case PNPX_PROBE_WINO8_GRAD:
      transpose_flip_conv_weights(w_host, C0, cout, cout, wt);
      host.resize(conv3x3_wino_floats(cout, C0));
      pack_conv_weights_wino(wt.data(), cout, C0, host.data());
      break;
    default:
      host.resize(conv3x3_wino_floats(cout, cin));
      pack_conv_weights_wino(w_host, cout, cin, host.data());
  }
  host.resize((host.size() + 255) & ~(size_t)255, 0.f);
  const size_t boff = host.size();
  if (grad) host.resize(boff + cout, 0.f);
  else host.insert(host.end(), bias_host, bias_host + cout);
  host.resize(host.size() + 1024, 0.f);

  DeviceBuf wbuf, ksbuf;
  auto release = [&]() {
    if (wbuf.p) (void)hipFree(wbuf.p);
    if (ksbuf.p) (void)hipFree(ksbuf.p);
  };
  int rc = alloc_dev(wbuf, host.size() * sizeof(float), "probe weight");
  if (rc == PNPX_OK && kind == PNPX_PROBE_WINO8_KSPLIT) rc = alloc_dev(ksbuf, conv3x3_wino8_ksplit_bytes_per_image() * (size_t)B, "probe K-split scratch");
  if (rc == PNPX_OK) {
    const hipError_t e = hipMemcpy(wbuf.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy(probe weights)", __FILE__, __LINE__);
  }
  if (rc == PNPX_OK) rc = launch(static_cast<float*>(wbuf.p), static_cast<float*>(wbuf.p) + boff, static_cast<float*>(ksbuf.p));
  // the weights and the scratch are this call's own: wait for the launch before they go
  const hipError_t e = hipStreamSynchronize(s);
  release();
  if (rc == PNPX_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(probe)", __FILE__, __LINE__);
  return rc;
}

// The fp32 family's separate up-sampling launch on tensors the caller laid out, for tests: what a decoder entry's second source is when
// no kernel up-samples it itself.
extern "C" int pnpx_upsample2x_probe(pnpx_ctx* ctx, const float* src, float* dst, int planes, int h, int w, void* stream) {
  if (!ctx || !src || !dst || planes <= 0 || h <= 0 || w <= 0) {
    set_error("pnpx_upsample2x_probe: null pointer or non-positive size");
    return PNPX_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  PNPX_HIP(hipSetDevice(ctx->device));
  return launch_upsample2x_f32(FG_AUTO, src, dst, (size_t)planes, h, w, 2 * h, 2 * w, static_cast<hipStream_t>(stream));
}
