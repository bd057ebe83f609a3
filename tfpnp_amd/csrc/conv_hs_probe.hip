// Single-layer probe of the half-split convolution launcher (conv_hs.hip), for tests (tests/test_gpu_conv_hs.py): packs one layer's
// weights with the library's own packers, uploads them as pnpx_unet_load / pack_layer do, makes ONE launch_conv_hs call on tensors the
// caller laid out, and returns the launcher's status.  pnpx_conv_hs_probe_plan runs the same call with a plan-only sink installed
// (conv_hs.h: HsPlanSink), so what it reports IS the launcher's decision.  Nothing in the library calls either; they add no option.
#include <vector>

#include "common.h"
#include "conv_hs.h"

using namespace pnpx;

namespace {

struct SinkScope {   // installs a sink on this thread for the life of the scope
  HsPlanSink sink;
  explicit SinkScope(bool plan_only) {
    sink.plan_only = plan_only;
    hs_plan_sink() = &sink;
  }
  ~SinkScope() { hs_plan_sink() = nullptr; }
};

// Operands launch_conv_hs would silently drop, or dereference although they are null: refused here.  B, H, W: the geometry of the call.
int validate(const pnpx_conv_hs_probe_desc& d, int B, int H, int W) {
  auto bad = [](const char* what) {
    set_error("pnpx_conv_hs_probe: %s", what);
    return PNPX_ERR_ARG;
  };
  if (B <= 0 || H <= 0 || W <= 0 || d.cin <= 0 || d.cout <= 0 || d.G0 <= 0 || d.G1 < 0) return bad("non-positive size");
  const int mt = conv_hs_mt(d.cout);
  if (d.cout % mt != 0) return bad("cout is no multiple of the tile conv_hs_mt gives");
  if (!d.in0 && !d.first_x) return bad("no first source");
  if ((d.G1 > 0) != (d.in1 != nullptr)) return bad("in1 and G1 do not go together");
  if (d.in0_groups != 0 && d.in0_groups < d.G0) return bad("in0_groups below G0");
  const bool outc = d.outc_w != nullptr;
  if (outc && (!d.outc_b || !d.x_in || !d.out_img)) return bad("the fused out-conv needs outc_b, x_in and out_img");
  if (!outc && (d.outc_b || d.x_in || d.out_img || d.out_pre)) return bad("out-conv operands without outc_w");
  if (!outc && !d.out) return bad("no output tensor");
  if (outc && (d.critic_epi || d.dmask || d.res || d.taps != 0x1FF || d.pool_out)) return bad("the fused out-conv takes no other fused work");
  const bool first = d.first_x != nullptr;
  if (first && (!d.first_sigma || !d.first_w || !d.first_b)) return bad("the folded first convolution needs first_sigma, first_w and first_b");
  if (!first && (d.first_sigma || d.first_w || d.first_b)) return bad("first-convolution operands without first_x");
  if (first && (d.dmask || d.res || d.critic_epi || outc)) return bad("the folded first convolution takes no other fused work");
  if (d.pool_out && (!conv_hs_can_pool(H, W) || d.dmask || d.res || d.critic_epi || d.taps != 0x1FF))
    return bad("pool_out where no pool is fused");
  if (!d.critic_epi) {
    if (d.dmask && d.res) return bad("res beside dmask outside the critic epilogues");
    if (d.res_groups != 0 || d.alpha != 0.f) return bad("alpha / res_groups outside the critic epilogues");
  } else if (d.res_groups != 0 && (d.critic_epi != 2 || !d.res)) {
    return bad("res_groups without the input-gradient epilogue's res");
  }
  if (d.critic_epi < 0 || d.critic_epi > 2) return bad("unknown critic epilogue");
  if ((d.ups_h != 0) != (d.ups_w != 0)) return bad("ups_h and ups_w do not go together");
  return PNPX_OK;
}

// the one launch_conv_hs call of a descriptor on a packed layer
int launch(const pnpx_conv_hs_probe_desc& d, int B, int H, int W, const char* wpk, const float* bias, float inv_scale, const float* outc_w,
           const float* outc_b, const float* first_w, const float* first_b, const float* zero, unsigned* range_flag, hipStream_t s) {
  ConvLayerHs L;
  L.cin = d.cin;
  L.cout = d.cout;
  L.cin_pad = (d.cin + 15) / 16 * 16;
  L.mt = conv_hs_mt(d.cout);
  L.w = wpk;
  L.b = bias;
  L.inv_scale = inv_scale;
  ConvHsFuse f;
  f.pool_out = static_cast<char*>(d.pool_out);
  f.outc_w = outc_w;
  f.outc_b = outc_b;
  f.x_in = d.x_in;
  f.out_img = d.out_img;
  f.out_pre = d.out_pre;
  f.dmask = static_cast<const char*>(d.dmask);
  f.slope = d.slope;
  f.res = static_cast<const char*>(d.res);
  f.range_flag = range_flag;
  f.ups_h = d.ups_h;
  f.ups_w = d.ups_w;
  f.wreg = d.wreg;
  f.taps = d.taps;
  f.in0_groups = d.in0_groups;
  f.first_x = d.first_x;
  f.first_sigma = d.first_sigma;
  f.first_w = first_w;
  f.first_b = first_b;
  f.first_zero = zero;
  f.first_sigma_stride = d.first_sigma_stride;
  f.first_slope = d.first_slope;
  f.share = d.share;
  f.critic_epi = d.critic_epi;
  f.alpha = d.alpha;
  f.res_groups = d.res_groups;
  return launch_conv_hs(L, static_cast<const char*>(d.in0), d.G0, static_cast<const char*>(d.in1), d.G1, static_cast<char*>(d.out), B, H, W, f, s);
}

}  // namespace

extern "C" int pnpx_conv_hs_probe_plan(const pnpx_conv_hs_probe_desc* desc, int B, int H, int W, int* out) {
  if (!desc || !out) return 0;
  for (int i = 0; i < PNPX_CONV_HS_PLAN_INTS; ++i) out[i] = 0;
  if (validate(*desc, B, H, W) != PNPX_OK) return 0;
  SinkScope sc(true);
  // operands the launcher only tests for presence keep the descriptor's own (never dereferenced) pointers; the uploaded ones stand in
  // by the host arrays they would be copied from
  const int rc = launch(*desc, B, H, W, nullptr, nullptr, 1.f, desc->outc_w, desc->outc_b, desc->first_w, desc->first_b, nullptr, nullptr, nullptr);
  if (rc != PNPX_OK || !sc.sink.filled) return 0;
  const HsPlan& p = sc.sink.plan;
  const int v[PNPX_CONV_HS_PLAN_INTS] = {p.mt, p.nbw, p.mbw, p.nw, p.epi, p.ups, p.wreg, p.taps, p.w_mt, p.grid, (int)p.ntiles, p.plain_walk};
  for (int i = 0; i < PNPX_CONV_HS_PLAN_INTS; ++i) out[i] = v[i];
  return 1;
}

extern "C" int pnpx_conv_hs_probe(pnpx_ctx* ctx, const pnpx_conv_hs_probe_desc* desc, void* stream) {
  if (!ctx || !desc) {
    set_error("pnpx_conv_hs_probe: null context or descriptor");
    return PNPX_ERR_ARG;
  }
  const pnpx_conv_hs_probe_desc& d = *desc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PNPX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  PNPX_TRY(validate(d, d.B, d.H, d.W));
  if (!d.w) {
    set_error("pnpx_conv_hs_probe: null weights");
    return PNPX_ERR_ARG;
  }
  {   // what the launcher refuses, it refuses before it touches a pointer: its own status and message, nothing packed, nothing launched
    SinkScope sc(true);
    const int rc = launch(d, d.B, d.H, d.W, nullptr, nullptr, 1.f, d.outc_w, d.outc_b, d.first_w, d.first_b, nullptr, nullptr, nullptr);
    if (rc != PNPX_OK) return rc;
  }

  // host blob like pnpx_unet_load's / pack_layer's: 256-float aligned blocks, slack for the last weight block's DMA over-read
  std::vector<float> host;
  auto align = [&]() { host.resize((host.size() + 255) & ~(size_t)255, 0.f); };
  auto add = [&](const float* p, size_t n) {
    align();
    const size_t off = host.size();
    if (p) host.insert(host.end(), p, p + n);
    else host.resize(off + n, 0.f);
    return off;
  };
  const int mt = conv_hs_mt(d.cout), cin_pad = (d.cin + 15) / 16 * 16;
  int nt = 0;
  for (int t = 0; t < 9; ++t) nt += (d.taps >> t) & 1;
  const size_t n16 = (size_t)d.cout * cin_pad * nt * 2;   // f16 elements (hi + lo)
  host.resize((n16 + 1) / 2, 0.f);
  const float scale = d.taps == 0x1FF ? pack_conv_weights_hs(d.w, d.cout, d.cin, mt, reinterpret_cast<uint16_t*>(host.data()))
                                      : pack_conv_weights_hs_taps(d.w, d.cout, d.cin, mt, d.taps, reinterpret_cast<uint16_t*>(host.data()));
  const size_t boff = add(d.bias, d.cout);
  const size_t ow = add(d.outc_w, 32), ob = add(d.outc_b, 1), fw = add(d.first_w, 32 * 2 * 9), fb = add(d.first_b, 32), zo = add(nullptr, 1);
  host.resize(host.size() + 8192, 0.f);

  DeviceBuf wbuf;
  void* flag_host = nullptr;
  unsigned* flag_dev = nullptr;
  auto release = [&]() {
    if (wbuf.p) (void)hipFree(wbuf.p);
    if (flag_host) (void)hipHostFree(flag_host);
  };
  int rc = alloc_dev(wbuf, host.size() * sizeof(float), "probe weight");
  if (rc == PNPX_OK) {
    const hipError_t e = hipMemcpy(wbuf.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy(probe weights)", __FILE__, __LINE__);
  }
  if (rc == PNPX_OK && d.want_range_flag) {   // a word of its own, mapped like the context's (api.hip)
    hipError_t e = hipHostMalloc(&flag_host, 64, hipHostMallocMapped);
    if (e == hipSuccess) {
      *static_cast<unsigned*>(flag_host) = 0;
      void* dev = nullptr;
      e = hipHostGetDevicePointer(&dev, flag_host, 0);
      flag_dev = static_cast<unsigned*>(dev);
    }
    if (e != hipSuccess) rc = hip_fail(e, "hipHostMalloc(probe range flag)", __FILE__, __LINE__);
  }
  if (rc == PNPX_OK) {
    const float* base = static_cast<const float*>(wbuf.p);
    SinkScope sc(false);
    rc = launch(d, d.B, d.H, d.W, reinterpret_cast<const char*>(base), base + boff, 1.0f / (scale * HS_ASCALE), d.outc_w ? base + ow : nullptr,
                d.outc_w ? base + ob : nullptr, d.first_x ? base + fw : nullptr, d.first_x ? base + fb : nullptr, base + zo, flag_dev, s);
  }
  // the weights are this call's own: wait for the launch before they go
  const hipError_t e = hipStreamSynchronize(s);
  if (d.range_flag_out) *d.range_flag_out = flag_host ? *static_cast<volatile unsigned*>(flag_host) : 0u;
  release();
  if (rc == PNPX_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(probe)", __FILE__, __LINE__);
  return rc;
}
