// DRUNet denoiser forward on gfx950 (BASELINE config #5: "Poisson prox + DRUNet denoiser").
//
// The reference ships the KAIR building blocks but no model (tfpnp/pnp/denoiser/models/basicblock.py: conv :61-101,
// ResBlock :211-227, upsample_convtranspose :413-419, downsample_strideconv :437-446); the topology is KAIR's UNetRes
// (DRUNet, Zhang et al. 2021): bias-free, 4 scales of 64-128-256-512 channels, nb ResBlocks per scale each way,
//   x1 = head(cat[x, sigma]);  x2 = down1(x1) = strided2x2(ResBlocks(x1));  x3, x4 likewise;  v = body(x4);
//   v = up3(v + x4) = ResBlocks(convT2x2(v + x4));  up2(v + x3);  up1(v + x2);  out = tail(v + x1),
// behind the denoiser contract of UNetDenoiser2D.forward (denoiser/base.py:23-32): noise-level map as second input
// channel, output clamped to [0, 1].
//
// Everything runs on the half-split f16x3 MFMA convolution of the UNet (conv_hs.hip) over HS8 tensors:
//   * ResBlock = conv3x3 + ReLU (EPI_ACT, slope 0), then conv3x3 + residual add in the epilogue (EPI_RES, linear);
//   * strided 2x2 conv = space-to-depth re-layout (record copies) + a 1x1 convolution over 4*Cin channels;
//   * transposed 2x2 conv = a 1x1 convolution to 4*Cout channels + depth-to-space re-layout;
//     (1x1 convolutions are sparse-tap launches, conv_hs_taps.hip: only the centre tap is stored, copied and multiplied);
//   * head (K = 18) on the vector ALU straight from the fp32 image (conv_first_hs_kernel, as the UNet's first layer);
//   * tail (64 -> 1) as a 32-cout launch with the fused "1x1 + residual + clamp" epilogue (EPI_OUTC) selecting channel 0.
//
// The network itself -- layer table, weight tensors, topology walks, arena reservation -- is written once for both kernel
// families in drunet_net.h; this file is the half-split family: its launches, its weight packing and its arena plan.
#include <vector>

#include "common.h"
#include "conv_hs.h"
#include "drunet_net.h"
#include "fwd_glue.h"
#include "grad_common.h"
#include "hs_rec.h"
#include "hs_relayout.h"

namespace pnpx {

namespace {

// out = a + b on interior records (fp32 add of the recombined halves, re-split)
__global__ __launch_bounds__(256) void dru_add_kernel(const HsRec* __restrict__ a, const HsRec* __restrict__ b,
                                                      HsRec* __restrict__ out, int H, int W, size_t n) {   // n = B*G*H*W
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % W);
  size_t t = i / W;
  const int y = (int)(t % H);
  const size_t bg = t / H;
  const size_t r = (bg * (H + 2) + (y + 1)) * (W + 2) + x + 1;
  float va[8], vb[8];
  hs_unpack(a[r], va);
  hs_unpack(b[r], vb);
#pragma unroll
  for (int k = 0; k < 8; ++k) va[k] += vb[k];
  out[r] = hs_pack(va);
}

inline dim3 g1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

size_t drunet_num_params(int nb) {
  size_t n = 0;
  for (const DruLayer& d : dru_layers(nb)) n += layer_params(d);
  return n;
}

void drunet_free(pnpx_ctx* ctx) {
  DruNet& N = ctx->drunet;
  (void)hipDeviceSynchronize();
  if (N.weights.p) (void)hipFree(N.weights.p);
  dru_arena_free(N.arena);
  dru_arena_free(N.arena_grad);
  drunet_f32_free(ctx);
  N = DruNet();
}

int drunet_load(pnpx_ctx* ctx, const float* params, size_t n, int nb) {
  if (nb < 1 || nb > 8 || !params || n != drunet_num_params(nb)) {
    set_error("pnpx_drunet_load: expected %zu parameters for nb=%d (1..8), got %zu", nb >= 1 && nb <= 8 ? drunet_num_params(nb) : (size_t)0, nb, n);
    return PNPX_ERR_ARG;
  }
  const std::vector<DruLayer> L = dru_layers(nb);
  std::vector<float> host;   // blob: packed HS weights per MFMA layer, head weights (native), zero bias, e0, 0
  auto align = [&]() { host.resize((host.size() + 255) & ~(size_t)255, 0.f); };
  std::vector<size_t> off(L.size(), 0), offb(L.size(), 0);
  std::vector<ConvLayerHsDev> dev(L.size()), devb(L.size());
  std::vector<int> taps(L.size(), 0x1FF);
  std::vector<float> w3, wa;
  size_t head_off = 0, tailb_off = 0;
  // appends w[cout][cin][9] to the blob as one MFMA layer (the taps of tapmask only)
  auto pack = [&](const float* w, int cout, int cin, int tapmask, size_t* off_o, ConvLayerHsDev* D) {
    const int mt = conv_hs_mt(cout), cin_pad = (cin + 15) / 16 * 16;
    int ntap = 0;
    for (int t = 0; t < 9; ++t) ntap += (tapmask >> t) & 1;
    align();
    *off_o = host.size();
    const size_t n16 = (size_t)cout * cin_pad * ntap * 2;
    host.resize(host.size() + (n16 + 1) / 2, 0.f);
    const float scale = pack_conv_weights_hs_taps(w, cout, cin, mt, tapmask, reinterpret_cast<uint16_t*>(host.data() + *off_o));
    D->cin = cin;
    D->cout = cout;
    D->cin_pad = cin_pad;
    D->mt = mt;
    D->inv_scale = 1.0f / (scale * HS_ASCALE);
  };
  const float* src = params;
  for (size_t i = 0; i < L.size(); ++i) {
    const DruLayer& d = L[i];
    const float* w = src;
    src += layer_params(d);
    int cin, cout;
    dru_layer_w3(d, w, &cin, &cout, w3);
    const int tapmask = dru_is_1x1(d) ? 0x010 : 0x1FF;   // 1x1 layers store / multiply the centre tap only
    if (d.kind == 0) {   // head: native [64][2][3][3] for the VALU kernel
      align();
      head_off = host.size();
      host.insert(host.end(), w, w + layer_params(d));
    } else {
      pack(w3.data(), cout, cin, tapmask, &off[i], &dev[i]);
      taps[i] = tapmask;
    }
    if (d.kind == 5) {   // tail adjoint (1 -> 64 channels) on the vector ALU: conv_first weights [64][2][9], noise-map half zero
      align();
      tailb_off = host.size();
      host.resize(host.size() + 64 * 18, 0.f);
      for (int c = 0; c < 64; ++c)
        for (int t = 0; t < 9; ++t) host[tailb_off + (size_t)c * 18 + t] = w[(size_t)c * 9 + (8 - t)];
    } else {             // adjoint on the MFMA kernel, packed like a forward layer (the head's: 64 -> 2, padded to 32)
      const int rows = dru_adjoint_w3(w3, cin, cout, wa);
      pack(wa.data(), rows, cout, tapmask, &offb[i], &devb[i]);
    }
  }
  align();
  const size_t zoff = host.size();
  host.resize(host.size() + 1024, 0.f);          // zero bias (largest cout: 1024)
  align();
  const size_t eoff = host.size();
  host.resize(host.size() + 5 * 32, 0.f);        // e0 table: the fused tail epilogue's 1x1 weights select channel 0 (x 2^(4k): DruNet::shift)
  for (int k = 0; k < 5; ++k) host[eoff + 32 * k] = std::ldexp(1.0f, 4 * k);
  host.resize(host.size() + 1024, 0.f);          // + a zero scalar (outc bias) and DMA over-read slack
  drunet_free(ctx);
  if (ctx->weights.p) {           // a context holds ONE denoiser: loading a DRUNet unloads the UNet
    (void)hipFree(ctx->weights.p);
    ctx->weights = DeviceBuf();
    ctx->has_weights = false;
    train_cache_free(ctx);
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, host.size() * sizeof(float));
  if (e != hipSuccess) {
    set_error("DRUNet weight allocation of %zu bytes failed: %s", host.size() * sizeof(float), hipGetErrorString(e));
    return PNPX_ERR_ALLOC;
  }
  PNPX_HIP(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  DruNet& N = ctx->drunet;
  float* d = static_cast<float*>(p);
  for (size_t i = 0; i < L.size(); ++i) {
    dev[i].w = reinterpret_cast<char*>(d + off[i]);
    devb[i].w = reinterpret_cast<char*>(d + offb[i]);
  }
  N.layers = dev;
  N.layers_bwd = devb;
  N.tail_bwd_w = d + tailb_off;
  N.taps = taps;
  N.head_w = d + head_off;
  N.zero = d + zoff;
  N.e0 = d + eoff;
  N.nb = nb;
  N.weights.p = p;
  N.weights.bytes = host.size() * sizeof(float);
  N.params_host.assign(params, params + n);   // conv_mode 0 packs its own layouts from these on first use (drunet_f32.hip)
  N.loaded = true;
  return PNPX_OK;
}

namespace {

struct DruPlan : DruOffsets {   // byte offsets
  size_t IN0;         // gradient arena only: 32-channel output of the head's adjoint
  size_t zimg;        // [B][H][W] fp32 zeros (residual operand of the fused tail epilogue)
  size_t total;
};
size_t rec_bytes(int C, int h, int w) { return (size_t)(C / 8) * (h + 2) * (w + 2) * 32; }
DruPlan dru_plan(int capB, int H, int W, int nb_keep = 0, bool grad = false) {
  DruPlan P{};
  size_t off = 0;
  auto add = [&](size_t& o, size_t bytes_per_image) {
    o = off;
    off += bytes_per_image * capB;
    off = (off + 255) & ~(size_t)255;
  };
  for (int l = 0; l < 4; ++l) {
    const int h = H >> l, w = W >> l, c = DRU_NC[l];
    add(P.S[l], rec_bytes(c, h, w));
    add(P.P[l], rec_bytes(c, h, w));
    add(P.Q[l], rec_bytes(c, h, w));
    add(P.M[l], rec_bytes(c, h, w));
    if (l <= 2) add(P.U[l], rec_bytes(c, h, w));
    if (l >= 1) add(P.DT[l], rec_bytes(2 * c, h, w));
    for (int j = 0; j < (l == 3 ? 1 : 2) * nb_keep; ++j) add(P.MK[l][j], rec_bytes(c, h, w));
  }
  if (grad) add(P.IN0, rec_bytes(32, H, W));
  add(P.zimg, sizeof(float) * (size_t)H * W);
  P.total = off + (1u << 20);
  return P;
}

// The re-layouts and the skip sum, as both walks launch them on B images at H x W (level 0) on stream s.
struct HsGlue {
  int B, H, W;
  hipStream_t s;
  static const HsRec* rec(const char* p) { return reinterpret_cast<const HsRec*>(p); }
  static HsRec* rec(char* p) { return reinterpret_cast<HsRec*>(p); }
  int s2d(int l, const char* in, char* out) const { return launch_s2d_hs(rec(in), rec(out), B, DRU_NC[l] / 8, H >> l, W >> l, s); }
  int d2s(int l, const char* in, char* out) const { return launch_d2s_hs(rec(in), rec(out), B, DRU_NC[l] / 8, H >> (l + 1), W >> (l + 1), s); }
  int add(int l, const char* a, const char* b, char* o) const {
    return launch_add_hs(rec(a), rec(b), rec(o), (size_t)B * (DRU_NC[l] / 8), H >> l, W >> l, s);
  }
};

// The forward's launches over one slice of the batch (x / sigma / out / out_pre / zimg point at its first image).
struct HsForward : HsGlue {
  const DruNet& N;
  const float *x, *sigma;
  int sigma_stride;
  float *out, *out_pre;
  const float* zimg;
  char* unwritten;   // the tail launch's record output operand: not written (EPI_OUTC stores the images)
  unsigned* range_flag;
  int chains;        // launch chains running side by side: the launch table plans for all of them (f.share)

  // one MFMA convolution launch: layer li, `in` (cin channels) -> `outp`
  int conv(size_t li, const char* in, char* outp, int h, int w, float slope, const char* res, bool tail = false) const {
    const ConvLayerHsDev& D = N.layers[li];
    const ConvLayerHs Lh = hs_layer(D, N.zero);
    ConvHsFuse f;
    f.slope = slope;
    f.res = res;
    f.range_flag = range_flag;
    f.wreg = 0;
    f.taps = N.taps[li];
    f.share = chains;
    if (tail) {
      f.outc_w = N.e0 + 32 * (N.shift / 4);   // selects channel 0 and multiplies the 2^-shift of the head back
      f.outc_b = N.e0 + 5 * 32;               // a zero
      f.x_in = zimg;
      f.out_img = out;
      f.out_pre = out_pre;
    }
    return launch_conv_hs(Lh, in, D.cin_pad / 8, nullptr, 0, outp, B, h, w, f, s);
  }
  // head: cat[x, sigma] -> 64 channels, linear (VALU, exact fp32 FMA chains); this pass runs on inputs scaled by 2^-shift (DruNet::shift)
  int head(char* s0) const {
    return launch_conv_first_hs(x, sigma, sigma_stride, N.head_w, N.zero, rec(s0), DRU_NC[0], B, H, W, 1.0f, std::ldexp(HS_ASCALE, -N.shift), s);
  }
  int tail(size_t li, const char* m0) const { return conv(li, m0, unwritten, H, W, 1.f, nullptr, true); }
};

}  // namespace

int drunet_denoise(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, float* out, float* out_pre,
                   int B, int H, int W, hipStream_t s, bool keep_mids) {
  DruNet& N = ctx->drunet;
  if (!N.loaded) {
    set_error("DRUNet denoiser called before pnpx_drunet_load");
    return PNPX_ERR_NO_WEIGHTS;
  }
  if (B <= 0 || H < 8 || W < 8 || (H & 7) || (W & 7)) {
    set_error("DRUNet: need B > 0 and H, W positive multiples of 8 (three 2x2 strided convolutions; got B=%d H=%d W=%d)", B, H, W);
    return PNPX_ERR_SHAPE;
  }
  if (ctx->conv_mode != CONV_HS) {
    return drunet_denoise_f32(ctx, x, sigma, sigma_stride, out, out_pre, B, H, W, s, keep_mids);   // fp32 arithmetic throughout (drunet_f32.hip)
  }
  PNPX_TRY(dru_arena_reserve(N.arena, B, H, W, keep_mids, KEEPS_STAY, "arena",
                             [&](int images, bool keeps) { return dru_plan(images, H, W, keeps ? N.nb : 0).total; }));
  const DruPlan Pl = dru_plan(N.arena.capB, H, W, N.arena.keeps ? N.nb : 0);
  char* const A = static_cast<char*>(N.arena.buf.p);
  unsigned* const range_flag = ctx->opt_range_guard ? ctx->range_flag_dev : nullptr;
  const int chains = keep_mids ? 1 : launch_chains(ctx, B, H, W);
  // The forward over images b0 .. b0 + nB - 1 of the arena on stream st (x / sigma / out already point at the first of them): every
  // tensor is [image][group][h + 2][w + 2] records, so a slice of the batch is a contiguous piece of each -- independent launch
  // chains over slices run side by side on side streams exactly as for the UNet (unet.hip: launch_chains; bit-identical per image).
  auto run = [&](int b0, int nB, const float* x, const float* sigma, float* out, float* out_pre, hipStream_t st) -> int {
    const DruOffsets o = dru_slice(Pl, b0, [&](int C, int l) { return rec_bytes(C, H >> l, W >> l); });
    const float* zimg = reinterpret_cast<const float*>(A + Pl.zimg) + (size_t)H * W * b0;
    const HsForward f{{nB, H, W, st}, N, x, sigma, sigma_stride, out, out_pre, zimg, A + o.P[0], range_flag, chains};
    return dru_forward_walk(f, A, o, N.nb, H, W, keep_mids);
  };
  if (chains <= 1) return run(0, B, x, sigma, out, out_pre, s);
  const size_t px = (size_t)H * W;
  return fan_out_chains(ctx, chains, B, s, [&](int lo, int hi, hipStream_t st) -> int {
    return run(lo, hi - lo, x + lo * px, sigma + (size_t)lo * sigma_stride, out + lo * px, out_pre ? out_pre + lo * px : nullptr, st);
  });
}

// ------------------------------------------------------------------------------------------------ VJP
namespace {

// g_pre = grad_out / m on pixels whose pre-clamp output lies in [0, 1] (torch.clamp's backward mask is inclusive), else 0
__global__ __launch_bounds__(256) void dru_tail_mask_kernel(const float* __restrict__ g_out, const float* __restrict__ pre,
                                                            const float2* __restrict__ sc, float* __restrict__ g_pre, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p = pre[i];
  g_pre[i] = (p >= 0.f && p <= 1.f) ? g_out[i] * sc->x : 0.f;
}

// The VJP's launches (dataflow: drunet_net.h dru_backward_walk) on the forward kernels with the adjoint layers (layers_bwd).
// Gradients are HS8 tensors scaled to max |grad_out| <= 1 (unet_bwd.hip): gscale = {1/m, m}.
struct HsBackward : HsGlue {
  const DruNet& N;
  const float *grad_out, *pre;
  float *g_pre, *part, *grad_x, *grad_sigma;
  float2* gscale;
  unsigned *gmax_bits, *range_flag;
  char* in0;           // 32-channel output of the head's adjoint
  const float* zimg;   // zeros: the DRUNet has no input residual

  int conv(int li, const char* in, char* outp, int h, int w, const char* dmask, const char* res) const {
    const ConvLayerHsDev& D = N.layers_bwd[li];
    const ConvLayerHs Lh = hs_layer(D, N.zero);
    ConvHsFuse f;
    f.slope = dmask ? 0.f : 1.f;
    f.dmask = dmask;
    f.res = res;
    f.range_flag = range_flag;
    f.wreg = 0;
    f.taps = N.taps[li];
    return launch_conv_hs(Lh, in, D.cin_pad / 8, nullptr, 0, outp, B, h, w, f, s);
  }
  int seed(char* s0) const {
    const size_t npix = (size_t)B * H * W;
    PNPX_HIP(hipMemsetAsync(gmax_bits, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(absmax_kernel, dim3(512), dim3(256), 0, s, grad_out, npix, gmax_bits);
    hipLaunchKernelGGL(grad_scale_kernel, dim3(1), dim3(1), 0, s, gmax_bits, gscale);
    PNPX_TRY(launch_tail_mask_hs(grad_out, pre, gscale, g_pre, npix, s));
    return launch_conv_first_hs(g_pre, N.zero, 0, N.tail_bwd_w, N.zero, rec(s0), DRU_NC[0], B, H, W, 1.0f, HS_ASCALE, s);
  }
  // head: 64 -> (image, noise map) gradients; no residual path (g_res = zeros)
  int input_grad(const char* m0) const {
    PNPX_TRY(conv(0, m0, in0, H, W, nullptr, nullptr));
    hipLaunchKernelGGL(input_grad_hs_kernel, dim3(SIG_CHUNKS, B), dim3(256), 0, s, reinterpret_cast<const HsRec*>(in0), zimg, grad_x,
                       part, gscale, H, W);
    PNPX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sigma_grad_final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, part, grad_sigma, B);
    PNPX_LAUNCH_CHECK();
    return PNPX_OK;
  }
};

}  // namespace

// ---- the launchers of the kernels above and of hs_relayout.h (fwd_glue.h): the walks and, for tests, pnpx_fwd_glue_probe go through them
int launch_s2d_hs(const HsRec* in, HsRec* out, int B, int G, int h, int w, hipStream_t s) {
  const size_t n = (size_t)B * 4 * G * (h / 2) * (w / 2) * 2;
  hipLaunchKernelGGL(hs_s2d_kernel, g1(n), dim3(256), 0, s, reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out), G, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_d2s_hs(const HsRec* in, HsRec* out, int B, int G, int h, int w, hipStream_t s) {
  const size_t n = (size_t)B * G * (2 * h) * (2 * w) * 2;
  hipLaunchKernelGGL(hs_d2s_kernel, g1(n), dim3(256), 0, s, reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out), G, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_add_hs(const HsRec* a, const HsRec* b, HsRec* o, size_t planes, int h, int w, hipStream_t s) {
  const size_t n = planes * h * w;
  hipLaunchKernelGGL(dru_add_kernel, g1(n), dim3(256), 0, s, a, b, o, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_tail_mask_hs(const float* g_out, const float* pre, const float2* sc, float* g_pre, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(dru_tail_mask_kernel, g1(n), dim3(256), 0, s, g_out, pre, sc, g_pre, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int drunet_denoise_backward(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, const float* grad_out,
                            float* grad_x, float* grad_sigma, int B, int H, int W, hipStream_t s) {
  DruNet& N = ctx->drunet;
  const size_t npix = (size_t)B * H * W;
  void* sp;
  PNPX_TRY(ctx_scratch(ctx, (3 * npix + (size_t)B * SIG_CHUNKS) * sizeof(float) + 8192, &sp));
  float* out_tmp = static_cast<float*>(sp);
  float* pre = out_tmp + npix;
  float* g_pre = pre + npix;
  float* part = g_pre + npix;
  float2* gscale = reinterpret_cast<float2*>(part + (((size_t)B * SIG_CHUNKS + 63) & ~(size_t)63));   // {1/m, m}
  unsigned* gmax_bits = reinterpret_cast<unsigned*>(gscale + 1);

  // forward of the context's family, keeping the ReLU output of every ResBlock
  PNPX_TRY(drunet_denoise(ctx, x, sigma, sigma_stride, out_tmp, pre, B, H, W, s, true));
  if (ctx->conv_mode != CONV_HS)      // fp32 arithmetic throughout (drunet_f32.hip, r5)
    return drunet_denoise_backward_f32(ctx, grad_out, pre, g_pre, part, grad_x, grad_sigma, B, H, W, s);
  const DruPlan F = dru_plan(N.arena.capB, H, W, N.nb);
  char* const FA = static_cast<char*>(N.arena.buf.p);
  // gradient arena (zero borders: gradients are convolution inputs of the adjoint convolutions)
  PNPX_TRY(dru_arena_reserve(N.arena_grad, B, H, W, false, KEEPS_STAY, "gradient arena",
                             [&](int images, bool) { return dru_plan(images, H, W, 0, true).total; }));
  const DruPlan G = dru_plan(N.arena_grad.capB, H, W, 0, true);
  char* const GA = static_cast<char*>(N.arena_grad.buf.p);
  const HsBackward f{{B, H, W, s}, N, grad_out, pre, g_pre, part, grad_x, grad_sigma, gscale, gmax_bits,
                     ctx->opt_range_guard ? ctx->range_flag_dev : nullptr, GA + G.IN0, reinterpret_cast<const float*>(FA + F.zimg)};
  return dru_backward_walk(f, GA, G, FA, F, N.nb, H, W);
}

}  // namespace pnpx
