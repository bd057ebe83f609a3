// DRUNet denoiser forward on the fp32 kernel family (conv_mode 0): the precision-matched mode of BASELINE config #5's prior.
//
// Same network and same denoiser contract as drunet.hip (KAIR UNetRes assembled from the reference's building blocks,
// tfpnp/pnp/denoiser/models/basicblock.py: conv :61-101, ResBlock :211-227, upsample_convtranspose :413-419,
// downsample_strideconv :437-446; denoiser/base.py:23-32), in fp32 arithmetic throughout like the reference's:
//   * 3x3 layers: Winograd F(2x2,3x3) on the fp32 MFMA (conv3x3_wino.hip) where the level's size is a multiple of 16, the direct
//     fp32 MFMA kernel (conv3x3.hip) elsewhere; ReLU = negative slope 0, the ResBlock skip = the kernels' residual operand;
//   * strided 2x2 conv = space-to-depth re-layout + 1x1 conv over 4*Cin phase-major channels, transposed 2x2 conv = 1x1 conv to
//     4*Cout phase-major channels + depth-to-space; the 1x1 convolutions run on the direct kernel's one-tap instance
//     (conv3x3.hip: launch_conv1x1_act; as centre-tap 3x3 launches they took 23 of 89 ms);
//   * head (2 -> 64) on the direct kernel's 2-channel path from a padded [x | sigma] tensor, tail (64 -> 1) as a 32-cout launch whose
//     channel 0 is clamped into the output image.
// Activations are padded planar fp32 tensors (common.h), one arena per context.  Weights are packed on the first conv_mode-0 call
// from the host copy drunet_load keeps (the fp64 Winograd transform of 32 M weights takes seconds; a context that never leaves
// conv_mode 1 does not pay for it).  r5: the VJP in the same arithmetic (drunet_denoise_backward_f32, bottom of this file): the forward is
// re-computed keeping every ResBlock's ReLU output, then the adjoint chain runs on the fp32 kernels (Winograd adjoints with the
// ReLU' mask / the skip's add in their epilogues).
//
// The network itself -- layer table, weight tensors, topology walks, arena reservation -- is written once for both kernel
// families in drunet_net.h; this file is the fp32 family: its launches, its weight packing and its arena plan.
#include <vector>

#include "common.h"
#include "conv_f32_select.h"
#include "drunet_net.h"
#include "fwd_glue.h"
#include "grad_common.h"

namespace pnpx {

namespace {

inline dim3 g1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// ([x | sigma] -> padded 2-channel tensor: unet.hip's prep_input_kernel, launch_prep_input_f32)
// space-to-depth: in [B][C][h][w] -> out [B][4C][h/2][w/2], channel (2 dy + dx) * C + c = in[c][2y + dy][2x + dx]
__global__ __launch_bounds__(256) void f32_s2d_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int h, int w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // over out interior: B * 4C * (h/2) * (w/2)
  if (i >= n) return;
  const int wo = w / 2, ho = h / 2;
  const int x = (int)(i % wo);
  size_t t = i / wo;
  const int y = (int)(t % ho);
  t /= ho;
  const int k = (int)(t % (4 * C));
  const size_t b = t / (4 * C);
  const int ph = k / C, c = k - ph * C;
  const int dy = ph >> 1, dx = ph & 1;
  const float v = in[((b * C + c) * padded_h(h) + (2 * y + dy + 1)) * padded_w(w) + 2 * x + dx + PADL];
  out[((b * 4 * C + k) * padded_h(ho) + (y + 1)) * padded_w(wo) + x + PADL] = v;
}

// depth-to-space: in [B][4C][h][w] -> out [B][C][2h][2w], out[c][2y + dy][2x + dx] = in[(2 dy + dx) * C + c][y][x]
__global__ __launch_bounds__(256) void f32_d2s_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int h, int w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // over out interior: B * C * 2h * 2w
  if (i >= n) return;
  const int W2 = 2 * w, H2 = 2 * h;
  const int X = (int)(i % W2);
  size_t t = i / W2;
  const int Y = (int)(t % H2);
  t /= H2;
  const int c = (int)(t % C);
  const size_t b = t / C;
  const int ph = (Y & 1) * 2 + (X & 1);
  const float v = in[((b * 4 * C + ph * C + c) * padded_h(h) + (Y / 2 + 1)) * padded_w(w) + X / 2 + PADL];
  out[((b * C + c) * padded_h(H2) + (Y + 1)) * padded_w(W2) + X + PADL] = v;
}

// o = a + b on the interior (borders stay zero)
__global__ __launch_bounds__(256) void f32_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, int h,
                                                      int w, size_t n) {   // n = B * C * h * w
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % w);
  const size_t t = i / w;
  const int y = (int)(t % h);
  const size_t bc = t / h;
  const size_t r = (bc * padded_h(h) + (y + 1)) * padded_w(w) + x + PADL;
  o[r] = a[r] + b[r];
}

// channel 0 of the tail's 32-channel output -> pre-clamp image and clamped image
__global__ void f32_out_kernel(const float* __restrict__ t32, float* __restrict__ out, float* __restrict__ out_pre, int H, int W) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= W) return;
  const float v = t32[((size_t)b * 32 * padded_h(H) + (y + 1)) * padded_w(W) + xx + PADL];
  const size_t o = ((size_t)b * H + y) * W + xx;
  if (out_pre) out_pre[o] = v;
  out[o] = fminf(fmaxf(v, 0.f), 1.f);
}

size_t plane(int C, int h, int w) { return (size_t)C * padded_h(h) * padded_w(w); }   // floats per image

struct F32Plan : DruOffsets {   // float offsets
  size_t in2;   // padded [x | sigma]
  size_t T32;   // 32-channel output of the tail (forward) / of the head's adjoint (gradient arena)
  size_t total;
};
F32Plan f32_plan(int B, int H, int W, int nb_keep = 0) {
  F32Plan P{};
  size_t off = 0;
  auto add = [&](size_t& o, size_t floats_per_image) {
    o = off;
    off += floats_per_image * B;
    off = (off + 63) & ~(size_t)63;
  };
  add(P.in2, plane(2, H, W));
  for (int l = 0; l < 4; ++l) {
    const int h = H >> l, w = W >> l, c = DRU_NC[l];
    add(P.S[l], plane(c, h, w));
    add(P.P[l], plane(c, h, w));
    add(P.Q[l], plane(c, h, w));
    add(P.M[l], plane(c, h, w));
    if (l <= 2) add(P.U[l], plane(c, h, w));
    if (l >= 1) add(P.DT[l], plane(2 * c, h, w));
  }
  add(P.T32, plane(32, H, W));
  for (int l = 0; l < 4; ++l)
    for (int j = 0; j < (l == 3 ? 1 : 2) * nb_keep; ++j) add(P.MK[l][j], plane(DRU_NC[l], H >> l, W >> l));
  P.total = off + 4096;   // slack for the LDS-DMA gathers' over-read lanes
  return P;
}

// The fp32 packings of every layer (direct kernel; Winograd for the 3x3 ResBlock layers; the one-tap instance for the 1x1 layers of
// the strided / transposed 2x2 convolutions), or of every layer's adjoint, index-parallel to the forward layers: the adjoint of a
// convolution is the convolution with the transposed, tap-mirrored weights (the head's: 64 -> 2, zero-padded to 32 couts; the tail's
// runs on the vector ALU with the half-split context's [64][2][9] table and is not packed here).
int prepare_weights(pnpx_ctx* ctx, bool adjoint) {
  DruNet& N = ctx->drunet;
  DruF32Pack& K = adjoint ? N.f32_bwd : N.f32;
  if (K.ready) return PNPX_OK;
  const std::vector<DruLayer> L = dru_layers(N.nb);
  std::vector<float> host, w3, wa, w1;
  auto align = [&]() { host.resize((host.size() + 63) & ~(size_t)63, 0.f); };
  std::vector<size_t> woff(L.size(), 0), uoff(L.size(), 0);
  std::vector<ConvLayer> lay(L.size());
  const float* src = N.params_host.data();
  for (size_t i = 0; i < L.size(); ++i) {
    const DruLayer& d = L[i];
    int cin, cout;
    dru_layer_w3(d, src, &cin, &cout, w3);
    src += layer_params(d);
    if (adjoint) {
      if (d.kind == 5) continue;
      const int rows = dru_adjoint_w3(w3, cin, cout, wa);
      cin = cout;
      cout = rows;
      w3.swap(wa);
    }
    const int cc = adjoint ? 8 : conv_pack_cc(cin), mt = (cc == 2) ? 32 : conv_pack_mt(cout);   // (the 2-channel path exists for 32-cout tiles)
    align();
    woff[i] = host.size();
    if (dru_is_1x1(d)) {       // the centre taps of w3, packed for the one-tap instance
      w1.resize((size_t)cout * cin);
      for (size_t q = 0; q < w1.size(); ++q) w1[q] = w3[q * 9 + 4];
      host.resize(host.size() + w1.size());
      pack_conv_weights_1x1(w1.data(), cout, cin, host.data() + woff[i]);
    } else {
      host.resize(host.size() + (size_t)cout * cin * 9);
      pack_conv_weights(w3.data(), cout, cin, mt, cc, host.data() + woff[i]);
    }
    lay[i].cin = cin;
    lay[i].cout = cout;
    lay[i].mt = mt;
    lay[i].cc = cc;
    if ((d.kind == 1 || d.kind == 2) && conv3x3_wino_packs(cout, cin)) {
      align();
      uoff[i] = host.size();
      host.resize(host.size() + conv3x3_wino_floats(cout, cin));
      pack_conv_weights_wino(w3.data(), cout, cin, host.data() + uoff[i]);
    }
  }
  align();
  const size_t zoff = host.size();
  host.resize(host.size() + 1024 + 4096, 0.f);   // zero bias of the bias-free network (largest cout: 1024) + DMA over-read slack
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, host.size() * sizeof(float));
  if (e != hipSuccess) {
    set_error("DRUNet fp32 %s allocation of %zu bytes failed: %s", adjoint ? "adjoint-weight" : "weight", host.size() * sizeof(float),
              hipGetErrorString(e));
    return PNPX_ERR_ALLOC;
  }
  PNPX_HIP(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  float* d = static_cast<float*>(p);
  K.wino.assign(L.size(), nullptr);
  for (size_t i = 0; i < L.size(); ++i) {
    lay[i].w = d + woff[i];
    lay[i].b = d + zoff;
    if (uoff[i]) K.wino[i] = d + uoff[i];
  }
  K.layers = lay;
  K.weights.p = p;
  K.weights.bytes = host.size() * sizeof(float);
  K.ready = true;
  return PNPX_OK;
}

// The re-layouts and the skip sum, as both walks launch them on B images at H x W (level 0) on stream s.
struct F32Glue {
  int B, H, W;
  hipStream_t s;
  int s2d(int l, const float* in, float* out) const { return launch_s2d_f32(in, out, B, DRU_NC[l], H >> l, W >> l, s); }
  int d2s(int l, const float* in, float* out) const { return launch_d2s_f32(in, out, B, DRU_NC[l], H >> (l + 1), W >> (l + 1), s); }
  int add(int l, const float* a, const float* b, float* o) const { return launch_add_f32(a, b, o, (size_t)B * DRU_NC[l], H >> l, W >> l, s); }
};

struct F32Forward : F32Glue {
  pnpx_ctx* ctx;
  const std::vector<DruLayer>& L;
  const float *x, *sigma;
  int sigma_stride;
  float *out, *out_pre;
  float *in2, *t32;

  // layer li: `in` -> `outp` at h x w, negative slope (0 ReLU / 1 linear), optional residual
  int conv(size_t li, const float* in, float* outp, int h, int w, float slope, const float* res) const {
    const DruF32Pack& K = ctx->drunet.f32;
    const ConvLayer& Lc = K.layers[li];
    if (dru_is_1x1(L[li])) return launch_conv1x1_act(Lc, in, outp, B, h, w, slope, res, s);
    const ConvF32Sel v = conv_f32_sel_drunet(ctx, K.wino[li], nullptr);
    ConvF32Operands a{in, Lc.cin, nullptr, 0, outp, B, h, w, slope, res};
    return launch_conv_f32(conv_f32_forward(v, Lc.cin, 0, Lc.cout, h, w, B), v, Lc, a, s);
  }
  int head(float* s0) const {
    PNPX_TRY(launch_prep_input_f32(x, sigma, sigma_stride, in2, B, H, W, s));
    return conv(0, in2, s0, H, W, 1.f, nullptr);
  }
  // linear, 32 couts (channel 0 real)
  int tail(size_t li, const float* m0) const {
    PNPX_TRY(conv(li, m0, t32, H, W, 1.f, nullptr));
    return launch_tail_out_f32(t32, out, out_pre, B, H, W, s);
  }
};

// ---- VJP (r5)
// g_pre = grad_out on pixels whose pre-clamp output lies in [0, 1] (torch.clamp's backward mask is inclusive), else 0
__global__ __launch_bounds__(256) void f32_tail_mask_kernel(const float* __restrict__ g_out, const float* __restrict__ pre, float* __restrict__ g_pre,
                                                            size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p = pre[i];
  g_pre[i] = (p >= 0.f && p <= 1.f) ? g_out[i] : 0.f;
}
// gx = g_in0[:, 0];  gsigma[b] = sum over pixels of g_in0[:, 1]   (two-stage, deterministic; the DRUNet has no input residual)
__global__ __launch_bounds__(256) void f32_input_grad_kernel(const float* __restrict__ g_in0, int Cg, float* __restrict__ gx,
                                                             float* __restrict__ part, int H, int W) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int n = H * W, per = (n + SIG_CHUNKS - 1) / SIG_CHUNKS;
  const int lo = chunk * per, hi = min(n, lo + per);
  const int Hp = padded_h(H), Wp = padded_w(W);
  const float* g0 = g_in0 + (size_t)b * Cg * Hp * Wp;
  const float* g1c = g0 + (size_t)Hp * Wp;
  float acc = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int y = i / W, x = i - y * W;
    const size_t o = (size_t)(y + 1) * Wp + x + PADL;
    gx[(size_t)b * n + i] = g0[o];
    acc += g1c[o];
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ float w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[b * SIG_CHUNKS + chunk] = (w[0] + w[1]) + (w[2] + w[3]);
}

// The VJP's launches (dataflow: drunet_net.h dru_backward_walk) on the fp32 kernels with the adjoint packings -- the ReLU' mask and the
// skip's add sit in the epilogues of the (Winograd) adjoint convolutions.
struct F32Backward : F32Glue {
  pnpx_ctx* ctx;
  const std::vector<DruLayer>& L;
  const float *grad_out, *pre;
  float *g_pre, *part, *grad_x, *grad_sigma;
  float* t32;   // 32-channel output of the head's adjoint

  // adjoint of layer li: `in` -> `outp` at h x w; dmask (ReLU' of the saved activation) or res (added), not both
  int conv(int li, const float* in, float* outp, int h, int w, const float* dmask, const float* res) const {
    const DruF32Pack& K = ctx->drunet.f32_bwd;
    const ConvLayer& Lc = K.layers[li];
    if (dru_is_1x1(L[li])) return launch_conv1x1_act(Lc, in, outp, B, h, w, 1.f, res, s);
    // the adjoint layer is a packed layer of its own: its Winograd weights serve the decision (u_bwd) and the launch helper (u)
    const float* u = K.wino[li];
    const ConvF32Sel v = conv_f32_sel_drunet(ctx, u, u);
    const ConvF32Choice c = conv_f32_adjoint(v, Lc.cin, Lc.cout, h, w);
    if (!dmask) {      // linear, + res
      ConvF32Operands a{in, Lc.cin, nullptr, 0, outp, B, h, w, 1.f, res};
      return launch_conv_f32(c, v, Lc, a, s);
    }
    if (c.wino()) return launch_conv3x3_wino8_grad(u, Lc.b, Lc.cout, in, Lc.cin, outp, dmask, 0.f, B, h, w, s);
    return launch_conv3x3_grad(Lc, in, outp, dmask, B, h, w, s, nullptr, 0.f);
  }
  // clamp + tail (64 <- 1 channel: vector ALU, the [64][2][9] table of the half-split context; its second input channel is zero)
  int seed(float* s0) const {
    PNPX_TRY(launch_tail_mask_f32(grad_out, pre, g_pre, (size_t)B * H * W, s));
    return launch_conv_first_f32(g_pre, ctx->drunet.zero, 0, ctx->drunet.tail_bwd_w, ctx->drunet.zero, s0, DRU_NC[0], B, H, W, 1.0f, s);
  }
  // head: 64 -> (image, noise map) gradients
  int input_grad(const float* m0) const {
    PNPX_TRY(conv(0, m0, t32, H, W, nullptr, nullptr));
    return launch_dru_input_grad_f32(t32, 32, grad_x, part, grad_sigma, B, H, W, s);
  }
};

}  // namespace

// ---- the launchers of the kernels above (fwd_glue.h): the walks and, for tests, pnpx_fwd_glue_probe go through them
int launch_s2d_f32(const float* in, float* out, int B, int C, int h, int w, hipStream_t s) {
  const size_t n = (size_t)B * 4 * C * (h / 2) * (w / 2);
  hipLaunchKernelGGL(f32_s2d_kernel, g1(n), dim3(256), 0, s, in, out, C, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_d2s_f32(const float* in, float* out, int B, int C, int h, int w, hipStream_t s) {
  const size_t n = (size_t)B * C * (2 * h) * (2 * w);
  hipLaunchKernelGGL(f32_d2s_kernel, g1(n), dim3(256), 0, s, in, out, C, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_add_f32(const float* a, const float* b, float* o, size_t planes, int h, int w, hipStream_t s) {
  const size_t n = planes * h * w;
  hipLaunchKernelGGL(f32_add_kernel, g1(n), dim3(256), 0, s, a, b, o, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_tail_out_f32(const float* t32, float* out, float* out_pre, int B, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(f32_out_kernel, dim3((W + 63) / 64, H, B), dim3(64), 0, s, t32, out, out_pre, H, W);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_tail_mask_f32(const float* g_out, const float* pre, float* g_pre, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(f32_tail_mask_kernel, g1(n), dim3(256), 0, s, g_out, pre, g_pre, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}
int launch_dru_input_grad_f32(const float* g_in0, int Cg, float* gx, float* part, float* gsigma, int B, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(f32_input_grad_kernel, dim3(SIG_CHUNKS, B), dim3(256), 0, s, g_in0, Cg, gx, part, H, W);
  PNPX_LAUNCH_CHECK();
  hipLaunchKernelGGL(sigma_grad_final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, part, gsigma, B);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

void drunet_f32_free(pnpx_ctx* ctx) {
  DruNet& N = ctx->drunet;
  for (DruF32Pack* K : {&N.f32, &N.f32_bwd}) {
    if (K->weights.p) (void)hipFree(K->weights.p);
    *K = DruF32Pack();
  }
  dru_arena_free(N.f32_arena);
  dru_arena_free(N.f32_arena_grad);
}

int drunet_denoise_f32(pnpx_ctx* ctx, const float* x, const float* sigma, int sigma_stride, float* out, float* out_pre, int B, int H,
                       int W, hipStream_t s, bool keep_mids) {
  DruNet& N = ctx->drunet;
  PNPX_TRY(prepare_weights(ctx, false));
  PNPX_TRY(dru_arena_reserve(N.f32_arena, B, H, W, keep_mids, KEEPS_DROP, "fp32 arena",
                             [&](int images, bool keeps) { return f32_plan(images, H, W, keeps ? N.nb : 0).total * sizeof(float); }));
  const F32Plan Pl = f32_plan(N.f32_arena.capB, H, W, N.f32_arena.keeps ? N.nb : 0);
  float* const A = static_cast<float*>(N.f32_arena.buf.p);
  const std::vector<DruLayer> L = dru_layers(N.nb);
  const F32Forward f{{B, H, W, s}, ctx, L, x, sigma, sigma_stride, out, out_pre, A + Pl.in2, A + Pl.T32};
  return dru_forward_walk(f, A, Pl, N.nb, H, W, keep_mids);
}

// The adjoint chain after drunet_denoise_f32(.., keep_mids = true) of the same call left `pre` and the arena's keep planes
// (drunet.hip: drunet_denoise_backward owns the scratch and that forward for both families).
int drunet_denoise_backward_f32(pnpx_ctx* ctx, const float* grad_out, const float* pre, float* g_pre, float* part, float* grad_x,
                                float* grad_sigma, int B, int H, int W, hipStream_t s) {
  DruNet& N = ctx->drunet;
  PNPX_TRY(prepare_weights(ctx, true));
  const F32Plan F = f32_plan(N.f32_arena.capB, H, W, N.nb);
  float* const FA = static_cast<float*>(N.f32_arena.buf.p);
  // gradient arena (zero borders: gradients are convolution inputs of the adjoint convolutions)
  PNPX_TRY(dru_arena_reserve(N.f32_arena_grad, B, H, W, false, KEEPS_DROP, "fp32 gradient arena",
                             [&](int images, bool) { return f32_plan(images, H, W).total * sizeof(float); }));
  const F32Plan G = f32_plan(N.f32_arena_grad.capB, H, W);
  float* const GA = static_cast<float*>(N.f32_arena_grad.buf.p);
  const std::vector<DruLayer> L = dru_layers(N.nb);
  const F32Backward f{{B, H, W, s}, ctx, L, grad_out, pre, g_pre, part, grad_x, grad_sigma, GA + G.T32};
  return dru_backward_walk(f, GA, G, FA, F, N.nb, H, W);
}

}  // namespace pnpx
