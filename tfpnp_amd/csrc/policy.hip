// Policy actor forward (eval mode) -- SURVEY section 8(f) rank 2.
//
// Replaces ResNetActorBase.forward up to the head activations (tfpnp/policy/network.py:129-147):
//     x = ResNetEncoder(18)(state)            network.py:87-125  (3x3 stride-2 stem, 4 stages of 2 BasicBlocks, each
//                                             stage entered with stride 2; BasicBlock network.py:33-58)
//     x = adaptive_avg_pool2d(x, 1).view(B, 512)
//     probs = softmax(fc_softmax(x));  det = sigmoid(fc_deterministic(x))      (SPI head: 512-64-ReLU-n, :262-268)
// with SynchronizedBatchNorm2d in eval mode (= F.batch_norm on running statistics, sync_batchnorm/batchnorm.py:63-68;
// both the rollout, trainer.py:216-221, and the evaluator, evaluator.py:23, run the actor that way).  Sampling /
// arg-max of idx_stop, log-probabilities and the action range mapping stay in the host mirror (O(B) scalars).
//
// MI355X design: every convolution is one launch of the fp32 MFMA kernel in policy_conv.hip:
//   * BatchNorm folded into weights and bias on the host; ReLU / residual add in the epilogue.
//   * stride-2 3x3 convolutions read a SPACE-TO-DEPTH copy of their input ([4*C][H/2][W/2], written directly by the
//     producer's epilogue): on that grid the convolution is stride 1, and of the 36 (phase, tap) pairs only 9 are
//     non-zero -- a per-(cout tile, K-chunk) tap mask skips the other MFMAs, so no arithmetic is wasted on stride.
//   * the 1x1 stride-2 shortcut is the centre tap of phase (0,0): it rides in the same launch as extra cout tiles
//     (all other chunks masked out) and is written, without ReLU, to a second output.
// policy_load folds and packs on the host (a checkpoint); policy_pack.hip derives the same layouts on the device from a live
// parameter vector (pnpx_policy_load_device).
// By default (option policy_s2_hs = 1) every convolution runs on the half-split launches instead: the trunk the critic shares,
// resnet18_hs.hip::trunk_forward (layer numbering, host packing of a layer, arena), then the heads here.  The fp32 launches
// above remain as the stem and stage entries of policy_s2_hs = 0 (forward_f32_entries).
#include <cmath>
#include <cstring>

#include "common.h"
#include "conv_hs.h"
#include "hs_rec.h"
#include "hs_relayout.h"
#include "policy_conv.h"
#include "resnet18_hs.h"

namespace pnpx {
namespace {

constexpr float BN_EPS = 1e-5f;

// observation [B][C][H][W] -> space-to-depth padded planar [B][4*Cp][H/2+2][W/2+8] (channels >= C stay zero)
__global__ __launch_bounds__(256) void pack_ob_s2d_kernel(const float* __restrict__ ob, float* __restrict__ out, int C,
                                                          int Cp, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % W);
  size_t t = i / W;
  const int y = (int)(t % H);
  t /= H;
  const int c = (int)(t % C);
  const size_t b = t / C;
  const int Hp2 = padded_h(H >> 1), Wp2 = pol_wp(W >> 1);
  const int ph = (y & 1) * 2 + (x & 1);
  out[((b * 4 * Cp + (size_t)ph * Cp + c) * Hp2 + (y >> 1) + 1) * Wp2 + (x >> 1) + POL_PADL] = ob[i];
}

// half-split HS8 [B][C/8][h+2][w+2] -> space-to-depth fp32 planar [B][4*C][h/2+2][w/2+8] (input of a stride-2 conv)
__global__ __launch_bounds__(256) void hs8_to_s2d_kernel(const HsRec* __restrict__ src, float* __restrict__ dst, int C,
                                                         int h, int w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % w);
  size_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int g = (int)(t % (C >> 3));
  const size_t b = t / (C >> 3);
  float v[8];
  hs_unpack(src[((b * (C >> 3) + g) * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1)], v);
  const int Hp2 = padded_h(h >> 1), Wp2 = pol_wp(w >> 1);
  const int ph = (y & 1) * 2 + (x & 1);
  float* o = dst + ((b * 4 * C + (size_t)ph * C + g * 8) * Hp2 + (y >> 1) + 1) * Wp2 + (x >> 1) + POL_PADL;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[(size_t)k * Hp2 * Wp2] = v[k] * (1.f / HS_ASCALE);
}

// global average pool over the last HS8 activation [B][512][h][w] + the two heads.  One workgroup per observation.
__global__ __launch_bounds__(256) void pool_heads_kernel(const HsRec* __restrict__ feat, int h, int w,
                                                         const float* __restrict__ sm_w, const float* __restrict__ sm_b,
                                                         const float* __restrict__ d_w, const float* __restrict__ d_b,
                                                         const float* __restrict__ d2_w, const float* __restrict__ d2_b,
                                                         int n_det, int spi, float* __restrict__ probs,
                                                         float* __restrict__ det) {
  __shared__ float f[512];
  __shared__ float hid[64];
  __shared__ float logit[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float inv = 1.f / ((float)(h * w) * HS_ASCALE);
  for (int c = tid; c < 512; c += 256) f[c] = hs_pooled(feat, b, 64, c, h, w, inv);
  __syncthreads();
  auto dot512 = [&](const float* wrow) {
    float s = 0.f;
    for (int k = 0; k < 512; ++k) s = fmaf(wrow[k], f[k], s);
    return s;
  };
  if (tid < 2) logit[tid] = dot512(sm_w + tid * 512) + sm_b[tid];
  if (spi) {
    if (tid >= 64 && tid < 128) hid[tid - 64] = fmaxf(dot512(d_w + (tid - 64) * 512) + d_b[tid - 64], 0.f);
  } else if (tid >= 64 && tid < 64 + n_det) {
    const int j = tid - 64;
    det[(size_t)b * n_det + j] = 1.f / (1.f + expf(-(dot512(d_w + j * 512) + d_b[j])));
  }
  __syncthreads();
  if (tid == 0) {
    const float m = fmaxf(logit[0], logit[1]);
    const float e0 = expf(logit[0] - m), e1 = expf(logit[1] - m);
    probs[b * 2 + 0] = e0 / (e0 + e1);
    probs[b * 2 + 1] = e1 / (e0 + e1);
  }
  if (spi && tid < n_det) {
    float s = d2_b[tid];
    for (int k = 0; k < 64; ++k) s = fmaf(d2_w[tid * 64 + k], hid[k], s);
    det[(size_t)b * n_det + tid] = 1.f / (1.f + expf(-s));
  }
}

// ------------------------------------------------------------------------------------------- parameter layout
struct BnView {
  const float *g, *b, *m, *v;
};
BnView take_bn(Reader& R, int c) {
  BnView r;
  r.g = R.take(c);
  r.b = R.take(c);
  r.m = R.take(c);
  r.v = R.take(c);
  return r;
}
inline void bn_fold(const BnView& bn, int c, float* scale, float* shift) {
  for (int i = 0; i < c; ++i) {
    scale[i] = bn.g[i] / std::sqrt(bn.v[i] + BN_EPS);
    shift[i] = bn.b[i] - bn.m[i] * scale[i];
  }
}
// conv + BN: the dense weights [cout][fan] times the per-channel scale (one fp32 rounding), the shift as the bias
struct Folded {
  std::vector<float> w, shift;
};
Folded bn_folded(const float* w, const BnView& bn, int cout, size_t fan) {
  Folded F;
  std::vector<float> sc(cout);
  F.shift.resize(cout);
  F.w.resize((size_t)cout * fan);
  bn_fold(bn, cout, sc.data(), F.shift.data());
  for (int co = 0; co < cout; ++co)
    for (size_t i = 0; i < fan; ++i) F.w[co * fan + i] = w[co * fan + i] * sc[co];
  return F;
}

struct ConvOff {
  size_t w, bias, steps, nsteps;
};
// Pack one launch: per cout tile the list of K-chunks that carry any weight (PolStep), and only their present tap
// slices [8 channels][64 couts], in list order.  Presence is decided on the values (an all-zero slice contributes
// exactly nothing).
ConvOff pack_eff(HostBlob& H, Eff& E) {
  const int nct = E.cout / 64, nch = E.K / 8;
  ConvOff o;
  H.align();
  o.w = H.f.size();
  std::vector<PolStep> steps((size_t)nct * nch, PolStep{0, 0, 0});
  std::vector<int> nsteps(nct, 0);
  std::vector<float> slice(512);
  unsigned int nslices = 0;
  for (int ct = 0; ct < nct; ++ct)
    for (int ch = 0; ch < nch; ++ch) {
      unsigned short mask = 0;
      const unsigned int first = nslices;
      for (int tap = 0; tap < 9; ++tap) {
        bool any = false;
        for (int c = 0; c < 8; ++c)
          for (int m = 0; m < 64; ++m) {
            const float v = E.at(ct * 64 + m, ch * 8 + c, tap);
            any |= (v != 0.f);
            slice[c * 64 + m] = v;
          }
        if (!any) continue;
        mask |= (unsigned short)(1u << tap);
        H.f.insert(H.f.end(), slice.begin(), slice.end());
        ++nslices;
      }
      if (mask) steps[(size_t)ct * nch + nsteps[ct]++] = PolStep{mask, (unsigned short)ch, first};
    }
  H.f.resize(H.f.size() + 1024, 0.f);   // the 16-byte DMA of the last slice may not over-read, but keep a guard
  o.bias = H.add(E.bias.data(), E.bias.size());
  static_assert(sizeof(PolStep) == 8, "PolStep layout");
  H.align();
  o.steps = H.f.size();
  H.f.resize(H.f.size() + steps.size() * 2, 0.f);
  std::memcpy(H.f.data() + o.steps, steps.data(), steps.size() * sizeof(PolStep));
  H.align();
  o.nsteps = H.f.size();
  H.f.resize(H.f.size() + nsteps.size(), 0.f);
  std::memcpy(H.f.data() + o.nsteps, nsteps.data(), nsteps.size() * sizeof(int));
  return o;
}

// ------------------------------------------------------------------------------------------- activation plan
struct PolicyPlan {
  TrunkPlan T;                   // HS8; o1s holds fp32 planar data under policy_s2_hs = 0 and is sized for that form, the larger
  TrunkAct ob, stem;             // option policy_s2_hs = 0: fp32 planar space-to-depth observation and stem output
  size_t total = 0;              // floats for capB observations
};
PolicyPlan make_policy_plan(int capB, int cin_pad, int H, int W) {
  PolicyPlan P;
  size_t off = 0;
  auto place = [&](TrunkAct& d, int C, int h, int w, size_t floats) {
    d.off = off;
    d.C = C;
    d.H = h;
    d.W = w;
    off += floats * capB;
    off = (off + 63) & ~(size_t)63;
  };
  auto add = [&](TrunkAct& d, int C, int h, int w) { place(d, C, h, w, (size_t)C * padded_h(h) * pol_wp(w)); };   // fp32 planar
  auto add_hs = [&](TrunkAct& d, int C, int h, int w) { place(d, C, h, w, hs_act_floats(C, h, w)); };
  add(P.ob, 4 * cin_pad, H / 2, W / 2);
  add(P.stem, 4 * 64, H / 4, W / 4);
  add_hs(P.T.stem_s, 4 * 64, H / 4, W / 4);
  add_hs(P.T.ob_s, 4 * cin_pad, H / 2, W / 2);
  add_hs(P.T.stem_o, 64, H / 2, W / 2);
  for (int n = 0; n < 4; ++n) {
    const int p = stage_planes(n), h = H >> (n + 2), w = W >> (n + 2);
    add_hs(P.T.t1[n], p, h, w);
    add_hs(P.T.sc[n], p, h, w);
    add_hs(P.T.o0[n], p, h, w);
    add_hs(P.T.t2[n], p, h, w);
    add_hs(P.T.o1[n], p, h, w);
    if (n < 3) add(P.T.o1s[n], 4 * p, h / 2, w / 2);
  }
  P.total = off + (1u << 18);   // slack: overhanging tiles read past their tensor
  return P;
}

}  // namespace

int policy_launch_pack_ob_f32(const float* ob, float* out, int C, int Cp, int B, int H, int W, hipStream_t s) {
  const size_t n = (size_t)B * C * H * W;
  hipLaunchKernelGGL(pack_ob_s2d_kernel, g1(n), dim3(256), 0, s, ob, out, C, Cp, H, W, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int policy_launch_heads(const PolicyPack& P, int n_det, int spi_head, const char* feat_hs, int h, int w, int B, float* probs, float* det,
                        hipStream_t s) {
  hipLaunchKernelGGL(pool_heads_kernel, dim3(B), dim3(256), 0, s, reinterpret_cast<const HsRec*>(feat_hs), h, w, P.fc_sm_w, P.fc_sm_b,
                     P.fc_det_w, P.fc_det_b, P.fc_det2_w, P.fc_det2_b, n_det, spi_head, probs, det);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

size_t policy_num_params(int num_inputs, int n_det, int spi_head) {
  size_t n = (size_t)64 * num_inputs * 9 + 4 * 64;
  int in_planes = 64;
  for (int s = 0; s < 4; ++s) {
    const int p = stage_planes(s);
    n += (size_t)p * in_planes * 9 + 4 * p + (size_t)p * p * 9 + 4 * p + (size_t)p * in_planes + 4 * p;  // block 0
    n += 2 * ((size_t)p * p * 9 + 4 * p);                                                                 // block 1
    in_planes = p;
  }
  n += 2 * 512 + 2;
  n += spi_head ? (size_t)64 * 512 + 64 + (size_t)n_det * 64 + n_det : (size_t)n_det * 512 + n_det;
  return n;
}

void policy_free(pnpx_ctx* ctx) {
  PolicyNet& N = ctx->policy;
  if (N.weights.p) (void)hipFree(N.weights.p);
  if (N.arena.p) (void)hipFree(N.arena.p);
  N.live.free();
  N.pack_ws.free();
  if (N.raw.weights.p) (void)hipFree(N.raw.weights.p);
  N.raw_ws.free();
  if (N.train_ws.p) (void)hipFree(N.train_ws.p);
  if (N.bn_buf.p) (void)hipFree(N.bn_buf.p);
  if (N.raw_adj.p) (void)hipFree(N.raw_adj.p);
  if (N.raw_adj_table.p) (void)hipFree(N.raw_adj_table.p);
  if (N.grad_ws.p) (void)hipFree(N.grad_ws.p);
  if (N.grad_slab.p) (void)hipFree(N.grad_slab.p);
  N = PolicyNet();
}

int policy_load(pnpx_ctx* ctx, const float* params, size_t n, int num_inputs, int n_det, int spi_head) {
  if (!params || num_inputs < 1 || num_inputs > 64 || n_det < 1 || n_det > 64 ||
      n != policy_num_params(num_inputs, n_det, spi_head)) {
    set_error("pnpx_policy_load: expected %zu parameters for (%d inputs, %d outputs, spi %d), got %zu",
              policy_num_params(num_inputs, n_det, spi_head), num_inputs, n_det, spi_head, n);
    return PNPX_ERR_ARG;
  }
  PNPX_HIP(hipDeviceSynchronize());
  policy_free(ctx);
  PolicyNet& N = ctx->policy;
  N.num_inputs = num_inputs;
  N.cin_pad = (num_inputs + 7) / 8 * 8;
  N.n_det = n_det;
  N.spi_head = spi_head;
  Reader R{params};
  HostBlob H;
  ConvOff off[5];          // the fp32 tap-sparse launches of option policy_s2_hs = 0: stem, four stage entries (conv1 + shortcut rows)
  int cins[5], couts[5], splits[5];
  Packed pk[TRUNK_LAYERS];
  auto finish_f32 = [&](int fi, Eff& E, int split) {
    off[fi] = pack_eff(H, E);
    cins[fi] = E.K;
    couts[fi] = E.cout;
    splits[fi] = split;
  };
  auto conv_s1 = [&](int li, int p) {   // 3x3 stride-1 conv + BN, the next entry of the parameter vector
    const float* w = R.take((size_t)p * p * 9);
    const Folded F = bn_folded(w, take_bn(R, p), p, (size_t)p * 9);
    Eff E(p, p);
    put_conv_s1(E, 0, F.w.data(), F.shift.data(), p, p);
    pk[li] = pack_layer(H, E, trunk_taps(li, false), true);
  };
  {  // stem: conv3x3(num_inputs, 64, stride 2) + bn1
    const float* w = R.take((size_t)64 * num_inputs * 9);
    const Folded F = bn_folded(w, take_bn(R, 64), 64, (size_t)num_inputs * 9);
    Eff E(64, 4 * N.cin_pad);
    put_conv_s2(E, 0, F.w.data(), F.shift.data(), 64, num_inputs, N.cin_pad);
    finish_f32(0, E, 64);
    // ... and as a 2x2-window sparse-tap half-split launch over the HS8 space-to-depth observation
    pk[0] = pack_layer(H, E, trunk_taps(0, false), true);
  }
  int in_planes = 64;
  for (int s = 0; s < 4; ++s) {
    const int p = stage_planes(s), l0 = 1 + 5 * s;
    // block 0 (stride 2): conv1, bn1, conv2, bn2, shortcut.0 (1x1), shortcut.1 (bn)   -- state_dict order
    const float* w1 = R.take((size_t)p * in_planes * 9);
    const BnView b1 = take_bn(R, p);
    const float* w2 = R.take((size_t)p * p * 9);
    const BnView b2 = take_bn(R, p);
    const float* ws = R.take((size_t)p * in_planes);
    const BnView bs = take_bn(R, p);
    const Folded F1 = bn_folded(w1, b1, p, (size_t)in_planes * 9), Fs = bn_folded(ws, bs, p, (size_t)in_planes);
    {
      Eff E(2 * p, 4 * in_planes);
      put_conv_s2(E, 0, F1.w.data(), F1.shift.data(), p, in_planes, in_planes);
      put_shortcut(E, p, Fs.w.data(), Fs.shift.data(), p, in_planes);
      finish_f32(1 + s, E, p);
    }
    {   // the same two convolutions packed for the sparse-tap half-split instances
      Eff E1(p, 4 * in_planes), Es(p, in_planes);
      put_conv_s2(E1, 0, F1.w.data(), F1.shift.data(), p, in_planes, in_planes);
      put_shortcut(Es, 0, Fs.w.data(), Fs.shift.data(), p, in_planes);
      pk[l0 + 0] = pack_layer(H, E1, trunk_taps(l0 + 0, false), true);
      pk[l0 + 2] = pack_layer(H, Es, trunk_taps(l0 + 2, false), true);
    }
    {
      const Folded F2 = bn_folded(w2, b2, p, (size_t)p * 9);
      Eff E(p, p);
      put_conv_s1(E, 0, F2.w.data(), F2.shift.data(), p, p);
      pk[l0 + 1] = pack_layer(H, E, trunk_taps(l0 + 1, false), true);
    }
    // block 1 (stride 1, identity shortcut)
    conv_s1(l0 + 3, p);
    conv_s1(l0 + 4, p);
    in_planes = p;
  }
  const size_t o_smw = H.add(R.take(2 * 512), 2 * 512);
  const size_t o_smb = H.add(R.take(2), 2);
  size_t o_dw, o_db, o_d2w = 0, o_d2b = 0;
  if (spi_head) {
    o_dw = H.add(R.take((size_t)64 * 512), (size_t)64 * 512);
    o_db = H.add(R.take(64), 64);
    o_d2w = H.add(R.take((size_t)n_det * 64), (size_t)n_det * 64);
    o_d2b = H.add(R.take(n_det), n_det);
  } else {
    o_dw = H.add(R.take((size_t)n_det * 512), (size_t)n_det * 512);
    o_db = H.add(R.take(n_det), n_det);
  }
  H.f.resize(H.f.size() + 8192, 0.f);   // DMA over-read slack
  PNPX_TRY(alloc_dev(N.weights, H.f.size() * sizeof(float), "policy weight"));
  PNPX_HIP(hipMemcpy(N.weights.p, H.f.data(), N.weights.bytes, hipMemcpyHostToDevice));
  const float* base = static_cast<const float*>(N.weights.p);
  for (int i = 0; i < 5; ++i) {
    N.f32[i].w = base + off[i].w;
    N.f32[i].bias = base + off[i].bias;
    N.f32[i].steps = reinterpret_cast<const PolStep*>(base + off[i].steps);
    N.f32[i].nsteps = reinterpret_cast<const int*>(base + off[i].nsteps);
    N.f32[i].cin = cins[i];
    N.f32[i].cout = couts[i];
    N.f32[i].split_c = splits[i];
  }
  for (int li = 0; li < TRUNK_LAYERS; ++li) {
    bind_packed(N.hs[li], pk[li], base);
    N.hs_bias[li] = base + pk[li].b;
  }
  N.fc_sm_w = base + o_smw;
  N.fc_sm_b = base + o_smb;
  N.fc_det_w = base + o_dw;
  N.fc_det_b = base + o_db;
  N.fc_det2_w = spi_head ? base + o_d2w : nullptr;
  N.fc_det2_b = spi_head ? base + o_d2b : nullptr;
  // live weights: the raw parameters stay on the device for pnpx_policy_params / another device's context
  int st = N.live.alloc(n, "policy parameter");
  if (st == PNPX_OK) st = N.live.set_host(params);
  if (st != PNPX_OK) {
    policy_free(ctx);
    return st;
  }
  N.loaded = true;
  return PNPX_OK;
}

namespace {

// Option policy_s2_hs = 0: the stem and the stage entries (conv1 + 1x1 shortcut, one launch) on the fp32 tap-sparse kernel
// (policy_conv.hip) over fp32 space-to-depth tensors; each entry writes its two outputs as HS8 tensors, the three stride-1
// convolutions of the stage run on the half-split kernel, and the stage output is re-laid out space-to-depth in fp32 for the next
// entry.  One launch chain.
int forward_f32_entries(pnpx_ctx* ctx, const PolicyPlan& P, const float* ob, float* probs, float* det, int B, int H, int W, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  float* A = static_cast<float*>(N.arena.p);
  auto ptr = [&](const TrunkAct& d) { return A + d.off; };
  auto hsc = [&](const TrunkAct& d) { return reinterpret_cast<char*>(A + d.off); };
  auto conv_hs = [&](int li, const TrunkAct& in, const TrunkAct& out, const TrunkAct* res, int h, int w) -> int {
    HsLaunch L;
    L.D = &N.hs[li];
    L.bias = N.hs_bias[li];
    L.slope = 0.f;                          // ReLU
    L.range_flag = ctx->opt_range_guard ? ctx->range_flag_dev : nullptr;
    return launch_hs_conv(L, hsc(in), in.C, hsc(out), out.C, res ? hsc(*res) : nullptr, res ? res->C : 0, nullptr, 0, B, h, w, s);
  };
  PNPX_TRY(policy_launch_pack_ob_f32(ob, ptr(P.ob), N.num_inputs, N.cin_pad, B, H, W, s));
  // stem (on the H/2 grid) -> space-to-depth for stage 1
  PNPX_TRY(launch_policy_conv(N.f32[0], ptr(P.ob), ptr(P.stem), nullptr, nullptr, true, B, H / 2, W / 2, s));
  const float* xin = ptr(P.stem);
  for (int st = 0; st < 4; ++st) {
    const int h = H >> (st + 2), w = W >> (st + 2), l0 = 1 + 5 * st;
    const TrunkPlan& T = P.T;
    PNPX_TRY(launch_policy_conv(N.f32[1 + st], xin, ptr(T.t1[st]), ptr(T.sc[st]), nullptr, false, B, h, w, s, true));
    PNPX_TRY(conv_hs(l0 + 1, T.t1[st], T.o0[st], &T.sc[st], h, w));
    PNPX_TRY(conv_hs(l0 + 3, T.o0[st], T.t2[st], nullptr, h, w));
    PNPX_TRY(conv_hs(l0 + 4, T.t2[st], T.o1[st], &T.o0[st], h, w));
    if (st < 3) {
      const size_t n8 = (size_t)B * (T.o1[st].C / 8) * h * w;
      hipLaunchKernelGGL(hs8_to_s2d_kernel, g1(n8), dim3(256), 0, s, reinterpret_cast<const HsRec*>(hsc(T.o1[st])), ptr(T.o1s[st]),
                         T.o1[st].C, h, w, n8);
      PNPX_LAUNCH_CHECK();
      xin = ptr(T.o1s[st]);
    }
  }
  return policy_launch_heads(N, N.n_det, N.spi_head, hsc(P.T.o1[3]), H / 32, W / 32, B, probs, det, s);
}

}  // namespace

int policy_forward(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  if (!N.loaded) {
    set_error("policy forward called before pnpx_policy_load");
    return PNPX_ERR_NO_WEIGHTS;
  }
  if (B <= 0 || H < 32 || W < 32 || (H % 32) || (W % 32)) {
    set_error("policy forward: need B > 0 and H, W positive multiples of 32 (got %d x %d x %d)", B, H, W);
    return PNPX_ERR_SHAPE;
  }
  // a train forward moved the running statistics: fold and pack again, once, before the first eval forward that follows
  if (N.eval_stale) PNPX_TRY(policy_refresh_eval(ctx, s));
  PNPX_TRY(reserve_arena_hs(N.arena, N.capB, N.capH, N.capW, B, H, W,
                            [&](int nb) { return make_policy_plan(nb, N.cin_pad, H, W).total; }, "policy arena"));
  const PolicyPlan P = make_policy_plan(N.capB, N.cin_pad, H, W);
  float* A = static_cast<float*>(N.arena.p);
  if (!ctx->opt_policy_s2_hs) return forward_f32_entries(ctx, P, ob, probs, det, B, H, W, s);

  // Every activation is an HS8 tensor [image][group][h + 2][w + 2] (the default), so a slice of the batch is a contiguous piece of
  // each: slices run as independent launch chains on side streams like the denoisers' (unet.hip: launch_chains; bit-identical per
  // image) -- the deep 8 x 8 / 16 x 16 stages otherwise step up at every round boundary (B = 33: 1.34 ms against 1.02 at B = 32).
  // option "chains": n = exactly n chains (when B >= n); 0 = automatic, from the table of every batch size 1..48 at 256 x 256 with
  // one and two chains: two chains pay between the round boundaries of the 8 x 8 / 16 x 16 stages -- B = 9..15
  // (-3..-6 %), 17..24 (-2..-7 %), 33..48 (-8..-15 %) -- and cost up to 12 % elsewhere (B = 32).  q = batch in 256 x 256 images.
  int chains = 1;
  if (ctx->opt_chains != 0) {
    chains = launch_chains(ctx, B, H, W);
  } else {
    const long long q = (long long)B * H * W / (256 * 256);
    chains = ((q >= 9 && q <= 15) || (q >= 17 && q <= 24) || q >= 33) ? 2 : 1;
  }
  if (chains > B) chains = B;
  unsigned* range_flag = ctx->opt_range_guard ? ctx->range_flag_dev : nullptr;
  // observations lo .. hi - 1 on stream st: trunk, then heads
  auto run = [&](int lo, int hi, hipStream_t st) -> int {
    PNPX_TRY(trunk_forward(N.hs, N.hs_bias, P.T, A, lo, ob + (size_t)lo * N.num_inputs * H * W, N.num_inputs, N.cin_pad, hi - lo, H, W, chains,
                           0, nullptr, range_flag, st));
    const char* feat = reinterpret_cast<const char*>(A + P.T.o1[3].off + (size_t)lo * hs_act_floats(512, H / 32, W / 32));
    return policy_launch_heads(N, N.n_det, N.spi_head, feat, H / 32, W / 32, hi - lo, probs + (size_t)lo * 2, det + (size_t)lo * N.n_det, st);
  };
  if (chains <= 1) return run(0, B, s);
  return fan_out_chains(ctx, chains, B, s, run);
}

}  // namespace pnpx
