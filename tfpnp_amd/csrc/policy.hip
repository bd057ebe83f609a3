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
// MI355X design: every convolution runs on the half-split launches of the trunk the critic shares, resnet18_hs.hip::trunk_forward
// (layer numbering, host packing of a layer, arena): BatchNorm folded into weights and bias, ReLU / residual add in the epilogue, the
// stride-2 convolutions as 2x2-window sparse-tap launches over an HS8 space-to-depth copy of their input.  Then the heads here.
// policy_load folds and packs on the host (a checkpoint); policy_pack.hip derives the same layout on the device from a live
// parameter vector (pnpx_policy_load_device).
#include <cmath>

#include "common.h"
#include "conv_hs.h"
#include "hs_rec.h"
#include "resnet18_hs.h"

namespace pnpx {
namespace {

constexpr float BN_EPS = 1e-5f;

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

// ------------------------------------------------------------------------------------------- activation plan
struct PolicyPlan {
  TrunkPlan T;
  size_t total = 0;              // floats for capB observations
};
PolicyPlan make_policy_plan(int capB, int cin_pad, int H, int W) {
  PolicyPlan P;
  size_t off = 0;
  auto add_hs = [&](TrunkAct& d, int C, int h, int w) {
    d.off = off;
    d.C = C;
    d.H = h;
    d.W = w;
    off += hs_act_floats(C, h, w) * capB;
    off = (off + 63) & ~(size_t)63;
  };
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
    if (n < 3) add_hs(P.T.o1s[n], 4 * p, h / 2, w / 2);
  }
  P.total = off + (1u << 18);   // slack: overhanging tiles read past their tensor
  return P;
}

}  // namespace

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
  N.optim.free();
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
  Packed pk[TRUNK_LAYERS];
  auto conv_s1 = [&](int li, int p) {   // 3x3 stride-1 conv + BN, the next entry of the parameter vector
    const float* w = R.take((size_t)p * p * 9);
    const Folded F = bn_folded(w, take_bn(R, p), p, (size_t)p * 9);
    Eff E(p, p);
    put_conv_s1(E, 0, F.w.data(), F.shift.data(), p, p);
    pk[li] = pack_layer(H, E, trunk_taps(li, false), true);
  };
  {  // stem: conv3x3(num_inputs, 64, stride 2) + bn1, a 2x2-window sparse-tap launch over the HS8 space-to-depth observation
    const float* w = R.take((size_t)64 * num_inputs * 9);
    const Folded F = bn_folded(w, take_bn(R, 64), 64, (size_t)num_inputs * 9);
    Eff E(64, 4 * N.cin_pad);
    put_conv_s2(E, 0, F.w.data(), F.shift.data(), 64, num_inputs, N.cin_pad);
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
    {   // the entry and the 1x1 shortcut: the sparse-tap half-split instances
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
  // the head matrices as they are: fc_softmax, then fc_deterministic (two Linears with the SPI head)
  size_t heads[6] = {};
  const size_t head_n[6] = {2 * 512, 2, (size_t)(spi_head ? 64 : n_det) * 512, (size_t)(spi_head ? 64 : n_det), (size_t)n_det * 64, (size_t)n_det};
  for (int i = 0; i < (spi_head ? 6 : 4); ++i) heads[i] = H.add(R.take(head_n[i]), head_n[i]);
  H.f.resize(H.f.size() + 8192, 0.f);   // DMA over-read slack
  PNPX_TRY(alloc_dev(N.weights, H.f.size() * sizeof(float), "policy weight"));
  PNPX_HIP(hipMemcpy(N.weights.p, H.f.data(), N.weights.bytes, hipMemcpyHostToDevice));
  // live weights: the raw parameters stay on the device as the vector every later refresh packs from, into this blob
  int st = policy_adopt_host_blob(ctx, pk, heads, H.f.size());
  if (st == PNPX_OK) st = N.live.alloc(n, "policy parameter");
  if (st == PNPX_OK) st = N.live.set_host(params);
  if (st == PNPX_OK) st = policy_upload_frozen(ctx);
  if (st != PNPX_OK) {
    policy_free(ctx);
    return st;
  }
  N.loaded = true;
  return PNPX_OK;
}

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
  // Every activation is an HS8 tensor [image][group][h + 2][w + 2], so a slice of the batch is a contiguous piece of
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
