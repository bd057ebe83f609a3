// Policy actor forward in TRAIN mode: every BatchNorm normalises with the statistics of the batch and moves its running statistics
// (tfpnp/policy/sync_batchnorm/batchnorm.py:63-68 on one device = F.batch_norm(training=True, momentum, eps = 1e-5); the reference
// runs the actor this way in MDDPGTrainer._update, trainer.py:128,171).
//
// Batch statistics sit between a convolution and its activation, so nothing can be folded into the weights.  Each of the 21
// convolutions runs on the instance the eval forward uses, over a second, FOLD-FREE packing (PolicyNet::raw: scale exactly 1, shift
// exactly 0, derived from the live parameter vector by policy_pack.hip) with the linear epilogue, and writes its raw output z as an
// HS8 tensor.  Three plain passes per BatchNorm layer follow:
//   bn_partial_kernel   per (piece of BN_PIECE pixels, group of 8 channels): sum and sum of squares in DOUBLE, interior pixels only,
//                       reduced in a fixed order (no atomics; the piece size is a constant, so the result does not depend on the launch)
//   bn_finish_kernel    per channel: the pieces in order -> mean, biased variance, scale = weight * rsqrt(var + eps),
//                       shift = bias - mean * scale; optionally the running-statistics update, written into the live vector
//   bn_apply_kernel     relu((z - mean) * scale + bias [+ the same of the shortcut's z | + residual]) -> the HS8 activation the next
//                       convolution reads and, before a stride-2 entry, its HS8 space-to-depth copy.
//                       (z - mean) * scale + bias is z * scale + shift without the cancellation of two large terms.
// Batch statistics couple the images: the forward is ONE launch chain whatever the "chains" option says.  Pool and heads are the
// eval forward's.  Nothing is kept for a backward pass; fusing the passes into the convolutions is a later step.
//
// The same launch sequence (train_forward_launches) over a plan that keeps every z and every activation is the re-computation of
// policy_param_grad at the end of this file, the driver of the parameter gradients (kernels: policy_grad.hip), and
// policy_forward_train_keep, after which policy_param_grad_kept runs that driver's backward half on what was kept.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "conv_hs.h"
#include "critic_grad.h"
#include "hs_rec.h"
#include "hs_relayout.h"
#include "policy_grad.h"
#include "resnet18_hs.h"

namespace pnpx {
namespace {

constexpr double BN_EPS = 1e-5;
constexpr int NBN = TRUNK_LAYERS;    // one BatchNorm behind every convolution: the trunk's layer numbering (resnet18_hs.h)
constexpr int BN_PIECE = BN_FWD_PIECE;   // pixels per partial sum: 256 threads x 8

struct BnLayer {
  size_t bn;       // floats into the parameter vector: weight, bias, running_mean, running_var (cout each)
  unsigned chan0;  // first channel in the per-channel arrays
  int cout;
};
void bn_layers(int num_inputs, BnLayer* L) {
  size_t off = 0;
  unsigned chan = 0;
  int li = 0;
  auto conv = [&](int cout, int cin, int ks) {
    off += (size_t)cout * cin * ks;
    L[li++] = BnLayer{off, chan, cout};
    off += (size_t)4 * cout;
    chan += cout;
  };
  conv(64, num_inputs, 9);
  int in_planes = 64;
  for (int s = 0; s < 4; ++s) {
    const int p = stage_planes(s);
    conv(p, in_planes, 9);
    conv(p, p, 9);
    conv(p, in_planes, 1);
    conv(p, p, 9);
    conv(p, p, 9);
    in_planes = p;
  }
}

// z: HS8 [B][Gt][h+2][w+2] -> part[piece][Gt * 8][2] = (sum, sum of squares) over the piece's interior pixels (pixel index =
// (b * h + y) * w + x).  grid (pieces, Gt)
__global__ __launch_bounds__(256) void bn_partial_kernel(const HsRec* __restrict__ z, int Gt, int h, int w, long long npix,
                                                         double* __restrict__ part) {
  __shared__ double red[16][256];
  const int tid = threadIdx.x, g = blockIdx.y;
  const long long i0 = (long long)blockIdx.x * BN_PIECE;
  double acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0;
  for (int k = 0; k < BN_PIECE / 256; ++k) {
    const long long i = i0 + k * 256 + tid;
    if (i >= npix) break;
    const int x = (int)(i % w);
    const long long t = i / w;
    const int y = (int)(t % h);
    const long long b = t / h;
    float v[8];
    hs_unpack(z[((b * Gt + g) * (h + 2) + (y + 1)) * (long long)(w + 2) + (x + 1)], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double d = (double)v[e] * (1.0 / HS_ASCALE);
      acc[e] += d;
      acc[8 + e] += d * d;
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) red[e][tid] = acc[e];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
#pragma unroll
      for (int e = 0; e < 16; ++e) red[e][tid] += red[e][tid + st];
    }
    __syncthreads();
  }
  if (tid < 16) part[(((size_t)blockIdx.x * Gt + g) * 8 + (tid & 7)) * 2 + (tid >> 3)] = red[tid][0];
}

struct BnFinishArgs {
  const double* part;
  int cout, npieces;             // channels of the layer = of the tensor behind `part`
  long long n;                   // values per channel
  float* params;                 // the live parameter vector
  size_t bn;                     // BnLayer::bn
  float *mean, *var, *scale, *shift;   // at this layer's first channel
  float momentum;
  int update;
};
__global__ __launch_bounds__(64) void bn_finish_kernel(BnFinishArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.cout) return;
  double s = 0.0, q = 0.0;
  for (int p = 0; p < a.npieces; ++p) {
    const double* e = a.part + ((size_t)p * a.cout + c) * 2;
    s += e[0];
    q += e[1];
  }
  const double n = (double)a.n, mean = s / n;
  double var = q / n - mean * mean;
  if (var < 0.0) var = 0.0;
  float* bn = a.params + a.bn + c;
  const double sc = (double)bn[0] / sqrt(var + BN_EPS);
  a.mean[c] = (float)mean;
  a.var[c] = (float)var;
  a.scale[c] = (float)sc;
  a.shift[c] = (float)((double)bn[a.cout] - mean * sc);
  if (a.update) {
    const double m = (double)a.momentum;
    float* rm = bn + 2 * (size_t)a.cout;
    float* rv = bn + 3 * (size_t)a.cout;
    *rm = (float)((1.0 - m) * (double)*rm + m * mean);
    *rv = (float)((1.0 - m) * (double)*rv + m * var * (n / (n - 1.0)));
  }
}

struct BnApplyArgs {
  BnSrc a, b;          // b: the second normalised summand (block 0: the shortcut)
  const HsRec* res;    // identity residual, HS8 [B][G][h+2][w+2], or null
  HsRec* out;          // HS8 [B][G][h+2][w+2] or null
  HsRec* s2d_hs;       // HS8 [B][4G][h/2+2][w/2+2] (phase-major groups, hs_relayout.h) or null
  int G, h, w;
  size_t n;            // B * G * h * w records
};
__device__ __forceinline__ void bn_term(const BnSrc& s, size_t b, int G, int g, int y, int x, int h, int w, float v[8], bool add) {
  float zz[8];
  hs_unpack(s.z[((b * G + g) * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1)], zz);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = g * 8 + e;
    const float t = (zz[e] * (1.f / HS_ASCALE) - s.mean[c]) * s.scale[c] + s.beta[c];
    v[e] = add ? v[e] + t : t;
  }
}
__global__ __launch_bounds__(256) void bn_apply_kernel(BnApplyArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int h = a.h, w = a.w, G = a.G;
  const int x = (int)(i % w);
  size_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int g = (int)(t % G);
  const size_t b = t / G;
  float v[8];
  bn_term(a.a, b, G, g, y, x, h, w, v, false);
  if (a.b.z) bn_term(a.b, b, G, g, y, x, h, w, v, true);
  if (a.res) {
    float r[8];
    hs_unpack(a.res[((b * G + g) * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1)], r);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += r[e] * (1.f / HS_ASCALE);
  }
  float u[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    v[e] = fmaxf(v[e], 0.f);
    u[e] = v[e] * HS_ASCALE;
  }
  const HsRec rec = hs_pack(u);
  if (a.out) a.out[((b * G + g) * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1)] = rec;
  const int ph = (y & 1) * 2 + (x & 1), h2 = h >> 1, w2 = w >> 1;
  if (a.s2d_hs) a.s2d_hs[((b * 4 * G + (size_t)ph * G + g) * (h2 + 2) + ((y >> 1) + 1)) * (size_t)(w2 + 2) + (x >> 1) + 1] = rec;
}

// ------------------------------------------------------------------------------------------- workspace plan (offsets in floats)
constexpr size_t NONE = ~(size_t)0;
struct TrainPlan {
  size_t ob = 0, zstem = 0, stem_s = 0;   // observation (space-to-depth), the stem's z, the stem's space-to-depth activation
  size_t za[4], t1[4], o0[4], t2[4], o1[4], o1s[3];
  // the raw outputs of conv2 and of block 1's two convolutions: ONE buffer per stage reused three times in the forward's plan (nothing is
  // kept), three buffers in the gradient's
  size_t z2[4], z3[4], z4[4];
  size_t stem_a = NONE;                   // gradient plan only: the stem's activation in place (the mask of its BatchNorm backward)
  // gradient plan only, per stage at planes x h x w: the gradient of o1 / o0 / t1, t2; dz of the layer at hand, dz of the shortcut, the
  // identity branch's dy; the shortcut's adjoint (in_planes x h x w) and the entry's (4 in_planes x h x w); of the stem's activation
  size_t gA[4], gB[4], gM[4], dZ[4], dZs[4], dY[4], gR[4], gS[4], g_stem = 0, dz_stem = 0;
  size_t part = 0;                        // doubles: the partial sums of the largest layer
  size_t total = 0;
};
inline size_t bn_pieces(long long npix) { return bn_fwd_pieces(npix); }
// every tensor is HS8.  keep: the gradient's plan
TrainPlan make_train_plan(int capB, int cin_pad, int H, int W, bool keep = false) {
  TrainPlan P;
  size_t off = 0, part = 0;
  auto add = [&](size_t& d, int C, int h, int w) {
    d = off;
    off += hs_act_floats(C, h, w) * capB;
    off = (off + 63) & ~(size_t)63;
  };
  auto stat = [&](int C, int h, int w) {
    const size_t n = bn_pieces((long long)capB * h * w) * C * 2;
    if (n > part) part = n;
  };
  add(P.ob, 4 * cin_pad, H / 2, W / 2);
  add(P.zstem, 64, H / 2, W / 2);
  stat(64, H / 2, W / 2);
  add(P.stem_s, 4 * 64, H / 4, W / 4);
  if (keep) {
    add(P.stem_a, 64, H / 2, W / 2);
    add(P.g_stem, 64, H / 2, W / 2);
    add(P.dz_stem, 64, H / 2, W / 2);
  }
  int in_planes = 64;
  for (int n = 0; n < 4; ++n) {
    const int p = stage_planes(n), h = H >> (n + 2), w = W >> (n + 2);
    add(P.za[n], 2 * p, h, w);   // the entry's two outputs, conv1 and the shortcut: two tensors of p channels back to back
    add(P.z2[n], p, h, w);
    P.z3[n] = P.z4[n] = P.z2[n];
    add(P.t1[n], p, h, w);
    add(P.o0[n], p, h, w);
    add(P.t2[n], p, h, w);
    add(P.o1[n], p, h, w);
    if (n < 3) add(P.o1s[n], 4 * p, h / 2, w / 2);
    stat(p, h, w);
    if (keep) {
      add(P.z3[n], p, h, w);
      add(P.z4[n], p, h, w);
      for (size_t* g : {&P.gA[n], &P.gB[n], &P.gM[n], &P.dZ[n], &P.dZs[n], &P.dY[n]}) add(*g, p, h, w);
      add(P.gR[n], in_planes, h, w);
      add(P.gS[n], 4 * in_planes, h, w);
    }
    in_planes = p;
  }
  off = (off + 63) & ~(size_t)63;
  P.part = off;                      // 256-byte aligned: doubles
  off += part * 2;
  P.total = off + (1u << 18);        // slack: overhanging tiles read past their tensor
  return P;
}

int check_train_call(const PolicyNet& N, const char* who, int B, int H, int W) {
  if (!N.loaded) {
    set_error("%s called before pnpx_policy_load", who);
    return PNPX_ERR_NO_WEIGHTS;
  }
  if (B <= 0 || H < 32 || W < 32 || (H % 32) || (W % 32)) {
    set_error("%s: need B > 0 and H, W positive multiples of 32 (got %d x %d x %d)", who, B, H, W);
    return PNPX_ERR_SHAPE;
  }
  if ((long long)B * (H / 32) * (W / 32) < 2) {
    set_error("%s: batch statistics need more than 1 value per channel in the last stage (got %d x %d x %d)", who, B, H, W);
    return PNPX_ERR_ARG;
  }
  return PNPX_OK;
}

// The launch sequence of the train-mode forward over plan P in workspace A: shared by policy_forward_train (plan without `keep`: the
// three stride-1 z of a stage share a buffer) and by the re-computation of policy_param_grad (everything kept).
// probs == null: no head launch.
int train_forward_launches(pnpx_ctx* ctx, const TrainPlan& P, float* A, const float* ob, float* probs, float* det, int B, int H,
                           int W, float momentum, int update_running, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  auto hsc = [&](size_t off) { return reinterpret_cast<char*>(A + off); };
  auto rec = [&](size_t off) { return reinterpret_cast<HsRec*>(A + off); };
  double* part = reinterpret_cast<double*>(A + P.part);
  float* params = N.live.p();
  float* st_mean = static_cast<float*>(N.bn_buf.p);
  float* st_var = st_mean + POLICY_BN_CHANNELS;
  float* st_scale = st_var + POLICY_BN_CHANNELS;
  float* st_shift = st_scale + POLICY_BN_CHANNELS;
  BnLayer BL[NBN];
  bn_layers(N.num_inputs, BL);
  unsigned* range_flag = ctx->opt_range_guard ? ctx->range_flag_dev : nullptr;

  // the raw convolution: linear epilogue, zero bias (the fold-free packing's shifts)
  auto conv_hs = [&](int li, size_t in, int in_groups, size_t out, int h, int w) -> int {
    const ConvLayerHsDev& D = N.raw.hs[li];
    const int taps = trunk_taps(li, false);
    ConvHsFuse f;
    f.slope = 1.f;
    f.taps = taps;
    if (taps != 0x1FF) {
      f.wreg = 0;
      f.in0_groups = in_groups;
    }
    f.range_flag = range_flag;
    return launch_conv_hs(hs_layer(D, N.raw.hs_bias[li]), hsc(in), D.cin_pad / 8, nullptr, 0, hsc(out), B, h, w, f, s);
  };
  // statistics of layer l's raw output at `z` (h x w)
  auto stats = [&](size_t z, int h, int w, int l) -> int {
    const BnLayer& L = BL[l];
    BnStatsJob J;
    J.z = rec(z);
    J.G = L.cout / 8;
    J.B = B;
    J.h = h;
    J.w = w;
    J.part = part;
    J.params = params;
    J.bn = L.bn;
    J.mean = st_mean + L.chan0;
    J.var = st_var + L.chan0;
    J.scale = st_scale + L.chan0;
    J.shift = st_shift + L.chan0;
    J.momentum = momentum;
    J.update = update_running ? 1 : 0;
    return launch_bn_stats(J, s);
  };
  auto src = [&](size_t z, int l) {
    const BnLayer& L = BL[l];
    return BnSrc{rec(z), st_mean + L.chan0, st_scale + L.chan0, params + L.bn + L.cout};
  };
  // `sd`: the space-to-depth copy for a following stride-2 entry (offset; NONE = none); out / res: NONE = none
  auto apply = [&](BnSrc a0, BnSrc b0, size_t res, size_t out, size_t sd, int G, int h, int w) -> int {
    BnApplyJob J;
    J.a = a0;
    J.b = b0;
    J.res = res == NONE ? nullptr : rec(res);
    J.out = out == NONE ? nullptr : rec(out);
    J.s2d_hs = sd == NONE ? nullptr : rec(sd);
    J.G = G;
    J.B = B;
    J.h = h;
    J.w = w;
    return launch_bn_apply(J, s);
  };
  const BnSrc no_src{nullptr, nullptr, nullptr, nullptr};

  // stem: conv3x3 stride 2 over the space-to-depth observation -> bn1 -> ReLU -> space-to-depth for the stage-0 entry
  PNPX_TRY(launch_pack_ob_hs(ob, hsc(P.ob), N.num_inputs, N.cin_pad, B, H, W, s));
  PNPX_TRY(conv_hs(0, P.ob, 4 * N.cin_pad / 8, P.zstem, H / 2, W / 2));
  PNPX_TRY(stats(P.zstem, H / 2, W / 2, 0));
  PNPX_TRY(apply(src(P.zstem, 0), no_src, NONE, P.stem_a, P.stem_s, 8, H / 2, W / 2));
  for (int st = 0; st < 4; ++st) {
    const int h = H >> (st + 2), w = W >> (st + 2), p = stage_planes(st), G = p / 8, c0 = 1 + 5 * st;
    const size_t s2in = st == 0 ? P.stem_s : P.o1s[st - 1];
    const int in_planes = st == 0 ? 64 : stage_planes(st - 1);
    // conv1 and the 1x1 shortcut on the sparse-tap half-split instances: two tensors of p channels, back to back in za
    const size_t zs_off = P.za[st] + (size_t)B * p * (h + 2) * (w + 2);
    PNPX_TRY(conv_hs(c0 + 0, s2in, 4 * in_planes / 8, P.za[st], h, w));
    PNPX_TRY(conv_hs(c0 + 2, s2in, 4 * in_planes / 8, zs_off, h, w));
    PNPX_TRY(stats(P.za[st], h, w, c0 + 0));
    PNPX_TRY(stats(zs_off, h, w, c0 + 2));
    PNPX_TRY(apply(src(P.za[st], c0 + 0), no_src, NONE, P.t1[st], NONE, G, h, w));
    // block 0: relu(bn2(conv2) + shortcut_bn(shortcut_conv))
    PNPX_TRY(conv_hs(c0 + 1, P.t1[st], 0, P.z2[st], h, w));
    PNPX_TRY(stats(P.z2[st], h, w, c0 + 1));
    PNPX_TRY(apply(src(P.z2[st], c0 + 1), src(zs_off, c0 + 2), NONE, P.o0[st], NONE, G, h, w));
    // block 1: relu(bn2(conv2(relu(bn1(conv1(x))))) + x)
    PNPX_TRY(conv_hs(c0 + 3, P.o0[st], 0, P.z3[st], h, w));
    PNPX_TRY(stats(P.z3[st], h, w, c0 + 3));
    PNPX_TRY(apply(src(P.z3[st], c0 + 3), no_src, NONE, P.t2[st], NONE, G, h, w));
    PNPX_TRY(conv_hs(c0 + 4, P.t2[st], 0, P.z4[st], h, w));
    PNPX_TRY(stats(P.z4[st], h, w, c0 + 4));
    PNPX_TRY(apply(src(P.z4[st], c0 + 4), no_src, P.o0[st], P.o1[st], st < 3 ? P.o1s[st] : NONE, G, h, w));
  }
  if (probs) PNPX_TRY(policy_launch_heads(N.raw, N.n_det, N.spi_head, hsc(P.o1[3]), H / 32, W / 32, B, probs, det, s));
  N.bn_have_stats = true;
  if (update_running) N.eval_stale = true;
  return PNPX_OK;
}

}  // namespace

int launch_bn_stats(const BnStatsJob& J, hipStream_t s) {
  const long long npix = (long long)J.B * J.h * J.w;
  const int np = (int)bn_pieces(npix), cout = J.G * 8;
  hipLaunchKernelGGL(bn_partial_kernel, dim3(np, J.G), dim3(256), 0, s, J.z, J.G, J.h, J.w, npix, J.part);
  PNPX_LAUNCH_CHECK();
  BnFinishArgs a;
  a.part = J.part;
  a.cout = cout;
  a.npieces = np;
  a.n = npix;
  a.params = J.params;
  a.bn = J.bn;
  a.mean = J.mean;
  a.var = J.var;
  a.scale = J.scale;
  a.shift = J.shift;
  a.momentum = J.momentum;
  a.update = J.update ? 1 : 0;
  hipLaunchKernelGGL(bn_finish_kernel, dim3((cout + 63) / 64), dim3(64), 0, s, a);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_bn_apply(const BnApplyJob& J, hipStream_t s) {
  BnApplyArgs a;
  a.a = J.a;
  a.b = J.b;
  a.res = J.res;
  a.out = J.out;
  a.s2d_hs = J.s2d_hs;
  a.G = J.G;
  a.h = J.h;
  a.w = J.w;
  a.n = (size_t)J.B * J.G * J.h * J.w;
  hipLaunchKernelGGL(bn_apply_kernel, g1(a.n), dim3(256), 0, s, a);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int policy_forward_train(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                         int update_running, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  PNPX_TRY(check_train_call(N, "policy train forward", B, H, W));
  if (!(momentum >= 0.f && momentum <= 1.f)) {
    set_error("policy train forward: momentum %g outside [0, 1]", (double)momentum);
    return PNPX_ERR_ARG;
  }
  if (!N.raw_valid) PNPX_TRY(policy_pack_raw(ctx, s));
  if (!N.bn_buf.p) PNPX_TRY(alloc_dev(N.bn_buf, 4 * POLICY_BN_CHANNELS * sizeof(float), "policy batch-statistics"));
  policy_kept_drop(N, "pnpx_policy_forward_train overwrote the batch statistics of the kept forward");
  PNPX_TRY(reserve_arena_hs(N.train_ws, N.tcapB, N.tcapH, N.tcapW, B, H, W,
                            [&](int nb) { return make_train_plan(nb, N.cin_pad, H, W).total; }, "policy train workspace"));
  const TrainPlan P = make_train_plan(N.tcapB, N.cin_pad, H, W);
  return train_forward_launches(ctx, P, static_cast<float*>(N.train_ws.p), ob, probs, det, B, H, W, momentum, update_running, s);
}

namespace {

// a buffer outside the workspace: grows to the largest size seen (with the workspace, the only place the call synchronises the device)
int grow(DeviceBuf& b, size_t bytes, const char* what) {
  if (bytes <= b.bytes) return PNPX_OK;
  PNPX_HIP(hipDeviceSynchronize());
  if (b.p) PNPX_HIP(hipFree(b.p));
  b = DeviceBuf();
  return alloc_dev(b, bytes, what);
}

}  // namespace

// d sum(grad_probs * probs + grad_det * det) / d params through the train-mode forward (policy_loss.backward(), trainer.py:171-212).
// policy_param_grad re-computes the forward with update_running = 0 into a workspace of its own that keeps every z and every activation;
// policy_forward_train_keep is that forward as a call of its own (heads and running-statistics update included), after which
// policy_param_grad_kept runs the backward pass alone.  The weight-gradient GEMM reads its HS8 operands (space-to-depth tensors
// included) from the workspace.  Backwards (DESIGN.md section 9c has the table of launches): heads and the gradient range
// (policy_grad.hip), and per layer BatchNorm
// backward -> weight gradient (critic_grad.hip's GEMM, G = dz, X = what the forward launch read) -> adjoint convolution.  The adjoint
// convolutions are linear (the ReLU mask is taken by the BatchNorm backward of the layer below): the critic's input-gradient instance
// without a mask (EPI_DTHR; windows 0x1FF, 0x1B0 with the shortcut's adjoint as residual on the phase-(0,0) groups, then depth-to-space)
// and the plain 1x1 instance for the shortcut.  The stem's adjoint is not run (no observation gradient).  Every element of grad_params
// is written.  The backward pass reads the forward's tensors and the batch statistics and writes gradient tensors only: it can run any
// number of times on one forward.
namespace {

// steps 2 onward on the forward kept under plan P in workspace A (batch statistics in bn_buf)
int param_grad_backward(pnpx_ctx* ctx, const TrainPlan& P, float* A, const float* grad_probs, const float* grad_det, float* grad_params,
                        int B, int H, int W, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  const size_t want = policy_num_params(N.num_inputs, N.n_det, N.spi_head);
  PackDesc PD[NBN];
  PNPX_TRY(policy_pack_descs(N, PD));
  BnLayer BL[NBN];
  bn_layers(N.num_inputs, BL);
  auto rec = [&](size_t off) { return reinterpret_cast<HsRec*>(A + off); };
  auto hsc = [&](size_t off) { return reinterpret_cast<char*>(A + off); };
  const int hl = H / 32, wl = W / 32;

  // outside the workspace: the K-split slabs of the largest layer; then g_f [B][512], the head scratch, gv [B], the BatchNorm-backward
  // coefficients [3][4864], the scale slot and its bits; then (doubles) the BatchNorm-backward partial sums of the largest layer
  size_t slab_floats = 0, part_doubles = 0;
  auto shape_of = [&](int li, int& h, int& w) {
    const int st = li == 0 ? -1 : (li - 1) / 5;
    h = H >> (st + 2);
    w = W >> (st + 2);
  };
  for (int li = 0; li < NBN; ++li) {
    int h, w;
    shape_of(li, h, w);
    const PackDesc& D = PD[li];
    slab_floats = std::max(slab_floats, (size_t)critic_wgrad_pieces(D.rows, D.K, B, h, w) * critic_wgrad_piece_floats(D.rows, D.K, D.nt));
    part_doubles = std::max(part_doubles, bn_bwd_pieces((long long)B * h * w) * D.rows * 3);
  }
  const size_t slab_bytes = (slab_floats * sizeof(float) + 255) & ~(size_t)255;
  const size_t small_floats = ((size_t)B * 512 + (size_t)B * POL_HEAD_STRIDE + B + 3 * POLICY_BN_CHANNELS + 4 + 63) & ~(size_t)63;
  PNPX_TRY(grow(N.grad_slab, slab_bytes + small_floats * sizeof(float) + part_doubles * sizeof(double), "policy gradient slab"));
  float* slab = static_cast<float*>(N.grad_slab.p);
  float* gf = reinterpret_cast<float*>(static_cast<char*>(N.grad_slab.p) + slab_bytes);
  float* head_rows = gf + (size_t)B * 512;
  float* coef = head_rows + (size_t)B * POL_HEAD_STRIDE;
  float2* slot = reinterpret_cast<float2*>(coef + 3 * POLICY_BN_CHANNELS);
  unsigned* bits = reinterpret_cast<unsigned*>(slot + 1);
  float* gv = reinterpret_cast<float*>(bits + 1) + 1;
  double* part = reinterpret_cast<double*>(gf + small_floats);

  const float* st_mean = static_cast<const float*>(N.bn_buf.p);
  const float* st_var = st_mean + POLICY_BN_CHANNELS;
  unsigned* range_flag = ctx->opt_range_guard ? ctx->range_flag_dev : nullptr;

  // 2. heads; 3. the gradient range: s from max |g_f| on the device, boost = 2^(1 + ceil(log2(h w))): the last activation's gradient
  // s * boost * g_f / (h w) has its largest entry in [1, 4)
  PolHeadGradJob HJ;
  HJ.feat = rec(P.o1[3]);
  HJ.h = hl;
  HJ.w = wl;
  HJ.B = B;
  HJ.n_det = N.n_det;
  HJ.spi = N.spi_head;
  HJ.sm_w = N.raw.fc_sm_w;
  HJ.sm_b = N.raw.fc_sm_b;
  HJ.d_w = N.raw.fc_det_w;
  HJ.d_b = N.raw.fc_det_b;
  HJ.d2_w = N.raw.fc_det2_w;
  HJ.d2_b = N.raw.fc_det2_b;
  HJ.gp = grad_probs;
  HJ.gd = grad_det;
  HJ.gf = gf;
  HJ.rows = head_rows;
  HJ.grad = grad_params;
  HJ.head_src = want - (2 * 512 + 2) -
                (N.spi_head ? (size_t)64 * 512 + 64 + (size_t)N.n_det * 64 + N.n_det : (size_t)N.n_det * 512 + N.n_det);
  PNPX_TRY(launch_pol_head_grad(HJ, s));
  int e2 = 0;
  while ((1 << e2) < hl * wl) ++e2;
  const float boost = std::ldexp(1.0f, 1 + e2), inv_boost = 1.0f / boost;
  PNPX_TRY(launch_pol_grad_seed(gf, bits, slot, rec(P.gA[3]), gv, boost, B, hl, wl, s));

  // BatchNorm backward of layer l0 [and l1] from the activation gradient g masked by the saved activation act
  auto bn_layer = [&](int li, size_t z, size_t dz) {
    BnBwdLayer L;
    L.z = rec(z);
    L.mean = st_mean + BL[li].chan0;
    L.var = st_var + BL[li].chan0;
    L.bn = BL[li].bn;
    L.coef = coef + 3 * (size_t)BL[li].chan0;
    L.dz = rec(dz);
    return L;
  };
  auto bn_bwd = [&](size_t g, size_t act, const BnBwdLayer& l0, const BnBwdLayer* l1, size_t dy_out, int G, int h, int w) -> int {
    BnBwdJob J;
    J.g = rec(g);
    J.act = rec(act);
    J.l0 = l0;
    if (l1) J.l1 = *l1;
    J.dy_out = dy_out == NONE ? nullptr : rec(dy_out);
    J.G = G;
    J.B = B;
    J.h = h;
    J.w = w;
    J.part = part;
    J.params = N.live.p();
    J.grad = grad_params;
    J.slot = slot;
    J.inv_boost = inv_boost;
    J.range_flag = range_flag;
    return launch_bn_bwd(J, s);
  };
  // gradient of convolution li: G = dz (cout channels), X = the tensor its forward launch read (Xc channels)
  auto wgrad = [&](int li, size_t G, size_t X, int Xc, int h, int w) -> int {
    const PackDesc& D = PD[li];
    WgradJob Wj;
    Wj.G = rec(G);
    Wj.X = rec(X);
    Wj.gv = gv;
    Wj.Gg = D.rows / 8;
    Wj.Xg = Xc / 8;
    Wj.cout = D.rows;
    Wj.K = D.K;
    Wj.nt = D.nt;
    for (int t = 0; t < D.nt; ++t) Wj.tap[t] = D.tap[t];
    Wj.B = B;
    Wj.h = h;
    Wj.w = w;
    PNPX_TRY(launch_critic_wgrad(Wj, slab, s));
    return launch_pol_wgrad_finish(D, (int)(BL[li].bn - D.src_v) / D.rows, critic_wgrad_pieces(D.rows, D.K, B, h, w),
                                   1.0f / (HS_ASCALE * HS_ASCALE), slab, grad_params, s);
  };
  // adjoint convolution of layer li: out = W^T in [+ res on the first resC channels]; epi 2 = the critic's input-gradient instance
  // (no mask), 0 = the plain linear one (the 1x1 shortcut)
  auto adjoint = [&](int li, int epi, size_t in, int inC, size_t out, int outC, size_t res, int resC, int h, int w) -> int {
    HsLaunch L;
    L.D = &N.raw_bwd[li];
    L.bias = N.raw_adj_zero;
    L.taps = trunk_taps(li, true);
    L.epi = epi;
    L.range_flag = range_flag;
    return launch_hs_conv(L, hsc(in), inC, hsc(out), outC, res == NONE ? nullptr : hsc(res), resC, nullptr, 0, B, h, w, s);
  };

  for (int st = 3; st >= 0; --st) {
    const int h = H >> (st + 2), w = W >> (st + 2), p = stage_planes(st), G = p / 8, l0 = 1 + 5 * st;
    const int in_planes = st == 0 ? 64 : stage_planes(st - 1);
    const size_t x = st == 0 ? P.stem_s : P.o1s[st - 1];
    const size_t zs = P.za[st] + (size_t)B * p * (h + 2) * (w + 2);
    // block 1: o1 = relu(bn(conv2(t2)) + o0), t2 = relu(bn(conv1(o0)))
    PNPX_TRY(bn_bwd(P.gA[st], P.o1[st], bn_layer(l0 + 4, P.z4[st], P.dZ[st]), nullptr, P.dY[st], G, h, w));
    PNPX_TRY(wgrad(l0 + 4, P.dZ[st], P.t2[st], p, h, w));
    PNPX_TRY(adjoint(l0 + 4, 2, P.dZ[st], p, P.gM[st], p, NONE, 0, h, w));
    PNPX_TRY(bn_bwd(P.gM[st], P.t2[st], bn_layer(l0 + 3, P.z3[st], P.dZ[st]), nullptr, NONE, G, h, w));
    PNPX_TRY(wgrad(l0 + 3, P.dZ[st], P.o0[st], p, h, w));
    PNPX_TRY(adjoint(l0 + 3, 2, P.dZ[st], p, P.gB[st], p, P.dY[st], p, h, w));
    // block 0: o0 = relu(bn(conv2(t1)) + bn(shortcut(x))), t1 = relu(bn(conv1(x))), x = space-to-depth input
    const BnBwdLayer sc = bn_layer(l0 + 2, zs, P.dZs[st]);
    PNPX_TRY(bn_bwd(P.gB[st], P.o0[st], bn_layer(l0 + 1, P.z2[st], P.dZ[st]), &sc, NONE, G, h, w));
    PNPX_TRY(wgrad(l0 + 1, P.dZ[st], P.t1[st], p, h, w));
    PNPX_TRY(wgrad(l0 + 2, P.dZs[st], x, 4 * in_planes, h, w));
    PNPX_TRY(adjoint(l0 + 1, 2, P.dZ[st], p, P.gM[st], p, NONE, 0, h, w));
    PNPX_TRY(bn_bwd(P.gM[st], P.t1[st], bn_layer(l0 + 0, P.za[st], P.dZ[st]), nullptr, NONE, G, h, w));
    PNPX_TRY(wgrad(l0 + 0, P.dZ[st], x, 4 * in_planes, h, w));
    // shortcut adjoint (1x1, to the phase-(0,0) groups) = the residual of the entry's adjoint (mirrored window); then depth-to-space
    PNPX_TRY(adjoint(l0 + 2, 0, P.dZs[st], p, P.gR[st], in_planes, NONE, 0, h, w));
    PNPX_TRY(adjoint(l0 + 0, 2, P.dZ[st], p, P.gS[st], 4 * in_planes, P.gR[st], in_planes, h, w));
    const size_t below = st == 0 ? P.g_stem : P.gA[st - 1];
    const int Gb = in_planes / 8;
    const size_t nq = (size_t)B * Gb * (2 * h) * (2 * w) * 2;
    hipLaunchKernelGGL(hs_d2s_kernel, g1(nq), dim3(256), 0, s, reinterpret_cast<const uint4*>(A + P.gS[st]), reinterpret_cast<uint4*>(A + below),
                       Gb, h, w, nq);
    PNPX_LAUNCH_CHECK();
  }
  PNPX_TRY(bn_bwd(P.g_stem, P.stem_a, bn_layer(0, P.zstem, P.dz_stem), nullptr, NONE, 8, H / 2, W / 2));
  return wgrad(0, P.dz_stem, P.ob, 4 * N.cin_pad, H / 2, W / 2);
}

int check_grad_room(const PolicyNet& N, const char* who, size_t n) {
  const size_t want = policy_num_params(N.num_inputs, N.n_det, N.spi_head);
  if (n != want) {
    set_error("%s: the loaded actor (%d inputs, %d outputs, spi %d) has %zu parameters, got room for %zu", who, N.num_inputs, N.n_det,
              N.spi_head, want, n);
    return PNPX_ERR_ARG;
  }
  return PNPX_OK;
}

// the gradient workspace for B x H x W under the keep plan; whatever was kept in it is gone from here on
int reserve_grad_ws(PolicyNet& N, int B, int H, int W, const char* lost) {
  policy_kept_drop(N, lost);
  if (!N.bn_buf.p) PNPX_TRY(alloc_dev(N.bn_buf, 4 * POLICY_BN_CHANNELS * sizeof(float), "policy batch-statistics"));
  return reserve_arena_hs(N.grad_ws, N.gcapB, N.gcapH, N.gcapW, B, H, W,
                          [&](int nb) { return make_train_plan(nb, N.cin_pad, H, W, true).total; }, "policy gradient workspace");
}

}  // namespace

// Nothing is kept between calls; weights and running statistics do not change, the batch statistics in bn_buf are those of a train
// forward on `ob`.  A kept forward is overwritten.
int policy_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_probs, const float* grad_det, float* grad_params, size_t n, int B,
                      int H, int W, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  PNPX_TRY(check_train_call(N, "policy parameter gradient", B, H, W));
  PNPX_TRY(check_grad_room(N, "pnpx_policy_param_grad", n));
  if (!N.raw_valid) PNPX_TRY(policy_pack_raw(ctx, s));
  if (!N.adj_valid) PNPX_TRY(policy_pack_adj(ctx, s));
  PNPX_TRY(reserve_grad_ws(N, B, H, W, "pnpx_policy_param_grad overwrote the workspace of the kept forward"));
  const TrainPlan P = make_train_plan(N.gcapB, N.cin_pad, H, W, true);
  float* A = static_cast<float*>(N.grad_ws.p);
  // 1. forward re-computation (the batch statistics land in bn_buf)
  PNPX_TRY(train_forward_launches(ctx, P, A, ob, nullptr, nullptr, B, H, W, 0.f, 0, s));
  return param_grad_backward(ctx, P, A, grad_probs, grad_det, grad_params, B, H, W, s);
}

// policy_forward_train's launch sequence over the keep plan in the gradient workspace: the same probs, det, batch statistics and moved
// running statistics, and every raw output and activation left where policy_param_grad_kept reads them.
int policy_forward_train_keep(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                              int update_running, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  PNPX_TRY(check_train_call(N, "policy kept train forward", B, H, W));
  if (!(momentum >= 0.f && momentum <= 1.f)) {
    set_error("policy kept train forward: momentum %g outside [0, 1]", (double)momentum);
    return PNPX_ERR_ARG;
  }
  if (!N.raw_valid) PNPX_TRY(policy_pack_raw(ctx, s));
  PNPX_TRY(reserve_grad_ws(N, B, H, W, "a later pnpx_policy_forward_train_keep failed"));
  const TrainPlan P = make_train_plan(N.gcapB, N.cin_pad, H, W, true);
  PNPX_TRY(train_forward_launches(ctx, P, static_cast<float*>(N.grad_ws.p), ob, probs, det, B, H, W, momentum, update_running, s));
  N.kept_valid = true;
  N.keptB = B;
  N.keptH = H;
  N.keptW = W;
  N.kept_capB = N.gcapB;
  N.kept_capH = N.gcapH;
  N.kept_capW = N.gcapW;
  return PNPX_OK;
}

int policy_param_grad_kept(pnpx_ctx* ctx, const float* grad_probs, const float* grad_det, float* grad_params, size_t n, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  if (!N.loaded) {
    set_error("pnpx_policy_param_grad_kept called before pnpx_policy_load");
    return PNPX_ERR_NO_WEIGHTS;
  }
  if (!N.kept_valid) {
    set_error("pnpx_policy_param_grad_kept: there is no kept forward: %s", N.kept_lost);
    return PNPX_ERR_ARG;
  }
  if (!N.raw_valid || !N.grad_ws.p || N.kept_capB != N.gcapB || N.kept_capH != N.gcapH || N.kept_capW != N.gcapW) {
    policy_kept_drop(N, "the gradient workspace was allocated again or the weights changed after the kept forward");
    set_error("pnpx_policy_param_grad_kept: there is no kept forward: %s", N.kept_lost);
    return PNPX_ERR_ARG;
  }
  PNPX_TRY(check_grad_room(N, "pnpx_policy_param_grad_kept", n));
  if (!N.adj_valid) PNPX_TRY(policy_pack_adj(ctx, s));
  const TrainPlan P = make_train_plan(N.kept_capB, N.cin_pad, N.keptH, N.keptW, true);
  return param_grad_backward(ctx, P, static_cast<float*>(N.grad_ws.p), grad_probs, grad_det, grad_params, N.keptB, N.keptH, N.keptW, s);
}

int policy_bn_stats(pnpx_ctx* ctx, float* mean_dev, float* var_dev, size_t n, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  if (!N.loaded || !N.bn_have_stats) {
    set_error("pnpx_policy_bn_stats called before a train-mode forward (pnpx_policy_forward_train)");
    return PNPX_ERR_NO_WEIGHTS;
  }
  if (!mean_dev || !var_dev || n != POLICY_BN_CHANNELS) {
    set_error("pnpx_policy_bn_stats: the actor has %zu BatchNorm channels, got room for %zu", POLICY_BN_CHANNELS, n);
    return PNPX_ERR_ARG;
  }
  const float* m = static_cast<const float*>(N.bn_buf.p);
  PNPX_HIP(hipMemcpyAsync(mean_dev, m, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  PNPX_HIP(hipMemcpyAsync(var_dev, m + POLICY_BN_CHANNELS, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return PNPX_OK;
}

}  // namespace pnpx
