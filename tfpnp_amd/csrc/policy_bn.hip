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
//                       convolution reads and, before a stride-2 entry, its space-to-depth copy (HS8, or fp32 planar with
//                       policy_s2_hs = 0).  (z - mean) * scale + bias is z * scale + shift without the cancellation of two large terms.
// Batch statistics couple the images: the forward is ONE launch chain whatever the "chains" option says.  Pool and heads are the
// eval forward's.  Nothing is kept for a backward pass; fusing the passes into the convolutions is a later step.
#include <cmath>

#include "common.h"
#include "conv_hs.h"
#include "hs_rec.h"
#include "policy_conv.h"
#include "resnet18_hs.h"

namespace pnpx {
namespace {

constexpr double BN_EPS = 1e-5;
constexpr int NBN = TRUNK_LAYERS;    // one BatchNorm behind every convolution: the trunk's layer numbering (resnet18_hs.h)
constexpr int BN_PIECE = 2048;       // pixels per partial sum: 256 threads x 8

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
  int C, c_off, cout, npieces;   // channels of the tensor behind `part`; this layer's first channel in it and its size
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
    const double* e = a.part + ((size_t)p * a.C + a.c_off + c) * 2;
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

struct BnSrc {
  const HsRec* z;      // null: absent
  int Gt, g0;          // channel groups per image of the tensor; the first group of this layer in it
  const float *mean, *scale, *beta;   // at the layer's first channel
};
struct BnApplyArgs {
  BnSrc a, b;          // b: the second normalised summand (block 0: the shortcut)
  const HsRec* res;    // identity residual, HS8 [B][G][h+2][w+2], or null
  HsRec* out;          // HS8 [B][G][h+2][w+2] or null
  HsRec* s2d_hs;       // HS8 [B][4G][h/2+2][w/2+2] (phase-major groups, hs_relayout.h) or null
  float* s2d_f32;      // fp32 planar [B][4 * 8G][h/2+2][pol_wp(w/2)] or null
  int G, h, w;
  size_t n;            // B * G * h * w records
};
__device__ __forceinline__ void bn_term(const BnSrc& s, size_t b, int g, int y, int x, int h, int w, float v[8], bool add) {
  float zz[8];
  hs_unpack(s.z[((b * s.Gt + s.g0 + g) * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1)], zz);
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
  bn_term(a.a, b, g, y, x, h, w, v, false);
  if (a.b.z) bn_term(a.b, b, g, y, x, h, w, v, true);
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
  if (a.s2d_f32) {
    const int C = 8 * G, Hp2 = padded_h(h2), Wp2 = pol_wp(w2);
    float* o = a.s2d_f32 + ((b * 4 * C + (size_t)ph * C + g * 8) * Hp2 + (y >> 1) + 1) * Wp2 + (x >> 1) + POL_PADL;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[(size_t)e * Hp2 * Wp2] = v[e];
  }
}

// ------------------------------------------------------------------------------------------- workspace plan (offsets in floats)
struct TrainPlan {
  size_t ob = 0, zstem = 0, stem_s = 0;   // observation (space-to-depth), the stem's z, the stem's space-to-depth activation
  size_t za[4], zb[4], t1[4], o0[4], t2[4], o1[4], o1s[3];
  size_t part = 0;                        // doubles: the partial sums of the largest layer
  size_t total = 0;
};
inline size_t bn_pieces(long long npix) { return (size_t)((npix + BN_PIECE - 1) / BN_PIECE); }
// s2_hs: the observation and the space-to-depth activations are HS8 tensors (else fp32 planar)
TrainPlan make_train_plan(int capB, int cin_pad, int H, int W, bool s2_hs) {
  TrainPlan P;
  size_t off = 0, part = 0;
  auto add = [&](size_t& d, int C, int h, int w, bool hs) {
    d = off;
    off += (hs ? (size_t)C * (h + 2) * (w + 2) : (size_t)C * padded_h(h) * pol_wp(w)) * capB;
    off = (off + 63) & ~(size_t)63;
  };
  auto stat = [&](int C, int h, int w) {
    const size_t n = bn_pieces((long long)capB * h * w) * C * 2;
    if (n > part) part = n;
  };
  add(P.ob, 4 * cin_pad, H / 2, W / 2, s2_hs);
  add(P.zstem, 64, H / 2, W / 2, true);
  stat(64, H / 2, W / 2);
  add(P.stem_s, 4 * 64, H / 4, W / 4, s2_hs);
  for (int n = 0; n < 4; ++n) {
    const int p = stage_planes(n), h = H >> (n + 2), w = W >> (n + 2);
    add(P.za[n], 2 * p, h, w, true);   // the entry's two outputs: one tensor of 2p channels (fp32 launch) or two of p, back to back
    add(P.zb[n], p, h, w, true);
    add(P.t1[n], p, h, w, true);
    add(P.o0[n], p, h, w, true);
    add(P.t2[n], p, h, w, true);
    add(P.o1[n], p, h, w, true);
    if (n < 3) add(P.o1s[n], 4 * p, h / 2, w / 2, s2_hs);
    stat(2 * p, h, w);
  }
  off = (off + 63) & ~(size_t)63;
  P.part = off;                      // 256-byte aligned: doubles
  off += part * 2;
  P.total = off + (1u << 18);        // slack: overhanging tiles read past their tensor
  return P;
}

}  // namespace

int policy_forward_train(pnpx_ctx* ctx, const float* ob, float* probs, float* det, int B, int H, int W, float momentum,
                         int update_running, hipStream_t s) {
  PolicyNet& N = ctx->policy;
  if (!N.loaded) {
    set_error("policy train forward called before pnpx_policy_load");
    return PNPX_ERR_NO_WEIGHTS;
  }
  if (B <= 0 || H < 32 || W < 32 || (H % 32) || (W % 32)) {
    set_error("policy train forward: need B > 0 and H, W positive multiples of 32 (got %d x %d x %d)", B, H, W);
    return PNPX_ERR_SHAPE;
  }
  if ((long long)B * (H / 32) * (W / 32) < 2) {
    set_error("policy train forward: batch statistics need more than 1 value per channel in the last stage (got %d x %d x %d)", B, H, W);
    return PNPX_ERR_ARG;
  }
  if (!(momentum >= 0.f && momentum <= 1.f)) {
    set_error("policy train forward: momentum %g outside [0, 1]", (double)momentum);
    return PNPX_ERR_ARG;
  }
  if (!N.raw_valid) PNPX_TRY(policy_pack_raw(ctx, s));
  const bool s2_hs = ctx->opt_policy_s2_hs != 0;
  if (!N.bn_buf.p) PNPX_TRY(alloc_dev(N.bn_buf, 4 * POLICY_BN_CHANNELS * sizeof(float), "policy batch-statistics"));
  PNPX_TRY(reserve_arena_hs(N.train_ws, N.tcapB, N.tcapH, N.tcapW, B, H, W,
                            [&](int nb) { return make_train_plan(nb, N.cin_pad, H, W, s2_hs).total; }, "policy train workspace"));
  const TrainPlan P = make_train_plan(N.tcapB, N.cin_pad, H, W, s2_hs);
  float* A = static_cast<float*>(N.train_ws.p);
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
  auto conv_f32 = [&](PolicyConv C, size_t in, size_t out, int h, int w) -> int {
    C.split_c = 0;   // every cout tile takes the linear epilogue and lands in ONE HS8 tensor of C.cout channels
    return launch_policy_conv(C, A + in, nullptr, A + out, nullptr, false, B, h, w, s, true);
  };
  // statistics of the C-channel tensor at `z` (h x w), finished for layers l0 [and l1: the second half of the channels]
  auto stats = [&](size_t z, int C, int h, int w, int l0, int l1) -> int {
    const long long npix = (long long)B * h * w;
    const int np = (int)bn_pieces(npix);
    hipLaunchKernelGGL(bn_partial_kernel, dim3(np, C / 8), dim3(256), 0, s, rec(z), C / 8, h, w, npix, part);
    PNPX_LAUNCH_CHECK();
    const int ls[2] = {l0, l1};
    int c_off = 0;
    for (int k = 0; k < 2 && ls[k] >= 0; ++k) {
      const BnLayer& L = BL[ls[k]];
      BnFinishArgs a;
      a.part = part;
      a.C = C;
      a.c_off = c_off;
      a.cout = L.cout;
      a.npieces = np;
      a.n = npix;
      a.params = params;
      a.bn = L.bn;
      a.mean = st_mean + L.chan0;
      a.var = st_var + L.chan0;
      a.scale = st_scale + L.chan0;
      a.shift = st_shift + L.chan0;
      a.momentum = momentum;
      a.update = update_running ? 1 : 0;
      hipLaunchKernelGGL(bn_finish_kernel, dim3((L.cout + 63) / 64), dim3(64), 0, s, a);
      PNPX_LAUNCH_CHECK();
      c_off += L.cout;
    }
    return PNPX_OK;
  };
  auto src = [&](size_t z, int Gt, int g0, int l) {
    const BnLayer& L = BL[l];
    return BnSrc{rec(z), Gt, g0, st_mean + L.chan0, st_scale + L.chan0, params + L.bn + L.cout};
  };
  // `sd`: the space-to-depth copy for a following stride-2 entry (offset; SIZE_MAX = none); out / res: SIZE_MAX = none
  constexpr size_t NONE = ~(size_t)0;
  auto apply = [&](BnSrc a0, BnSrc b0, size_t res, size_t out, size_t sd, int G, int h, int w) -> int {
    BnApplyArgs a;
    a.a = a0;
    a.b = b0;
    a.res = res == NONE ? nullptr : rec(res);
    a.out = out == NONE ? nullptr : rec(out);
    a.s2d_hs = (sd != NONE && s2_hs) ? rec(sd) : nullptr;
    a.s2d_f32 = (sd != NONE && !s2_hs) ? A + sd : nullptr;
    a.G = G;
    a.h = h;
    a.w = w;
    a.n = (size_t)B * G * h * w;
    hipLaunchKernelGGL(bn_apply_kernel, g1(a.n), dim3(256), 0, s, a);
    PNPX_LAUNCH_CHECK();
    return PNPX_OK;
  };
  const BnSrc no_src{nullptr, 0, 0, nullptr, nullptr, nullptr};

  // stem: conv3x3 stride 2 over the space-to-depth observation -> bn1 -> ReLU -> space-to-depth for the stage-0 entry
  if (s2_hs) {
    PNPX_TRY(launch_pack_ob_hs(ob, hsc(P.ob), N.num_inputs, N.cin_pad, B, H, W, s));
    PNPX_TRY(conv_hs(0, P.ob, 4 * N.cin_pad / 8, P.zstem, H / 2, W / 2));
  } else {
    PNPX_TRY(policy_launch_pack_ob_f32(ob, A + P.ob, N.num_inputs, N.cin_pad, B, H, W, s));
    PNPX_TRY(conv_f32(N.raw.f32[0], P.ob, P.zstem, H / 2, W / 2));
  }
  PNPX_TRY(stats(P.zstem, 64, H / 2, W / 2, 0, -1));
  PNPX_TRY(apply(src(P.zstem, 8, 0, 0), no_src, NONE, NONE, P.stem_s, 8, H / 2, W / 2));
  for (int st = 0; st < 4; ++st) {
    const int h = H >> (st + 2), w = W >> (st + 2), p = stage_planes(st), G = p / 8, c0 = 1 + 5 * st;
    const size_t s2in = st == 0 ? P.stem_s : P.o1s[st - 1];
    const int in_planes = st == 0 ? 64 : stage_planes(st - 1);
    BnSrc z1, zs;
    if (s2_hs) {   // conv1 and the 1x1 shortcut on the sparse-tap half-split instances: two tensors of p channels
      const size_t zs_off = P.za[st] + (size_t)B * p * (h + 2) * (w + 2);
      PNPX_TRY(conv_hs(c0 + 0, s2in, 4 * in_planes / 8, P.za[st], h, w));
      PNPX_TRY(conv_hs(c0 + 2, s2in, 4 * in_planes / 8, zs_off, h, w));
      PNPX_TRY(stats(P.za[st], p, h, w, c0 + 0, -1));
      PNPX_TRY(stats(zs_off, p, h, w, c0 + 2, -1));
      z1 = src(P.za[st], G, 0, c0 + 0);
      zs = src(zs_off, G, 0, c0 + 2);
    } else {       // one fp32 tap-sparse launch: conv1 in channels [0, p), the shortcut in [p, 2p) of one tensor
      PNPX_TRY(conv_f32(N.raw.f32[1 + st], s2in, P.za[st], h, w));
      PNPX_TRY(stats(P.za[st], 2 * p, h, w, c0 + 0, c0 + 2));
      z1 = src(P.za[st], 2 * G, 0, c0 + 0);
      zs = src(P.za[st], 2 * G, G, c0 + 2);
    }
    PNPX_TRY(apply(z1, no_src, NONE, P.t1[st], NONE, G, h, w));
    // block 0: relu(bn2(conv2) + shortcut_bn(shortcut_conv))
    PNPX_TRY(conv_hs(c0 + 1, P.t1[st], 0, P.zb[st], h, w));
    PNPX_TRY(stats(P.zb[st], p, h, w, c0 + 1, -1));
    PNPX_TRY(apply(src(P.zb[st], G, 0, c0 + 1), zs, NONE, P.o0[st], NONE, G, h, w));
    // block 1: relu(bn2(conv2(relu(bn1(conv1(x))))) + x)
    PNPX_TRY(conv_hs(c0 + 3, P.o0[st], 0, P.zb[st], h, w));
    PNPX_TRY(stats(P.zb[st], p, h, w, c0 + 3, -1));
    PNPX_TRY(apply(src(P.zb[st], G, 0, c0 + 3), no_src, NONE, P.t2[st], NONE, G, h, w));
    PNPX_TRY(conv_hs(c0 + 4, P.t2[st], 0, P.zb[st], h, w));
    PNPX_TRY(stats(P.zb[st], p, h, w, c0 + 4, -1));
    PNPX_TRY(apply(src(P.zb[st], G, 0, c0 + 4), no_src, P.o0[st], P.o1[st], st < 3 ? P.o1s[st] : NONE, G, h, w));
  }
  PNPX_TRY(policy_launch_heads(N.raw, N.n_det, N.spi_head, hsc(P.o1[3]), H / 32, W / 32, B, probs, det, s));
  N.bn_have_stats = true;
  if (update_running) N.eval_stale = true;
  return PNPX_OK;
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
