// Value network (critic) forward, input gradient and parameter gradients, live weights.
//
// Live weights: the context keeps the flat fp32 parameter vector on the device (CriticNet::live).  pnpx_critic_load folds
// weight-norm and packs on the host; pnpx_critic_load_device and pnpx_critic_soft_update derive the same packed blob from
// the device vector with four launches ("device-side packing" below) and refresh an already loaded critic in place -- no
// allocation, no device-wide synchronisation, the arena is kept.  Thresholds, weight scales and max |fc_w| are launch
// arguments, so each refresh ends with one small read-back and a synchronisation of the caller's stream: a refresh cannot be
// captured into a graph and has to be issued on the stream the critic's other calls use.  Parameter gradients: critic_param_grad below,
// kernels in critic_grad.hip; critic_value_loss_grad takes value_loss and its backward from one forward.  The optimiser step
// (critic_adam_step: clip + Adam on the live vector, then the refresh; kernels in live_optim.hip) keeps its moments in the context.
// (The actor's refresh: policy_pack.hip.)
//
// Replaces ResNet_wobn(num_inputs, 18, 1).forward (tfpnp/trainer/mddpg/critic.py:95-131) and the autograd pass through it
// with respect to its INPUT, which is how the actor loss uses it (trainer/mddpg/trainer.py:180-192: V_next = critic(eval_ob2)
// is differentiated into the actions; the critic's own weight gradients from that loss are discarded, :206):
//     x = TReLU(conv3x3(num_inputs, 64, stride 2)(ob))                       critic.py:102,122
//     4 stages of 2 BasicBlocks (critic.py:37-60), each stage entered with stride 2 and a 1x1 stride-2 shortcut
//     V = fc(adaptive_avg_pool2d(x, 1))                                      critic.py:128-130
// Convolutions are weight-normalised with bias (w = g * v / ||v||, norm per output channel: folded whenever the weights change);
// TReLU(t) = relu(t - alpha) + alpha = max(t, alpha) with one scalar alpha per activation (critic.py:11-19).
//
// The topology is the actor's, so the forward IS the actor's: resnet18_hs.hip::trunk_forward (layer numbering, host packing of a
// layer, arena and plan of the forward tensors are shared there) -- the stem and the stage entries as 2x2-window convolutions
// (tap mask 0x01B) over HS8 space-to-depth tensors, the shortcut as the 1x1 instance (linear epilogue), the stride-1
// convolutions with the residual operand -- with the TReLU epilogue (conv_hs_trelu.hip) in place of ReLU.
// alpha cannot be folded into the bias: `+ alpha` behind the rectifier would leak into the zero border of the next layer.
//
// Backward (dV/d ob times grad_value): the forward is re-computed (every activation stays in the arena; nothing is kept
// between calls), then the adjoint chain runs on the input-gradient epilogue (conv_hs_dthr.hip):
//     out = (W^T g [+ res]) * (saved activation > alpha)
// where the mask is the one of the layer BELOW (the tensor the forward layer read), so every tensor of the chain is the
// gradient with respect to a pre-activation and each block costs two launches; the sum of a block's two branches is the
// residual operand.  A stride-2 entry is a stride-1 2x2-window convolution on the space-to-depth grid, so its adjoint is the
// mirrored window (0x1B0) on the same grid, masked by the saved space-to-depth tensor, followed by depth-to-space; the
// shortcut's adjoint (1x1, existing linear instance) is its residual operand on the phase-(0,0) channel groups.
// Gradients are carried as HS8 tensors of  s * dV/d(.)  with s a power of two that brings the head's largest entry into [1, 2);
// grad_value[b] / s is applied by the last kernel in fp32, so the result is exactly linear in grad_value.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "conv_hs.h"
#include "critic_grad.h"
#include "hs_rec.h"
#include "hs_relayout.h"
#include "pack_desc.h"
#include "resnet18_hs.h"

namespace pnpx {
namespace {

// what a stored TReLU output equal to its threshold reads back as (the hi/lo split of 16 * alpha, conv_hs_kernel.h)
inline float hs_roundtrip16(float alpha) {
  const float a16 = alpha * HS_ASCALE;
  const _Float16 hi = (_Float16)a16;
  return (float)hi + (float)(_Float16)(a16 - (float)hi);
}

// global average pool over HS8 [B][64 groups][h+2][w+2] + Linear(512, 1).  One workgroup per observation; fixed summation
// order (a result does not depend on the batch it arrives in).
__global__ __launch_bounds__(256) void critic_pool_fc_kernel(const HsRec* __restrict__ feat, int h, int w,
                                                             const float* __restrict__ fc_w, const float* __restrict__ fc_b,
                                                             float* __restrict__ value) {
  __shared__ float part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float inv = 1.f / ((float)(h * w) * HS_ASCALE);
  float acc = 0.f;
  for (int c = tid; c < 512; c += 256) acc = fmaf(hs_pooled(feat, b, 64, c, h, w, inv), fc_w[c], acc);
  part[tid] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) part[tid] += part[tid + st];
    __syncthreads();
  }
  if (tid == 0) value[b] = part[0] + fc_b[0];
}

// head of the backward pass: g[b][c][y][x] = gsc * fc_w[c] where the last TReLU output lies above its threshold
// (gsc = s * HS_ASCALE / (h * w): pool and fc are linear)
__global__ __launch_bounds__(256) void critic_head_grad_kernel(const HsRec* __restrict__ feat, HsRec* __restrict__ g,
                                                               const float* __restrict__ fc_w, float thr, float gsc, int h,
                                                               int w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % w);
  size_t t = i / w;
  const int y = (int)(t % h);
  t /= h;   // t = b * 64 + group
  const int grp = (int)(t % 64);
  const size_t rec = (t * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1);
  const HsRec r = feat[rec];
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = ((float)r.hi[k] + (float)r.lo[k]) > thr ? fc_w[grp * 8 + k] * gsc : 0.f;
  g[rec] = hs_pack(v);
}

// tail of the backward pass: HS8 space-to-depth gradient [B][4*Cp/8][H/2+2][W/2+2] -> grad_ob [B][C][H][W] fp32, times
// grad_value[b] * inv (inv = 1 / (s * HS_ASCALE), a power of two)
__global__ __launch_bounds__(256) void critic_ob_grad_kernel(const HsRec* __restrict__ g, const float* __restrict__ grad_value,
                                                             float* __restrict__ grad_ob, int C, int Cp, int H, int W,
                                                             float inv, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % W);
  size_t t = i / W;
  const int y = (int)(t % H);
  t /= H;
  const int c = (int)(t % C);
  const size_t b = t / C;
  const int Gp = Cp >> 3, ph = (y & 1) * 2 + (x & 1);
  const HsRec& r = g[((b * 4 * Gp + (size_t)ph * Gp + (c >> 3)) * ((H >> 1) + 2) + (y >> 1) + 1) * (size_t)((W >> 1) + 2) + (x >> 1) + 1];
  grad_ob[i] = ((float)r.hi[c & 7] + (float)r.lo[c & 7]) * (grad_value[b] * inv);
}

// nn.MSELoss()(Q_target, V_cur) and d loss / d V (trainer/mddpg/trainer.py:198): gv[b] = 2 (V_b - Q_b) / B in the fp32 steps torch
// takes for `2.0 * (V - Q) / B` on a device tensor, loss = (sum_b (V_b - Q_b)^2) / B with the fp32 squares added in index order in
// double.  torch divides a device tensor by a Python number as a product with inv_b = (float)(1.0 / (double)B) (its
// div_true kernel's scalar branch), which differs from the true quotient in the last bit for some operands unless B is a power of
// two: to return the composed path's bytes the kernel does the same, with inv_b computed by the host.  One block.
__global__ __launch_bounds__(256) void critic_mse_kernel(const float* __restrict__ value, const float* __restrict__ q, float* __restrict__ gv,
                                                         float* __restrict__ loss, int B, float inv_b) {
#pragma clang fp contract(off)
  for (int b = threadIdx.x; b < B; b += 256) gv[b] = (2.0f * (value[b] - q[b])) * inv_b;
  if (threadIdx.x != 0) return;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) {
    const float d = value[b] - q[b];
    acc += (double)(d * d);
  }
  loss[0] = (float)(acc / (double)B);
}

// ------------------------------------------------------------------------------------------- parameter layout
struct WnConv {   // registration order of a weight-normalised Conv2d: bias, weight_g, weight_v
  const float *b, *g, *v;
};
// weight = weight_g * weight_v / ||weight_v||, norm over everything but the output channel (torch.nn.utils.weight_norm, dim 0)
std::vector<float> wn_fold(const WnConv& c, int cout, size_t fan) {
  std::vector<float> w((size_t)cout * fan);
  for (int co = 0; co < cout; ++co) {
    double ss = 0.0;
    for (size_t i = 0; i < fan; ++i) ss += (double)c.v[co * fan + i] * c.v[co * fan + i];
    const double sc = (double)c.g[co] / std::sqrt(ss);
    for (size_t i = 0; i < fan; ++i) w[co * fan + i] = (float)(c.v[co * fan + i] * sc);
  }
  return w;
}
// adjoint with respect to the input: channels transposed, taps mirrored (tap t -> 8 - t), no bias
Eff adjoint(const Eff& E) {
  Eff A(E.K, E.cout);
  for (int co = 0; co < E.cout; ++co)
    for (int k = 0; k < E.K; ++k)
      for (int t = 0; t < 9; ++t) A.at(k, co, 8 - t) = E.at(co, k, t);
  return A;
}

constexpr int NL = TRUNK_LAYERS;   // layer index: resnet18_hs.h

// ------------------------------------------------------------------------------------------- device-side packing
// The same weight blob from a parameter vector in DEVICE memory, bit for bit (header comment, "Live weights").  One table
// describes all 21 convolutions; a refresh is four launches over it:
//   critic_fold_kernel   per output channel: sc = g / ||v|| in double (the host's summation order) and max |folded weight|
//   critic_scale_kernel  per convolution: the power-of-two weight scale; thresholds and max |fc_w| into the read-back block
//   critic_pack_kernel   per 16-byte destination fragment pair (hi, lo): gathers its eight source elements, or zeros
//   live_copy_kernel     biases and fc (live_params.hip, shared with the actor)
struct FoldDesc {     // one weight-normalised convolution of the parameter vector
  unsigned src_g, src_v;   // floats into the parameter vector
  unsigned chan0;          // its first output channel in the per-channel arrays
  int cout, fan;
  int alpha_src;           // threshold of the TReLU behind it (floats into the parameter vector), -1: none (shortcuts)
};
// PackDesc (one packing, forward or adjoint) and CopyDesc: pack_desc.h
constexpr int NCOPY = NL + 2, NREAD = 2 * NL + 1;   // read-back block: NL weight scales, NL thresholds, max |fc_w|
constexpr int RB_NORM = NREAD;                      // behind it, written by critic_adam_step alone: gradient norm, clip coefficient
struct PackTable {
  FoldDesc fold[NL];
  PackDesc pack[2 * NL];   // 2 * li: forward, 2 * li + 1: adjoint
  CopyDesc copy[NCOPY];
  unsigned nchan, src_fcw;
};
struct CriticLayout {     // PackTable + the blob offsets (floats) the host needs
  PackTable T;
  size_t bias[NL], fcw, fcb, zero, total;
  PackDims dims;          // the launch dimensions of T (stored with the workspace the table is uploaded to)
};

// Offsets of HostBlob as critic_load fills it (256-float alignment before every entry), sources in registration order.
bool make_layout(int num_inputs, CriticLayout& L) {
  std::memset(&L, 0, sizeof(L));
  const int cin_pad = (num_inputs + 7) / 8 * 8;
  BlobCursor cur;
  unsigned chan = 0;
  int ncopy = 0;
  bool ok = true;
  struct Src {
    unsigned b, g, v;
    int cout, cin, ks;
  };
  // the next convolution of the parameter vector = layer li (registration order is the layer numbering)
  auto take_wn = [&](int li, int cout, int cin, int ks) {
    Src c;
    c.b = cur.take(cout);
    c.g = cur.take(cout);
    c.v = cur.take((size_t)cout * cin * ks);
    c.cout = cout;
    c.cin = cin;
    c.ks = ks;
    FoldDesc& F = L.T.fold[li];
    F.src_g = c.g;
    F.src_v = c.v;
    F.chan0 = chan;
    F.cout = cout;
    F.fan = cin * ks;
    F.alpha_src = -1;
    chan += cout;
    return c;
  };
  // its two packings and its bias, the next entries of the blob (critic_load's order: the shortcut before conv2)
  auto finish = [&](int li, const Src& c, int kind, int Cp, int K) {
    const unsigned chan0 = L.T.fold[li].chan0;
    for (int adj = 0; adj < 2; ++adj) {
      PackDesc& P = L.T.pack[2 * li + adj];
      P.src_v = c.v;
      P.chan0 = chan0;
      P.conv = li;
      P.rows = adj ? K : c.cout;
      P.K = adj ? c.cout : K;
      P.mt = (P.rows % 64 == 0) ? 64 : 32;
      pack_desc_window(P, trunk_taps(li, adj != 0));
      P.kind = kind;
      P.cin = c.cin;
      P.Cp = Cp;
      P.adj = adj;
      P.items = (unsigned)((size_t)P.rows * (P.K / 8) * P.nt);
      P.dst = (unsigned)cur.put((size_t)P.rows * P.K * P.nt);
      ok = ok && P.rows % P.mt == 0 && P.K % 16 == 0;
      if (P.items > L.dims.max_items) L.dims.max_items = P.items;
      if (!adj) {
        L.bias[li] = cur.put(c.cout);
        L.T.copy[li] = CopyDesc{c.b, (unsigned)L.bias[li], (unsigned)c.cout};   // copy[li]: the bias of layer li
        ++ncopy;
      }
    }
  };
  finish(0, take_wn(0, 64, num_inputs, 9), 1, cin_pad, 4 * cin_pad);
  int in_planes = 64;
  for (int s = 0; s < 4; ++s) {
    const int p = stage_planes(s), l0 = 1 + 5 * s;
    const Src c1 = take_wn(l0 + 0, p, in_planes, 9), c2 = take_wn(l0 + 1, p, p, 9), cs = take_wn(l0 + 2, p, in_planes, 1);
    const unsigned a0 = cur.take(1), a1 = cur.take(1);
    finish(l0 + 0, c1, 1, in_planes, 4 * in_planes);
    finish(l0 + 2, cs, 2, 0, in_planes);
    finish(l0 + 1, c2, 0, 0, p);
    const Src d1 = take_wn(l0 + 3, p, p, 9), d2 = take_wn(l0 + 4, p, p, 9);
    const unsigned a3 = cur.take(1), a4 = cur.take(1);
    finish(l0 + 3, d1, 0, 0, p);
    finish(l0 + 4, d2, 0, 0, p);
    L.T.fold[l0 + 0].alpha_src = (int)a0;
    L.T.fold[l0 + 1].alpha_src = (int)a1;
    L.T.fold[l0 + 3].alpha_src = (int)a3;
    L.T.fold[l0 + 4].alpha_src = (int)a4;
    in_planes = p;
  }
  L.T.src_fcw = cur.take(512);
  L.fcw = cur.put(512);
  L.T.copy[ncopy++] = CopyDesc{L.T.src_fcw, (unsigned)L.fcw, 512u};   // (ncopy == NL here: behind the 21 biases)
  L.fcb = cur.put(1);
  L.T.copy[ncopy++] = CopyDesc{cur.take(1), (unsigned)L.fcb, 1u};
  L.T.fold[0].alpha_src = (int)cur.take(1);
  L.zero = cur.put(1024);
  L.total = cur.dst + 8192;   // DMA over-read slack
  L.T.nchan = L.dims.nchan = chan;
  L.dims.ncopy = ncopy;
  return ok && ncopy == NCOPY && cur.src == critic_num_params(num_inputs);
}

// device workspace: the table, then sc[nchan] (double), chmax[nchan], the read-back block
struct PackWs {
  PackTable* T;
  double* sc;
  float *chmax, *rb;
};
inline size_t pack_ws_table_bytes() { return (sizeof(PackTable) + 255) & ~(size_t)255; }
inline PackWs pack_ws(const PackWorkspace& W) {
  const unsigned nchan = W.dims.nchan;
  char* p = static_cast<char*>(W.ws.p);
  PackWs w;
  w.T = reinterpret_cast<PackTable*>(p);
  w.sc = reinterpret_cast<double*>(p + pack_ws_table_bytes());
  w.chmax = reinterpret_cast<float*>(w.sc + nchan);
  w.rb = w.chmax + nchan;
  return w;
}

// wn_fold's scale of one output channel.  One thread walks the channel's fan in index order: (double)v * v is exact, so the
// sum has the host's bits whether or not the multiply-add is contracted; sqrt and divide are correctly rounded.  The largest
// folded weight of the channel is the fold of the largest |v| (both roundings are monotonic); NaNs drop out of fmaxf as they
// drop out of the host's std::fmax.
__global__ __launch_bounds__(64) void critic_fold_kernel(const PackTable* __restrict__ T, const float* __restrict__ P,
                                                         double* __restrict__ sc, float* __restrict__ chmax) {
  const unsigned ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= T->nchan) return;
  int li = 0;
  while (li + 1 < NL && T->fold[li + 1].chan0 <= ch) ++li;
  const FoldDesc F = T->fold[li];
  const unsigned co = ch - F.chan0;
  const float* v = P + F.src_v + (size_t)co * F.fan;
  double ss = 0.0;
  float vmax = 0.f;
  for (int i = 0; i < F.fan; ++i) {
    const float x = v[i];
    ss += (double)x * (double)x;
    vmax = fmaxf(vmax, fabsf(x));
  }
  const double s = __ddiv_rn((double)P[F.src_g + co], __dsqrt_rn(ss));
  sc[ch] = s;
  chmax[ch] = fabsf((float)((double)vmax * s));
}

// blocks 0..NL-1: scale 2^(14 - exponent(max |w|)) of a convolution (pack_conv_weights_hs_taps) and its threshold;
// block NL: max |fc_w|
__global__ __launch_bounds__(256) void critic_scale_kernel(const PackTable* __restrict__ T, const float* __restrict__ P,
                                                           const float* __restrict__ chmax, float* __restrict__ rb) {
  __shared__ float part[256];
  const int li = blockIdx.x, tid = threadIdx.x;
  float m = 0.f;
  if (li < NL) {
    for (int c = tid; c < T->fold[li].cout; c += 256) m = fmaxf(m, chmax[T->fold[li].chan0 + c]);
  } else {
    for (int c = tid; c < 512; c += 256) m = fmaxf(m, fabsf(P[T->src_fcw + c]));
  }
  part[tid] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) part[tid] = fmaxf(part[tid], part[tid + st]);
    __syncthreads();
  }
  if (tid != 0) return;
  m = part[0];
  if (li < NL) {
    int e = 0;
    if (m > 0.f) {
      (void)frexpf(m, &e);
      e = 14 - e;
    }
    rb[li] = ldexpf(1.0f, e);
    rb[NL + li] = T->fold[li].alpha_src >= 0 ? P[T->fold[li].alpha_src] : 0.f;
  } else {
    rb[2 * NL] = m;
  }
}

// element (co, k, tap) of the dense effective weights of a launch (put_conv_s1 / put_conv_s2 / put_shortcut), folded
__device__ inline float critic_eff_at(const PackDesc& D, const float* __restrict__ P, const double* __restrict__ sc, int co, int k,
                                      int tap) {
  const long long off = eff_src_offset(D, co, k, tap);
  if (off < 0) return 0.f;
  return (float)((double)P[D.src_v + off] * sc[D.chan0 + co]);
}

// One thread per (cout tile, K chunk, tap, K half, row): the hi and the lo fragment of eight consecutive K elements.
__global__ __launch_bounds__(256) void critic_pack_kernel(const PackTable* __restrict__ T, const float* __restrict__ P,
                                                          const double* __restrict__ sc, const float* __restrict__ rb,
                                                          float* __restrict__ blob) {
  const PackDesc& D = T->pack[blockIdx.y];
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.items) return;
  hs_pack_item(D, i, rb[D.conv], blob, [&](int row, int k, int tap) {
    return D.adj ? critic_eff_at(D, P, sc, k, row, 8 - tap) : critic_eff_at(D, P, sc, row, k, tap);
  });
}

// utils/misc.py:81-85: target * (1.0 - tau) + source * tau on fp32 tensors -- two rounded products, one rounded sum.  A fused
// multiply-add would differ in the last bit of about a quarter of the elements.
__global__ __launch_bounds__(256) void critic_soft_update_kernel(float* __restrict__ master, const float* __restrict__ src, float a,
                                                                 float b, size_t n) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = master[i] * a;
  const float y = src[i] * b;
  master[i] = x + y;
}

// ------------------------------------------------------------------------------------------- activation plan
struct CriticPlan {
  TrunkPlan T;                                // forward (all kept: the backward pass reads them as masks)
  // gradients with respect to pre-activations, scaled (header comment)
  TrunkAct gA[4], gB[4], gM[4];                  // planes x h x w: of o1, of o0, of t1 / t2
  TrunkAct gR[4], gS[4];                         // shortcut adjoint (in_planes x h x w), entry adjoint (4*in_planes x h x w)
  TrunkAct g_stem, g_ob;                         // of the stem output (64, H/2); of the space-to-depth observation
  size_t total = 0;
};
CriticPlan make_plan(int capB, int cin_pad, int H, int W) {
  CriticPlan P;
  TrunkPlan& T = P.T;
  size_t off = 0;
  auto add = [&](TrunkAct& d, int C, int h, int w) {
    d.off = off;
    d.C = C;
    d.H = h;
    d.W = w;
    off += hs_act_floats(C, h, w) * capB;
    off = (off + 63) & ~(size_t)63;
  };
  add(T.ob_s, 4 * cin_pad, H / 2, W / 2);
  add(T.stem_o, 64, H / 2, W / 2);
  add(T.stem_s, 4 * 64, H / 4, W / 4);
  add(P.g_stem, 64, H / 2, W / 2);
  add(P.g_ob, 4 * cin_pad, H / 2, W / 2);
  int in_planes = 64;
  for (int n = 0; n < 4; ++n) {
    const int p = stage_planes(n), h = H >> (n + 2), w = W >> (n + 2);
    add(T.t1[n], p, h, w);
    add(T.sc[n], p, h, w);
    add(T.o0[n], p, h, w);
    add(T.t2[n], p, h, w);
    add(T.o1[n], p, h, w);
    if (n < 3) add(T.o1s[n], 4 * p, h / 2, w / 2);
    add(P.gA[n], p, h, w);
    add(P.gB[n], p, h, w);
    add(P.gM[n], p, h, w);
    add(P.gR[n], in_planes, h, w);
    add(P.gS[n], 4 * in_planes, h, w);
    in_planes = p;
  }
  P.total = off + (1u << 18);   // slack: overhanging tiles read past their tensor
  return P;
}

int check_call(const CriticNet& N, const char* who, int B, int H, int W) {
  if (!N.loaded) {
    set_error("%s called before pnpx_critic_load", who);
    return PNPX_ERR_NO_WEIGHTS;
  }
  if (B <= 0 || H < 32 || W < 32 || (H % 32) || (W % 32)) {
    set_error("%s: need B > 0 and H, W positive multiples of 32 (got %d x %d x %d)", who, B, H, W);
    return PNPX_ERR_SHAPE;
  }
  return PNPX_OK;
}

// the entries that take or fill a whole parameter vector of `n` floats: a critic is loaded, the pointers are there (`have`) and
// n is its parameter count.  expected: "expected <expected>N parameters ..." for a vector taken ("" / "a gradient of "); null for
// one filled.
int check_vector(const CriticNet& N, const char* entry, bool have, size_t n, const char* expected) {
  if (!N.loaded) {
    set_error("%s called before a critic was loaded", entry);
    return PNPX_ERR_NO_WEIGHTS;
  }
  const size_t want = critic_num_params(N.num_inputs);
  if (have && n == want) return PNPX_OK;
  if (expected)
    set_error("%s: expected %s%zu parameters for the loaded critic (%d inputs), got %zu", entry, expected, want, N.num_inputs, n);
  else
    set_error("%s: the loaded critic (%d inputs) has %zu parameters, got room for %zu", entry, N.num_inputs, want, n);
  return PNPX_ERR_ARG;
}

int reserve(CriticNet& N, int B, int H, int W) {
  return reserve_arena_hs(N.arena, N.capB, N.capH, N.capW, B, H, W, [&](int nb) { return make_plan(nb, N.cin_pad, H, W).total; },
                          "critic arena");
}

// one launch of the adjoint chain (or a plain forward instance): layer D, tap mask, epilogue
HsLaunch chain_launch(pnpx_ctx* ctx, const ConvLayerHsDev& D, const float* bias, int taps, int epi, float alpha) {
  HsLaunch L;
  L.D = &D;
  L.bias = bias;
  L.taps = taps;
  L.epi = epi;
  L.alpha = alpha;
  L.range_flag = ctx->opt_range_guard ? ctx->range_flag_dev : nullptr;
  return L;
}
int run_conv(float* A, const HsLaunch& L, const TrunkAct& in, const TrunkAct& out, const TrunkAct* res, const TrunkAct* mask, int B, int h, int w,
             hipStream_t s) {
  return launch_hs_conv(L, reinterpret_cast<const char*>(A + in.off), in.C, reinterpret_cast<char*>(A + out.off), out.C,
                        res ? reinterpret_cast<const char*>(A + res->off) : nullptr, res ? res->C : 0,
                        mask ? reinterpret_cast<const char*>(A + mask->off) : nullptr, mask ? mask->C : 0, B, h, w, s);
}

// forward over B observations; every activation stays in the arena
int run_forward(pnpx_ctx* ctx, const CriticPlan& P, const float* ob, int B, int H, int W, hipStream_t s) {
  CriticNet& N = ctx->critic;
  return trunk_forward(N.fwd, N.bias, P.T, static_cast<float*>(N.arena.p), 0, ob, N.num_inputs, N.cin_pad, B, H, W, 1, 1, N.alpha,
                       ctx->opt_range_guard ? ctx->range_flag_dev : nullptr, s);
}

}  // namespace

size_t critic_num_params(int num_inputs) {
  size_t n = 2 * 64 + (size_t)64 * num_inputs * 9;
  int in_planes = 64;
  for (int s = 0; s < 4; ++s) {
    const size_t p = stage_planes(s);
    n += (2 * p + p * in_planes * 9) + (2 * p + p * p * 9) + (2 * p + p * in_planes) + 2;   // block 0
    n += 2 * (2 * p + p * p * 9) + 2;                                                       // block 1
    in_planes = (int)p;
  }
  return n + 512 + 1 + 1;   // fc.weight, fc.bias, relu_1.alpha
}

void critic_free(pnpx_ctx* ctx) {
  CriticNet& N = ctx->critic;
  if (N.weights.p) (void)hipFree(N.weights.p);
  if (N.arena.p) (void)hipFree(N.arena.p);
  N.live.free();
  N.pack_ws.free();
  if (N.grad_m.p) (void)hipFree(N.grad_m.p);
  if (N.grad_wm.p) (void)hipFree(N.grad_wm.p);
  if (N.grad_slab.p) (void)hipFree(N.grad_slab.p);
  N.optim.free();
  N = CriticNet();
}

namespace {

// the parameter vector on the device, the layer table and the read-back block (at a load that allocates)
int alloc_live_state(CriticNet& N, const CriticLayout& L, size_t n) {
  PNPX_TRY(N.live.alloc(n, "critic parameter"));
  return N.pack_ws.alloc(&L.T, sizeof(PackTable), (size_t)L.dims.nchan * 12, 64, L.dims, "critic packing workspace");
}

// launch descriptors over the blob at `base`
void bind_blob(CriticNet& N, const CriticLayout& L) {
  float* base = static_cast<float*>(N.weights.p);
  for (int i = 0; i < NL; ++i) {
    for (int adj = 0; adj < 2; ++adj) {
      const PackDesc& P = L.T.pack[2 * i + adj];
      ConvLayerHsDev& D = adj ? N.bwd[i] : N.fwd[i];
      D.cin = D.cin_pad = P.K;
      D.cout = P.rows;
      D.mt = P.mt;
      D.w = reinterpret_cast<char*>(base + P.dst);
    }
    N.bias[i] = base + L.bias[i];
  }
  N.fc_w = base + L.fcw;
  N.fc_b = base + L.fcb;
  N.zero = base + L.zero;
}

// master -> weight blob on stream s, then the one read-back: scales, thresholds, max |fc_w|
int repack(pnpx_ctx* ctx, hipStream_t s) {
  CriticNet& N = ctx->critic;
  const PackDims& d = N.pack_ws.dims;
  const PackWs w = pack_ws(N.pack_ws);
  const float* P = N.live.p();
  float* blob = static_cast<float*>(N.weights.p);
  float* const rb_host = N.pack_ws.readback;
  hipLaunchKernelGGL(critic_fold_kernel, dim3((d.nchan + 63) / 64), dim3(64), 0, s, w.T, P, w.sc, w.chmax);
  PNPX_LAUNCH_CHECK();
  hipLaunchKernelGGL(critic_scale_kernel, dim3(NL + 1), dim3(256), 0, s, w.T, P, w.chmax, w.rb);
  PNPX_LAUNCH_CHECK();
  hipLaunchKernelGGL(critic_pack_kernel, dim3((d.max_items + 255) / 256, 2 * NL), dim3(256), 0, s, w.T, P, w.sc, w.rb, blob);
  PNPX_LAUNCH_CHECK();
  PNPX_TRY(launch_live_copy(w.T->copy, dim3(2, NCOPY), P, nullptr, blob, s));
  PNPX_HIP(hipMemcpyAsync(rb_host, w.rb, (NREAD + 1) * sizeof(float), hipMemcpyDeviceToHost, s));   // + the optimiser's norm
  PNPX_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < NL; ++i)
    if (!std::isfinite(rb_host[NL + i])) {
      set_error("critic refresh: TReLU threshold %d is not finite", i);
      PNPX_HIP(hipDeviceSynchronize());
      critic_free(ctx);
      return PNPX_ERR_ARG;
    }
  for (int i = 0; i < NL; ++i) {
    N.fwd[i].inv_scale = N.bwd[i].inv_scale = 1.0f / (rb_host[i] * HS_ASCALE);
    N.alpha[i] = rb_host[NL + i];
  }
  N.fc_wmax = rb_host[2 * NL];
  N.loaded = true;
  return PNPX_OK;
}

}  // namespace

int critic_load_device(pnpx_ctx* ctx, const float* params_dev, size_t n, int num_inputs, hipStream_t s) {
  if (!params_dev || num_inputs < 1 || num_inputs > 64 || n != critic_num_params(num_inputs)) {
    set_error("pnpx_critic_load_device: expected %zu parameters for %d inputs (1..64), got %zu",
              (num_inputs >= 1 && num_inputs <= 64) ? critic_num_params(num_inputs) : (size_t)0, num_inputs, n);
    return PNPX_ERR_ARG;
  }
  CriticNet& N = ctx->critic;
  if (!(N.loaded && N.num_inputs == num_inputs)) {   // first load / another network: allocate (a refresh allocates nothing)
    CriticLayout L;
    if (!make_layout(num_inputs, L)) {
      set_error("pnpx_critic_load_device: internal layout error for %d inputs", num_inputs);
      return PNPX_ERR_SHAPE;
    }
    PNPX_HIP(hipDeviceSynchronize());
    critic_free(ctx);
    N.num_inputs = num_inputs;
    N.cin_pad = (num_inputs + 7) / 8 * 8;
    int st = alloc_dev(N.weights, L.total * sizeof(float), "critic weight");
    if (st == PNPX_OK) st = alloc_live_state(N, L, n);
    if (st == PNPX_OK && hipMemset(N.weights.p, 0, N.weights.bytes) != hipSuccess) st = PNPX_ERR_HIP;   // padding and the zero block
    if (st == PNPX_OK && hipDeviceSynchronize() != hipSuccess) st = PNPX_ERR_HIP;
    if (st != PNPX_OK) {
      if (st == PNPX_ERR_HIP) set_error("pnpx_critic_load_device: clearing the weight blob failed: %s", hipGetErrorString(hipGetLastError()));
      critic_free(ctx);
      return st;
    }
    bind_blob(N, L);
  }
  PNPX_TRY(N.live.set_device(params_dev, s));
  return repack(ctx, s);
}

int critic_soft_update(pnpx_ctx* ctx, const float* src_dev, size_t n, float one_minus_tau, float tau, hipStream_t s) {
  CriticNet& N = ctx->critic;
  PNPX_TRY(check_vector(N, "pnpx_critic_soft_update", src_dev != nullptr, n, ""));
  hipLaunchKernelGGL(critic_soft_update_kernel, g1(n), dim3(256), 0, s, N.live.p(), src_dev, one_minus_tau, tau, n);
  PNPX_LAUNCH_CHECK();
  return repack(ctx, s);
}

int critic_params(pnpx_ctx* ctx, float* dst_dev, size_t n, hipStream_t s) {
  CriticNet& N = ctx->critic;
  PNPX_TRY(check_vector(N, "pnpx_critic_params", dst_dev != nullptr, n, nullptr));
  return N.live.copy_out(dst_dev, s);
}

int critic_load(pnpx_ctx* ctx, const float* params, size_t n, int num_inputs) {
  if (!params || num_inputs < 1 || num_inputs > 64 || n != critic_num_params(num_inputs)) {
    set_error("pnpx_critic_load: expected %zu parameters for %d inputs (1..64), got %zu",
              (num_inputs >= 1 && num_inputs <= 64) ? critic_num_params(num_inputs) : (size_t)0, num_inputs, n);
    return PNPX_ERR_ARG;
  }
  PNPX_HIP(hipDeviceSynchronize());
  critic_free(ctx);
  CriticNet& N = ctx->critic;
  N.num_inputs = num_inputs;
  N.cin_pad = (num_inputs + 7) / 8 * 8;
  Reader R{params};
  auto take_wn = [&](int cout, size_t fan) {
    WnConv c;
    c.b = R.take(cout);
    c.g = R.take(cout);
    c.v = R.take((size_t)cout * fan);
    return c;
  };
  HostBlob H;
  Packed pf[NL], pb[NL];
  float alpha[NL] = {};
  auto finish = [&](int li, const Eff& E) {
    pf[li] = pack_layer(H, E, trunk_taps(li, false), true);
    pb[li] = pack_layer(H, adjoint(E), trunk_taps(li, true), false);
  };
  auto conv_s1 = [&](int li, const WnConv& c, int p) {
    Eff E(p, p);
    put_conv_s1(E, 0, wn_fold(c, p, (size_t)p * 9).data(), c.b, p, p);
    finish(li, E);
  };
  {
    const WnConv c = take_wn(64, (size_t)num_inputs * 9);
    Eff E(64, 4 * N.cin_pad);
    put_conv_s2(E, 0, wn_fold(c, 64, (size_t)num_inputs * 9).data(), c.b, 64, num_inputs, N.cin_pad);
    finish(0, E);
  }
  int in_planes = 64;
  for (int s = 0; s < 4; ++s) {
    const int p = stage_planes(s), l0 = 1 + 5 * s;
    // block 0: conv1 (stride 2), conv2, shortcut.0, relu_1.alpha, relu_2.alpha -- registration order
    const WnConv c1 = take_wn(p, (size_t)in_planes * 9);
    const WnConv c2 = take_wn(p, (size_t)p * 9);
    const WnConv cs = take_wn(p, (size_t)in_planes);
    alpha[l0 + 0] = *R.take(1);
    alpha[l0 + 1] = *R.take(1);
    {
      Eff E(p, 4 * in_planes);
      put_conv_s2(E, 0, wn_fold(c1, p, (size_t)in_planes * 9).data(), c1.b, p, in_planes, in_planes);
      finish(l0 + 0, E);
    }
    {   // (the blob keeps the shortcut in front of conv2)
      Eff E(p, in_planes);
      put_shortcut(E, 0, wn_fold(cs, p, (size_t)in_planes).data(), cs.b, p, in_planes);
      finish(l0 + 2, E);
    }
    conv_s1(l0 + 1, c2, p);
    // block 1: conv1, conv2, relu_1.alpha, relu_2.alpha
    const WnConv d1 = take_wn(p, (size_t)p * 9);
    const WnConv d2 = take_wn(p, (size_t)p * 9);
    alpha[l0 + 3] = *R.take(1);
    alpha[l0 + 4] = *R.take(1);
    conv_s1(l0 + 3, d1, p);
    conv_s1(l0 + 4, d2, p);
    in_planes = p;
  }
  const float* fcw = R.take(512);
  const size_t o_fcw = H.add(fcw, 512);
  const size_t o_fcb = H.add(R.take(1), 1);
  alpha[0] = *R.take(1);
  float wmax = 0.f;
  for (int i = 0; i < 512; ++i) wmax = std::fmax(wmax, std::fabs(fcw[i]));
  for (int i = 0; i < NL; ++i)
    if (!std::isfinite(alpha[i])) {
      set_error("pnpx_critic_load: TReLU threshold %d is not finite", i);
      critic_free(ctx);
      return PNPX_ERR_ARG;
    }
  H.align();
  const size_t o_zero = H.f.size();
  H.f.resize(H.f.size() + 1024, 0.f);
  H.f.resize(H.f.size() + 8192, 0.f);   // DMA over-read slack
  PNPX_TRY(alloc_dev(N.weights, H.f.size() * sizeof(float), "critic weight"));
  PNPX_HIP(hipMemcpy(N.weights.p, H.f.data(), N.weights.bytes, hipMemcpyHostToDevice));
  const float* base = static_cast<const float*>(N.weights.p);
  for (int i = 0; i < NL; ++i) {
    bind_packed(N.fwd[i], pf[i], base);
    bind_packed(N.bwd[i], pb[i], base);
    N.bias[i] = base + pf[i].b;
    N.alpha[i] = alpha[i];
  }
  N.fc_w = base + o_fcw;
  N.fc_b = base + o_fcb;
  N.zero = base + o_zero;
  N.fc_wmax = wmax;
  // live weights: the raw parameters stay on the device as the vector pnpx_critic_soft_update moves, whose device-side
  // packing writes into this blob -- so its layer table has to describe exactly the offsets used above
  CriticLayout L;
  bool same = make_layout(num_inputs, L) && L.total == H.f.size() && L.fcw == o_fcw && L.fcb == o_fcb && L.zero == o_zero;
  for (int i = 0; same && i < NL; ++i)
    same = L.T.pack[2 * i].dst == pf[i].w && L.T.pack[2 * i + 1].dst == pb[i].w && L.bias[i] == pf[i].b && L.T.pack[2 * i].mt == pf[i].mt &&
           L.T.pack[2 * i + 1].mt == pb[i].mt && L.T.pack[2 * i].K == pf[i].cin && L.T.pack[2 * i + 1].K == pb[i].cin;
  if (!same) {
    set_error("pnpx_critic_load: the device packing table disagrees with the host layout (%d inputs)", num_inputs);
    critic_free(ctx);
    return PNPX_ERR_SHAPE;
  }
  int st = alloc_live_state(N, L, n);
  if (st == PNPX_OK) st = N.live.set_host(params);
  if (st != PNPX_OK) {
    critic_free(ctx);
    return st;
  }
  N.loaded = true;
  return PNPX_OK;
}

int critic_forward(pnpx_ctx* ctx, const float* ob, float* value, int B, int H, int W, hipStream_t s) {
  CriticNet& N = ctx->critic;
  PNPX_TRY(check_call(N, "critic forward", B, H, W));
  PNPX_TRY(reserve(N, B, H, W));
  const CriticPlan P = make_plan(N.capB, N.cin_pad, H, W);
  PNPX_TRY(run_forward(ctx, P, ob, B, H, W, s));
  const float* A = static_cast<const float*>(N.arena.p);
  hipLaunchKernelGGL(critic_pool_fc_kernel, dim3(B), dim3(256), 0, s, reinterpret_cast<const HsRec*>(A + P.T.o1[3].off), H / 32, W / 32,
                     N.fc_w, N.fc_b, value);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

namespace {

// Parameter-gradient work interleaved with the adjoint chain (critic_param_grad); the input gradient runs the chain without one.
// gM[st] is written twice per stage, so each gradient is launched while both of its operands are still in place.
struct GradJob {
  const CriticLayout* L;
  const float* gv;     // grad_value [B]
  float* out;          // grad_params
  HsRec *m, *wm;       // clip indicator of one activation; the forward convolution of it
  float* slab;         // K-split pieces of one layer
  double* dots;        // [NL][B]: per threshold and image, <g, W m> + <res, m> as stored (times s * 256)
};

inline float grad_scale(const CriticNet& N, int hl, int wl) {
  // a power of two that brings the head's largest entry max|fc_w| / (h w) into [1, 2)
  float gs = 1.f;
  if (N.fc_wmax > 0.f) {
    int e = 0;
    std::frexp(N.fc_wmax / (float)(hl * wl), &e);
    gs = std::ldexp(1.0f, 1 - e);
  }
  return gs;
}

// head gradient and the four stages of the adjoint chain, down to g_stem (the forward has just run: every activation is in the arena)
int run_chain(pnpx_ctx* ctx, const CriticPlan& P, float gs, int B, int H, int W, hipStream_t s, const GradJob* J) {
  CriticNet& N = ctx->critic;
  float* A = static_cast<float*>(N.arena.p);
  auto rec = [&](const TrunkAct& d) { return reinterpret_cast<HsRec*>(A + d.off); };
  auto u4 = [&](const TrunkAct& d) { return reinterpret_cast<uint4*>(A + d.off); };
  // (W^T g [+ res]) masked by the saved activation `mask` against the threshold of layer `mask_li`
  auto grad = [&](int li, const TrunkAct& in, const TrunkAct& out, const TrunkAct* res, const TrunkAct* mask, int mask_li, int h, int w) -> int {
    return run_conv(A, chain_launch(ctx, N.bwd[li], N.zero, trunk_taps(li, true), 2, mask ? N.alpha[mask_li] : 0.f), in, out, res, mask, B, h,
                    w, s);
  };
  // gradient of convolution li: G = gradient with respect to its output, X = the tensor its forward launch read
  auto wgrad = [&](int li, const TrunkAct& G, const TrunkAct& X, int h, int w) -> int {
    if (!J) return PNPX_OK;
    const PackDesc& D = J->L->T.pack[2 * li];
    WgradJob Wj;
    Wj.G = rec(G);
    Wj.X = rec(X);
    Wj.gv = J->gv;
    Wj.Gg = G.C / 8;
    Wj.Xg = X.C / 8;
    Wj.cout = D.rows;
    Wj.K = D.K;
    Wj.nt = D.nt;
    for (int t = 0; t < D.nt; ++t) Wj.tap[t] = D.tap[t];
    Wj.B = B;
    Wj.h = h;
    Wj.w = w;
    PNPX_TRY(launch_critic_wgrad(Wj, J->slab, s));
    WnGradJob F;
    F.D = D;
    F.src_b = J->L->T.copy[li].src;
    F.src_g = J->L->T.fold[li].src_g;
    F.fan = J->L->T.fold[li].fan;
    F.pieces = critic_wgrad_pieces(D.rows, D.K, B, h, w);
    F.inv_w = 1.0f / (gs * HS_ASCALE * HS_ASCALE);
    F.inv_b = 1.0f / (gs * HS_ASCALE);
    return launch_critic_wn_grad(F, J->slab, N.live.p(), J->out, s);
  };
  // threshold ali of the saved activation `act`, read by forward convolution cli whose output gradient is g; res: what the chain
  // adds to W^T g before the mask
  auto athr = [&](int ali, int cli, const TrunkAct& act, const TrunkAct& g, const TrunkAct* res, int h, int w) -> int {
    if (!J) return PNPX_OK;
    PNPX_TRY(launch_critic_clip_mask(rec(act), J->m, hs_roundtrip16(N.alpha[ali]), B, act.C / 8, h, w, s));
    // the plain linear instance, no bias (the two tensors live outside the arena)
    PNPX_TRY(launch_hs_conv(chain_launch(ctx, N.fwd[cli], N.zero, trunk_taps(cli, false), 0, 0.f), reinterpret_cast<const char*>(J->m), act.C,
                            reinterpret_cast<char*>(J->wm), g.C, nullptr, 0, nullptr, 0, B, h, w, s));
    return launch_critic_alpha_dot(rec(g), J->wm, g.C / 8, res ? rec(*res) : nullptr, res ? res->C / 8 : 0, J->m, act.C / 8, B, h, w,
                                   J->dots + (size_t)ali * B, s);
  };
  const int hl = H / 32, wl = W / 32;
  {
    const size_t n = (size_t)B * 64 * hl * wl;
    hipLaunchKernelGGL(critic_head_grad_kernel, g1(n), dim3(256), 0, s, rec(P.T.o1[3]), rec(P.gA[3]), N.fc_w, hs_roundtrip16(N.alpha[20]),
                       gs * HS_ASCALE / (float)(hl * wl), hl, wl, n);
    PNPX_LAUNCH_CHECK();
  }
  for (int st = 3; st >= 0; --st) {
    const int h = H >> (st + 2), w = W >> (st + 2), l0 = 1 + 5 * st;
    // block 1: o1 = TReLU(conv2(t2) + o0), t2 = TReLU(conv1(o0))
    PNPX_TRY(wgrad(l0 + 4, P.gA[st], P.T.t2[st], h, w));
    PNPX_TRY(athr(l0 + 3, l0 + 4, P.T.t2[st], P.gA[st], nullptr, h, w));
    PNPX_TRY(grad(l0 + 4, P.gA[st], P.gM[st], nullptr, &P.T.t2[st], l0 + 3, h, w));
    PNPX_TRY(wgrad(l0 + 3, P.gM[st], P.T.o0[st], h, w));
    PNPX_TRY(athr(l0 + 1, l0 + 3, P.T.o0[st], P.gM[st], &P.gA[st], h, w));
    PNPX_TRY(grad(l0 + 3, P.gM[st], P.gB[st], &P.gA[st], &P.T.o0[st], l0 + 1, h, w));
    // block 0: o0 = TReLU(conv2(t1) + shortcut(x)), t1 = TReLU(conv1(x)), x = space-to-depth input
    const TrunkAct& x = st == 0 ? P.T.stem_s : P.T.o1s[st - 1];
    PNPX_TRY(wgrad(l0 + 1, P.gB[st], P.T.t1[st], h, w));
    PNPX_TRY(wgrad(l0 + 2, P.gB[st], x, h, w));
    PNPX_TRY(athr(l0 + 0, l0 + 1, P.T.t1[st], P.gB[st], nullptr, h, w));
    PNPX_TRY(grad(l0 + 1, P.gB[st], P.gM[st], nullptr, &P.T.t1[st], l0 + 0, h, w));
    // shortcut adjoint: 1x1, linear (the existing sparse-tap instance), to the phase-(0,0) channel groups
    PNPX_TRY(run_conv(A, chain_launch(ctx, N.bwd[l0 + 2], N.zero, trunk_taps(l0 + 2, true), 0, 0.f), P.gB[st], P.gR[st], nullptr, nullptr, B, h,
                      w, s));
    PNPX_TRY(wgrad(l0 + 0, P.gM[st], x, h, w));
    PNPX_TRY(athr(st == 0 ? 0 : l0 - 1, l0 + 0, x, P.gM[st], &P.gR[st], h, w));
    PNPX_TRY(grad(l0 + 0, P.gM[st], P.gS[st], &P.gR[st], &x, st == 0 ? 0 : l0 - 1, h, w));
    const TrunkAct& below = st == 0 ? P.g_stem : P.gA[st - 1];
    const int G = below.C / 8;
    const size_t n = (size_t)B * G * (2 * h) * (2 * w) * 2;
    hipLaunchKernelGGL(hs_d2s_kernel, g1(n), dim3(256), 0, s, u4(P.gS[st]), u4(below), G, h, w, n);
    PNPX_LAUNCH_CHECK();
  }
  PNPX_TRY(wgrad(0, P.g_stem, P.T.ob_s, H / 2, W / 2));
  return PNPX_OK;
}

}  // namespace

int critic_backward(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_ob, int B, int H, int W, hipStream_t s) {
  CriticNet& N = ctx->critic;
  PNPX_TRY(check_call(N, "critic backward", B, H, W));
  PNPX_TRY(reserve(N, B, H, W));
  const CriticPlan P = make_plan(N.capB, N.cin_pad, H, W);
  PNPX_TRY(run_forward(ctx, P, ob, B, H, W, s));   // re-computation: every activation is now in the arena
  float* A = static_cast<float*>(N.arena.p);
  auto rec = [&](const TrunkAct& d) { return reinterpret_cast<HsRec*>(A + d.off); };
  const float gs = grad_scale(N, H / 32, W / 32);
  PNPX_TRY(run_chain(ctx, P, gs, B, H, W, s, nullptr));
  // stem adjoint: linear
  PNPX_TRY(run_conv(A, chain_launch(ctx, N.bwd[0], N.zero, trunk_taps(0, true), 2, 0.f), P.g_stem, P.g_ob, nullptr, nullptr, B, H / 2, W / 2, s));
  const size_t n = (size_t)B * N.num_inputs * H * W;
  hipLaunchKernelGGL(critic_ob_grad_kernel, g1(n), dim3(256), 0, s, rec(P.g_ob), grad_value, grad_ob, N.num_inputs, N.cin_pad, H, W,
                     1.0f / (gs * HS_ASCALE), n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

namespace {

// a buffer of the parameter-gradient workspace: grows to the largest size seen (the only place the call synchronises the device)
int grow(DeviceBuf& b, size_t bytes, bool zero, const char* what) {
  if (bytes <= b.bytes) return PNPX_OK;
  PNPX_HIP(hipDeviceSynchronize());
  if (b.p) PNPX_HIP(hipFree(b.p));
  b = DeviceBuf();
  PNPX_TRY(alloc_dev(b, bytes, what));
  if (zero) {   // record buffers: what an overhanging tile reads past its tensor has to be finite
    PNPX_HIP(hipMemset(b.p, 0, bytes));
    PNPX_HIP(hipDeviceSynchronize());
  }
  return PNPX_OK;
}

}  // namespace

// d(sum_b grad_value[b] * V_b) / d(params), pnpx_critic_load's order (value_loss.backward(), trainer/mddpg/trainer.py:198,207).
// Forward re-computation, then the adjoint chain of critic_backward with the gradient launches between its steps (run_chain);
// fc and the head's threshold are closed forms of the last activation.  Every element of grad_params is written.
//
// q_target != NULL (critic_value_loss_grad): grad_value is not an argument but d mean((V - q_target)^2) / d V, taken from the
// forward this call runs anyway -- the head writes `value` as critic_forward does, critic_mse_kernel turns it into grad_value
// (context-owned scratch behind the reduction blocks) and `loss`.
namespace {

int param_grad_run(pnpx_ctx* ctx, const char* entry, const char* who, const float* ob, const float* grad_value, const float* q_target,
                   float* value, float* loss, float* grad_params, size_t n, int B, int H, int W, hipStream_t s) {
  CriticNet& N = ctx->critic;
  PNPX_TRY(check_call(N, who, B, H, W));
  PNPX_TRY(check_vector(N, entry, true, n, nullptr));
  CriticLayout L;
  if (!make_layout(N.num_inputs, L)) {
    set_error("%s: internal layout error for %d inputs", entry, N.num_inputs);
    return PNPX_ERR_SHAPE;
  }
  PNPX_TRY(reserve(N, B, H, W));
  const CriticPlan P = make_plan(N.capB, N.cin_pad, H, W);
  // workspace: the largest clip indicator (the space-to-depth input of stage 0), the largest W * indicator, the largest layer's slabs
  size_t m_floats = 0, wm_floats = 0, slab_floats = 0;
  auto hs_floats = [&](int C, int h, int w) { return (size_t)C * (h + 2) * (w + 2) * B; };
  auto slab_of = [&](int li, int h, int w) {
    const PackDesc& D = L.T.pack[2 * li];
    const size_t f = (size_t)critic_wgrad_pieces(D.rows, D.K, B, h, w) * critic_wgrad_piece_floats(D.rows, D.K, D.nt);
    if (f > slab_floats) slab_floats = f;
  };
  slab_of(0, H / 2, W / 2);
  int in_planes = 64;
  for (int st = 0; st < 4; ++st) {
    const int p = stage_planes(st), h = H >> (st + 2), w = W >> (st + 2);
    m_floats = std::max(m_floats, std::max(hs_floats(4 * in_planes, h, w), hs_floats(p, h, w)));
    wm_floats = std::max(wm_floats, hs_floats(p, h, w));
    for (int k = 0; k < 5; ++k) slab_of(1 + 5 * st + k, h, w);
    in_planes = p;
  }
  const size_t slack = (size_t)1 << 20;   // bytes: overhanging tiles read past their tensor (the arena's slack)
  PNPX_TRY(grow(N.grad_m, m_floats * sizeof(float) + slack, true, "critic gradient mask"));
  PNPX_TRY(grow(N.grad_wm, wm_floats * sizeof(float) + slack, true, "critic gradient mask convolution"));
  const size_t slab_bytes = (slab_floats * sizeof(float) + 255) & ~(size_t)255;
  const size_t red_bytes = ((size_t)NL * B + 512) * sizeof(double);   // the reduction blocks; behind them grad_value of the loss entry
  PNPX_TRY(grow(N.grad_slab, slab_bytes + red_bytes + (size_t)B * sizeof(float), false, "critic gradient slab"));

  PNPX_TRY(run_forward(ctx, P, ob, B, H, W, s));   // re-computation: every activation is now in the arena
  const int hl = H / 32, wl = W / 32;
  const float* A = static_cast<const float*>(N.arena.p);
  if (q_target) {
    float* gv = reinterpret_cast<float*>(static_cast<char*>(N.grad_slab.p) + slab_bytes + red_bytes);
    hipLaunchKernelGGL(critic_pool_fc_kernel, dim3(B), dim3(256), 0, s, reinterpret_cast<const HsRec*>(A + P.T.o1[3].off), hl, wl, N.fc_w,
                       N.fc_b, value);
    PNPX_LAUNCH_CHECK();
    hipLaunchKernelGGL(critic_mse_kernel, dim3(1), dim3(256), 0, s, value, q_target, gv, loss, B, (float)(1.0 / (double)B));
    PNPX_LAUNCH_CHECK();
    grad_value = gv;
  }
  GradJob J;
  J.L = &L;
  J.gv = grad_value;
  J.out = grad_params;
  J.m = static_cast<HsRec*>(N.grad_m.p);
  J.wm = static_cast<HsRec*>(N.grad_wm.p);
  J.slab = static_cast<float*>(N.grad_slab.p);
  J.dots = reinterpret_cast<double*>(static_cast<char*>(N.grad_slab.p) + slab_bytes);
  double* a20 = J.dots + (size_t)NL * B;
  const float gs = grad_scale(N, hl, wl);
  PNPX_TRY(run_chain(ctx, P, gs, B, H, W, s, &J));
  PNPX_TRY(launch_critic_fc_grad(reinterpret_cast<const HsRec*>(A + P.T.o1[3].off), grad_value, N.fc_w, hs_roundtrip16(N.alpha[20]), B, hl, wl,
                                 grad_params + L.T.src_fcw, a20, s));
  AlphaFinishJob F;
  for (int i = 0; i < NL; ++i) F.alpha_src[i] = i == NL - 1 ? -1 : L.T.fold[i].alpha_src;   // the head's threshold: closed form
  F.head_src = L.T.fold[NL - 1].alpha_src;
  F.fcb_src = (int)L.T.copy[NCOPY - 1].src;
  F.B = B;
  F.inv = 1.0f / (gs * HS_ASCALE * HS_ASCALE);
  return launch_critic_alpha_finish(F, J.dots, a20, grad_value, grad_params, s);
}

}  // namespace

int critic_param_grad(pnpx_ctx* ctx, const float* ob, const float* grad_value, float* grad_params, size_t n, int B, int H, int W,
                      hipStream_t s) {
  return param_grad_run(ctx, "pnpx_critic_param_grad", "critic parameter gradient", ob, grad_value, nullptr, nullptr, nullptr, grad_params,
                        n, B, H, W, s);
}

int critic_value_loss_grad(pnpx_ctx* ctx, const float* ob, const float* q_target, float* value, float* loss, float* grad_params, size_t n,
                           int B, int H, int W, hipStream_t s) {
  return param_grad_run(ctx, "pnpx_critic_value_loss_grad", "critic value loss gradient", ob, nullptr, q_target, value, loss, grad_params, n,
                        B, H, W, s);
}

// ------------------------------------------------------------------------------------------- optimiser
// clip_grad_norm_(max_norm) + Adam.step() (trainer/mddpg/trainer.py:208-209) on the live vector, then repack: sum of squares, finish
// (norm and clip coefficient into the read-back block's spare floats), the fused update (LiveOptim, live_optim.hip), the refresh.  The
// update reads the coefficient on the device and does nothing when the norm is not finite; the host learns the norm from the
// refresh's own read-back and only then advances the step counter.
int critic_adam_step(pnpx_ctx* ctx, const float* grad_dev, size_t n, float lr, float beta1, float beta2, float eps, float max_norm,
                     float* grad_norm_dev, hipStream_t s) {
  CriticNet& N = ctx->critic;
  PNPX_TRY(check_vector(N, "pnpx_critic_adam_step", grad_dev != nullptr, n, "a gradient of "));
  if (!(lr >= 0.f) || !std::isfinite(lr) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) ||
      !std::isfinite(eps) || !(max_norm > 0.f)) {
    set_error("pnpx_critic_adam_step: need lr >= 0 and finite, betas in [0, 1), eps > 0 and finite, max_norm > 0 (got lr %g, betas %g %g, "
              "eps %g, max_norm %g)", (double)lr, (double)beta1, (double)beta2, (double)eps, (double)max_norm);
    return PNPX_ERR_ARG;
  }
  float* slot = pack_ws(N.pack_ws).rb + RB_NORM;
  PNPX_TRY(N.optim.launch_step(N.live, grad_dev, lr, beta1, beta2, eps, max_norm, slot, grad_norm_dev, "critic optimiser state", s));
  PNPX_TRY(repack(ctx, s));   // (a threshold stepped to a non-finite value: the critic is gone, as after any such refresh)
  const float norm = N.pack_ws.readback[RB_NORM];
  if (!std::isfinite(norm)) {
    set_error("pnpx_critic_adam_step: the gradient norm is not finite (%g); parameters and optimiser state are unchanged", (double)norm);
    return PNPX_ERR_ARG;
  }
  N.optim.commit();
  return PNPX_OK;
}

int critic_optim_state(pnpx_ctx* ctx, float* exp_avg_dst, float* exp_avg_sq_dst, size_t n, long long* step_host, hipStream_t s) {
  CriticNet& N = ctx->critic;
  PNPX_TRY(check_vector(N, "pnpx_critic_optim_state", exp_avg_dst && exp_avg_sq_dst, n, nullptr));
  return N.optim.copy_state(n, exp_avg_dst, exp_avg_sq_dst, step_host, s);
}

// back to "before the first step": the next step allocates zero-filled moments and counts as step 1
int critic_optim_reset(pnpx_ctx* ctx) {
  return ctx->critic.optim.reset();
}

}  // namespace pnpx
