// Parameter gradients of the value network (value_loss.backward(), tfpnp/trainer/mddpg/trainer.py:198,207): the kernels.
// The driver (critic.hip::critic_param_grad) re-computes the forward into the arena and walks the adjoint chain of
// critic_backward; every tensor of that chain is the gradient with respect to a pre-activation, so the gradient of a
// convolution's effective weights is the correlation of two HS8 tensors that already exist:
//     dW_eff[co][tap][k] = sum_{b,y,x} grad_value[b] * G[b,co,y,x] * X[b,k,y+dy,x+dx]          (dy, dx: the tap's offset)
// One kernel serves every window (0x1FF stride-1 layers, 0x01B stem / stage entries on the space-to-depth grid, 0x010
// shortcuts over the phase-(0,0) groups): a GEMM with M = cout, N = K * taps, K-axis = B * h * w pixels on
// v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain, so no three-product split is needed).
//
// Workgroup = 4 waves, tile = 32 couts x 32 input channels x every tap of the window; the taps are dealt to the waves
// (tap index = wave + 4 j).  Per chunk of 32 pixels the workgroup rebuilds fp32 operands from the records (hi + lo, the
// gradient times grad_value[b]) into LDS as [pixel][channel]; an MFMA k-step is two pixels.  The arena's zero border is the
// padding: shifted reads go straight to memory and never branch on the position.  The power-of-two scales of the records
// (16 for activations, s * 16 for gradients) are undone once, by the finishing kernel.
//
// K-split: where the tiles alone cannot fill the chip, the pixel axis is cut into pieces (critic_wgrad_pieces: a function of
// the layer and (B, h, w) only); each piece writes its partial tile block to a slab and the finishing kernel adds the pieces
// in piece order in double -- no floating-point atomics, no arrival protocol, the same bits on every call.  The bias gradient
// (the same sum without X) rides along: the 32 threads that own a cout column add the gradient tile in pixel order.
//
// Finishing kernel (one workgroup per output channel): each raw weight element has exactly one effective position
// (eff_pos_of_src, the inverse of the map the device packing uses), so un-packing is a gather; then weight-norm, with
// n = ||v||:  dg = <dW, v> / n,  dv = (g / n) * (dW - (<dW, v> / n^2) * v), dot products in double in a fixed order.
//
// Thresholds: TReLU(t) = max(t, alpha) has d/d alpha = sum g_out * [t <= alpha], and the chain keeps only the masked
// g_out * [t > alpha].  With m the clip indicator of the activation and g_out = W^T g + res:
//     sum m * (W^T g + res) = <g, W m> + <res, m>
// -- one launch of the existing linear convolution instance on m (driver) and the dot-product kernel here, per threshold;
// never "everything minus the masked part", which cancels where few positions clip.
#include "critic_grad.h"

#include "conv_hs.h"
#include "grad_common.h"

namespace pnpx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_KC = 32;   // pixels per chunk
constexpr int WG_LD = 36;   // LDS row stride in floats (16-byte aligned rows, rows two apart on different banks)

struct WgradArgs {
  const HsRec* G;
  const HsRec* X;
  const float* gv;
  float* slab;
  int Gg, Xg, cout, K, nt, B, h, w;
  int tilesM, cpp, nchunks;   // cout tiles; chunks per piece; chunks in all
  size_t stride;              // floats per piece
  int tap[9];
};

__global__ __launch_bounds__(256) void critic_wgrad_kernel(const WgradArgs a) {
  __shared__ float sG[WG_KC * WG_LD];
  __shared__ float sX[9 * WG_KC * WG_LD];
  __shared__ int sTap[12];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tm = blockIdx.x % a.tilesM, tn = blockIdx.x / a.tilesM;
  const int m0 = tm * 32, n0 = tn * 32;
  const int c0 = blockIdx.y * a.cpp, c1 = min(c0 + a.cpp, a.nchunks);
  if (tid < 9) sTap[tid] = a.tap[tid];
  __syncthreads();
  // loader role: pixel p of the chunk, channel group g of the tile, operands t0, t0 + 2, ... (operand nt = the gradient tile)
  const int p = tid & 31, g = (tid >> 5) & 3, t0 = tid >> 7;
  const int hw = a.h * a.w, ktot = a.B * hw;
  const size_t Hp = a.h + 2, Wp = a.w + 2;
  f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float bacc = 0.f;
  for (int c = c0; c < c1; ++c) {
    const int kp = c * WG_KC + p;
    const bool live = kp < ktot;
    int b = 0, y = 0, x = 0;
    if (live) {
      b = kp / hw;
      const int r = kp - b * hw;
      y = r / a.w;
      x = r - y * a.w;
    }
    for (int t = t0; t <= a.nt; t += 2) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (live) {
        if (t == a.nt) {
          const HsRec r = a.G[(((size_t)b * a.Gg + (m0 >> 3) + g) * Hp + (y + 1)) * Wp + (x + 1)];
          const float gvb = a.gv[b];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = ((float)r.hi[e] + (float)r.lo[e]) * gvb;
        } else {
          const int tap = sTap[t], ty = tap / 3, tx = tap - 3 * ty;   // the tap reads (y + ty - 1, x + tx - 1): padded row y + ty
          const HsRec r = a.X[(((size_t)b * a.Xg + (n0 >> 3) + g) * Hp + (y + ty)) * Wp + (x + tx)];
          hs_unpack(r, v);
        }
      }
      float* d = (t == a.nt ? sG : sX + t * (WG_KC * WG_LD)) + p * WG_LD + g * 8;
      *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    if (tn == 0 && tid < 32) {
      for (int k = 0; k < WG_KC; ++k) bacc += sG[k * WG_LD + tid];
    }
    for (int kk = 0; kk < WG_KC / 2; ++kk) {
      const int k = 2 * kk + (lane >> 5);
      const float av = sG[k * WG_LD + (lane & 31)];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int ti = wave + 4 * j;
        if (ti < a.nt) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, sX[(ti * WG_KC + k) * WG_LD + (lane & 31)], acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // C layout: column (input channel) = lane & 31, row (cout) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  float* out = a.slab + (size_t)blockIdx.y * a.stride;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int ti = wave + 4 * j;
    if (ti >= a.nt) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      out[((size_t)(m0 + row) * a.nt + ti) * a.K + n0 + (lane & 31)] = acc[j][r];
    }
  }
  if (tn == 0 && tid < 32) out[(size_t)a.cout * a.nt * a.K + m0 + tid] = bacc;
}

// sum of v over the 256 threads in a fixed tree order; every thread returns the total
__device__ inline double block_sum256(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) sh[tid] += sh[tid + st];
    __syncthreads();
  }
  return sh[0];
}

struct WnGradArgs {
  PackDesc D;
  unsigned src_b, src_g;
  int fan, pieces;
  size_t stride;
  float inv_w, inv_b;
};

__global__ __launch_bounds__(256) void critic_wn_grad_kernel(const WnGradArgs a, const float* __restrict__ slab,
                                                             const float* __restrict__ P, float* __restrict__ grad) {
  __shared__ double sh[256];
  __shared__ int sTi[9];   // tap -> its index in the packing's window (-1: absent)
  const int tid = threadIdx.x, co = blockIdx.x;
  wgrad_tap_index(a.D, sTi);
  __syncthreads();
  const float* v = P + a.D.src_v + (size_t)co * a.fan;
  float* gout = grad + a.D.src_v + (size_t)co * a.fan;
  const int nt = a.D.nt, K = a.D.K;
  double dot = 0.0, nn = 0.0;
  for (int i = tid; i < a.fan; i += 256) {
    const double sum = wgrad_gather(a.D, sTi, slab, a.stride, a.pieces, co, i);
    const float dw = (float)(sum * (double)a.inv_w);
    gout[i] = dw;   // parked: replaced by dv below (same thread)
    const double vi = (double)v[i];
    dot += (double)dw * vi;
    nn += vi * vi;
  }
  dot = block_sum256(dot, sh);
  nn = block_sum256(nn, sh);
  const double n = sqrt(nn), c1 = (double)P[a.src_g + co] / n, c2 = dot / nn;
  for (int i = tid; i < a.fan; i += 256) gout[i] = (float)(c1 * ((double)gout[i] - c2 * (double)v[i]));
  if (tid == 0) {
    grad[a.src_g + co] = (float)(dot / n);
    const float* bs = slab + (size_t)a.D.rows * nt * K + co;
    double sum = 0.0;
    for (int pc = 0; pc < a.pieces; ++pc) sum += (double)bs[(size_t)pc * a.stride];
    grad[a.src_b + co] = (float)(sum * (double)a.inv_b);
  }
}

// m over the whole padded tensor [B * groups][h+2][w+2]: 16 (hi) where the saved TReLU output does not exceed thr, zero elsewhere
// and on the border
__global__ __launch_bounds__(256) void critic_clip_mask_kernel(const HsRec* __restrict__ act, HsRec* __restrict__ m, float thr, int h,
                                                               int w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % (w + 2)), y = (int)((i / (w + 2)) % (h + 2));
  HsRec o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o.hi[e] = o.lo[e] = (_Float16)0.f;
  if (x >= 1 && x <= w && y >= 1 && y <= h) {
    const HsRec r = act[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) o.hi[e] = ((float)r.hi[e] + (float)r.lo[e]) > thr ? (_Float16)0.f : (_Float16)HS_ASCALE;
  }
  m[i] = o;
}

__device__ inline double rec_dot(const HsRec& p, const HsRec& q) {
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += (double)((float)p.hi[e] + (float)p.lo[e]) * (double)((float)q.hi[e] + (float)q.lo[e]);
  return s;
}

// one workgroup per image
__global__ __launch_bounds__(256) void critic_alpha_dot_kernel(const HsRec* __restrict__ g, const HsRec* __restrict__ wm, int G,
                                                               const HsRec* __restrict__ res, int resG, const HsRec* __restrict__ m,
                                                               int mG, int h, int w, double* __restrict__ out) {
  __shared__ double sh[256];
  const int b = blockIdx.x, tid = threadIdx.x, hw = h * w;
  const size_t plane = (size_t)(h + 2) * (w + 2);
  double acc = 0.0;
  for (int i = tid; i < G * hw; i += 256) {
    const int grp = i / hw, r = i - grp * hw, y = r / w, x = r - y * w;
    const size_t pix = (size_t)(y + 1) * (w + 2) + (x + 1);
    const size_t rec = ((size_t)b * G + grp) * plane + pix;
    acc += rec_dot(g[rec], wm[rec]);
    if (res && grp < resG) acc += rec_dot(res[((size_t)b * resG + grp) * plane + pix], m[((size_t)b * mG + grp) * plane + pix]);
  }
  acc = block_sum256(acc, sh);
  if (tid == 0) out[b] = acc;
}

// one thread per channel of the last activation [B][64 groups][h+2][w+2]; images and pixels in index order
__global__ __launch_bounds__(64) void critic_fc_grad_kernel(const HsRec* __restrict__ feat, const float* __restrict__ gv,
                                                            const float* __restrict__ fc_w, float thr, int B, int h, int w,
                                                            float* __restrict__ grad_fcw, double* __restrict__ a20) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const size_t plane = (size_t)(h + 2) * (w + 2);
  double pooled = 0.0, clipped = 0.0;
  for (int b = 0; b < B; ++b) {
    const HsRec* p = feat + ((size_t)b * 64 + (c >> 3)) * plane;
    double s = 0.0;
    int cnt = 0;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const HsRec& r = p[(y + 1) * (w + 2) + x + 1];
        const float val = (float)r.hi[c & 7] + (float)r.lo[c & 7];
        s += (double)val;
        cnt += val > thr ? 0 : 1;
      }
    const double gb = (double)gv[b];
    pooled += gb * s;
    clipped += gb * (double)cnt;
  }
  const double inv = 1.0 / (double)(h * w);
  grad_fcw[c] = (float)(pooled * inv / (double)HS_ASCALE);
  a20[c] = clipped * inv * (double)fc_w[c];
}

__global__ __launch_bounds__(64) void critic_alpha_finish_kernel(const AlphaFinishJob J, const double* __restrict__ dots,
                                                                 const double* __restrict__ a20, const float* __restrict__ gv,
                                                                 float* __restrict__ grad) {
  const int t = threadIdx.x;
  if (t < 21) {
    if (J.alpha_src[t] < 0) return;
    double s = 0.0;
    for (int b = 0; b < J.B; ++b) s += dots[(size_t)t * J.B + b] * (double)gv[b];
    grad[J.alpha_src[t]] = (float)(s * (double)J.inv);
  } else if (t == 21) {
    double s = 0.0;
    for (int c = 0; c < 512; ++c) s += a20[c];
    grad[J.head_src] = (float)s;
  } else if (t == 22) {
    double s = 0.0;
    for (int b = 0; b < J.B; ++b) s += (double)gv[b];
    grad[J.fcb_src] = (float)s;
  }
}

inline dim3 g1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

// Pieces of the pixel axis: enough workgroups for two rounds of the 256 CUs, at most 64 pieces, at least two chunks of 32
// pixels per piece.  Depends on the layer's shape and (B, h, w) only.
int critic_wgrad_pieces(int cout, int K, int B, int h, int w) {
  const long long tiles = (long long)(cout / 32) * (K / 32);
  const long long nchunks = ((long long)B * h * w + WG_KC - 1) / WG_KC;
  long long want = (512 + tiles - 1) / tiles;
  if (want > 64) want = 64;
  if (want > nchunks / 2) want = nchunks / 2;
  if (want < 1) want = 1;
  const long long cpp = (nchunks + want - 1) / want;
  return (int)((nchunks + cpp - 1) / cpp);   // no empty piece
}

int critic_wgrad_chunks_per_piece(int cout, int K, int B, int h, int w) {
  const long long nchunks = ((long long)B * h * w + WG_KC - 1) / WG_KC;
  const int pieces = critic_wgrad_pieces(cout, K, B, h, w);
  return (int)((nchunks + pieces - 1) / pieces);
}

int launch_critic_wgrad(const WgradJob& J, float* slab, hipStream_t s) {
  if (J.cout % 32 || J.K % 32 || J.nt < 1 || J.nt > 9 || J.K / 8 > J.Xg || J.cout / 8 > J.Gg || (long long)J.B * J.h * J.w >= (1LL << 31) - WG_KC) {
    set_error("critic weight gradient: unsupported geometry (%d x %d channels, %d taps, %d x %d x %d)", J.cout, J.K, J.nt, J.B, J.h, J.w);
    return PNPX_ERR_SHAPE;
  }
  WgradArgs a;
  a.G = J.G;
  a.X = J.X;
  a.gv = J.gv;
  a.slab = slab;
  a.Gg = J.Gg;
  a.Xg = J.Xg;
  a.cout = J.cout;
  a.K = J.K;
  a.nt = J.nt;
  a.B = J.B;
  a.h = J.h;
  a.w = J.w;
  a.tilesM = J.cout / 32;
  a.nchunks = (int)(((long long)J.B * J.h * J.w + WG_KC - 1) / WG_KC);
  const int pieces = critic_wgrad_pieces(J.cout, J.K, J.B, J.h, J.w);
  a.cpp = critic_wgrad_chunks_per_piece(J.cout, J.K, J.B, J.h, J.w);
  a.stride = critic_wgrad_piece_floats(J.cout, J.K, J.nt);
  for (int i = 0; i < 9; ++i) a.tap[i] = i < J.nt ? J.tap[i] : 0;
  hipLaunchKernelGGL(critic_wgrad_kernel, dim3((unsigned)(a.tilesM * (J.K / 32)), (unsigned)pieces), dim3(256), 0, s, a);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_critic_wn_grad(const WnGradJob& J, const float* slab, const float* params, float* grad, hipStream_t s) {
  WnGradArgs a;
  a.D = J.D;
  a.src_b = J.src_b;
  a.src_g = J.src_g;
  a.fan = J.fan;
  a.pieces = J.pieces;
  a.stride = critic_wgrad_piece_floats(J.D.rows, J.D.K, J.D.nt);
  a.inv_w = J.inv_w;
  a.inv_b = J.inv_b;
  hipLaunchKernelGGL(critic_wn_grad_kernel, dim3((unsigned)J.D.rows), dim3(256), 0, s, a, slab, params, grad);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_critic_clip_mask(const HsRec* act, HsRec* m, float thr, int B, int groups, int h, int w, hipStream_t s) {
  const size_t n = (size_t)B * groups * (h + 2) * (w + 2);
  hipLaunchKernelGGL(critic_clip_mask_kernel, g1(n), dim3(256), 0, s, act, m, thr, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_critic_alpha_dot(const HsRec* g, const HsRec* wm, int G, const HsRec* res, int resG, const HsRec* m, int mG, int B, int h, int w,
                            double* out, hipStream_t s) {
  hipLaunchKernelGGL(critic_alpha_dot_kernel, dim3((unsigned)B), dim3(256), 0, s, g, wm, G, res, resG, m, mG, h, w, out);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_critic_fc_grad(const HsRec* feat, const float* gv, const float* fc_w, float thr, int B, int h, int w, float* grad_fcw, double* a20,
                          hipStream_t s) {
  hipLaunchKernelGGL(critic_fc_grad_kernel, dim3(8), dim3(64), 0, s, feat, gv, fc_w, thr, B, h, w, grad_fcw, a20);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_critic_alpha_finish(const AlphaFinishJob& J, const double* dots, const double* a20, const float* gv, float* grad, hipStream_t s) {
  hipLaunchKernelGGL(critic_alpha_finish_kernel, dim3(1), dim3(64), 0, s, J, dots, a20, gv, grad);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

}  // namespace pnpx
