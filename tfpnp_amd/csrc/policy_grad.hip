// Parameter gradients of the actor through its train-mode forward (policy_loss.backward(), tfpnp/trainer/mddpg/trainer.py:171-212):
// the kernels.  The driver (policy_bn.hip::policy_param_grad) re-computes the train forward into a workspace that keeps every raw
// convolution output z and every activation, then walks the network backwards.  Per BatchNorm layer (n = B h w values per channel,
// dy = g_a * [a > 0] with a the saved activation, g_a the gradient of that activation):
//     d bias = S1 = sum dy          d weight = S2 * rstd,  S2 = sum dy (z - mean)
//     dz = weight * rstd * (dy - S1 / n - (z - mean) * rstd^2 * S2 / n)
// in three passes that mirror the forward's (bn_partial / bn_finish / bn_apply):
//   bn_bwd_partial_kernel  per (piece of BN_BWD_PIECE pixels, group of 8 channels): S1 and S2 in DOUBLE, interior pixels only, fixed-order
//                          block reduction (no atomics; the piece size is a constant, so the result does not depend on the launch)
//   bn_bwd_finish_kernel   per channel: the pieces in order -> d weight, d bias (scale undone) straight into grad_params, zeros into the
//                          running-statistics slots, and the coefficients A, c1, c2 of the apply pass
//   bn_bwd_apply_kernel    dz = A * dy - c1 - c2 * (z - mean) -> an HS8 tensor (interior only: the workspace border stays zero)
// On a block tail one dy feeds two layers -- bn2 and the shortcut's BatchNorm in block 0 (two z tensors, two S2, two dz), bn2 and the
// identity in block 1 (dy itself is written as a tensor: the residual operand of the adjoint convolution below) -- and is read once.
// dz is the G operand of the critic's weight-gradient GEMM (critic_grad.hip::critic_wgrad_kernel, K-split, deterministic) and the
// input of the adjoint convolution; pol_wgrad_finish_kernel turns the GEMM's pieces into the convolution's raw gradient.
//
// Gradient range: the tensors hold s * boost * g.  s is the power of two that brings max |g_f| (gradient of the pooled feature, over the
// batch) into [0.5, 1); it is DEVICE data (pol_grad_scale: absmax_kernel + grad_scale_kernel of grad_common.h, an integer atomicMax on
// the bits of a non-negative float -- order-independent), no host read-back.  boost is a host-side power of two (driver).  Every kernel
// that leaves the scaled domain multiplies by 1 / s (and 1 / boost), two exact fp32 products, so the result is exactly homogeneous in
// powers of two of the upstream gradients; all-zero upstream gradients give s = 1 / s = 0 and an all-zero vector.
//
// Heads (pol_head_grad_kernel, one workgroup per observation): pool, logits, probs, det re-derived with pool_heads_kernel's arithmetic;
// softmax backward gl_j = p_j (gp_j - sum_k gp_k p_k), sigmoid backward gd * d (1 - d), the SPI head through Linear(64, n_det), the ReLU
// and Linear(512, 64); g_f[b][512] in fp32.  The head tensors' gradients are sums over the batch in index order, one workgroup per
// output row (pol_head_param_grad_kernel).
#include "policy_grad.h"

#include "conv_hs.h"
#include "grad_common.h"

namespace pnpx {
namespace {

constexpr double BN_EPS = 1e-5;

// ------------------------------------------------------------------------------------------- heads
struct HeadArgs {
  const HsRec* feat;
  int h, w, n_det, spi;
  const float *sm_w, *sm_b, *d_w, *d_b, *d2_w, *d2_b, *gp, *gd;
  float *gf, *rows;
};
__global__ __launch_bounds__(256) void pol_head_grad_kernel(const HeadArgs a) {
  __shared__ float f[512];
  __shared__ float hid[64], pre[64], g1[64], g2[64];
  __shared__ float logit[2], gl[2];
  const int b = blockIdx.x, tid = threadIdx.x, n_det = a.n_det;
  const float inv = 1.f / ((float)(a.h * a.w) * HS_ASCALE);
  for (int c = tid; c < 512; c += 256) f[c] = hs_pooled(a.feat, b, 64, c, a.h, a.w, inv);
  if (tid < 64) hid[tid] = pre[tid] = g1[tid] = g2[tid] = 0.f;
  __syncthreads();
  auto dot512 = [&](const float* wrow) {
    float s = 0.f;
    for (int k = 0; k < 512; ++k) s = fmaf(wrow[k], f[k], s);
    return s;
  };
  if (tid < 2) logit[tid] = dot512(a.sm_w + tid * 512) + a.sm_b[tid];
  if (a.spi) {
    if (tid >= 64 && tid < 128) hid[tid - 64] = fmaxf(dot512(a.d_w + (tid - 64) * 512) + a.d_b[tid - 64], 0.f);
  } else if (tid >= 64 && tid < 64 + n_det) {
    pre[tid - 64] = dot512(a.d_w + (tid - 64) * 512) + a.d_b[tid - 64];
  }
  __syncthreads();
  if (tid == 0) {
    const float m = fmaxf(logit[0], logit[1]);
    const float e0 = expf(logit[0] - m), e1 = expf(logit[1] - m);
    const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
    const float gp0 = a.gp[b * 2 + 0], gp1 = a.gp[b * 2 + 1];
    const float dotp = gp0 * p0 + gp1 * p1;
    gl[0] = p0 * (gp0 - dotp);
    gl[1] = p1 * (gp1 - dotp);
  }
  if (a.spi && tid < n_det) {
    float s = a.d2_b[tid];
    for (int k = 0; k < 64; ++k) s = fmaf(a.d2_w[tid * 64 + k], hid[k], s);
    pre[tid] = s;
  }
  __syncthreads();
  if (tid < n_det) {
    const float d = 1.f / (1.f + expf(-pre[tid]));
    const float g = a.gd[(size_t)b * n_det + tid] * (d * (1.f - d));
    if (a.spi)
      g2[tid] = g;
    else
      g1[tid] = g;
  }
  __syncthreads();
  if (a.spi && tid < 64) {   // through Linear(64, n_det) and the ReLU
    float s = 0.f;
    for (int j = 0; j < n_det; ++j) s = fmaf(g2[j], a.d2_w[j * 64 + tid], s);
    g1[tid] = hid[tid] > 0.f ? s : 0.f;
  }
  __syncthreads();
  const int n1 = a.spi ? 64 : n_det;
  float* row = a.rows + (size_t)b * POL_HEAD_STRIDE;
  for (int c = tid; c < 512; c += 256) {
    float s = fmaf(gl[1], a.sm_w[512 + c], gl[0] * a.sm_w[c]);
    for (int r = 0; r < n1; ++r) s = fmaf(g1[r], a.d_w[r * 512 + c], s);
    a.gf[(size_t)b * 512 + c] = s;
    row[c] = f[c];
  }
  if (tid < 2) row[POL_HEAD_GL + tid] = gl[tid];
  if (tid < 64) {
    row[POL_HEAD_G1 + tid] = g1[tid];
    row[POL_HEAD_HID + tid] = hid[tid];
    row[POL_HEAD_G2 + tid] = g2[tid];
  }
}

// one workgroup per output row of fc_softmax.0 (2), the first deterministic Linear (n1) and, with the SPI head, the second (n_det):
// weight row = sum_b g[b][row] * in[b][:], bias = sum_b g[b][row], images in index order
__global__ __launch_bounds__(256) void pol_head_param_grad_kernel(const float* __restrict__ rows, int B, int n_det, int spi,
                                                                  float* __restrict__ grad, size_t head_src) {
  const int r = blockIdx.x, tid = threadIdx.x, n1 = spi ? 64 : n_det;
  int g_off, in_off, fan, j;
  size_t w_off, b_off;
  const size_t sm_b = head_src + 1024, d_w = sm_b + 2, d_b = d_w + (size_t)n1 * 512, d2_w = d_b + n1, d2_b = d2_w + (size_t)n_det * 64;
  if (r < 2) {
    j = r, g_off = POL_HEAD_GL, in_off = 0, fan = 512, w_off = head_src, b_off = sm_b;
  } else if (r < 2 + n1) {
    j = r - 2, g_off = POL_HEAD_G1, in_off = 0, fan = 512, w_off = d_w, b_off = d_b;
  } else {
    j = r - 2 - n1, g_off = POL_HEAD_G2, in_off = POL_HEAD_HID, fan = 64, w_off = d2_w, b_off = d2_b;
  }
  for (int k = tid; k < fan; k += 256) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
      const float* row = rows + (size_t)b * POL_HEAD_STRIDE;
      s += (double)row[g_off + j] * (double)row[in_off + k];
    }
    grad[w_off + (size_t)j * fan + k] = (float)s;
  }
  if (tid == 0) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)rows[(size_t)b * POL_HEAD_STRIDE + g_off + j];
    grad[b_off + j] = (float)s;
  }
}

// ------------------------------------------------------------------------------------------- gradient range
// ga: every interior pixel of [B][64][h+2][w+2] = (g_f * s) * k16 with k16 = boost * HS_ASCALE / (h w); gv[b] = (1 / s) * inv_boost
__global__ __launch_bounds__(256) void pol_grad_seed_kernel(const float* __restrict__ gf, const float2* __restrict__ slot, HsRec* __restrict__ ga,
                                                            float* __restrict__ gv, float k16, float inv_boost, int B, int h, int w, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float2 sc = *slot;
  if (i < (size_t)B) gv[i] = sc.y * inv_boost;
  if (i >= n) return;
  const int x = (int)(i % w);
  size_t t = i / w;
  const int y = (int)(t % h);
  t /= h;   // t = b * 64 + group
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = rounded_f32((gf[t * 8 + e] * sc.x) * k16);   // k16 is no power of two where h w is none
  ga[(t * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1)] = hs_pack(v);
}

// ------------------------------------------------------------------------------------------- BatchNorm backward
// part[piece][G * 8][3] = (S1, S2 of z0, S2 of z1) over the piece's interior pixels (pixel index = (b * h + y) * w + x), in the units the
// tensors carry (dy = stored / 16).  grid (pieces, G)
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const HsRec* __restrict__ g, const HsRec* __restrict__ act,
                                                             const HsRec* __restrict__ z0, const HsRec* __restrict__ z1,
                                                             const float* __restrict__ mean0, const float* __restrict__ mean1, int G, int h,
                                                             int w, long long npix, double* __restrict__ part) {
  __shared__ double red[8][256];
  const int tid = threadIdx.x, grp = blockIdx.y;
  const long long i0 = (long long)blockIdx.x * BN_BWD_PIECE;
  float m0[8], m1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m0[e] = mean0[grp * 8 + e];
    m1[e] = z1 ? mean1[grp * 8 + e] : 0.f;
  }
  double acc[24];
#pragma unroll
  for (int e = 0; e < 24; ++e) acc[e] = 0.0;
  for (int k = 0; k < BN_BWD_PIECE / 256; ++k) {
    const long long i = i0 + k * 256 + tid;
    if (i >= npix) break;
    const int x = (int)(i % w);
    const long long t = i / w;
    const int y = (int)(t % h);
    const long long b = t / h;
    const long long rec = ((b * G + grp) * (h + 2) + (y + 1)) * (long long)(w + 2) + (x + 1);
    float gv[8], av[8], zv[8];
    hs_unpack(g[rec], gv);
    hs_unpack(act[rec], av);
    hs_unpack(z0[rec], zv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double dy = av[e] > 0.f ? (double)gv[e] * (1.0 / HS_ASCALE) : 0.0;
      acc[e] += dy;
      acc[8 + e] += dy * ((double)zv[e] * (1.0 / HS_ASCALE) - (double)m0[e]);
      gv[e] = (float)dy;   // exact: a power-of-two multiple of an fp32 value
    }
    if (z1) {
      hs_unpack(z1[rec], zv);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[16 + e] += (double)gv[e] * ((double)zv[e] * (1.0 / HS_ASCALE) - (double)m1[e]);
    }
  }
  // three rounds of the fixed-order tree over 8 values each (LDS: 16 KiB)
  for (int q = 0; q < 3; ++q) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) red[e][tid] = acc[q * 8 + e];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[e][tid] += red[e][tid + st];
      }
      __syncthreads();
    }
    if (tid < 8) part[(((size_t)blockIdx.x * G + grp) * 8 + tid) * 3 + q] = red[tid][0];
  }
}

struct BnBwdFinishArgs {
  const double* part;
  int C, which, cout, npieces;   // channels of the tensor behind `part`; 0 / 1: S2 of l0 / l1
  long long n;
  const float* params;
  size_t bn;
  const float* var;
  float* grad;
  float* coef;
  const float2* slot;
  float inv_boost;
};
__global__ __launch_bounds__(64) void bn_bwd_finish_kernel(const BnBwdFinishArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.cout) return;
  double s1 = 0.0, s2 = 0.0;
  for (int p = 0; p < a.npieces; ++p) {
    const double* e = a.part + ((size_t)p * a.C + c) * 3;
    s1 += e[0];
    s2 += e[1 + a.which];
  }
  const double n = (double)a.n, rstd = 1.0 / sqrt((double)a.var[c] + BN_EPS);
  const float inv_s = a.slot->y;
  float* gr = a.grad + a.bn + c;
  gr[0] = ((float)(s2 * rstd) * inv_s) * a.inv_boost;
  gr[a.cout] = ((float)s1 * inv_s) * a.inv_boost;
  gr[2 * (size_t)a.cout] = 0.f;
  gr[3 * (size_t)a.cout] = 0.f;
  const double A = (double)a.params[a.bn + c] * rstd;
  a.coef[c] = (float)A;
  a.coef[a.cout + c] = (float)(A * s1 / n);
  a.coef[2 * a.cout + c] = (float)(A * rstd * rstd * s2 / n);
}

struct BnBwdApplyArgs {
  const HsRec *g, *act, *z0, *z1;
  const float *mean0, *mean1, *coef0, *coef1;
  HsRec *dz0, *dz1, *dy_out;
  int G, h, w, cout;
  size_t n;            // B * G * h * w records
  unsigned* range_flag;
};
__device__ __forceinline__ bool bn_bwd_term(const HsRec* __restrict__ z, HsRec* __restrict__ dz, const float* __restrict__ mean,
                                            const float* __restrict__ coef, int cout, int grp, size_t rec, const float dy[8]) {
  float zv[8], u[8];
  hs_unpack(z[rec], zv);
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = grp * 8 + e;
    const float v = coef[c] * dy[e] - coef[cout + c] - coef[2 * cout + c] * (zv[e] * (1.f / HS_ASCALE) - mean[c]);
    u[e] = v * HS_ASCALE;
    bad |= !(fabsf(v) < 4095.f);
  }
  dz[rec] = hs_pack(u);
  return bad;
}
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnBwdApplyArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int h = a.h, w = a.w, G = a.G;
  const int x = (int)(i % w);
  size_t t = i / w;
  const int y = (int)(t % h);
  t /= h;   // t = b * G + group
  const int grp = (int)(t % G);
  const size_t rec = (t * (h + 2) + (y + 1)) * (size_t)(w + 2) + (x + 1);
  float gv[8], av[8], dy[8];
  hs_unpack(a.g[rec], gv);
  hs_unpack(a.act[rec], av);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    gv[e] = av[e] > 0.f ? gv[e] : 0.f;
    dy[e] = gv[e] * (1.f / HS_ASCALE);
  }
  bool bad = bn_bwd_term(a.z0, a.dz0, a.mean0, a.coef0, a.cout, grp, rec, dy);
  if (a.z1) bad |= bn_bwd_term(a.z1, a.dz1, a.mean1, a.coef1, a.cout, grp, rec, dy);
  if (a.dy_out) a.dy_out[rec] = hs_pack(gv);
  if (bad && a.range_flag) __hip_atomic_fetch_or(a.range_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------------- weight gradients
__global__ __launch_bounds__(256) void pol_wgrad_finish_kernel(const PackDesc D, int fan, int pieces, size_t stride, float inv_w,
                                                               const float* __restrict__ slab, float* __restrict__ grad) {
  __shared__ int sTi[9];
  const int tid = threadIdx.x, co = blockIdx.x;
  wgrad_tap_index(D, sTi);
  __syncthreads();
  float* gout = grad + D.src_v + (size_t)co * fan;
  for (int i = tid; i < fan; i += 256) gout[i] = (float)(wgrad_gather(D, sTi, slab, stride, pieces, co, i) * (double)inv_w);
}

inline dim3 grid1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

int launch_pol_head_grad(const PolHeadGradJob& J, hipStream_t s) {
  HeadArgs a;
  a.feat = J.feat;
  a.h = J.h;
  a.w = J.w;
  a.n_det = J.n_det;
  a.spi = J.spi;
  a.sm_w = J.sm_w;
  a.sm_b = J.sm_b;
  a.d_w = J.d_w;
  a.d_b = J.d_b;
  a.d2_w = J.d2_w;
  a.d2_b = J.d2_b;
  a.gp = J.gp;
  a.gd = J.gd;
  a.gf = J.gf;
  a.rows = J.rows;
  hipLaunchKernelGGL(pol_head_grad_kernel, dim3((unsigned)J.B), dim3(256), 0, s, a);
  PNPX_LAUNCH_CHECK();
  const int nrows = 2 + (J.spi ? 64 + J.n_det : J.n_det);
  hipLaunchKernelGGL(pol_head_param_grad_kernel, dim3((unsigned)nrows), dim3(256), 0, s, J.rows, J.B, J.n_det, J.spi, J.grad, J.head_src);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_pol_grad_seed(const float* gf, unsigned* bits, float2* slot, HsRec* ga, float* gv, float boost, int B, int h, int w, hipStream_t s) {
  PNPX_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(absmax_kernel, dim3(64), dim3(256), 0, s, gf, (size_t)B * 512, bits);
  PNPX_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_scale_kernel, dim3(1), dim3(1), 0, s, bits, slot);
  PNPX_LAUNCH_CHECK();
  const size_t n = (size_t)B * 64 * h * w;
  hipLaunchKernelGGL(pol_grad_seed_kernel, grid1(n), dim3(256), 0, s, gf, slot, ga, gv, boost * HS_ASCALE / (float)(h * w), 1.0f / boost, B, h, w, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_bn_bwd(const BnBwdJob& J, hipStream_t s) {
  const long long npix = (long long)J.B * J.h * J.w;
  const int np = (int)bn_bwd_pieces(npix), cout = J.G * 8;
  hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((unsigned)np, (unsigned)J.G), dim3(256), 0, s, J.g, J.act, J.l0.z, J.l1.z, J.l0.mean, J.l1.mean,
                     J.G, J.h, J.w, npix, J.part);
  PNPX_LAUNCH_CHECK();
  const BnBwdLayer* Ls[2] = {&J.l0, &J.l1};
  for (int k = 0; k < 2; ++k) {
    if (!Ls[k]->z) continue;
    BnBwdFinishArgs f;
    f.part = J.part;
    f.C = cout;
    f.which = k;
    f.cout = cout;
    f.npieces = np;
    f.n = npix;
    f.params = J.params;
    f.bn = Ls[k]->bn;
    f.var = Ls[k]->var;
    f.grad = J.grad;
    f.coef = Ls[k]->coef;
    f.slot = J.slot;
    f.inv_boost = J.inv_boost;
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((unsigned)((cout + 63) / 64)), dim3(64), 0, s, f);
    PNPX_LAUNCH_CHECK();
  }
  BnBwdApplyArgs a;
  a.g = J.g;
  a.act = J.act;
  a.z0 = J.l0.z;
  a.z1 = J.l1.z;
  a.mean0 = J.l0.mean;
  a.mean1 = J.l1.mean;
  a.coef0 = J.l0.coef;
  a.coef1 = J.l1.coef;
  a.dz0 = J.l0.dz;
  a.dz1 = J.l1.dz;
  a.dy_out = J.dy_out;
  a.G = J.G;
  a.h = J.h;
  a.w = J.w;
  a.cout = cout;
  a.n = (size_t)J.B * J.G * J.h * J.w;
  a.range_flag = J.range_flag;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, grid1(a.n), dim3(256), 0, s, a);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_pol_wgrad_finish(const PackDesc& D, int fan, int pieces, float inv_w, const float* slab, float* grad, hipStream_t s) {
  const size_t stride = (size_t)D.rows * D.nt * D.K + D.rows;   // critic_wgrad_piece_floats
  hipLaunchKernelGGL(pol_wgrad_finish_kernel, dim3((unsigned)D.rows), dim3(256), 0, s, D, fan, pieces, stride, inv_w, slab, grad);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

}  // namespace pnpx
