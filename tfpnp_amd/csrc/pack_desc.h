// Device-side weight packing shared by the critic (critic.hip) and the actor (policy_pack.hip): the descriptor of one
// half-split packing, where an element of a launch's dense effective weights lives in the flat parameter vector, and the
// store of one (hi, lo) fragment pair.  The fold (weight-norm in double, BatchNorm in fp32) stays with each network.
#pragma once
#include "common.h"

namespace pnpx {

struct PackDesc {     // one packing: [rows/mt][K/16][nt][hi,lo][kg][mt][8] f16 at blob + dst
  unsigned src_v, chan0, dst;
  unsigned items;          // (hi, lo) fragment pairs = rows * K / 8 * nt
  int conv;                // convolution (scale index)
  int rows, K, mt, nt;
  int kind;                // 0: 3x3 stride 1 (put_conv_s1); 1: 3x3 stride 2 over the space-to-depth input (put_conv_s2); 2: 1x1 shortcut
  int cin, Cp;             // source input channels; channels per phase of the space-to-depth input (kind 1)
  int adj;                 // the adjoint: rows / K transposed, taps mirrored
  int tap[9];
};
// The window of a packing: its taps are the set bits of `mask` in ascending order.
inline void pack_desc_window(PackDesc& P, int mask) {
  P.nt = 0;
  for (int t = 0; t < 9; ++t)
    if ((mask >> t) & 1) P.tap[P.nt++] = t;
}
// The window a FORWARD packing of each kind has: 3x3 stride 1; 3x3 stride 2 on the space-to-depth grid; the 1x1 shortcut
inline int pack_kind_window(int kind) { return kind == 0 ? 0x1FF : kind == 1 ? 0x01B : 0x010; }
struct CopyDesc {
  unsigned src, dst, n;
  unsigned space;          // source: 0 = the parameter vector; 1 = the folded BatchNorm shifts (actor only)
};
// blob[dst + i] = (space ? sh : P)[src + i] for the descriptors copy_dev[0 .. grid.y) (device memory), grid.x blocks of 256
// elements each (live_params.hip).  sh may be null when no descriptor has space 1 (the critic).
int launch_live_copy(const CopyDesc* copy_dev, dim3 grid, const float* P, const float* sh, float* blob, hipStream_t s);

__device__ inline int hs_row_channel_dev(int row) {   // conv_hs.hip::hs_row_channel
  const int kg = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3);
  return 16 * kg + r;
}

// Where element (co, k, tap) of the dense effective weights of a launch (put_conv_s1 / put_conv_s2 / put_shortcut) sits in
// the convolution's native [cout][cin][kh][kw] weights; -1: a structural zero (padding channel, absent phase / tap).
__device__ inline long long eff_src_offset(const PackDesc& D, int co, int k, int tap) {
  if (D.kind == 0) {
    if (k >= D.cin) return -1;
    return ((long long)co * D.cin + k) * 9 + tap;
  }
  if (D.kind == 1) {
    const int ph = k / D.Cp, ci = k - ph * D.Cp, ty = tap / 3, tx = tap - 3 * ty;
    if (ph >= 4 || ci >= D.cin || ty > 1 || tx > 1) return -1;
    // phase 0 holds the centre row / column (window position 1); phase 1 the row above (position 0) and below (position 1)
    const int dy = (ph >> 1) ? (ty ? 2 : 0) : (ty ? 1 : -1), dx = (ph & 1) ? (tx ? 2 : 0) : (tx ? 1 : -1);
    if (dy < 0 || dx < 0) return -1;
    return ((long long)co * D.cin + ci) * 9 + dy * 3 + dx;
  }
  if (tap != 4 || k >= D.cin) return -1;
  return (long long)co * D.cin + k;
}

// The inverse: raw element i of an output channel's fan ([cin][kh][kw], i < cin * kh * kw) sits at exactly one effective position
// (k, tap) of the launch -- un-packing a gradient of the effective weights is a gather per raw element (critic_grad.hip).
__device__ inline void eff_pos_of_src(const PackDesc& D, int i, int& k, int& tap) {
  if (D.kind == 0) {
    k = i / 9;
    tap = i - 9 * k;
  } else if (D.kind == 1) {
    const int ci = i / 9, t = i - 9 * ci, dy = t / 3, dx = t - 3 * dy;
    const int py = (dy == 1) ? 0 : 1, ty = (dy == 0) ? 0 : 1, px = (dx == 1) ? 0 : 1, tx = (dx == 0) ? 0 : 1;   // put_conv_s2
    k = (py * 2 + px) * D.Cp + ci;
    tap = ty * 3 + tx;
  } else {
    k = i;
    tap = 4;
  }
}

// Item i of packing D = (cout tile, K chunk, tap, K half, row): the hi and the lo fragment of eight consecutive K elements of
// s * eff(row, k, tap), as pack_conv_weights_hs_taps lays them out.  The caller has checked i < D.items.
template <class EffAt>
__device__ inline void hs_pack_item(const PackDesc& D, unsigned i, float s, float* __restrict__ blob, EffAt eff) {
  const int mt = D.mt, nch = D.K / 16, nt = D.nt;
  const int m = (int)(i % mt);
  unsigned t = i / mt;
  const int kg = (int)(t & 1);
  t >>= 1;
  const int ti = (int)(t % nt);
  t /= nt;
  const int ch = (int)(t % nch), ct = (int)(t / nch);
  const int row = ct * mt + (m & ~31) + hs_row_channel_dev(m & 31), tap = D.tap[ti];
  union {
    _Float16 h[8];
    uint4 q;
  } hi, lo;
#pragma unroll
  for (int el = 0; el < 8; ++el) {
    const float v = eff(row, ch * 16 + kg * 8 + el, tap) * s;
    hi.h[el] = (_Float16)v;
    lo.h[el] = (_Float16)(v - (float)hi.h[el]);
  }
  uint16_t* dst = reinterpret_cast<uint16_t*>(blob + D.dst) + ((((size_t)ct * nch + ch) * nt + ti) * 2) * 2 * mt * 8;
  *reinterpret_cast<uint4*>(dst + ((size_t)(0 * 2 + kg) * mt + m) * 8) = hi.q;
  *reinterpret_cast<uint4*>(dst + ((size_t)(1 * 2 + kg) * mt + m) * 8) = lo.q;
}

}  // namespace pnpx
