// The DRUNet written once for its two kernel families (drunet.hip: half-split HS8 records; drunet_f32.hip: padded planar fp32):
// the layer table and the VJP's index arithmetic, the host weight tensors both packings start from, the arena reservation, and
// the forward / backward walks over the topology.  Nothing here launches a kernel of its own or chooses one: a walk calls the
// family (a plain struct of launch functions, passed as a template argument) where a launch stands, and owns only the topology:
// which buffer is current, which layer is next.
#pragma once
#include <cstring>
#include <vector>

#include "common.h"

namespace pnpx {

constexpr int DRU_NC[4] = {64, 128, 256, 512};

// ------------------------------------------------------------------ layer table
struct DruLayer {
  int kind;   // 0 head, 1 res conv a (ReLU), 2 res conv b (+res), 3 strided 2x2, 4 transposed 2x2, 5 tail
  int cin, cout;
};
// state_dict order (KAIR UNetRes): head; down1..3 = nb x (res.0, res.2) + strided conv; body; up3..1 = convT + nb x (..); tail
inline std::vector<DruLayer> dru_layers(int nb) {
  std::vector<DruLayer> L;
  L.push_back({0, 2, DRU_NC[0]});
  auto res = [&](int c) {
    for (int i = 0; i < nb; ++i) {
      L.push_back({1, c, c});
      L.push_back({2, c, c});
    }
  };
  for (int l = 0; l < 3; ++l) {
    res(DRU_NC[l]);
    L.push_back({3, DRU_NC[l], DRU_NC[l + 1]});
  }
  res(DRU_NC[3]);
  for (int l = 2; l >= 0; --l) {
    L.push_back({4, DRU_NC[l + 1], DRU_NC[l]});
    res(DRU_NC[l]);
  }
  L.push_back({5, DRU_NC[0], 1});
  return L;
}
inline bool dru_is_1x1(const DruLayer& d) { return d.kind == 3 || d.kind == 4; }   // the 2x2 layers run as 1x1 over phase-major channels
inline size_t layer_params(const DruLayer& d) { return (size_t)d.cin * d.cout * (dru_is_1x1(d) ? 4 : 9); }
// layer indices of the table above, as the backward walk needs them
struct DruIdx {
  int nb;
  int down(int l) const { return 1 + l * (2 * nb + 1); }                       // first conv of the encoder ResBlocks of level l
  int strided(int l) const { return down(l) + 2 * nb; }                        // level l -> l + 1
  int body() const { return 1 + 3 * (2 * nb + 1); }
  int convT(int l) const { return body() + 2 * nb + (2 - l) * (2 * nb + 1); }   // level l + 1 -> l
  int up(int l) const { return convT(l) + 1; }
  size_t count() const { return (size_t)up(0) + 2 * nb + 1; }                  // = dru_layers(nb).size()
};

// ------------------------------------------------------------------ weight tensors
// The tensor w3[cout][cin][3][3] a layer runs with, from its state_dict tensor w: the strided / transposed 2x2 convolutions as the
// centre tap of a 1x1 over phase-major channel stacks, the tail widened to 32 couts (rows 1..31 zero).
inline void dru_layer_w3(const DruLayer& d, const float* w, int* cin_o, int* cout_o, std::vector<float>& w3) {
  int cin = d.cin, cout = d.cout;
  if (d.kind == 3) {          // Conv2d k2 s2 [cout][cin][2][2] -> 1x1 over the space-to-depth input
    cin = 4 * d.cin;
    w3.assign((size_t)cout * cin * 9, 0.f);
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < d.cin; ++ci)
        for (int ph = 0; ph < 4; ++ph) w3[((size_t)co * cin + ph * d.cin + ci) * 9 + 4] = w[((size_t)co * d.cin + ci) * 4 + ph];
  } else if (d.kind == 4) {   // ConvTranspose2d k2 s2 [cin][cout][2][2] -> 1x1 to 4*cout channels, then depth-to-space
    cout = 4 * d.cout;
    w3.assign((size_t)cout * cin * 9, 0.f);
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < d.cout; ++co)
        for (int ph = 0; ph < 4; ++ph) w3[((size_t)(ph * d.cout + co) * cin + ci) * 9 + 4] = w[((size_t)ci * d.cout + co) * 4 + ph];
  } else if (d.kind == 5) {   // tail [1][64][3][3]
    cout = 32;
    w3.assign((size_t)cout * cin * 9, 0.f);
    std::memcpy(w3.data(), w, sizeof(float) * (size_t)cin * 9);
  } else {
    w3.assign(w, w + (size_t)cout * cin * 9);
  }
  *cin_o = cin;
  *cout_o = cout;
}
// Its adjoint: a convolution's adjoint is the convolution with the transposed, tap-mirrored weights, wa[ci][co][tap] =
// w3[co][ci][8 - tap] -- a [cin][cout][9] tensor, zero-padded to max(cin, 32) output channels (the head's adjoint: 64 -> 2 of 32).
inline int dru_adjoint_w3(const std::vector<float>& w3, int cin, int cout, std::vector<float>& wa) {
  const int rows = cin < 32 ? 32 : cin;
  wa.assign((size_t)rows * cout * 9, 0.f);
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int t = 0; t < 9; ++t) wa[((size_t)ci * cout + co) * 9 + t] = w3[((size_t)co * cin + ci) * 9 + (8 - t)];
  return rows;
}

// ------------------------------------------------------------------ arena
// Offsets of the level tensors in an arena, in the family's unit (bytes / floats).  Per level l: S (skip / level input), P, Q
// (ResBlock outputs, alternating), M (ResBlock middle; skip sums), U (decoder level input, l <= 2), DT (space-to-depth input of
// the strided conv / output of the transposed conv, l >= 1: 2 * C_l channels), MK (keep plans only: the ReLU output of every
// ResBlock, encoder blocks 0..nb-1, decoder blocks nb..2nb-1).  Each family's plan adds its own extra tensors.
struct DruOffsets {
  size_t S[4], P[4], Q[4], M[4], U[4], DT[4], MK[4][16];
};
// The offsets of images b0.. of every tensor: each is [image][...] with per_image(C, l) units per image of C channels at level l.
template <class PerImage>
DruOffsets dru_slice(DruOffsets o, int b0, PerImage&& per_image) {
  for (int l = 0; l < 4; ++l) {
    const size_t per = per_image(DRU_NC[l], l) * (size_t)b0;
    for (size_t* t : {o.S, o.P, o.Q, o.M, o.U}) t[l] += per;
    o.DT[l] += per_image(2 * DRU_NC[l], l) * (size_t)b0;
    for (size_t& m : o.MK[l]) m += per;
  }
  return o;
}

// What becomes of an arena's keep planes (MK) when a call that does not need them re-lays the arena out.
//   KEEPS_STAY (half-split family): they stay while the image size stays -- a VJP followed by same-shape inference calls and
//     another VJP lays the arena out once, and the batch capacity never shrinks at one image size;
//   KEEPS_DROP (fp32 family): any re-layout for an inference call drops them, and a layout WITH keep planes is sized for the
//     batch of the call that needs them, not for the largest batch seen (~1 GB per 512 x 512 image at nb = 4).
// The gradient arenas never hold keep planes; the two policies agree there.
enum DruKeepPolicy { KEEPS_STAY, KEEPS_DROP };

// Makes arena A fit a call of B images at H x W (with keep planes if want_keeps): nothing if it does; else the new layout's
// size comes from total_bytes(images, keeps), the allocation grows if it must, and the whole arena is zeroed -- the zero
// borders of every tensor are written here, once.  `what` names the arena in the allocation error.
template <class TotalBytes>
int dru_arena_reserve(DruArena& A, int B, int H, int W, bool want_keeps, DruKeepPolicy policy, const char* what,
                      TotalBytes&& total_bytes) {
  const bool same = H == A.capH && W == A.capW;
  if (B <= A.capB && same && (!want_keeps || A.keeps)) return PNPX_OK;
  const bool keeps = want_keeps || (policy == KEEPS_STAY && A.keeps && same);
  const int nb_img = (same && A.capB > B && (policy == KEEPS_STAY || !keeps)) ? A.capB : B;
  const size_t total = total_bytes(nb_img, keeps);
  PNPX_HIP(hipDeviceSynchronize());
  if (A.buf.bytes < total) {
    if (A.buf.p) PNPX_HIP(hipFree(A.buf.p));
    A.buf = DeviceBuf();
    A.capB = A.capH = A.capW = 0;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, total);
    if (e != hipSuccess) {
      set_error("DRUNet %s allocation of %zu bytes failed: %s", what, total, hipGetErrorString(e));
      return PNPX_ERR_ALLOC;
    }
    A.buf.p = p;
    A.buf.bytes = total;
  }
  PNPX_HIP(hipMemset(A.buf.p, 0, A.buf.bytes));
  A.capB = nb_img;
  A.capH = H;
  A.capW = W;
  A.keeps = keeps;
  return PNPX_OK;
}
inline void dru_arena_free(DruArena& A) {
  if (A.buf.p) (void)hipFree(A.buf.p);
  A = DruArena();
}

// ------------------------------------------------------------------ forward walk
//   x1 = head(cat[x, sigma]);  x_{l+1} = strided2x2(ResBlocks(x_l));  v = body(x4);  v = ResBlocks(convT2x2(v + x_{l+1}));
//   out = tail(v + x1)
// over the tensors at offsets o of arena A (dru_slice: one slice of the batch).  The family F launches (each returns a status):
//   head(S0)                                   cat[x, sigma] -> 64 channels, linear (layer 0)
//   conv(li, in, out, h, w, slope, res)        layer li at h x w, negative slope 0 (ReLU) / 1 (linear), optional residual
//   s2d(l, in, out) / d2s(l, in, out)          C_l channels at level l <-> 4 * C_l channels at level l + 1
//   add(l, a, b, out)                          skip sum at level l
//   tail(li, m0)                               last layer -> the output images
// keep_mids: every ResBlock's ReLU output goes to a plane of its own (MK) for the VJP.
template <class T, class F>
int dru_forward_walk(const F& f, T* A, const DruOffsets& o, int nb, int H, int W, bool keep_mids) {
  size_t li = 1;
  auto resblocks = [&](int l, int dec, T* cur, T** result) -> int {
    const int h = H >> l, w = W >> l;
    T* pq[2] = {A + o.P[l], A + o.Q[l]};
    int k = 0;
    for (int i = 0; i < nb; ++i) {
      T* mid = keep_mids ? A + o.MK[l][dec * nb + i] : A + o.M[l];
      PNPX_TRY(f.conv(li++, cur, mid, h, w, 0.f, nullptr));       // conv + ReLU
      T* dst = pq[k];
      if (dst == cur) dst = pq[k ^= 1];
      PNPX_TRY(f.conv(li++, mid, dst, h, w, 1.f, cur));            // conv + x
      cur = dst;
      k ^= 1;
    }
    *result = cur;
    return PNPX_OK;
  };
  PNPX_TRY(f.head(A + o.S[0]));
  T* cur = A + o.S[0];
  for (int l = 0; l < 3; ++l) {
    PNPX_TRY(resblocks(l, 0, cur, &cur));
    PNPX_TRY(f.s2d(l, cur, A + o.DT[l + 1]));
    PNPX_TRY(f.conv(li++, A + o.DT[l + 1], A + o.S[l + 1], H >> (l + 1), W >> (l + 1), 1.f, nullptr));
    cur = A + o.S[l + 1];
  }
  PNPX_TRY(resblocks(3, 0, cur, &cur));
  for (int l = 2; l >= 0; --l) {
    PNPX_TRY(f.add(l + 1, cur, A + o.S[l + 1], A + o.M[l + 1]));
    PNPX_TRY(f.conv(li++, A + o.M[l + 1], A + o.DT[l + 1], H >> (l + 1), W >> (l + 1), 1.f, nullptr));   // 1x1 to 4 * C_l phase-major channels
    PNPX_TRY(f.d2s(l, A + o.DT[l + 1], A + o.U[l]));
    PNPX_TRY(resblocks(l, 1, A + o.U[l], &cur));
  }
  PNPX_TRY(f.add(0, cur, A + o.S[0], A + o.M[0]));
  PNPX_TRY(f.tail(li++, A + o.M[0]));
  if (li != DruIdx{nb}.count()) {
    set_error("DRUNet: internal layer walk mismatch (%zu of %zu)", li, DruIdx{nb}.count());
    return PNPX_ERR_ARG;
  }
  return PNPX_OK;
}

// ------------------------------------------------------------------ backward walk
// Back-propagation through  out = clamp(tail(m0), 0, 1)  down to (x, sigma).  Every step is the adjoint of a forward step on the
// same kernels: a 3x3 convolution's adjoint is the convolution with the transposed, tap-mirrored weights; a ResBlock
// out = B(relu(A(in))) + in  back-propagates as
//     g_mid = B^T g_out * 1[mid > 0]   (the saved ReLU output as mask)
//     g_in  = A^T g_mid + g_out        (linear, residual)
// the strided 2x2 convolution (s2d + 1x1) as 1x1^T + d2s, the transposed 2x2 convolution (1x1 + d2s) as s2d + 1x1^T; skip sums
// pass their gradient to both operands.  GA / go: the gradient arena, FA / fo: the forward arena (its MK planes are read).
// The family F launches s2d / d2s / add as above and
//   seed(S0)                                   clamp mask + the tail's adjoint: grad_out -> gradient of m0
//   conv(li, in, out, h, w, dmask, res)        adjoint of layer li; dmask (ReLU' of a saved activation) or res (added), not both
//   input_grad(m0)                             the head's adjoint and the reduction to (grad_x, grad_sigma)
template <class T, class F>
int dru_backward_walk(const F& f, T* GA, const DruOffsets& go, T* FA, const DruOffsets& fo, int nb, int H, int W) {
  const DruIdx ix{nb};
  // adjoint of the nb ResBlocks of (level l, encoder / decoder side) applied to the gradient in `cur`; result pointer returned
  auto resblocks_bwd = [&](int l, int dec, int idx0, T* cur, T** result) -> int {
    const int h = H >> l, w = W >> l;
    T* pq[2] = {GA + go.P[l], GA + go.Q[l]};
    int k = 0;
    for (int i = nb - 1; i >= 0; --i) {
      PNPX_TRY(f.conv(idx0 + 2 * i + 1, cur, GA + go.M[l], h, w, FA + fo.MK[l][dec * nb + i], nullptr));   // B^T g_out * relu'(mid)
      T* dst = pq[k];
      if (dst == cur) dst = pq[k ^= 1];
      PNPX_TRY(f.conv(idx0 + 2 * i, GA + go.M[l], dst, h, w, nullptr, cur));   // A^T g_mid + g_out
      cur = dst;
      k ^= 1;
    }
    *result = cur;
    return PNPX_OK;
  };
  PNPX_TRY(f.seed(GA + go.S[0]));
  // decoder, level 0 up to level 2: go.S[l] = gradient of m_l = c_l + S[l] (kept: it is also the skip's gradient)
  T* cur = GA + go.S[0];
  for (int l = 0; l <= 2; ++l) {
    PNPX_TRY(resblocks_bwd(l, 1, ix.up(l), cur, &cur));   // -> gradient of U[l]
    PNPX_TRY(f.s2d(l, cur, GA + go.DT[l + 1]));         // adjoint of depth-to-space
    PNPX_TRY(f.conv(ix.convT(l), GA + go.DT[l + 1], GA + go.S[l + 1], H >> (l + 1), W >> (l + 1), nullptr, nullptr));
    cur = GA + go.S[l + 1];
  }
  // body and encoder, level 3 down to level 0: go.M[l] = total gradient of S[l]
  PNPX_TRY(resblocks_bwd(3, 0, ix.body(), cur, &cur));
  PNPX_TRY(f.add(3, cur, GA + go.S[3], GA + go.M[3]));
  for (int l = 2; l >= 0; --l) {
    PNPX_TRY(f.conv(ix.strided(l), GA + go.M[l + 1], GA + go.DT[l + 1], H >> (l + 1), W >> (l + 1), nullptr, nullptr));
    PNPX_TRY(f.d2s(l, GA + go.DT[l + 1], GA + go.U[l]));   // adjoint of space-to-depth
    PNPX_TRY(resblocks_bwd(l, 0, ix.down(l), GA + go.U[l], &cur));
    PNPX_TRY(f.add(l, cur, GA + go.S[l], GA + go.M[l]));
  }
  return f.input_grad(GA + go.M[0]);
}

}  // namespace pnpx
