// The ResNet-18 trunk on the half-split launches, shared by the actor (policy*.hip) and the critic (critic.hip): a 3x3 stride-2
// stem and four stages of two BasicBlocks, each stage entered with stride 2 and a 1x1 stride-2 shortcut.  Every stride-2
// convolution is a 2x2-window launch (tap mask 0x01B) over an HS8 space-to-depth tensor, the shortcut the 1x1 instance (0x010)
// over its phase-(0,0) channels, the stride-1 convolutions carry the residual operand.
//
// LAYER NUMBERING (the registration order of both parameter vectors), used by everything that indexes a trunk layer:
//     0 = stem,   1 + 5 * stage + {0 entry conv1, 1 conv2, 2 shortcut, 3 block-1 conv1, 4 block-1 conv2}
#pragma once
#include <vector>

#include "common.h"
#include "conv_hs.h"

namespace pnpx {

constexpr int TRUNK_LAYERS = 21;
inline int stage_planes(int n) { return 64 << n; }   // n = 0..3
inline dim3 g1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
// tap mask layer li is packed and launched with; adjoint: of its input-gradient launch (the mirrored window)
inline int trunk_taps(int li, bool adjoint) {
  const int k = li == 0 ? 0 : (li - 1) % 5;
  return k == 0 ? (adjoint ? 0x1B0 : 0x01B) : (k == 2 ? 0x010 : 0x1FF);
}

// ------------------------------------------------------------------------------------------- host packing
struct Reader {   // walks a flat parameter vector
  const float* p;
  const float* take(size_t n) {
    const float* r = p;
    p += n;
    return r;
  }
};
// Dense "effective" weights of one launch: E[cout][K][9] (+ bias[cout])
struct Eff {
  int cout, K;
  std::vector<float> w, bias;
  Eff(int cout_, int K_) : cout(cout_), K(K_), w((size_t)cout_ * K_ * 9, 0.f), bias(cout_, 0.f) {}
  float& at(int co, int k, int tap) { return w[((size_t)co * K + k) * 9 + tap]; }
  float at(int co, int k, int tap) const { return w[((size_t)co * K + k) * 9 + tap]; }
};
// w: the network's own fold already applied (BatchNorm scale / weight-norm), dense [cout][cin][k]; bias[cout].  Rows [row0, row0 + cout).
void put_conv_s1(Eff& E, int row0, const float* w, const float* bias, int cout, int cin);            // 3x3 stride 1
void put_conv_s2(Eff& E, int row0, const float* w, const float* bias, int cout, int cin, int Cp);    // 3x3 stride 2 over a space-to-depth input, Cp channels per phase
void put_shortcut(Eff& E, int row0, const float* w, const float* bias, int cout, int cin);           // 1x1 stride 2 = centre tap of phase (0,0)

struct HostBlob {   // the weight blob as the host lays it out: 256-float alignment before every entry
  std::vector<float> f;
  void align() { f.resize((f.size() + 255) & ~(size_t)255, 0.f); }
  size_t add(const float* p, size_t n) {
    align();
    const size_t off = f.size();
    f.insert(f.end(), p, p + n);
    return off;
  }
};
struct Packed {   // one half-split packing inside a HostBlob (offsets in floats)
  size_t w = 0, b = 0;
  float scale = 1.f;
  int cin = 0, cout = 0, mt = 0;
};
Packed pack_layer(HostBlob& H, const Eff& E, int tapmask, bool with_bias);
// the launch descriptor of a packing once the blob is at `base` on the device
void bind_packed(ConvLayerHsDev& D, const Packed& P, const float* base);

// ------------------------------------------------------------------------------------------- activations
struct TrunkAct {   // where an activation tensor of C x H x W per image sits in an arena; whoever places it decides its layout and size
  size_t off = 0;   // floats; an HS8 tensor [C/8][H+2][W+2] of 32-byte records takes C*(H+2)*(W+2) floats per image (hs_act_floats)
  int C = 0, H = 0, W = 0;
};
inline size_t hs_act_floats(int C, int h, int w) { return (size_t)C * (h + 2) * (w + 2); }
struct TrunkPlan {   // the forward tensors (each network lays them out in its own arena order)
  TrunkAct ob_s, stem_o, stem_s;   // space-to-depth observation; stem output (64, H/2); its space-to-depth copy
  TrunkAct t1[4], sc[4], o0[4], t2[4], o1[4];
  TrunkAct o1s[3];                 // space-to-depth copy of o1 (next stage's entry)
};
// arena for B observations of H x W (grows to the largest batch seen at one size; zero borders written once); floats_for(nb): its size
template <class FloatsFor>
int reserve_arena_hs(DeviceBuf& arena, int& capB, int& capH, int& capW, int B, int H, int W, FloatsFor floats_for, const char* what) {
  if (B <= capB && H == capH && W == capW) return PNPX_OK;
  const bool same = (H == capH && W == capW);
  const int nb = same ? (B > capB ? B : capB) : B;
  const size_t bytes = floats_for(nb) * sizeof(float);
  PNPX_HIP(hipDeviceSynchronize());
  if (arena.bytes < bytes) {
    if (arena.p) PNPX_HIP(hipFree(arena.p));
    arena = DeviceBuf();
    capB = capH = capW = 0;   // nothing is reserved until the allocation below succeeds
    PNPX_TRY(alloc_dev(arena, bytes, what));
  }
  PNPX_HIP(hipMemset(arena.p, 0, bytes));
  PNPX_HIP(hipDeviceSynchronize());
  capB = nb;
  capH = H;
  capW = W;
  return PNPX_OK;
}

// ------------------------------------------------------------------------------------------- launches
struct HsLaunch {   // one convolution launch of the trunk or of its adjoint chain
  const ConvLayerHsDev* D = nullptr;
  const float* bias = nullptr;
  int taps = 0x1FF;
  int epi = 0;            // ConvHsFuse::critic_epi (0: the plain instance, activation slope `slope`)
  float slope = 1.f;
  float alpha = 0.f;
  int share = 1;
  unsigned* range_flag = nullptr;
};
// tensors by address with their channel counts; res / mask may be null
int launch_hs_conv(const HsLaunch& L, const char* in, int inC, char* out, int outC, const char* res, int resC, const char* mask, int maskC,
                   int B, int h, int w, hipStream_t s);

// observation [B][C][H][W] fp32 -> HS8 space-to-depth tensor [B][4*Cp/8][H/2+2][W/2+2] (phase-major channel groups; channels >= C zero)
int launch_pack_ob_hs(const float* ob, char* out, int C, int Cp, int B, int H, int W, hipStream_t s);

// The forward over B observations whose tensors start b0 images into the plan's (arena base A): pack, stem, per stage entry, shortcut,
// conv2 + shortcut, block 1, space-to-depth.  Epilogue: epi / alpha[li] (ConvHsFuse::critic_epi and the threshold behind layer li), or
// alpha == null: ReLU on the plain instances.  The shortcut is always linear.
int trunk_forward(const ConvLayerHsDev* layers, const float* const* bias, const TrunkPlan& P, float* A, int b0, const float* ob, int C,
                  int Cp, int B, int H, int W, int share, int epi, const float* alpha, unsigned* range_flag, hipStream_t s);

}  // namespace pnpx
