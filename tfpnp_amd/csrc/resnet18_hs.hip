// The ResNet-18 half-split trunk shared by the actor and the critic (resnet18_hs.h): host packing of a layer, the arena, the
// observation packing kernel and the forward launch sequence.
#include "resnet18_hs.h"

#include "hs_rec.h"
#include "hs_relayout.h"

namespace pnpx {

// ------------------------------------------------------------------------------------------- host packing
void put_conv_s1(Eff& E, int row0, const float* w, const float* bias, int cout, int cin) {
  for (int co = 0; co < cout; ++co) {
    E.bias[row0 + co] = bias[co];
    for (int ci = 0; ci < cin; ++ci)
      for (int t = 0; t < 9; ++t) E.at(row0 + co, ci, t) = w[((size_t)co * cin + ci) * 9 + t];
  }
}
void put_conv_s2(Eff& E, int row0, const float* w, const float* bias, int cout, int cin, int Cp) {
  for (int co = 0; co < cout; ++co) {
    E.bias[row0 + co] = bias[co];
    for (int ci = 0; ci < cin; ++ci)
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
          // input row 2*yo + (dy - 1): offset 0 -> phase 0 / same half-res row (tap row 1); offset -1 -> phase 1 /
          // previous row (tap row 0); offset +1 -> phase 1 / same row (tap row 1).  Likewise in x.
          const int py = (dy == 1) ? 0 : 1, ty = (dy == 0) ? 0 : 1;
          const int px = (dx == 1) ? 0 : 1, tx = (dx == 0) ? 0 : 1;
          E.at(row0 + co, (py * 2 + px) * Cp + ci, ty * 3 + tx) = w[((size_t)co * cin + ci) * 9 + dy * 3 + dx];
        }
  }
}
void put_shortcut(Eff& E, int row0, const float* w, const float* bias, int cout, int cin) {
  for (int co = 0; co < cout; ++co) {
    E.bias[row0 + co] = bias[co];
    for (int ci = 0; ci < cin; ++ci) E.at(row0 + co, ci, 4) = w[(size_t)co * cin + ci];
  }
}

Packed pack_layer(HostBlob& H, const Eff& E, int tapmask, bool with_bias) {
  Packed P;
  int nt = 0;
  for (int t = 0; t < 9; ++t) nt += (tapmask >> t) & 1;
  H.align();
  P.w = H.f.size();
  const size_t n16 = (size_t)E.cout * E.K * nt * 2;
  H.f.resize(H.f.size() + (n16 + 1) / 2, 0.f);
  P.mt = (E.cout % 64 == 0) ? 64 : 32;
  P.scale = pack_conv_weights_hs_taps(E.w.data(), E.cout, E.K, P.mt, tapmask, reinterpret_cast<uint16_t*>(H.f.data() + P.w));
  if (with_bias) P.b = H.add(E.bias.data(), E.bias.size());
  P.cin = E.K;
  P.cout = E.cout;
  return P;
}

void bind_packed(ConvLayerHsDev& D, const Packed& P, const float* base) {
  D.cin = D.cin_pad = P.cin;
  D.cout = P.cout;
  D.mt = P.mt;
  D.w = const_cast<char*>(reinterpret_cast<const char*>(base + P.w));
  D.inv_scale = 1.0f / (P.scale * HS_ASCALE);
}

// ------------------------------------------------------------------------------------------- launches
int launch_hs_conv(const HsLaunch& L, const char* in, int inC, char* out, int outC, const char* res, int resC, const char* mask, int maskC,
                   int B, int h, int w, hipStream_t s) {
  ConvHsFuse f;
  f.slope = L.slope;       // (read by the plain instance only)
  f.taps = L.taps;
  f.wreg = 0;              // (read for 32 -> 32 layers only: none here)
  f.in0_groups = inC / 8;
  f.critic_epi = L.epi;
  f.alpha = L.alpha;
  f.res = res;
  f.res_groups = res ? resC / 8 : 0;
  f.dmask = mask;
  f.share = L.share;
  f.range_flag = L.range_flag;
  if (L.D->cout != outC || L.D->cin_pad > inC || (mask && maskC != outC) || (res && resC > outC)) {
    set_error("resnet18: internal launch geometry mismatch (%d -> %d channels over %d -> %d)", L.D->cin_pad, L.D->cout, inC, outC);
    return PNPX_ERR_SHAPE;
  }
  return launch_conv_hs(hs_layer(*L.D, L.bias), in, L.D->cin_pad / 8, nullptr, 0, out, B, h, w, f, s);
}

namespace {

__global__ __launch_bounds__(256) void pack_ob_s2d_hs_kernel(const float* __restrict__ ob, HsRec* __restrict__ out, int C, int Cp, int H,
                                                             int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int W2 = W >> 1, H2 = H >> 1, Gp = Cp >> 3;
  const int x2 = (int)(i % W2);
  size_t t = i / W2;
  const int y2 = (int)(t % H2);
  t /= H2;
  const int g = (int)(t % Gp);
  t /= Gp;
  const int ph = (int)(t % 4);
  const size_t b = t / 4;
  const int y = 2 * y2 + (ph >> 1), x = 2 * x2 + (ph & 1);
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = g * 8 + k;
    v[k] = c < C ? ob[((b * C + c) * H + y) * (size_t)W + x] * HS_ASCALE : 0.f;
  }
  out[((b * 4 * Gp + (size_t)ph * Gp + g) * (H2 + 2) + (y2 + 1)) * (size_t)(W2 + 2) + (x2 + 1)] = hs_pack(v);
}

}  // namespace

int launch_pack_ob_hs(const float* ob, char* out, int C, int Cp, int B, int H, int W, hipStream_t s) {
  const size_t n = (size_t)B * 4 * (Cp / 8) * (H / 2) * (W / 2);
  hipLaunchKernelGGL(pack_ob_s2d_hs_kernel, g1(n), dim3(256), 0, s, ob, reinterpret_cast<HsRec*>(out), C, Cp, H, W, n);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int trunk_forward(const ConvLayerHsDev* layers, const float* const* bias, const TrunkPlan& P, float* A, int b0, const float* ob, int C,
                  int Cp, int B, int H, int W, int share, int epi, const float* alpha, unsigned* range_flag, hipStream_t s) {
  auto at = [&](const TrunkAct& d) { return reinterpret_cast<char*>(A + d.off + (size_t)b0 * hs_act_floats(d.C, d.H, d.W)); };
  auto conv = [&](int li, const TrunkAct& in, const TrunkAct& out, const TrunkAct* res, int h, int w) -> int {
    const bool linear = trunk_taps(li, false) == 0x010;   // the shortcut
    HsLaunch L;
    L.D = &layers[li];
    L.bias = bias[li];
    L.taps = trunk_taps(li, false);
    L.epi = (alpha && !linear) ? epi : 0;
    L.slope = (alpha || linear) ? 1.f : 0.f;
    L.alpha = (alpha && !linear) ? alpha[li] : 0.f;
    L.share = share;
    L.range_flag = range_flag;
    return launch_hs_conv(L, at(in), in.C, at(out), out.C, res ? at(*res) : nullptr, res ? res->C : 0, nullptr, 0, B, h, w, s);
  };
  // HS8 -> HS8 space-to-depth (phase-major groups) for the next stride-2 entry
  auto s2d = [&](const TrunkAct& in, const TrunkAct& out, int h, int w) -> int {
    const int G = in.C / 8;
    const size_t n = (size_t)B * 4 * G * (h / 2) * (w / 2) * 2;
    hipLaunchKernelGGL(hs_s2d_kernel, g1(n), dim3(256), 0, s, reinterpret_cast<const uint4*>(at(in)), reinterpret_cast<uint4*>(at(out)), G, h,
                       w, n);
    PNPX_LAUNCH_CHECK();
    return PNPX_OK;
  };
  PNPX_TRY(launch_pack_ob_hs(ob, at(P.ob_s), C, Cp, B, H, W, s));
  PNPX_TRY(conv(0, P.ob_s, P.stem_o, nullptr, H / 2, W / 2));
  PNPX_TRY(s2d(P.stem_o, P.stem_s, H / 2, W / 2));
  for (int st = 0; st < 4; ++st) {
    const int h = H >> (st + 2), w = W >> (st + 2), l0 = 1 + 5 * st;
    const TrunkAct& s2in = st == 0 ? P.stem_s : P.o1s[st - 1];
    PNPX_TRY(conv(l0 + 0, s2in, P.t1[st], nullptr, h, w));
    PNPX_TRY(conv(l0 + 2, s2in, P.sc[st], nullptr, h, w));
    PNPX_TRY(conv(l0 + 1, P.t1[st], P.o0[st], &P.sc[st], h, w));
    PNPX_TRY(conv(l0 + 3, P.o0[st], P.t2[st], nullptr, h, w));
    PNPX_TRY(conv(l0 + 4, P.t2[st], P.o1[st], &P.o0[st], h, w));
    if (st < 3) PNPX_TRY(s2d(P.o1[st], P.o1s[st], h, w));
  }
  return PNPX_OK;
}

}  // namespace pnpx
