// Stand-alone host check of the F(4x4,3x3) kernel's 32-cout instance, meant to be built with the host sanitizers: the selector's forward
// and last-layer rows over a grid of options, geometries and batch classes (conv_f32_forward / conv_f32_last against
// pnpx_conv_f32_forward_plan and the rule restated here), and pack_conv_weights_winof4_c32 for the layer shapes it is used on (32 -> 32;
// 16 -> 32 and 24 -> 96 beside it) into buffers of exactly conv3x3_winof4_floats elements, every element of which must be written.  No GPU
// is touched: nothing is launched.
//
// The four translation units whose host code runs here are compiled with the sanitizers on the host pass only; everything else comes
// from the plain library:
//   mkdir -p tools/_build && cd tfpnp_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I. -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       ../../tools/check_winof4_c32.hip conv_f32_select.hip conv3x3_winof4.hip conv3x3_wino8.hip conv3x3_wino.hip \
//       -fsanitize=address,undefined -o ../../tools/_build/check_winof4_c32 -L.. -lpnpx -Wl,-rpath,$PWD/..
//   tools/_build/check_winof4_c32          (any box; prints "winof4 c32: ok"; exit status 0)
#include <cmath>
#include <cstdio>
#include <vector>

#include "conv_f32_select.h"
using namespace pnpx;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
  static const float packed = 0.f;
  const int geoms[][5] = {{32, 0, 32, 256, 256}, {32, 0, 32, 64, 64},  {16, 0, 32, 16, 64},   {24, 0, 96, 32, 128},  {32, 0, 32, 64, 96},  {32, 0, 32, 16, 32},
                          {32, 0, 32, 24, 64},   {8, 0, 32, 16, 64},   {12, 0, 32, 16, 64},   {32, 0, 64, 64, 64},   {64, 0, 128, 32, 64}, {32, 64, 32, 64, 64},
                          {32, 0, 48, 16, 64},   {256, 0, 256, 16, 16}};
  long rows = 0, c32 = 0;
  for (const auto& g : geoms)
    for (int B : {1, 6, 48})
      for (int ks = 0; ks <= 2; ++ks)
        for (int opts = 0; opts < 256; ++opts) {
          if ((opts & 128) && g[1]) continue;      // the last layer has one source
          ConvF32Sel v;
          v.winograd = opts & 1;
          v.wino8 = opts & 2;
          v.winof4 = opts & 4;
          v.winof4_c32 = opts & 8;
          v.u = (opts & 16) ? &packed : nullptr;
          v.u_f4 = (opts & 32) ? &packed : nullptr;
          v.u_f4c32 = (opts & 64) ? &packed : nullptr;
          v.ksplit = ks;
          const bool last = opts & 128;
          const ConvF32Choice c = last ? conv_f32_last(v, g[0], g[2], g[3], g[4], B) : conv_f32_forward(v, g[0], g[1], g[2], g[3], g[4], B);
          EXPECT(pnpx_conv_f32_forward_plan(opts, ks, 1, g[0], g[1], g[2], g[3], g[4], B) == (int)c.kernel + 16 * c.pieces + 256 * (c.fused ? 1 : 0));
          // the rule: the 32-cout instance exactly where the 8-wave kernel would run a plain single-source layer in one piece, the bit is
          // set, the weights exist and the geometry passes; everything else as without the bit and the weights
          ConvF32Sel w = v;
          w.winof4_c32 = false;
          w.u_f4c32 = nullptr;
          const ConvF32Choice base = last ? conv_f32_last(w, g[0], g[2], g[3], g[4], B) : conv_f32_forward(w, g[0], g[1], g[2], g[3], g[4], B);
          const bool fused_last = last && base.fused;
          const bool want = !fused_last && base.kernel == ConvF32Kernel::Wino8 && base.pieces == 1 && v.winof4_c32 && v.u_f4c32 && g[1] == 0 &&
                            conv3x3_winof4_c32_ok(g[0], 0, g[2], g[3], g[4]);
          EXPECT((c.kernel == ConvF32Kernel::WinoF4C32) == want);
          if (want) EXPECT(c.pieces == 1 && c.fused == base.fused);
          else EXPECT(c.kernel == base.kernel && c.pieces == base.pieces && c.fused == base.fused);
          ++rows;
          c32 += want;
        }
  EXPECT(c32 > 0 && c32 < rows);
  EXPECT(conv3x3_winof4_c32_ok(16, 0, 32, 16, 64) && !conv3x3_winof4_c32_ok(16, 0, 32, 16, 32) && !conv3x3_winof4_c32_ok(16, 0, 64, 16, 64) &&
         !conv3x3_winof4_c32_ok(16, 8, 32, 16, 64) && !conv3x3_winof4_c32_ok(8, 0, 32, 16, 64) && !conv3x3_winof4_c32_ok(16, 0, 32, 8, 64));

  const int layers[][2] = {{32, 32}, {32, 16}, {96, 24}};      // cout, cin
  for (const auto& l : layers) {
    const int cout = l[0], cin = l[1];
    EXPECT(conv3x3_winof4_c32_packs(cout, cin));
    std::vector<float> w((size_t)cout * cin * 9);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((i * 2654435761u) % 1024) / 1024.f - 0.5f;
    std::vector<float> dst(conv3x3_winof4_floats(cout, cin), NAN);
    pack_conv_weights_winof4_c32(w.data(), cout, cin, dst.data());
    size_t unwritten = 0;
    for (float x : dst) unwritten += std::isnan(x);
    EXPECT(unwritten == 0);
    std::vector<float> again(dst.size(), NAN);
    EXPECT(pnpx_winof4_c32_pack(w.data(), cout, cin, again.data()) == PNPX_OK && again == dst);
  }
  std::vector<float> none(4, 0.f);
  EXPECT(pnpx_winof4_c32_pack(none.data(), 48, 8, none.data()) != PNPX_OK && pnpx_winof4_c32_pack(none.data(), 32, 12, none.data()) != PNPX_OK);
  std::printf("%ld selector rows, %ld on the 32-cout F(4x4) instance; three layer shapes packed\n", rows, c32);
  std::printf(fails ? "winof4 c32: %d FAILED\n" : "winof4 c32: ok\n", fails);
  return fails ? 1 : 0;
}
