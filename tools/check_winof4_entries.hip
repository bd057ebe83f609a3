// Stand-alone host check of the decoder entries' F(4x4,3x3) selection and weight packing, meant to be built with the host sanitizers: the
// selector's entry rows over a grid of options, geometries and batch classes (conv_f32_entry against pnpx_conv_f32_entry_plan and the
// rule restated here), and pack_conv_weights_winof4 for the three entry shapes (768 -> 256, 384 -> 128, 192 -> 64) into buffers of exactly
// conv3x3_winof4_floats elements, every element of which must be written.  No GPU is touched: nothing is launched.
//
// The four translation units whose host code runs here are compiled with the sanitizers on the host pass only; everything else comes
// from the plain library:
//   mkdir -p tools/_build && cd tfpnp_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I. -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       ../../tools/check_winof4_entries.hip conv_f32_select.hip conv3x3_winof4.hip conv3x3_wino8.hip conv3x3_wino.hip \
//       -fsanitize=address,undefined -o ../../tools/_build/check_winof4_entries -L.. -lpnpx -Wl,-rpath,$PWD/..
//   tools/_build/check_winof4_entries          (any box; prints "winof4 entries: ok"; exit status 0)
#include <cmath>
#include <cstdio>
#include <vector>

#include "conv_f32_select.h"
using namespace pnpx;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
  static const float packed = 0.f;
  const int geoms[][5] = {{256, 512, 256, 32, 32}, {128, 256, 128, 64, 64}, {64, 128, 64, 128, 128}, {32, 64, 32, 256, 256}, {8, 8, 64, 16, 32},
                          {24, 40, 128, 32, 64},   {64, 128, 64, 16, 16},   {64, 12, 64, 16, 32},    {12, 64, 64, 16, 32},   {64, 128, 64, 17, 33},
                          {64, 128, 96, 16, 32},   {256, 512, 256, 8, 16}};
  long rows = 0, f4 = 0;
  for (const auto& g : geoms)
    for (int B : {1, 6, 48})
      for (int ks = 0; ks <= 2; ++ks)
        for (int opts = 0; opts < 128; ++opts) {
          ConvF32Sel v;
          v.winograd = opts & 1;
          v.wino8 = opts & 2;
          v.winof4 = opts & 4;
          v.winof4_entry = opts & 8;
          v.fuse_up = opts & 16;
          v.u = (opts & 32) ? &packed : nullptr;
          v.u_f4 = (opts & 64) ? &packed : nullptr;
          v.ksplit = ks;
          const ConvF32Choice c = conv_f32_entry(v, g[0], g[1], g[2], g[3], g[4], B);
          EXPECT(pnpx_conv_f32_entry_plan(opts, ks, 1, g[0], g[1], g[2], g[3], g[4], B) == (int)c.kernel + 16 * c.pieces + 256 * (c.fused ? 1 : 0));
          // the rule: F(4x4) exactly where the 8-wave kernel would run the entry in one piece, the bit is set, the weights exist and the
          // geometry passes; never fused; the plain layers' bit changes nothing
          ConvF32Sel w = v;
          w.winof4_entry = false;
          w.u_f4 = nullptr;
          const ConvF32Choice base = conv_f32_entry(w, g[0], g[1], g[2], g[3], g[4], B);
          const bool want = base.kernel == ConvF32Kernel::Wino8 && base.pieces == 1 && v.winof4_entry && v.u_f4 &&
                            conv3x3_winof4_entry_ok(g[0], g[1], g[2], g[3], g[4]);
          EXPECT((c.kernel == ConvF32Kernel::WinoF4) == want);
          if (want) EXPECT(!c.fused && c.pieces == 1);
          else EXPECT(c.kernel == base.kernel && c.pieces == base.pieces && c.fused == base.fused);
          w = v;
          w.winof4 = !v.winof4;
          const ConvF32Choice o = conv_f32_entry(w, g[0], g[1], g[2], g[3], g[4], B);
          EXPECT(o.kernel == c.kernel && o.pieces == c.pieces && o.fused == c.fused);
          ++rows;
          f4 += want;
        }
  EXPECT(f4 > 0 && f4 < rows);
  EXPECT(!conv3x3_winof4_entry_ok(0, 64, 64, 16, 32) && !conv3x3_winof4_entry_ok(64, 0, 64, 16, 32) && conv3x3_winof4_entry_ok(8, 8, 64, 16, 32));

  const int layers[][2] = {{256, 768}, {128, 384}, {64, 192}};      // cout, cin of layers 15, 18, 21
  for (const auto& l : layers) {
    const int cout = l[0], cin = l[1];
    EXPECT(conv3x3_winof4_packs(cout, cin));
    std::vector<float> w((size_t)cout * cin * 9);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((i * 2654435761u) % 1024) / 1024.f - 0.5f;
    std::vector<float> dst(conv3x3_winof4_floats(cout, cin), NAN);
    pack_conv_weights_winof4(w.data(), cout, cin, dst.data());
    size_t unwritten = 0;
    for (float x : dst) unwritten += std::isnan(x);
    EXPECT(unwritten == 0);
    std::vector<float> again(dst.size(), NAN);
    EXPECT(pnpx_winof4_pack(w.data(), cout, cin, again.data()) == PNPX_OK && again == dst);
  }
  std::printf("%ld selector rows, %ld on the F(4x4) kernel; three entry shapes packed\n", rows, f4);
  std::printf(fails ? "winof4 entries: %d FAILED\n" : "winof4 entries: ok\n", fails);
  return fails ? 1 : 0;
}
