// Stand-alone host check of the F(4x4,3x3) kernels' halo plan (pnpx_winof4_halo_plan: the tables by which the four instances gather a
// chunk's halo into LDS and the input transform reads it), meant to be built with the host sanitizers: a sweep over the instances and
// image sizes into buffers of exactly the sizes the plan reports, with the properties a kernel launch relies on checked per geometry --
// every halo element written once, from its own source, where the transform reads it; no LDS float written twice; dummy lanes where
// nothing reads; 16-byte pieces aligned at both ends; every source inside the chunk's eight padded planes for every region of the
// image; the counted waits against the per-wave instruction counts.  No GPU is touched: nothing is launched.
//
// The translation unit whose host code runs here is compiled with the sanitizers on the host pass only; everything else comes from the
// plain library:
//   mkdir -p tools/_build && cd tfpnp_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I. -I../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       ../../tools/check_winof4_halo.hip conv3x3_winof4.hip \
//       -fsanitize=address,undefined -o ../../tools/_build/check_winof4_halo -L.. -lpnpx -Wl,-rpath,$PWD/..
//   tools/_build/check_winof4_halo          (any box; prints "winof4 halo: ok"; exit status 0)
#include <algorithm>
#include <cstdio>
#include <vector>

#include "pnpx.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { if (fails < 20) std::printf("line %d: %s  (inst %d, %d x %d)\n", __LINE__, #c, g_inst, g_H, g_W); ++fails; } } while (0)
static int g_inst, g_H, g_W;

int main() {
  long geoms = 0, lanes = 0;
  for (int inst = 0; inst < 4; ++inst) {
    const int rw_min = inst == 3 ? 64 : 32;
    for (int H = 16; H <= 272; H += 16)
      for (int W = rw_min; W <= 320; W += rw_min) {
        if (H > 64 && W > 128 && (H != 256 || W != 256)) continue;      // the large sizes: the network's own only
        g_inst = inst, g_H = H, g_W = W;
        int info[PNPX_WINOF4_HALO_INFO];
        EXPECT(pnpx_winof4_halo_plan(inst, H, W, info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
        const int h16 = info[0], RW = info[2], RWL = info[3], RPXL = info[4], ORG = info[5], HCOL = info[6], NI = info[7], N16 = info[8];
        const int PER_WAVE = info[9], NRAW = info[10], RAW_BYTES = info[11], OFF_RAW = info[12], LDS_USED = info[13];
        const int n = NI * 64, nread = 8 * 18 * (RW + 2), nfl = RAW_BYTES / 4;
        std::vector<long long> src(n);
        std::vector<int> dst(n), width(n), wave(n), real(n), read(nread);
        EXPECT(pnpx_winof4_halo_plan(inst, H, W, info, src.data(), dst.data(), width.data(), wave.data(), real.data(), read.data()) == 0);
        const int Hp = H + 2, Wp = W + 8;
        const long long HpWp = (long long)Hp * Wp;
        std::vector<long long> img(nfl, -1);
        std::vector<char> dummy(nfl, 0);
        int per_wave[8] = {0};
        for (int j = 0; j < n; ++j) {
          const int i = j / 64, w = width[j];
          EXPECT(w == (i < N16 ? 16 : 4) && wave[j] == i % 8);
          EXPECT(dst[j] >= 0 && dst[j] + w <= RAW_BYTES && dst[j] % w == 0 && src[j] >= 0 && src[j] % w == 0);
          if (j % 64 == 0) ++per_wave[wave[j]];
          else EXPECT(dst[j] == dst[j - 1] + w);
          if (dst[j] < 0 || dst[j] + w > RAW_BYTES) continue;
          for (int k = 0; k < w / 4; ++k) {
            const int f = dst[j] / 4 + k;
            if (real[j]) {
              EXPECT(img[f] == -1);      // no LDS float receives real data twice
              img[f] = src[j] / 4 + k;
              // the source lies inside the chunk's 8 padded planes for the first and the last region both ways
              const long long s = src[j] / 4 + k, ch = s / HpWp, r = s % HpWp, row = r / Wp, col = r % Wp;
              EXPECT(ch >= 0 && ch < 8 && row + (H - 16) <= Hp - 1 && col + ORG + (W - RW) <= Wp - 1);
              EXPECT(ch * HpWp + (row + H - 16) * Wp + col + ORG + (W - RW) < 8 * HpWp);
            } else {
              EXPECT(src[j] == 0);
              dummy[f] = 1;
            }
          }
          ++lanes;
        }
        for (int c = 0; c < 8; ++c)
          for (int hy = 0; hy < 18; ++hy)
            for (int hx = 0; hx < RW + 2; ++hx) {
              const int rd = read[(c * 18 + hy) * (RW + 2) + hx];
              EXPECT(rd == (c * RPXL + hy * RWL + hx + HCOL) * 4 && rd >= 0 && rd + 4 <= RAW_BYTES);
              if (rd < 0 || rd + 4 > RAW_BYTES) continue;
              EXPECT(img[rd / 4] == c * HpWp + (long long)hy * Wp + hx + 3 - ORG);      // halo column hx = padded column x0 + 3 + hx
              EXPECT(!dummy[rd / 4]);
            }
        for (int f = 0; f < nfl; ++f) EXPECT(!(dummy[f] && img[f] >= 0));
        EXPECT(*std::min_element(per_wave, per_wave + 8) == NRAW && *std::max_element(per_wave, per_wave + 8) == PER_WAVE && PER_WAVE <= NRAW + 1);
        EXPECT(NI > N16);      // at least one dword gather stays in every kernel
        EXPECT(LDS_USED <= 160 * 1024 && OFF_RAW + 2 * RAW_BYTES <= LDS_USED && OFF_RAW % 16 == 0 && RAW_BYTES % 16 == 0);
        EXPECT(info[16] >= 0 && info[17] == (inst == 3 ? NRAW : info[14] + NRAW) && info[17] <= 63 && info[19] <= 63);
        if (inst == 2) EXPECT(info[18] == info[14] + info[15] && info[19] == info[14] + NRAW + info[15]);
        if (h16) EXPECT(RPXL % 4 == 0 && RWL % 4 == 0 && ORG == 0 && HCOL == 3 && Wp % 4 == 0 && HpWp % 4 == 0);
        ++geoms;
      }
  }
  int info[PNPX_WINOF4_HALO_INFO];
  g_inst = g_H = g_W = -1;
  EXPECT(pnpx_winof4_halo_plan(4, 16, 64, info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0);
  EXPECT(pnpx_winof4_halo_plan(3, 16, 32, info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0);
  EXPECT(pnpx_winof4_halo_plan(0, 24, 32, info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0);
  EXPECT(pnpx_winof4_halo_plan(0, 16, 32, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0);
  std::printf("%ld geometries, %ld lanes\n", geoms, lanes);
  std::printf(fails ? "winof4 halo: %d FAILED\n" : "winof4 halo: ok\n", fails);
  return fails ? 1 : 0;
}
