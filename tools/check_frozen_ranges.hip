// Stand-alone check of LiveOptim (csrc/live_optim.hip) with frozen ranges that do NOT start and end on multiples of four floats.  The
// actor's ranges always do, so no test of the suite reaches the element-by-element branch for 16-byte chunks that straddle a range
// boundary; this program does.  A step with a table and garbage (inf, NaN, 1e30) inside the ranges must give the bytes of a step without
// a table on the same gradient with zeros there (a zero gradient on zero moments moves nothing and adds nothing to the norm): norm,
// parameters, both moments, step counter, for an aligned and an unaligned gradient, at three vector lengths, two steps each.
//
//   mkdir -p tools/_build && hipcc --offload-arch=gfx950 -O2 -std=c++17 -Itfpnp_amd/csrc -Iinclude tools/check_frozen_ranges.hip \
//       -o tools/_build/check_frozen_ranges -Ltfpnp_amd -lpnpx -Wl,-rpath,$PWD/tfpnp_amd
//   tools/_build/check_frozen_ranges          (GPU box; prints one line per case and "frozen ranges: ok"; exit status 0)
//
// Last run on one MI355X: SAME BYTES in all six cases (n = 1003, 4098, 300001).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.h"
using namespace pnpx;

#define CK(x) do { if ((x) != hipSuccess) { printf("hip error line %d\n", __LINE__); return 2; } } while (0)

int run(const std::vector<float>& p0, const std::vector<float>& g, const FrozenRange* tab, int ntab, bool unaligned, std::vector<float>& out,
        float* norm) {
  const size_t n = p0.size();
  LiveParams live;
  LiveOptim opt;
  if (live.alloc(n, "check parameter") != PNPX_OK) return 2;
  if (live.set_host(p0.data()) != PNPX_OK) return 2;
  if (opt.set_frozen(tab, ntab, n, "check table") != PNPX_OK) return 2;
  float *gd = nullptr, *slot = nullptr;
  CK(hipMalloc(&gd, (n + 4) * sizeof(float)));
  CK(hipMalloc(&slot, 4 * sizeof(float)));
  float* gp = gd + (unaligned ? 1 : 0);
  CK(hipMemcpy(gp, g.data(), n * sizeof(float), hipMemcpyHostToDevice));
  for (int k = 0; k < 2; ++k) {
    if (opt.launch_step(live, gp, 1e-3f, 0.9f, 0.999f, 1e-8f, 50.f, slot, nullptr, "check optimiser state", nullptr) != PNPX_OK) return 2;
    CK(hipDeviceSynchronize());
    opt.commit();
  }
  out.assign(3 * n + 1, 0.f);
  std::vector<float> m(n), v(n);
  long long t = 0;
  float *md = nullptr, *vd = nullptr;
  CK(hipMalloc(&md, n * sizeof(float)));
  CK(hipMalloc(&vd, n * sizeof(float)));
  if (opt.copy_state(n, md, vd, &t, nullptr) != PNPX_OK) return 2;
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out.data(), live.p(), n * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(out.data() + n, md, n * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(out.data() + 2 * n, vd, n * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(norm, slot, sizeof(float), hipMemcpyDeviceToHost));
  out[3 * n] = (float)t;
  CK(hipFree(gd));
  CK(hipFree(slot));
  CK(hipFree(md));
  CK(hipFree(vd));
  opt.free();
  live.free();
  return 0;
}

int main() {
  const size_t sizes[3] = {1003, 4096 + 2, 300001};
  for (size_t n : sizes) {
    // ranges with every alignment of start and end, a one-element range, one inside a single chunk, one ending in the 4-byte tail
    std::vector<FrozenRange> tab = {{1, 2}, {5, 3}, {9, 1}, {14, 9}, {41, 2}, {100, 401}, {600, 4}, {n - 2, 1}};
    std::vector<float> p0(n), g(n), gz(n);
    unsigned s = 12345u + (unsigned)n;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)((s >> 8) & 0xffff) / 32768.f - 1.f; };
    for (size_t i = 0; i < n; ++i) {
      p0[i] = rnd();
      g[i] = gz[i] = rnd() * 3.f;
    }
    for (const auto& r : tab)
      for (size_t i = r.first; i < r.first + r.count; ++i) {
        gz[i] = 0.f;
        g[i] = (i % 3 == 0) ? INFINITY : (i % 3 == 1 ? NAN : 1e30f);
      }
    std::vector<float> ref, a;
    float nref = 0.f, na = 0.f;
    if (run(p0, gz, nullptr, 0, false, ref, &nref)) return 2;
    for (int un = 0; un < 2; ++un) {
      if (run(p0, g, tab.data(), (int)tab.size(), un != 0, a, &na)) return 2;
      const bool same = std::memcmp(ref.data(), a.data(), ref.size() * sizeof(float)) == 0 && std::memcmp(&nref, &na, 4) == 0;
      size_t moved = 0;
      for (size_t i = 0; i < n; ++i) moved += ref[i] != p0[i];
      printf("n %zu, %s gradient: norm %.6f (reference %.6f), %zu of %zu parameters moved, step %g: %s\n", n, un ? "unaligned" : "aligned", na, nref,
             moved, n, a[3 * n], same ? "SAME BYTES" : "DIFFERENT");
      if (!same || !std::isfinite(na)) return 1;
    }
    // and the reference itself through the 4-byte path
    if (run(p0, gz, nullptr, 0, true, a, &na)) return 2;
    if (std::memcmp(ref.data(), a.data(), ref.size() * sizeof(float)) != 0) { printf("reference: 4-byte path differs\n"); return 1; }
  }
  printf("frozen ranges: ok\n");
  return 0;
}
