// Winograd F(4x4, 3x3) on the exact-fp32 MFMA v_mfma_f32_16x16x4_f32: 36 products per 16 outputs instead of F(2x2)'s 16 per 4
// = 0.5625 x the MFMAs of conv3x3_wino8.hip.  64-cout-tile layers of the UNet's forward passes only: the plain single-source layers
// (option fp32_winof4_layers) and, as a second instance, the two-source decoder entries on an already up-sampled second source (option
// fp32_winof4_entries) or, as a third, on the low-resolution second source itself, up-sampled in the kernel (option fp32_winof4_fuse_up); and, as a
// separate kernel of the same per-wave structure on a 32-cout tile, the full-resolution 32 -> 32 layers (conv3x3_winof4_c32_f32_kernel
// below, option fp32_winof4_c32).  What the two kernels share stands once in front of them -- geometry (GeoF4), work decode, halo gather,
// input transform, a stage's MFMA block, accumulator clear, epilogue -- and each kernel keeps its own stage pipeline.  No residual, no
// K-split, no out-conv.  Same activation layout (padded planar fp32), WinoArgs, bias + LeakyReLU as max(y, slope y) and optional fused
// 2x2 max-pool as the F(2x2) kernels.
//
// Points (0, +-1, +-1/2, inf), rows scaled as tools/wino_f4_probe.py's cook_toom does (winof4_mats.h holds the matrices the packer uses;
// tests/test_winof4_pack.py checks them against a direct convolution).
//
// Geometry.  A workgroup (512 threads = 8 waves, two per SIMD, the whole LDS) owns 64 couts x a region of 16 x 32 px = 32 tiles of 4 x 4
// (4 tile rows x 8 tile columns).  The 16x16x4 MFMA keeps a 16 cout x 16 tile block in FOUR registers, so all 36 positions of such a
// block are 144 registers and live in ONE wave: wave (P, sw) -- P = wave / 4, sw = wave % 4, waves sw and sw + 4 share a SIMD -- owns
// couts 16 * (2 * (sw & 1) + P) .. + 15 and tiles 16 * (sw / 2) .. + 15.  The output transform A^T M A is then wave-local: no exchange
// through LDS and no barrier in the epilogue.  (Splitting the position COLUMNS over the SIMD's pair instead, as conv3x3_wino8.hip does,
// would share each V operand between two MFMAs -- 25 % fewer LDS operand bytes, at 256 B/clk not the limit here -- and pay for it with a
// 96 KB exchange per tile.)  C/D layout: tile = lane & 15, cout = 4 * (lane >> 4) + register: a finished cout row of a tile is four
// contiguous pixels = one 16-byte store.
//
// Pipeline.  8-channel chunks, two position rows per stage = 3 stages per chunk, 24 MFMAs per wave and stage (12 positions x 2 k-steps),
// operands as 16-byte LDS reads (two positions x two k-steps each).  LDS: weights 3 x 24 KiB (ring, stage s of every chunk = slot s, fetched
// two stages ahead by 16-byte LDS-DMA), V 3 x 12 KiB (stage s = slot s, written one stage ahead by the input transform), raw halo
// 2 x 23 KiB, fetched three stages ahead by LDS-DMA.  One counted vmcnt wait and one barrier per stage.  The accumulators and the stage
// schedule are the compiler's (MFMA builtins; at two waves per SIMD every value lives in the 256 architectural VGPRs, there are no AGPRs).
//
// Halo.  An LDS-DMA piece costs its issue slot whatever its width, so the halo of a chunk is fetched as 16-byte row gathers of the
// ALIGNED super-window: padded columns x0 .. x0 + RW + 7 (x0 a multiple of the region width, Wp and Hp Wp multiples of 4: every unit is
// 16-byte aligned at both ends and stays inside the padded plane) of rows y0 .. y0 + 17, 10 / 18 units per row, planes 18 rows + 16
// floats apart (= 32 mod 64 banks: the transform's 16-byte reads are conflict-free).  A chunk's LDS image is one linear run: 22 / 40
// whole 16-byte instructions (64 units = 1 KiB) and 4 dword instructions for the rest = 26 / 44 per chunk where the dword form (18 x 34
// / 18 x 66 per channel in rows of 40 / 72, + 2 floats per plane, the halo columns alone) needs 91 / 163; halo column hx sits at LDS
// column hx + 3, and the transform reads a tile's six columns as 8 + 16 + 8 bytes (12 LDS cycles a row against the dword form's 6: the
// one cost the form adds).  GeoF4 holds both forms and the plan (which lane moves what where) as host-visible functions
// (pnpx_winof4_halo_plan; tests/test_winof4_halo_host.py); the plain, two-source and 32-cout instances carry the 16-byte form, the
// up-sampling instance the dword form (WINOF4_H16 below).  What remains for these kernels: the weight ring (one stage of lead in the
// 32-cout kernel, weights re-fetched per region) and, for F(2x2), the 32-cout tile's LDS budget.
#include <cmath>
#include <mutex>
#include <utility>
#include <vector>

#include "common.h"
#include "conv3x3.h"
#include "wino_common.h"
#include "winof4_mats.h"

namespace pnpx {

namespace {

using namespace wino;

// Geometry of an instance: a workgroup owns CT couts x a region of 16 x RW px = RW tiles of 4 x 4 (4 tile rows x RW / 4 tile columns)
// and keeps rings of NS weight stages and NS V stages in front of two raw halo buffers.  (64, 32, 3) / (32, 64, 2) in the comments.
template <int CT_, int RW_, int NS, bool H16_>
struct GeoF4 {
  static constexpr int CT = CT_, RW = RW_, CK = 8;
  static constexpr bool H16 = H16_;                       // the halo as 16-byte row gathers of the aligned super-window (below), else as dword gathers
  static constexpr int RWL = RW + 8;                      // LDS row stride of the halo: tile rows land 32 banks apart (4 * RWL = 32 mod 64)
  // The fetched window.  Dword gathers: padded columns x0 + 3 .. of a region at x0 = the RW + 2 halo columns themselves.  16-byte gathers:
  // padded columns x0 .. x0 + RWL - 1, whole rows of RWL / 4 aligned units (x0 is a multiple of RW, Wp and Hp Wp of 4; the window ends at
  // Wp - 1 in the last region); halo column hx then sits at LDS column hx + 3.
  static constexpr int ORG = H16 ? 0 : PADL - 1;          // padded column of the window's column 0, from x0
  static constexpr int HCOL = PADL - 1 - ORG;             // LDS column of halo column 0
  // LDS plane stride.  Dword form: + 2, odd channels land on the bank pairs the even ones leave free (8-byte reads).  16-byte form: = 32
  // mod 64, the transform's 16-byte reads of a lane group (8 tiles x an even and an odd channel) then cover all 64 banks once.
  static constexpr int RPXL = 18 * RWL + (H16 ? 16 : 2);
  static constexpr int RAW_ELEMS = H16 ? (CK - 1) * RPXL + 18 * RWL : CK * RPXL;      // floats the gathers cover (16-byte form: not the last plane's slack)
  static constexpr int N16 = H16 ? RAW_ELEMS / 256 : 0;                               // whole 16-byte gathers (64 units = 1 KiB): 22 / 40
  static constexpr int N4 = (RAW_ELEMS - 256 * N16 + 63) / 64;                        // dword gathers of the rest: 4 / 4 (dword form: 91 / 163)
  static constexpr int RAW_INSTR = N16 + N4;                 // 26 / 44 (dword form: 91 / 163); instruction i is wave i % 8's gather i / 8
  static constexpr int RAW_BYTES = N16 * 1024 + N4 * 256;    // 23552 / 41984 (23296 / 41728): a chunk's image is one linear run
  static constexpr int RAW_PER_WAVE = (RAW_INSTR + 7) / 8;   // 4 / 6 (12 / 21), of which the last exists for the first RAW_INSTR % 8 waves only
  static constexpr int NRAW = RAW_INSTR / 8;                 // 3 / 5 (11 / 20): gathers every wave issues = what the counted waits assume
  static constexpr int USTG = 2 * 6 * CK * CT * 4;        // bytes of one stage of weights (two position rows): 24 / 12 KiB
  static constexpr int VSTG = 2 * 6 * CK * RW * 4;        // bytes of one stage of V: 12 / 24 KiB
  static constexpr int UCP = USTG / 6, VCP = VSTG / 6;    // ... of one column pair of a position row: 16 bytes per lane and 16-cout / 16-tile block
  static constexpr int OFF_U = 0, OFF_V = NS * USTG, OFF_RAW = OFF_V + NS * VSTG;
  static constexpr int LDS_USED = OFF_RAW + 2 * RAW_BYTES;   // 157696 / 157696
  static_assert(RPXL % 4 == 0 || !H16, "16-byte units must not straddle planes");
  static_assert(RAW_PER_WAVE <= NRAW + 1 && NRAW >= 1, "the waits count NRAW gathers per wave; a wave issues at most one more");

  // -- the halo plan, shared by the kernels and the host (pnpx_winof4_halo_plan).  Instruction i writes a linear run of 64 lanes x
  // width(i) bytes at dst(i) of the halo buffer; lane's piece starts at float first(i, lane) of the buffer's image.
  static constexpr __host__ __device__ int width(int i) { return i < N16 ? 16 : 4; }
  static constexpr __host__ __device__ int dst(int i) { return i < N16 ? i * 1024 : N16 * 1024 + (i - N16) * 256; }
  static constexpr __host__ __device__ int first(int i, int lane) { return dst(i) / 4 + lane * (width(i) / 4); }
  // byte offset of lane's source from the chunk's origin (channel 0, padded row y0, padded column x0 + ORG); lanes in the rows' and
  // planes' slack or behind the last plane are dummies: they read the origin itself and land where nothing reads
  static __host__ __device__ unsigned src(int i, int lane, int HpWp, int Wp, bool* real = nullptr) {
    const int f = first(i, lane);
    const int c = f / RPXL, r = f - c * RPXL;
    const int hy = r / RWL, col = r - hy * RWL;
    const bool ok = c < CK && hy < 18 && (H16 || col < RW + 2);
    if (real) *real = ok;
    return ok ? 4u * (unsigned)(c * HpWp + hy * Wp + col) : 0u;
  }
  // byte offset in the halo buffer of halo element (channel c of the chunk, row hy, column hx): where the transform reads it
  static constexpr __host__ __device__ int at(int c, int hy, int hx) { return (c * RPXL + hy * RWL + hx + HCOL) * 4; }
};
// Which instances carry the 16-byte gathers: a compile-time property of the instance, no run-time option.  The plain, the two-source
// and the 32-cout instance do; the up-sampling instance (bit 2) gathers only its first source's chunks, did not gain and keeps the
// dword form (profiles/winof4_halo16.md has the per-layer rows).  -DWINOF4_H16=mask: timing A/B builds.
#ifndef WINOF4_H16
#define WINOF4_H16 11
#endif
constexpr bool H16_PLAIN = WINOF4_H16 & 1, H16_ENTRY = WINOF4_H16 & 2, H16_UPS = WINOF4_H16 & 4, H16_C32 = WINOF4_H16 & 8;
template <bool H16>
struct CfgF4T : GeoF4<64, 32, 3, H16> {
  using G = GeoF4<64, 32, 3, H16>;
  static constexpr int NUW = G::USTG / 8192;              // 16-byte LDS-DMA instructions per wave and stage: 3
  // UPS instance: a V ring of TWO slots (below) makes room for two staging windows of the low-resolution second source -- 11 rows x 20
  // columns per channel, [channel quad 2][row][column][channel 4] so that a halo pixel's tap is one 16-byte read per quad -- and the
  // per-tile interpolation tables (18 halo rows + 34 halo columns, 16 bytes each)
  static constexpr int SR = 11, SC = 20;
  static constexpr int QPLANE = SR * SC * 16;                // bytes of one channel quad's window: 3520
  static constexpr int ST_INSTR = (2 * QPLANE + 255) / 256;  // dword gathers of 64 lanes: 28 (the last one half used)
  static constexpr int ST_STRIDE = ST_INSTR * 256;           // 7168
  static constexpr int ST_PER_WAVE = (ST_INSTR + 7) / 8;     // 4, of which the last exists for the first ST_INSTR % 8 waves only
  static constexpr int NST = ST_INSTR / 8;                   // 3: gathers every wave issues
  static constexpr int OFF_RAW_UPS = G::OFF_V + 2 * G::VSTG, OFF_ST = OFF_RAW_UPS + 2 * G::RAW_BYTES, OFF_TAB = OFF_ST + 2 * ST_STRIDE;
  static constexpr int LDS_USED_UPS = OFF_TAB + (18 + 34) * 16;   // 160576 (dword form: 160064)
  // VMEM operations a stage may leave in flight, per wave and the smallest any wave issues: its own weight slice and, around stage 2,
  // the halo gathers / (UPS) staging gathers issued behind it.  vmcnt counts loads and LDS-DMA alike, in issue order.
  static constexpr int WAIT_U = NUW, WAIT_HALO = NUW + G::NRAW, WAIT_ST = NUW + NST, WAIT_HALO_ST = NUW + G::NRAW + NST;
  static_assert(WAIT_HALO_ST <= 63, "vmcnt is six bits");
};
constexpr int LDS_REQF4 = 160 * 1024;
// -DWINOF4_ABL=bits (timing only, results wrong; tools/build_variant.sh): 1 no input transform, 2 no halo gathers, 4 no weight DMA,
// 8 no epilogue, 16 no MFMAs, 32 epilogue without its global stores
#ifndef WINOF4_ABL
#define WINOF4_ABL 0
#endif
// -DWINOF4_HSTEP=n (timing A/B of placements): 16-byte halo gather k of a wave stands n MFMAs behind gather k - 1; 0 = the shipped placement
#ifndef WINOF4_HSTEP
#define WINOF4_HSTEP 0
#endif
static_assert(CfgF4T<false>::LDS_USED <= LDS_REQF4 && CfgF4T<false>::LDS_USED_UPS <= LDS_REQF4 && CfgF4T<true>::LDS_USED <= LDS_REQF4 &&
              CfgF4T<true>::LDS_USED_UPS <= LDS_REQF4, "LDS budget");

// row A of B^T applied to six values (points 0, +-1, +-1/2, inf; winof4_mats.h WINOF4_BT)
template <int A>
__device__ __forceinline__ float bt_row(float d0, float d1, float d2, float d3, float d4, float d5) {
  if (A == 0) return fmaf(0.25f, d0, fmaf(-1.25f, d2, d4));
  if (A == 1) return fmaf(-0.25f, d2, d4) + fmaf(-0.25f, d1, d3);
  if (A == 2) return fmaf(-0.25f, d2, d4) - fmaf(-0.25f, d1, d3);
  if (A == 3) return fmaf(0.5f, d3 - d1, d4 - d2);
  if (A == 4) return fmaf(-0.5f, d3 - d1, d4 - d2);
  return fmaf(0.25f, d1, fmaf(-1.25f, d3, d5));
}
// A^T applied to six values (WINOF4_AT): four sums
__device__ __forceinline__ void at_rows(float m0, float m1, float m2, float m3, float m4, float m5, float& o0, float& o1, float& o2, float& o3) {
  const float p12 = m1 + m2, m12 = m1 - m2, p34 = m3 + m4, m34 = m3 - m4;
  o0 = (m0 + p12) + p34;
  o1 = fmaf(0.5f, m34, m12);
  o2 = fmaf(0.25f, p34, p12);
  o3 = fmaf(0.125f, m34, m12) + m5;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The pieces both kernels run, written once.  What differs between the instances reaches them as a geometry (C), as addresses or as
// the caller's own callable; the stage schedules, the weight DMA and the up-sampling stay with the kernels.

// -- work decode: the XCD-grouped walk over (region, cout tile) as conv3x3_wino8.hip (siblings share the halo in L2)
struct Walk {
  int nregions, nx, xcd, slot, nslot;
};
__device__ __forceinline__ Walk make_walk(const WinoArgs& a) {
  Walk wk;
  wk.nregions = a.rx * a.ry * a.B;
  wk.nx = (gridDim.x % 8 == 0 && wk.nregions >= 32) ? 8 : 1;
  wk.xcd = blockIdx.x % wk.nx;
  wk.slot = blockIdx.x / wk.nx;
  wk.nslot = gridDim.x / wk.nx;
  return wk;
}
struct Tile {
  const float* s0;   // halo origin in channel 0
  const float* w;    // weights of the cout tile
  int ct, b, x0, y0, ok;
};
template <class C>
__device__ __forceinline__ Tile decode_tile(const WinoArgs& a, const Walk& wk, int HpWp, int k) {      // work item k of this workgroup
  Tile T;
  const int j = wk.slot + wk.nslot * k;
  const int q = j / a.nct;
  T.ct = j - q * a.nct;
  const int reg = wk.nx * q + wk.xcd;
  T.ok = reg < wk.nregions;
  const int t1 = reg / a.rx;
  const int tx = reg - t1 * a.rx;
  const int t2 = t1 / a.ry;
  const int ty = t1 - t2 * a.ry;
  T.b = t2;
  T.x0 = tx * C::RW;
  T.y0 = ty * 16;
  T.s0 = a.in0 + (size_t)T.b * a.C0 * HpWp + (size_t)T.y0 * a.Wp + T.x0 + C::ORG;
  T.w = a.u + (size_t)T.ct * a.nch * 3 * (C::USTG / 4);
  return T;
}

__device__ __forceinline__ void sync_all() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// -- halo gather by LDS-DMA, an eighth per wave, after the geometry's plan (C::src / C::dst / C::width): instruction wave + 8 k is the
// wave's gather k, 16 bytes per lane while whole ones last and dwords for the rest; raw0 = LDS address of halo buffer 0
template <class C>
struct HaloGather {
  unsigned roff[C::RAW_PER_WAVE];
  unsigned raw0;
  int wave;
  __device__ __forceinline__ HaloGather(const WinoArgs& a, int HpWp, unsigned raw0_, int wave_, int lane) : raw0(raw0_), wave(wave_) {
#pragma unroll
    for (int k = 0; k < C::RAW_PER_WAVE; ++k) roff[k] = C::src(wave + 8 * k, lane, HpWp, a.Wp);
  }
  __device__ __forceinline__ void piece(const float* src, int rbuf, int k) const {      // gather k (of RAW_PER_WAVE per wave) of one chunk's halo
    if (WINOF4_ABL & 2) return;
    const int i = wave + 8 * k;
    if (k >= C::NRAW && i >= C::RAW_INSTR) return;
    const unsigned to = raw0 + rbuf * C::RAW_BYTES + C::dst(i);
    if (8 * k + 7 < C::N16 || (8 * k < C::N16 && i < C::N16)) glds16(src, roff[k], to);      // (the wave's index is uniform: a scalar branch)
    else glds4(src, roff[k], to);
  }
  __device__ __forceinline__ void all(const float* src, int rbuf) const {
#pragma unroll
    for (int k = 0; k < C::RAW_PER_WAVE; ++k) piece(src, rbuf, k);
  }
};

// -- input transform of one tile and one channel: position row A of B^T d B from the tile's 6 x 6 halo window at rb = C::at(channel,
// 4 tile row, 4 tile column) (rows RWL floats apart) to vb, the three column pairs VCP bytes apart.  Dword-gathered halo: the window's
// row starts 8-byte aligned, three 8-byte reads.  16-byte-gathered halo: it starts at LDS column 3 mod 4, so 8 bytes (second half used)
// + an aligned 16 + 8 (first half used); two 4-byte reads instead of the 8-byte ones would run four-way into banks (a / 4) mod 32.
template <int A, class C>
__device__ __forceinline__ void transform_tile(const char* rb, char* vb) {
  constexpr int RWL = C::RWL, VCP = C::VCP;
  float d[6][6];
#pragma unroll
  for (int y = 0; y < 6; ++y) {
    const bool need = (A == 0) ? (y % 2 == 0) : (A == 5) ? (y % 2 == 1) : (y >= 1 && y <= 4);
    if (!need) {
#pragma unroll
      for (int x = 0; x < 6; ++x) d[y][x] = 0.f;
    } else if constexpr (C::H16) {
      const f32x2 l = *reinterpret_cast<const f32x2*>(rb + (y * RWL - 1) * 4);
      const f32x4 m = *reinterpret_cast<const f32x4*>(rb + (y * RWL + 1) * 4);
      const f32x2 r = *reinterpret_cast<const f32x2*>(rb + (y * RWL + 5) * 4);
      d[y][0] = l[1];
      d[y][1] = m[0];
      d[y][2] = m[1];
      d[y][3] = m[2];
      d[y][4] = m[3];
      d[y][5] = r[0];
    } else {
#pragma unroll
      for (int x = 0; x < 6; x += 2) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(rb + (y * RWL + x) * 4);
        d[y][x] = v[0];
        d[y][x + 1] = v[1];
      }
    }
  }
  float t[6];
#pragma unroll
  for (int x = 0; x < 6; ++x) t[x] = bt_row<A>(d[0][x], d[1][x], d[2][x], d[3][x], d[4][x], d[5][x]);
  *reinterpret_cast<f32x2*>(vb) = (f32x2){bt_row<0>(t[0], t[1], t[2], t[3], t[4], t[5]), bt_row<1>(t[0], t[1], t[2], t[3], t[4], t[5])};
  *reinterpret_cast<f32x2*>(vb + VCP) = (f32x2){bt_row<2>(t[0], t[1], t[2], t[3], t[4], t[5]), bt_row<3>(t[0], t[1], t[2], t[3], t[4], t[5])};
  *reinterpret_cast<f32x2*>(vb + 2 * VCP) = (f32x2){bt_row<4>(t[0], t[1], t[2], t[3], t[4], t[5]), bt_row<5>(t[0], t[1], t[2], t[3], t[4], t[5])};
}

// -- the 24 MFMAs of stage S (position rows 2 S and 2 S + 1): operands as 16-byte LDS reads = (k-step 2) x (position 2 of a column
// pair) per lane at ua / vb, (row in stage * 3 + column pair) UCP / VCP bytes apart.  piece(m) is the caller's LDS-DMA schedule: one
// call behind MFMA m, so that its issue cost runs under the MFMAs.
template <int S, int UCP, int VCP, class Piece>
__device__ __forceinline__ void mfma_stage(f32x4 (&acc)[6][6], const char* ua, const char* vb, Piece&& piece) {
  f32x4 af[6], bf[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    af[q] = *reinterpret_cast<const f32x4*>(ua + q * UCP);
    bf[q] = *reinterpret_cast<const f32x4*>(vb + q * VCP);
  }
  static_for<6>([&](auto q_tag) {
    constexpr int Q = decltype(q_tag)::value, R = Q / 3, CP = Q % 3;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int pos = 0; pos < 2; ++pos) {
        acc[2 * S + R][2 * CP + pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[Q][2 * ks + pos], bf[Q][2 * ks + pos], acc[2 * S + R][2 * CP + pos], 0, 0, 0);
        piece(4 * Q + 2 * ks + pos);
        __builtin_amdgcn_sched_barrier(0);
      }
  });
}

__device__ __forceinline__ void clear_acc(f32x4 (&acc)[6][6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// -- epilogue, wave-local: Y = A^T M A per accumulator register (= cout cbase + register) of the lane's tile (ty, tx) of region T,
// bias + activation, one 16-byte store per tile row, optional fused 2x2 max-pool
__device__ __forceinline__ void epilogue_tile(const WinoArgs& a, const f32x4 (&acc)[6][6], int HpWp, const Tile& T, int ty, int tx, int cbase) {
  float* ob = a.out + ((size_t)T.b * a.Cout + cbase) * HpWp + (size_t)(T.y0 + 4 * ty + 1) * a.Wp + T.x0 + 4 * tx + PADL;
  const int Hp_pool = padded_h(a.H / 2), Wp_pool = padded_w(a.W / 2);
  const size_t HpWp_pool = (size_t)Hp_pool * Wp_pool;
  float* pb = a.pool ? a.pool + ((size_t)T.b * a.Cout + cbase) * HpWp_pool + (size_t)(T.y0 / 2 + 2 * ty + 1) * Wp_pool + T.x0 / 2 + 2 * tx + PADL : nullptr;
  float bias4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias4[j] = a.bias[cbase + j];
  static_for<4>([&](auto j_tag) {
    constexpr int j = decltype(j_tag)::value;
    float s[4][6];
#pragma unroll
    for (int b = 0; b < 6; ++b) at_rows(acc[0][b][j], acc[1][b][j], acc[2][b][j], acc[3][b][j], acc[4][b][j], acc[5][b][j], s[0][b], s[1][b], s[2][b], s[3][b]);
    const float bias = bias4[j];
    float* o = ob + (size_t)j * HpWp;
    f32x4 y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float y0, y1, y2, y3;
      at_rows(s[i][0], s[i][1], s[i][2], s[i][3], s[i][4], s[i][5], y0, y1, y2, y3);
      y0 += bias;
      y1 += bias;
      y2 += bias;
      y3 += bias;
      // LeakyReLU with 0 <= slope <= 1 as max(y, slope y)
      y[i] = (f32x4){fmaxf(y0, y0 * a.slope), fmaxf(y1, y1 * a.slope), fmaxf(y2, y2 * a.slope), fmaxf(y3, y3 * a.slope)};
      if (!(WINOF4_ABL & 32) || a.slope == 123.f) *reinterpret_cast<f32x4*>(o + i * a.Wp) = y[i];
    }
    if (a.pool && (!(WINOF4_ABL & 32) || a.slope == 123.f)) {      // four 2x2 windows per tile; same association as maxpool2_kernel
      float* p = pb + (size_t)j * HpWp_pool;
      *reinterpret_cast<f32x2*>(p) = (f32x2){fmaxf(fmaxf(y[0][0], y[0][1]), fmaxf(y[1][0], y[1][1])), fmaxf(fmaxf(y[0][2], y[0][3]), fmaxf(y[1][2], y[1][3]))};
      *reinterpret_cast<f32x2*>(p + Wp_pool) = (f32x2){fmaxf(fmaxf(y[2][0], y[2][1]), fmaxf(y[3][0], y[3][1])), fmaxf(fmaxf(y[2][2], y[2][3]), fmaxf(y[3][2], y[3][3]))};
    }
  });
}

// TWO: the channel chunks C0 / 8 .. of a tile come from in1 (C1 channels, same geometry as in0); the weights are packed over C0 + C1 and
// a.nch counts both sources' chunks.  A chunk lies in one source (C0 % 8 == 0), so only its halo origin differs.
//
// UPS (with TWO): in1 is the LOW-resolution second source (C1 channels at H/2 x W/2, padded planar) and the kernel interpolates its
// bilinear x2 (align_corners) itself, to the bits upsample2x_v4_kernel (unet.hip) writes.  A chunk of the second source never goes through
// the halo gathers: the low-resolution window of its 18 x 34 halo is staged by dword LDS-DMA (issued in stage 2 of the chunk three before
// it, beside the halo gathers of the chunk two before it, and waited for with them) and interpolated into the raw halo buffer in the side
// work of the three stages that buffer is free: stage 2 of the chunk two before (channels 0-3 of halo pixels 0 .. 511), stage 0 (channels
// 4-7 of them) and stage 1 (pixels 512 .. 611, two channels per thread) of the chunk before -- every wave the same amount.  From the
// halo buffer on nothing differs.  The V ring has two slots here (stage g reads slot g & 1 and writes the other one; the barrier between
// two stages separates a slot's last read from its next write), which is where the staging windows' LDS comes from.
template <bool TWO, bool UPS = false, bool H16 = false>
__global__ __launch_bounds__(512, 1) void conv3x3_winof4_f32_kernel(WinoArgs a) {
  static_assert(TWO || !UPS, "the up-sampled source is the second one");
  using C = CfgF4T<H16>;
  constexpr int CK = C::CK, RPXL = C::RPXL, RAW_BYTES = C::RAW_BYTES, RAW_PER_WAVE = C::RAW_PER_WAVE;
  constexpr int USTG = C::USTG, NUW = C::NUW, VSTG = C::VSTG, OFF_U = C::OFF_U, OFF_V = C::OFF_V, OFF_RAW = UPS ? C::OFF_RAW_UPS : C::OFF_RAW;
  constexpr int SC = C::SC, QPLANE = C::QPLANE, ST_STRIDE = C::ST_STRIDE, ST_PER_WAVE = C::ST_PER_WAVE, OFF_ST = C::OFF_ST, OFF_TAB = C::OFF_TAB;
  constexpr int UQ = USTG / 4;      // floats per weight stage
  // stage 2's halo gathers stand behind MFMAs 4, 4 + HSTEP, ..: the few 16-byte ones spread (UPS: short of the staging pieces at 16),
  // the dword ones one behind each MFMA as they always did
  constexpr int HSTEP = !H16 ? 1 : WINOF4_HSTEP > 0 ? WINOF4_HSTEP : UPS ? 3 : 4;
  static_assert(4 + HSTEP * (RAW_PER_WAVE - 1) < (UPS && H16 ? 16 : 24), "halo pieces behind the stage's MFMAs");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sw = wave & 3;
  const int HpWp = a.Hp * a.Wp;
  const unsigned lds0 = (unsigned)(size_t)(lptr_t)lds;
  const Walk wk = make_walk(a);

  struct Tile2 : Tile {
    const float* s1;   // halo origin of the second source (TWO)
    int rs, cs;        // UPS: padded row / column of the low-resolution tensor at which the tile's staging window starts (s1 points there)
  };
  struct UpsStage {      // UPS: what differs from chunk to chunk in a pipeline stage
    int vrd;             // V slot the stage reads; its transform writes the other one
    int wait_n;          // stages 0 and 2: VMEM operations the stage may leave in flight
    bool raw, st, ip;    // stage 2 gathers the halo of the chunk after next / stages the chunk three ahead; the stage's interpolation step runs
    const float* st_src;
    int st_buf, ip_sbuf, ip_rbuf;
  };
  // UPS: geometry of the low-resolution source
  const int h_lo = a.ups_h, w_lo = a.ups_w, hp_lo = padded_h(a.ups_h), wp_lo = padded_w(a.ups_w), hpwp_lo = hp_lo * wp_lo;
  auto decode = [&](int k) {
    Tile2 T;
    static_cast<Tile&>(T) = decode_tile<C>(a, wk, HpWp, k);
    if constexpr (UPS) {
      // The window starts at the first tap of the first halo row / column inside the image (the taps' indices grow with the halo index:
      // 18 rows span at most 10 source rows + the second tap, 34 columns at most 18 + 1), pulled back so that its SR rows and SC columns
      // stay inside the padded plane; a plane of fewer than SR rows (h = 8) repeats its last row instead (stoff below).
      const int rl = (int)__fmul_rn(a.ups_sy, (float)max(T.y0 - 1, 0)) + 1, cl = (int)__fmul_rn(a.ups_sx, (float)max(T.x0 - 1, 0)) + PADL;
      T.rs = min(rl, max(hp_lo - C::SR, 0));
      T.cs = min(cl, wp_lo - SC);
      T.s1 = a.in1 + (size_t)T.b * a.C1 * hpwp_lo + (size_t)T.rs * wp_lo + T.cs;
    } else {
      T.rs = T.cs = 0;
      T.s1 = TWO ? a.in1 + (size_t)T.b * a.C1 * HpWp + (size_t)T.y0 * a.Wp + T.x0 + C::ORG : nullptr;
    }
    return T;
  };
  const int nch0 = a.C0 / CK;      // chunks of the first source
  auto raw_of = [&](const Tile2& X, int c) {
    if (TWO && !UPS && c >= nch0) return X.s1 + (size_t)CK * (c - nch0) * HpWp;
    return X.s0 + (size_t)CK * c * HpWp;
  };
  auto st_of = [&](const Tile2& X, int c) { return X.s1 + (size_t)CK * (c - nch0) * hpwp_lo; };      // UPS: window origin of second-source chunk c

  const HaloGather<C> halo(a, HpWp, lds0 + OFF_RAW, wave, lane);
  const unsigned uoff = lane * 16u;
  auto dma_u_piece = [&](const float* src, int uslot, int k) {     // piece k (of NUW per wave) of one stage's weights -> ring slot uslot
    if (WINOF4_ABL & 4) return;
    glds16(src + wave * 256 + k * 2048, uoff, lds0 + OFF_U + uslot * USTG + (wave + 8 * k) * 1024);
  };
  auto dma_u = [&](const float* src, int uslot) {
#pragma unroll
    for (int k = 0; k < NUW; ++k) dma_u_piece(src, uslot, k);
  };

  // -- UPS: the staging window of a second-source chunk, an eighth per wave: per-lane byte offsets from the window's origin in the
  // chunk's channel 0 (lanes past the window read its first element into the slack behind it)
  unsigned stoff[UPS ? ST_PER_WAVE : 1];
  if constexpr (UPS) {
#pragma unroll
    for (int k = 0; k < ST_PER_WAVE; ++k) {
      const int idx = (wave + 8 * k) * 64 + lane;
      const int e = idx & 3, g = idx >> 2;
      const int sc = g % SC, g2 = g / SC;
      const int sr = g2 % C::SR, q = g2 / C::SR;
      stoff[k] = (q < CK / 4) ? 4u * (unsigned)((4 * q + e) * hpwp_lo + min(sr, hp_lo - 1) * wp_lo + sc) : 0u;
    }
  }
  auto dma_st_piece = [&](const float* src, int sbuf, int k) {      // gather k (of ST_PER_WAVE per wave) of one chunk's window
    if (WINOF4_ABL & 2) return;
    if (k < C::NST || wave + 8 * k < C::ST_INSTR) glds4(src, stoff[UPS ? k : 0], lds0 + OFF_ST + sbuf * ST_STRIDE + (wave + 8 * k) * 256);
  };
  // Per-tile tables of the interpolation, halo rows 0 .. 17 then halo columns 0 .. 33: (byte offset of the first tap in a staging plane,
  // its weight h, the second tap's weight l, byte offset of the second tap); h = -1 marks a row / column outside the image (the
  // convolution's zero padding).  The floats are upsample2x_v4_kernel's, operation by operation (its disassembly: no contraction here):
  // f = s * index, i0 = (int) f, l = f - i0, h = 1 - l, second tap i0 + (i0 < n - 1).
  auto write_tables = [&](const Tile2& X) {
    if (tid < 18 + 34) {
      const bool row = tid < 18;
      const int g = (row ? X.y0 : X.x0) - 1 + (row ? tid : tid - 18);      // image coordinate of the halo row / column
      const bool valid = g >= 0 && g < (row ? a.H : a.W);
      const float f = __fmul_rn(row ? a.ups_sy : a.ups_sx, (float)g);
      const int i0 = (int)f;
      const int i1 = i0 + (i0 < (row ? h_lo : w_lo) - 1 ? 1 : 0);
      const float l = __fsub_rn(f, (float)i0), h = __fsub_rn(1.f, l);
      f32x4 ent;
      ent[0] = __int_as_float(valid ? (row ? (i0 + 1 - X.rs) * SC * 16 : (i0 + PADL - X.cs) * 16) : 0);
      ent[1] = valid ? h : -1.f;
      ent[2] = valid ? l : 0.f;
      ent[3] = __int_as_float(valid ? (row ? (i1 + 1 - X.rs) * SC * 16 : (i1 + PADL - X.cs) * 16) : 0);
      *reinterpret_cast<f32x4*>(lds + OFF_TAB + tid * 16) = ent;
    }
  };
  // One interpolated value, in upsample2x_v4_kernel's rounding sequence (read in its disassembly): the products with l round on their own,
  // the products with h are fused into them: fma(hy, fma(hx, v00, lx v01), ly fma(hx, v10, lx v11))
  auto blend = [](float hy, float ly, float hx, float lx, float v00, float v01, float v10, float v11) {
    return fmaf(hy, fmaf(hx, v00, __fmul_rn(lx, v01)), __fmul_rn(ly, fmaf(hx, v10, __fmul_rn(lx, v11))));
  };
  // The three steps of a chunk's interpolation from staging window sbuf into halo buffer rbuf.  Steps 0 and 1: halo pixel `tid`, channel
  // quad 0 / 1 (four 16-byte taps, four values).  Step 2: the remaining 100 pixels 512 + tid / 4, channels 2 (tid % 4) and + 1 (four
  // 8-byte taps, two values; threads 400 .. repeat the last pixel).  A pixel outside the image gets +0 and forms no product.
  auto interp = [&](auto step_tag, int sbuf, int rbuf) {
    constexpr int STEP = decltype(step_tag)::value;
    if (WINOF4_ABL & 1) return;
    const int pix = STEP < 2 ? tid : min(512 + (tid >> 2), 18 * 34 - 1);
    const int hyi = pix / 34, hxi = pix - hyi * 34;
    const f32x4 rt = *reinterpret_cast<const f32x4*>(lds + OFF_TAB + hyi * 16);
    const f32x4 ct = *reinterpret_cast<const f32x4*>(lds + OFF_TAB + (18 + hxi) * 16);
    const bool inside = rt[1] >= 0.f && ct[1] >= 0.f;
    const int r0 = __float_as_int(rt[0]), r1 = __float_as_int(rt[3]), c0 = __float_as_int(ct[0]), c1 = __float_as_int(ct[3]);
    char* ob = lds + OFF_RAW + rbuf * RAW_BYTES + C::at(0, hyi, hxi);
    if (STEP < 2) {
      const char* sb = lds + OFF_ST + sbuf * ST_STRIDE + STEP * QPLANE;
      const f32x4 v00 = *reinterpret_cast<const f32x4*>(sb + r0 + c0), v01 = *reinterpret_cast<const f32x4*>(sb + r0 + c1);
      const f32x4 v10 = *reinterpret_cast<const f32x4*>(sb + r1 + c0), v11 = *reinterpret_cast<const f32x4*>(sb + r1 + c1);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        *reinterpret_cast<float*>(ob + (4 * STEP + e) * RPXL * 4) = inside ? blend(rt[1], rt[2], ct[1], ct[2], v00[e], v01[e], v10[e], v11[e]) : 0.f;
    } else {
      const int ch = 2 * (tid & 3);
      const char* sb = lds + OFF_ST + sbuf * ST_STRIDE + (ch >> 2) * QPLANE + (ch & 3) * 4;
      const f32x2 v00 = *reinterpret_cast<const f32x2*>(sb + r0 + c0), v01 = *reinterpret_cast<const f32x2*>(sb + r0 + c1);
      const f32x2 v10 = *reinterpret_cast<const f32x2*>(sb + r1 + c0), v11 = *reinterpret_cast<const f32x2*>(sb + r1 + c1);
#pragma unroll
      for (int e = 0; e < 2; ++e)
        *reinterpret_cast<float*>(ob + (ch + e) * RPXL * 4) = inside ? blend(rt[1], rt[2], ct[1], ct[2], v00[e], v01[e], v10[e], v11[e]) : 0.f;
    }
  };

  // The role P = wave / 4 is a compile-time parameter of the whole tile loop (one branch at the top): every stage stays one basic block.
  // The two waves of a SIMD run a stage's two halves in opposite order -- P = 0: MFMAs, then the input transform; P = 1: the input
  // transform, then MFMAs -- so that one wave's transform runs under the other's 24 MFMAs (24 x 32 clocks) and the matrix pipe never
  // waits for one.  The stage's LDS-DMA pieces are issued between the wave's own MFMAs.
  auto body = [&](auto role_tag) {
  constexpr int P = decltype(role_tag)::value;

  // -- input transform: one tile, one channel and one position row (row P of the stage's two) per thread.  Lanes: k-step bit, 16 tiles,
  // low bit of the channel group (a wave's V writes of a position pair are 512 contiguous bytes); sw: high bit of the channel group,
  // tile block.  Channel = 2 * group + k-step bit (the MFMA's k index is the group).
  const int t_ks = lane & 1, t_t16 = (lane >> 1) & 15, t_kq = (lane >> 5) | ((sw & 1) << 1), t_wn = sw >> 1;
  const int t_tile = t_wn * 16 + t_t16;
  const int t_rd = C::at(2 * t_kq + t_ks, 4 * (t_tile >> 3), 4 * (t_tile & 7));
  const int t_wr = (P * 3 * 2 + t_wn) * 1024 + (t_kq * 16 + t_t16) * 16 + t_ks * 8;       // + column pair * 2048 (+ slot)
  auto transform_row = [&](auto s_tag, int rbuf, int vslot_ups = 0) {      // this thread's row of stage S's two, into V slot S (UPS: vslot_ups)
    constexpr int S = decltype(s_tag)::value;
    if (WINOF4_ABL & 1) return;
    transform_tile<2 * S + P, C>(lds + OFF_RAW + rbuf * RAW_BYTES + t_rd, lds + OFF_V + (UPS ? vslot_ups : S) * VSTG + t_wr);
  };

  // -- MFMA operands: 16 bytes = (k-step 2) x (position 2 of a column pair) per lane; lane = 16 * channel group + cout / tile of the block
  const int mb = 2 * (sw & 1) + P, wn = sw >> 1;
  const int a_lane = mb * 1024 + lane * 16;      // + (row in stage * 3 + column pair) * 4096 (+ slot)
  const int b_lane = wn * 1024 + lane * 16;      // + (row in stage * 3 + column pair) * 2048 (+ slot)
  f32x4 acc[6][6];

  // One pipeline stage S of a chunk: fetch the weights of the stage after next (and, S == 2, the halo of the chunk after next), 24 MFMAs,
  // the input transform of the next stage, then the counted wait (WAITN = VMEM operations issued after the ones the next stage needs)
  // and the barrier.
  // UPS: x holds what differs from chunk to chunk there (the other instances ignore it).
  auto stage = [&](auto s_tag, auto wait_tag, const float* u_src, const float* raw_src, int raw_buf, int t_rbuf, const UpsStage& x) {
    constexpr int S = decltype(s_tag)::value, SN = (S + 1) % 3;
    constexpr int WAITN = decltype(wait_tag)::value;
    auto side = [&]() {
      transform_row(std::integral_constant<int, SN>{}, t_rbuf, x.vrd ^ 1);
      if constexpr (UPS) {      // step 0 in stage 2, step 1 in stage 0, step 2 in stage 1
        if (x.ip) interp(std::integral_constant<int, SN>{}, x.ip_sbuf, x.ip_rbuf);
      }
    };
    // the stage's LDS-DMA pieces, one behind each MFMA (their issue cost then runs under the MFMAs): the weight slice behind MFMAs
    // 0 .. 2, stage 2's halo gathers behind 4, 4 + HSTEP .. (UPS: when the chunk after next is gathered) and, UPS, the staging window
    // of the chunk three ahead behind 16 .. 19
    auto piece = [&](int m) {
      if (m < NUW) dma_u_piece(u_src, (S + 2) % 3, m);
      if (S == 2 && m >= 4 && (m - 4) % HSTEP == 0 && (m - 4) / HSTEP < RAW_PER_WAVE && (!UPS || x.raw)) halo.piece(raw_src, raw_buf, (m - 4) / HSTEP);
      if constexpr (UPS) {
        if (S == 2 && m >= 16 && m < 16 + ST_PER_WAVE && x.st) dma_st_piece(x.st_src, x.st_buf, m - 16);
      }
    };
    auto mfmas = [&]() {
      if (WINOF4_ABL & 16) return;      // (and none of the stage's pieces)
      mfma_stage<S, C::UCP, C::VCP>(acc, lds + OFF_U + S * USTG + a_lane, lds + OFF_V + (UPS ? x.vrd : S) * VSTG + b_lane, piece);
    };
    if (P == 0) {
      mfmas();
      __builtin_amdgcn_sched_barrier(0);
      side();
    } else {
      side();
      __builtin_amdgcn_sched_barrier(0);
      mfmas();
    }
    if constexpr (UPS && S != 1) {
      // The operations behind the weight slice the next stage needs: this stage's slice (stage 0: and, before it, what stage 2 issued
      // behind its own) + NRAW halo gathers when the chunk after next was gathered + NST staging gathers when the chunk three ahead was
      // staged = 3 + {0, NRAW} + {0, 3} (C::WAIT_*).  The count is per wave and the smallest any wave issues, so no wave waits for too
      // little.  Two of the four may coincide (NRAW = NST with the 16-byte gathers): each branch waits for the value it compares with.
      if (x.wait_n == C::WAIT_HALO_ST) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::WAIT_HALO_ST) : "memory");
      else if (x.wait_n == C::WAIT_HALO) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::WAIT_HALO) : "memory");
      else if (x.wait_n == C::WAIT_ST) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::WAIT_ST) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::WAIT_U) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(WAITN) : "memory");
    }
    __builtin_amdgcn_s_barrier();
  };

  // -- epilogue: the lane's tile of the wave's 16 and its four couts
  auto epilogue = [&](const Tile& T) {
    const int tile = wn * 16 + (lane & 15);
    epilogue_tile(a, acc, HpWp, T, tile >> 3, tile & 7, T.ct * 64 + mb * 16 + 4 * (lane >> 4));
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  // VMEM operations a stage may leave in flight: its own weight slice (and, around stage 2, the halo gathers issued behind it)
  using WaitHalo = std::integral_constant<int, C::WAIT_HALO>;
  using WaitU = std::integral_constant<int, C::WAIT_U>;

  int k = 0;
  Tile2 T = decode(0);
  if (!T.ok) return;
  // prologue: the first two halos and weight stages, the first transform
  halo.all(T.s0, 0);
  dma_u(T.w, 0);
  dma_u(T.w + UQ, 1);
  halo.all(raw_of(T, 1), 1);      // (nch >= 2: chunk 1 exists; chunk 0 lies in the first source)
  if constexpr (UPS) {           // (UPS: nch0 >= 2, chunks 0 and 1 are gathered; chunk 2 is staged here when it is the second source's first)
    if (nch0 == 2) {
#pragma unroll
      for (int q = 0; q < ST_PER_WAVE; ++q) dma_st_piece(st_of(T, 2), 0, q);
    }
  }
  sync_all();
  transform_row(I0{}, 0);
  sync_all();

  int cc = 0;
  int wait_prev = NUW;      // UPS: what the last stage 2 left in flight (nothing before the first chunk)
  for (;;) {
    Tile2 Tn = decode(k + 1);
    const bool more = Tn.ok;
    if (!more) Tn = T;      // after the walk's last chunks: surplus loads of this tile's first chunks into buffers nobody reads
    // UPS: the tile's tables.  Their last readers were the previous tile's last interpolation steps, two barriers back; their first
    // reader is stage 2 of chunk nch0 - 2, two barriers ahead.
    if constexpr (UPS) write_tables(T);
    clear_acc(acc);
    for (int c = 0; c < a.nch; ++c, ++cc) {
      const float* w_c = T.w + (size_t)c * 3 * UQ;
      const float* nu = (c + 1 < a.nch) ? w_c + 3 * UQ : Tn.w;                                    // the next chunk's weights
      const float* nraw = (c + 2 < a.nch) ? raw_of(T, c + 2) : raw_of(Tn, c + 2 - a.nch);         // the halo of the chunk after next
      const int rcur = cc & 1;
      if constexpr (UPS) {
        // Chunk c + 1 is interpolated in stages 0 and 1 (into the other halo buffer, from the staging window of its parity), chunk c + 2
        // in stage 2 (into this chunk's halo buffer, free since stage 1's barrier), when they lie in the second source of THIS tile:
        // the next tile's chunks 0 and 1 are gathered (nch0 >= 2).  Chunk c + 3 is staged in stage 2 into the window chunk c + 1 had
        // (last read in stage 1); it may be the next tile's chunk 2.  Halo buffers, staging windows and V slots alternate with the
        // running chunk count cc, which the tile boundary does not reset.
        const bool up1 = c + 1 < a.nch && c + 1 >= nch0, up2 = c + 2 < a.nch && c + 2 >= nch0;
        const bool up3 = c + 3 < a.nch ? c + 3 >= nch0 : c + 3 - a.nch >= nch0;
        const float* nst = c + 3 < a.nch ? st_of(T, c + 3) : st_of(Tn, c + 3 - a.nch);
        const int wait_cur = up2 ? (up3 ? C::WAIT_ST : C::WAIT_U) : (up3 ? C::WAIT_HALO_ST : C::WAIT_HALO);
        UpsStage x{};
        x.ip = up1;
        x.ip_sbuf = x.ip_rbuf = rcur ^ 1;
        x.vrd = rcur;      // stage g = 3 cc + s reads V slot g & 1 = (cc + s) & 1
        x.wait_n = wait_prev;
        stage(I0{}, WaitHalo{}, w_c + 2 * UQ, nullptr, 0, rcur, x);
        x.vrd = rcur ^ 1;
        stage(I1{}, WaitU{}, nu, nullptr, 0, rcur, x);
        x.vrd = rcur;
        x.ip = up2;
        x.ip_sbuf = x.ip_rbuf = rcur;
        x.raw = !up2;
        x.st = up3;
        x.st_src = nst;
        x.st_buf = rcur ^ 1;
        x.wait_n = wait_prev = wait_cur;
        stage(I2{}, WaitHalo{}, nu + UQ, nraw, rcur, rcur ^ 1, x);
        continue;
      }
      // stage g = 3 c + s reads weight and V slot s; the transform behind its MFMAs makes V of stage g + 1 (stage 2: from the next chunk's halo)
      stage(I0{}, WaitHalo{}, w_c + 2 * UQ, nullptr, 0, rcur, UpsStage{});
      stage(I1{}, WaitU{}, nu, nullptr, 0, rcur, UpsStage{});
      stage(I2{}, WaitHalo{}, nu + UQ, nraw, rcur, rcur ^ 1, UpsStage{});
    }
    if (!(WINOF4_ABL & 8)) epilogue(T);
    if (!more) break;
    T = Tn;
    ++k;
  }
  sync_all();   // the surplus loads of the last chunk
  };
  if (wave < 4) body(std::integral_constant<int, 0>{});
  else body(std::integral_constant<int, 1>{});
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The 32-cout instance (option fp32_winof4_c32): the full-resolution 32 -> 32 layers.  What differs from the kernel above: a workgroup
// owns 32 couts x 64 tiles, a region of 16 x 64 px = 4 tile rows x 16 tile columns; wave (P, sw) owns cout block P and tile row sw, so the
// two waves of a SIMD read the same V operands, and a thread transforms two tiles per stage.  LDS: weights 2 x 12 KiB and V 2 x 24 KiB
// (both: stage g of the running stage count reads slot g & 1 and fills the other one for stage g + 1; the barrier between two stages
// separates a slot's last read from its next write), raw halo 2 x 41 KiB (the aligned super-window of 18 rows x 72 columns per channel).  The
// weights of stage g + 1 are the last VMEM operations stage g needs, so stages 0 and 1 wait for everything in flight and stage 2 for all
// but the halo gathers it issued behind its weight slice; a halo therefore has one stage of lead before its wait, the weights less.
struct CfgF4C32 : GeoF4<32, 64, 2, H16_C32> {      // USTG = 12 16-byte LDS-DMA instructions: one per wave + one more on waves 4 .. 7
  static constexpr int HSTEP = !H16 ? 1 : WINOF4_HSTEP > 0 ? WINOF4_HSTEP : 3;      // stage 2's halo gathers behind MFMAs 3, 3 + HSTEP, ..
  static constexpr int WAIT_S2 = NRAW;      // what stage 2 may leave in flight: the halo gathers every wave issued behind its weight slice
};
static_assert(CfgF4C32::LDS_USED <= LDS_REQF4 && 3 + CfgF4C32::HSTEP * (CfgF4C32::RAW_PER_WAVE - 1) < 24 && CfgF4C32::USTG == 12 * 1024 &&
              CfgF4C32::WAIT_S2 <= 63, "32-cout instance");

__global__ __launch_bounds__(512, 1) void conv3x3_winof4_c32_f32_kernel(WinoArgs a) {
  using C = CfgF4C32;
  constexpr int CK = C::CK, RWL = C::RWL, RAW_BYTES = C::RAW_BYTES, RAW_PER_WAVE = C::RAW_PER_WAVE;
  constexpr int USTG = C::USTG, VSTG = C::VSTG, OFF_U = C::OFF_U, OFF_V = C::OFF_V, OFF_RAW = C::OFF_RAW;
  constexpr int UQ = USTG / 4;      // floats per weight stage
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sw = wave & 3;
  const int HpWp = a.Hp * a.Wp;
  const unsigned lds0 = (unsigned)(size_t)(lptr_t)lds;
  const Walk wk = make_walk(a);
  auto decode = [&](int k) { return decode_tile<C>(a, wk, HpWp, k); };
  auto raw_of = [&](const Tile& X, int c) { return X.s0 + (size_t)CK * c * HpWp; };

  const HaloGather<C> halo(a, HpWp, lds0 + OFF_RAW, wave, lane);
  const unsigned uoff = lane * 16u;
  auto dma_u_piece = [&](const float* src, int uslot, int p) {      // KiB p (of 12) of one stage's weights -> ring slot uslot
    if (WINOF4_ABL & 4) return;
    glds16(src + p * 256, uoff, lds0 + OFF_U + uslot * USTG + p * 1024);
  };

  auto body = [&](auto role_tag) {
  constexpr int P = decltype(role_tag)::value;

  // -- input transform: one channel, position row P of the stage's two and TWO tiles per thread (tile rows sw / 2 and sw / 2 + 2, the
  // same tile column).  Lanes as above: k-step bit, 16 tile columns, low bit of the channel group; sw: its high bit, tile row.
  const int t_ks = lane & 1, t_t16 = (lane >> 1) & 15, t_kq = (lane >> 5) | ((sw & 1) << 1), t_wn = sw >> 1;
  const int t_rd = C::at(2 * t_kq + t_ks, 4 * t_wn, 4 * t_t16);                           // + 8 tile-row strides for the second tile
  const int t_wr = (P * 3 * 4 + t_wn) * 1024 + (t_kq * 16 + t_t16) * 16 + t_ks * 8;       // + column pair * 4096 (+ slot); + 2048 for the second tile
  auto transform_row = [&](auto s_tag, int rbuf, int vslot) {      // this thread's two tiles of row P of stage S's two
    constexpr int S = decltype(s_tag)::value;
    if (WINOF4_ABL & 1) return;
    const char* rb = lds + OFF_RAW + rbuf * RAW_BYTES + t_rd;
    char* vb = lds + OFF_V + vslot * VSTG + t_wr;
    transform_tile<2 * S + P, C>(rb, vb);
    transform_tile<2 * S + P, C>(rb + 8 * RWL * 4, vb + 2048);
  };

  // -- MFMA operands: 16 bytes = (k-step 2) x (position 2 of a column pair) per lane; lane = 16 * channel group + cout / tile of the block
  const int a_lane = P * 1024 + lane * 16;       // + (row in stage * 3 + column pair) * 2048 (+ slot)
  const int b_lane = sw * 1024 + lane * 16;      // + (row in stage * 3 + column pair) * 4096 (+ slot)
  f32x4 acc[6][6];

  // One pipeline stage S of a chunk, reading weight and V slot vrd: fetch the next stage's weights (and, S == 2, the halo of the chunk
  // after next) into the other slots between the 24 MFMAs, transform the next stage's V, then the counted wait and the barrier.
  auto stage = [&](auto s_tag, const float* u_src, const float* raw_src, int raw_buf, int t_rbuf, int vrd) {
    constexpr int S = decltype(s_tag)::value, SN = (S + 1) % 3;
    // the stage's LDS-DMA pieces, one behind each MFMA: the weight slice behind MFMA 0 (waves 4 .. 7: and 1), stage 2's halo gathers
    // behind 3, 3 + HSTEP, ..
    auto piece = [&](int m) {
      if (m == 0) dma_u_piece(u_src, vrd ^ 1, wave);
      if (m == 1 && P == 1) dma_u_piece(u_src, vrd ^ 1, 4 + wave);
      if (S == 2 && m >= 3 && (m - 3) % C::HSTEP == 0 && (m - 3) / C::HSTEP < RAW_PER_WAVE) halo.piece(raw_src, raw_buf, (m - 3) / C::HSTEP);
    };
    auto mfmas = [&]() {
      if (WINOF4_ABL & 16) {      // data movement alone: the stage's LDS-DMA pieces without the MFMAs they stand behind
#pragma unroll
        for (int m = 0; m < 24; ++m) piece(m);
        return;
      }
      mfma_stage<S, C::UCP, C::VCP>(acc, lds + OFF_U + vrd * USTG + a_lane, lds + OFF_V + vrd * VSTG + b_lane, piece);
    };
    if (P == 0) {
      mfmas();
      __builtin_amdgcn_sched_barrier(0);
      transform_row(std::integral_constant<int, SN>{}, t_rbuf, vrd ^ 1);
    } else {
      transform_row(std::integral_constant<int, SN>{}, t_rbuf, vrd ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      mfmas();
    }
    // stage 2 leaves the halo gathers every wave issued behind its weight slice in flight (a wave with one more waits for that one too)
    // (the timing build without halo gathers issues nothing behind the weight slice: it waits for everything)
    if (S == 2 && !(WINOF4_ABL & 2)) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::WAIT_S2) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  // -- epilogue: tile row sw, tile column lane & 15
  auto epilogue = [&](const Tile& T) { epilogue_tile(a, acc, HpWp, T, sw, lane & 15, T.ct * 32 + P * 16 + 4 * (lane >> 4)); };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;

  int k = 0;
  Tile T = decode(0);
  if (!T.ok) return;
  // prologue: the first two halos, the first weight stage, the first transform (nch >= 2: chunk 1 exists)
  halo.all(T.s0, 0);
  dma_u_piece(T.w, 0, wave);
  if (P == 1) dma_u_piece(T.w, 0, 4 + wave);
  halo.all(raw_of(T, 1), 1);
  sync_all();
  transform_row(I0{}, 0, 0);
  sync_all();

  int cc = 0;
  for (;;) {
    Tile Tn = decode(k + 1);
    const bool more = Tn.ok;
    if (!more) Tn = T;      // after the walk's last chunks: surplus loads of this tile's first chunks into buffers nobody reads
    clear_acc(acc);
    for (int c = 0; c < a.nch; ++c, ++cc) {
      const float* w_c = T.w + (size_t)c * 3 * UQ;
      const float* nu = (c + 1 < a.nch) ? w_c + 3 * UQ : Tn.w;                                    // the next chunk's weights
      const float* nraw = (c + 2 < a.nch) ? raw_of(T, c + 2) : raw_of(Tn, c + 2 - a.nch);         // the halo of the chunk after next
      const int rcur = cc & 1;      // the chunk's halo buffer; stage g = 3 cc + s reads weight and V slot g & 1 = (cc + s) & 1
      stage(I0{}, w_c + UQ, nullptr, 0, rcur, rcur);
      stage(I1{}, w_c + 2 * UQ, nullptr, 0, rcur, rcur ^ 1);
      stage(I2{}, nu, nraw, rcur, rcur ^ 1, rcur);
    }
    if (!(WINOF4_ABL & 8)) epilogue(T);
    if (!more) break;
    T = Tn;
    ++k;
  }
  sync_all();   // the surplus loads of the last chunk
  };
  if (wave < 4) body(std::integral_constant<int, 0>{});
  else body(std::integral_constant<int, 1>{});
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
bool conv3x3_winof4_ok(int C0, int C1, int cout, int H, int W) {
  return C1 == 0 && C0 >= 16 && C0 % 8 == 0 && cout > 0 && cout % 64 == 0 && H >= 16 && H % 16 == 0 && W >= 32 && W % 32 == 0;
}
// Decoder entry: C0 channels of in0 and C1 of in1, whole chunks of each.  The pipeline needs ONE chunk of the first source (the prologue
// fetches chunk 0 from it) and two chunks in all; C0 = 0 is refused.
bool conv3x3_winof4_entry_ok(int C0, int C1, int cout, int H, int W) {
  return conv3x3_winof4_ok(16, 0, cout, H, W) && H % 2 == 0 && W % 2 == 0 && C0 >= 8 && C0 % 8 == 0 && C1 >= 8 && C1 % 8 == 0;
}
// ... with the second source at H/2 x W/2, up-sampled in the kernel: the pipeline gathers the first TWO chunks of every tile before it can
// interpolate one (the prologue and the tile boundary fetch chunks 0 and 1 from the first source), so C0 >= 16.  H and W are even
// (multiples of 16 and 32): the target is exactly twice the low-resolution size.
bool conv3x3_winof4_ups_ok(int C0, int C1, int cout, int H, int W) { return conv3x3_winof4_entry_ok(C0, C1, cout, H, W) && C0 >= 16; }
bool conv3x3_winof4_packs(int cout, int cin) { return conv3x3_winof4_ok(cin, 0, cout, 16, 32); }
size_t conv3x3_winof4_floats(int cout, int cin) { return (size_t)36 * cout * cin; }

// U = G g G^T in double, rounded once; layout [cout / CT][cin / 8][stage 3][row in stage 2][column pair 3][cout block CT / 16][channel group 4]
// [cout 16][k-step 2][column in pair 2]: position (2 * stage + row, 2 * pair + column), channel 8 * chunk + 2 * group + k-step
static void pack_winof4(const float* w, int cout, int cin, float* dst, int CT) {
  const int nch = cin / 8, nmb = CT / 16;
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci) {
      const float* g = w + ((size_t)co * cin + ci) * 9;
      double gg[6][3], u[6][6];
      for (int i = 0; i < 6; ++i)
        for (int x = 0; x < 3; ++x) gg[i][x] = WINOF4_G[i][0] * g[0 * 3 + x] + WINOF4_G[i][1] * g[1 * 3 + x] + WINOF4_G[i][2] * g[2 * 3 + x];
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) u[i][j] = gg[i][0] * WINOF4_G[j][0] + gg[i][1] * WINOF4_G[j][1] + gg[i][2] * WINOF4_G[j][2];
      const int ct = co / CT, mb = (co % CT) / 16, m = co % 16, ch = ci / 8, kq = (ci % 8) / 2, ks = ci % 2;
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
          const size_t idx = (((((((((size_t)ct * nch + ch) * 3 + i / 2) * 2 + i % 2) * 3 + j / 2) * nmb + mb) * 4 + kq) * 16 + m) * 2 + ks) * 2 + j % 2;
          dst[idx] = (float)u[i][j];
        }
    }
}
void pack_conv_weights_winof4(const float* w, int cout, int cin, float* dst) { pack_winof4(w, cout, cin, dst, CfgF4T<false>::CT); }

// The 32-cout instance: one source, cout tiles of 32 (cout a multiple of 32 but not of 64: the UNet's full-resolution 32 -> 32 layers),
// regions of 16 x 64 px; two chunks for the pipeline's prologue.
bool conv3x3_winof4_c32_ok(int C0, int C1, int cout, int H, int W) {
  return C1 == 0 && C0 >= 16 && C0 % 8 == 0 && cout > 0 && cout % 32 == 0 && cout % 64 != 0 && H >= 16 && H % 16 == 0 && W >= 64 && W % 64 == 0;
}
bool conv3x3_winof4_c32_packs(int cout, int cin) { return conv3x3_winof4_c32_ok(cin, 0, cout, 16, 64); }
void pack_conv_weights_winof4_c32(const float* w, int cout, int cin, float* dst) { pack_winof4(w, cout, cin, dst, CfgF4C32::CT); }

// One launch path for the four instances.  ups: in1 is the low-resolution second source (H/2 x W/2) and the kernel up-samples it
// (launch_conv3x3_winof4_ups); c32: the 32-cout kernel (one source).
enum class F4Inst { PLAIN, ENTRY, UPS, C32 };
static int launch_winof4(F4Inst inst, const float* u, const float* bias, int cout, const float* in0, int C0, const float* in1, int C1, float* out,
                         int B, int H, int W, hipStream_t s, float slope, float* pool_out) {
  const bool c32 = inst == F4Inst::C32, ups = inst == F4Inst::UPS;
  const bool ok = c32 ? conv3x3_winof4_c32_ok(C0, C1, cout, H, W)
                  : ups ? conv3x3_winof4_ups_ok(C0, C1, cout, H, W)
                        : inst == F4Inst::ENTRY ? conv3x3_winof4_entry_ok(C0, C1, cout, H, W) : conv3x3_winof4_ok(C0, C1, cout, H, W);
  if (!ok) {
    if (c32) set_error("conv3x3_winof4_c32: unsupported geometry (%d -> %d channels, %d x %d)", C0, cout, H, W);
    else set_error("conv3x3_winof4: unsupported geometry (%d + %d -> %d channels, %d x %d)", C0, C1, cout, H, W);
    return PNPX_ERR_SHAPE;
  }
  WinoArgs a{};
  a.in0 = in0;
  a.in1 = C1 != 0 ? in1 : in0;
  a.u = u;
  a.bias = bias;
  a.pool = pool_out;
  a.out = out;
  a.B = B;
  a.H = H;
  a.W = W;
  a.Hp = padded_h(H);
  a.Wp = padded_w(W);
  a.C0 = C0;
  a.C1 = C1;
  a.Cout = cout;
  a.slope = slope;
  a.nct = cout / (c32 ? CfgF4C32::CT : CfgF4T<false>::CT);
  a.nch = (C0 + C1) / CfgF4C32::CK;
  a.nch_all = a.nch;
  a.ksplit = 1;
  a.rx = W / (c32 ? CfgF4C32::RW : CfgF4T<false>::RW);
  a.ry = H / 16;
  if (ups) {
    a.ups_h = H / 2;
    a.ups_w = W / 2;
    // models/unet.py:99 (align_corners = True): source = destination * (in - 1) / (out - 1); the same two floats as unet.hip hands upsample2x_v4_kernel
    a.ups_sy = (float)(H / 2 - 1) / (float)(H - 1);
    a.ups_sx = (float)(W / 2 - 1) / (float)(W - 1);
  }
  using Kernel = void (*)(WinoArgs);
  static const Kernel kernels[4] = {conv3x3_winof4_f32_kernel<false, false, H16_PLAIN>, conv3x3_winof4_f32_kernel<true, false, H16_ENTRY>,
                                    conv3x3_winof4_f32_kernel<true, true, H16_UPS>, conv3x3_winof4_c32_f32_kernel};      // in F4Inst's order
  // the 16-byte halo gathers read whole aligned units: plane and row strides are multiples of 16 bytes (Wp = W + 8, W % 32 == 0), the
  // tensors' bases must be too
  const bool h16[4] = {H16_PLAIN, H16_ENTRY, H16_UPS, H16_C32};
  if (h16[(int)inst] && ((reinterpret_cast<uintptr_t>(in0) & 15) || (inst == F4Inst::ENTRY && (reinterpret_cast<uintptr_t>(in1) & 15)))) {
    set_error("conv3x3_winof4: the input tensors must be 16-byte aligned");
    return PNPX_ERR_SHAPE;
  }
  static std::once_flag attr_once[64];
  int dev = 0;
  PNPX_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64) {
    hipError_t e = hipSuccess;
    std::call_once(attr_once[dev], [&] {
      for (int i = 0; i < 4 && e == hipSuccess; ++i)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[i]), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_REQF4);
    });
    PNPX_HIP(e);
  }
  const long long nreg = (long long)a.rx * a.ry * a.B, ntiles = nreg * a.nct;
  long long grid = 256;
  if (grid >= ntiles) grid = ntiles;
  else if ((grid / 8) % a.nct != 0 && grid >= 8LL * a.nct) grid -= grid % (8 * a.nct);
  hipLaunchKernelGGL(kernels[(int)inst], dim3((unsigned)grid), dim3(512), LDS_REQF4, s, a);
  PNPX_LAUNCH_CHECK();
  return PNPX_OK;
}

int launch_conv3x3_winof4(const float* u, const float* bias, int cout, const float* in0, int C0, const float* in1, int C1, float* out, int B,
                          int H, int W, hipStream_t s, float slope, float* pool_out) {
  return launch_winof4(C1 != 0 ? F4Inst::ENTRY : F4Inst::PLAIN, u, bias, cout, in0, C0, in1, C1, out, B, H, W, s, slope, pool_out);
}
int launch_conv3x3_winof4_ups(const float* u, const float* bias, int cout, const float* in0, int C0, const float* in1_lowres, int C1,
                              float* out, int B, int H, int W, hipStream_t s, float slope) {
  return launch_winof4(F4Inst::UPS, u, bias, cout, in0, C0, in1_lowres, C1, out, B, H, W, s, slope, nullptr);
}
int launch_conv3x3_winof4_c32(const float* u, const float* bias, int cout, const float* in0, int C0, float* out, int B, int H, int W,
                              hipStream_t s, float slope, float* pool_out) {
  return launch_winof4(F4Inst::C32, u, bias, cout, in0, C0, nullptr, 0, out, B, H, W, s, slope, pool_out);
}

// The halo plan of an instance as the kernels run it (include/pnpx.h has the layout): every table entry comes from the geometry's own
// functions and constants, the ones HaloGather, transform_tile and the stages' waits use.
template <class C>
static void halo_plan_of(int H, int W, int off_raw, int lds_used, const int (&waits)[4], int nuw, int nst, int* info, long long* src, int* dst,
                         int* width, int* wave, int* real, int* read) {
  const int Hp = padded_h(H), Wp = padded_w(W), HpWp = Hp * Wp;
  const int v[PNPX_WINOF4_HALO_INFO] = {C::H16, C::CT, C::RW, C::RWL, C::RPXL, C::ORG, C::HCOL, C::RAW_INSTR, C::N16, C::RAW_PER_WAVE, C::NRAW,
                                        C::RAW_BYTES, off_raw, lds_used, nuw, nst, waits[0], waits[1], waits[2], waits[3]};
  for (int i = 0; i < PNPX_WINOF4_HALO_INFO; ++i) info[i] = v[i];
  for (int i = 0; i < C::RAW_INSTR && src; ++i)
    for (int lane = 0; lane < 64; ++lane) {
      bool ok = false;
      src[i * 64 + lane] = (long long)C::src(i, lane, HpWp, Wp, &ok);
      dst[i * 64 + lane] = C::dst(i) + lane * C::width(i);
      width[i * 64 + lane] = C::width(i);
      wave[i * 64 + lane] = i % 8;
      real[i * 64 + lane] = ok;
    }
  for (int c = 0; c < C::CK && read; ++c)
    for (int hy = 0; hy < 18; ++hy)
      for (int hx = 0; hx < C::RW + 2; ++hx) read[(c * 18 + hy) * (C::RW + 2) + hx] = C::at(c, hy, hx);
}

}  // namespace pnpx

extern "C" int pnpx_winof4_halo_plan(int inst, int H, int W, int* info, long long* src, int* dst, int* width, int* wave, int* real, int* read) {
  using namespace pnpx;
  if (!info || inst < 0 || inst > 3 || H < 16 || H % 16 != 0 || W < (inst == 3 ? 64 : 32) || W % (inst == 3 ? 64 : 32) != 0) return PNPX_ERR_SHAPE;
  if (src && !(dst && width && wave && real)) return PNPX_ERR_SHAPE;
  auto cfg64 = [&](auto h16_tag, bool ups) {
    using C = CfgF4T<decltype(h16_tag)::value>;
    const int w_plain[4] = {C::WAIT_U, C::WAIT_HALO, -1, -1}, w_ups[4] = {C::WAIT_U, C::WAIT_HALO, C::WAIT_ST, C::WAIT_HALO_ST};
    halo_plan_of<C>(H, W, ups ? C::OFF_RAW_UPS : C::OFF_RAW, ups ? C::LDS_USED_UPS : C::LDS_USED, ups ? w_ups : w_plain, C::NUW, ups ? C::NST : 0, info,
                    src, dst, width, wave, real, read);
  };
  const bool h16 = inst == 0 ? H16_PLAIN : inst == 1 ? H16_ENTRY : H16_UPS;
  if (inst == 3) {
    const int w_c32[4] = {0, CfgF4C32::WAIT_S2, -1, -1};      // stages 0 and 1 wait for everything
    halo_plan_of<CfgF4C32>(H, W, CfgF4C32::OFF_RAW, CfgF4C32::LDS_USED, w_c32, 1, 0, info, src, dst, width, wave, real, read);
  } else if (h16) {
    cfg64(std::true_type{}, inst == 2);
  } else {
    cfg64(std::false_type{}, inst == 2);
  }
  return PNPX_OK;
}

// the matrices the packer uses and the packer itself, for tests/test_winof4_pack.py (host only)
extern "C" void pnpx_winof4_matrices(double* g18, double* bt36, double* at24) {
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 3; ++j) g18[i * 3 + j] = pnpx::WINOF4_G[i][j];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) bt36[i * 6 + j] = pnpx::WINOF4_BT[i][j];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 6; ++j) at24[i * 6 + j] = pnpx::WINOF4_AT[i][j];
}
extern "C" int pnpx_winof4_pack(const float* w, int cout, int cin, float* dst) {
  if (!w || !dst || cout <= 0 || cout % 64 != 0 || cin <= 0 || cin % 8 != 0) return PNPX_ERR_SHAPE;
  pnpx::pack_conv_weights_winof4(w, cout, cin, dst);
  return PNPX_OK;
}
extern "C" int pnpx_winof4_c32_pack(const float* w, int cout, int cin, float* dst) {
  if (!w || !dst || cout <= 0 || cout % 32 != 0 || cin <= 0 || cin % 8 != 0) return PNPX_ERR_SHAPE;
  pnpx::pack_conv_weights_winof4_c32(w, cout, cin, dst);
  return PNPX_OK;
}
