"""The halo plan of the four Winograd F(4x4,3x3) instances (csrc/conv3x3_winof4.hip), through pnpx_winof4_halo_plan: the tables the kernels
themselves use for the LDS-DMA gathers of a chunk's halo and for the input transform's reads.  Coverage, overlap, dummy lanes, alignment,
source bounds, the counted waits, the LDS total and the bank model of the transform's and the MFMA operands' LDS reads.  No GPU."""
import numpy as np
import pytest

from tfpnp_amd import _lib

INSTANCES = {0: "plain", 1: "entry", 2: "fuse_up", 3: "c32"}
N_INFO = 20
(H16, CT, RW, RWL, RPXL, ORG, HCOL, N_INSTR, N16, PER_WAVE, NRAW, RAW_BYTES, OFF_RAW, LDS_USED, NUW, NST, W_U, W_HALO, W_ST, W_HALO_ST) = range(N_INFO)
PADL, CK = 4, 8


def _geoms(inst):
    """the smallest geometry, a non-square one and the per-level shapes of a 256 x 256 image the instance runs at"""
    if inst == 3:
        return ((16, 64), (32, 192), (256, 256))
    return ((16, 32), (48, 96), (128, 128), (64, 64), (32, 32))


def plan(inst, H, W):
    info = np.zeros(N_INFO, np.int32)
    L = _lib.lib()
    assert L.pnpx_winof4_halo_plan(inst, H, W, info.ctypes.data, None, None, None, None, None, None) == 0
    n = int(info[N_INSTR]) * 64
    src = np.zeros(n, np.int64)
    dst, width, wave, real = (np.zeros(n, np.int32) for _ in range(4))
    read = np.zeros((CK, 18, int(info[RW]) + 2), np.int32)
    assert L.pnpx_winof4_halo_plan(inst, H, W, info.ctypes.data, src.ctypes.data, dst.ctypes.data, width.ctypes.data, wave.ctypes.data,
                                   real.ctypes.data, read.ctypes.data) == 0
    return info.tolist(), src, dst, width, wave, real.astype(bool), read


CASES = [(i, H, W) for i in INSTANCES for H, W in _geoms(i)]


@pytest.mark.parametrize("inst,H,W", CASES)
def test_coverage_overlap_dummies_alignment_bounds(inst, H, W):
    info, src, dst, width, wave, real, read = plan(inst, H, W)
    Hp, Wp = H + 2, W + 2 * PADL
    HpWp = Hp * Wp
    rw, nfl = info[RW], info[RAW_BYTES] // 4
    # float-granular image of one halo buffer: which source float (from the chunk's origin) lands in which LDS float
    img = np.full(nfl, -1, np.int64)
    writes = np.zeros(nfl, np.int32)
    dummy = np.zeros(nfl, bool)
    for j in range(len(src)):
        assert width[j] in (4, 16) and src[j] % 4 == 0 and dst[j] % 4 == 0
        assert 0 <= dst[j] and dst[j] + width[j] <= info[RAW_BYTES], "a lane lands outside the halo buffer"
        if width[j] == 16:
            assert src[j] % 16 == 0 and dst[j] % 16 == 0, "16-byte gathers need aligned sources and destinations"
        f0, n = dst[j] // 4, width[j] // 4
        if real[j]:
            writes[f0:f0 + n] += 1
            img[f0:f0 + n] = src[j] // 4 + np.arange(n)
        else:
            assert src[j] == 0, "a dummy lane reads the chunk's origin"
            dummy[f0:f0 + n] = True
    assert writes.max() == 1, "an LDS byte receives real data twice"
    assert not (dummy & (writes > 0)).any(), "a dummy lane lands on real data"
    # instructions: whole 16-byte ones first, 64 lanes of a linear run each, dealt round-robin to the eight waves
    w_i, d_i = width.reshape(-1, 64), dst.reshape(-1, 64)
    assert (w_i == w_i[:, :1]).all() and (np.diff(d_i, axis=1) == w_i[:, :1]).all()
    assert (w_i[:info[N16], 0] == 16).all() and (w_i[info[N16]:, 0] == 4).all()
    assert (wave.reshape(-1, 64) == (np.arange(info[N_INSTR]) % 8)[:, None]).all()
    assert info[N_INSTR] > info[N16], "every kernel keeps at least one dword gather (tests/test_build_invariants_winof4.py)"
    # coverage: halo element (c, hy, hx) = padded (row y0 + hy, column x0 + 3 + hx) of channel c, read where the transform reads it
    rd = read // 4
    assert (read % 4 == 0).all() and len(np.unique(rd)) == rd.size
    c, hy, hx = np.meshgrid(np.arange(CK), np.arange(18), np.arange(rw + 2), indexing="ij")
    want = c * HpWp + hy * Wp + hx + (PADL - 1) - info[ORG]
    assert (writes[rd] == 1).all(), "a halo element is not written"
    assert (img[rd] == want).all(), "a halo element comes from the wrong source"
    assert not dummy[rd].any(), "a dummy lane lands where the transform reads"
    assert (read == ((c * info[RPXL] + hy * info[RWL] + hx + info[HCOL]) * 4)).all()
    # bounds: every real source float inside the chunk's 8 padded planes, for the first and the last region both ways (the origin is
    # channel 0 of the chunk, padded row y0, padded column x0 + ORG; the last chunk ends where the tensor ends)
    s = img[img >= 0]
    ch, r = s // HpWp, s % HpWp
    row, col = r // Wp, r % Wp
    assert ch.min() >= 0 and ch.max() <= CK - 1
    for y0 in (0, H - 16):
        for x0 in (0, W - rw):
            assert row.min() + y0 >= 0 and row.max() + y0 <= Hp - 1
            assert col.min() + x0 + info[ORG] >= 0 and col.max() + x0 + info[ORG] <= Wp - 1
            last = (ch * HpWp + (row + y0) * Wp + col + x0 + info[ORG]).max()
            assert last < CK * HpWp, "a source lies behind the chunk's planes"


@pytest.mark.parametrize("inst", INSTANCES)
def test_wait_counts_and_lds_total(inst):
    info, src, dst, width, wave, real, read = plan(inst, *_geoms(inst)[0])
    per_wave = np.bincount(wave.reshape(-1, 64)[:, 0], minlength=8)
    assert per_wave.min() == info[NRAW] and per_wave.max() == info[PER_WAVE] and info[PER_WAVE] <= info[NRAW] + 1
    if inst == 3:
        assert info[W_U] == 0 and info[W_HALO] == info[NRAW] and info[W_ST] == info[W_HALO_ST] == -1
    else:
        assert info[W_U] == info[NUW] == 3 and info[W_HALO] == info[NUW] + info[NRAW]
        if inst == 2:
            assert info[NST] == 3 and info[W_ST] == info[NUW] + info[NST] and info[W_HALO_ST] == info[NUW] + info[NRAW] + info[NST]
        else:
            assert info[W_ST] == info[W_HALO_ST] == -1
    assert max(info[W_U], info[W_HALO], info[W_ST], info[W_HALO_ST]) <= 63          # vmcnt is six bits
    assert info[LDS_USED] <= 160 * 1024 and info[OFF_RAW] % 16 == 0 and info[RAW_BYTES] % 16 == 0
    assert info[OFF_RAW] + 2 * info[RAW_BYTES] <= info[LDS_USED]
    if info[H16]:
        assert info[RPXL] % 4 == 0 and info[RWL] % 4 == 0 and info[HCOL] == 3 and info[ORG] == 0
        assert info[N_INSTR] == {32: 26, 64: 44}[info[RW]]
    else:
        assert info[HCOL] == 0 and info[ORG] == PADL - 1 and info[N_INSTR] == {32: 91, 64: 163}[info[RW]]


# ---------------------------------------------------------------------------------------------------------------------------------
# LDS bank model: lane groups and bank widths of MI355X_MICROARCH.md (LDS): an access is served in fixed lane groups, one cycle per group
# when conflict-free, one more per further distinct address on a busy bank.

def _b128_groups():
    g = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    return g + [[l + 32 for l in x] for x in g]


GROUPS = {8: ([list(range(32)), list(range(32, 64))], 64), 16: (_b128_groups(), 64)}


def extra_cycles(addr, nbytes):
    """conflict cycles of one wave-instruction reading nbytes per lane at byte addresses addr[64]"""
    groups, nbanks = GROUPS[nbytes]
    extra = 0
    for g in groups:
        per_bank = {}
        for l in g:
            for k in range(nbytes // 4):
                per_bank.setdefault((addr[l] // 4 + k) % nbanks, set()).add(addr[l] // 4 + k)
        extra += max(len(v) for v in per_bank.values()) - 1
    return extra


@pytest.mark.parametrize("inst", INSTANCES)
def test_bank_model_of_the_lds_reads(inst):
    info, *_, read = plan(inst, *_geoms(inst)[0])
    lane = np.arange(64)
    # MFMA operands: 16 bytes per lane, lane * 16 from a block's base (both operands, every instance): conflict-free
    assert extra_cycles((lane * 16).tolist(), 16) == 0
    # input transform (the kernels' lane roles): k-step bit, 16 tiles, low bit of the channel group; wave: high bit, tile block / row
    ks, t16 = lane & 1, (lane >> 1) & 15
    worst = {8: 0, 16: 0}
    for sw in range(4):
        ch = 2 * ((lane >> 5) | ((sw & 1) << 1)) + ks
        wn = sw >> 1
        if inst == 3:
            rows = [(4 * wn * np.ones(64, int), 4 * t16), (4 * (wn + 2) * np.ones(64, int), 4 * t16)]
        else:
            tile = wn * 16 + t16
            rows = [(4 * (tile >> 3), 4 * (tile & 7))]
        for hy0, hx0 in rows:
            base = read[ch, hy0, hx0]
            for y in range(6):
                row = base + y * info[RWL] * 4
                parts = ((-4, 8), (4, 16), (20, 8)) if info[H16] else ((0, 8), (8, 8), (16, 8))
                for off, nb in parts:
                    a = row + off
                    assert (a % nb == 0).all() and a.min() >= 0
                    worst[nb] = max(worst[nb], extra_cycles(a.tolist(), nb))
    # 16-byte reads and the dword form's 8-byte reads: none.  The 16-byte form's 8-byte reads start at column 2 mod 4 in every channel
    # (plane strides are multiples of four floats), so a 32-lane group's even and odd channels meet in the banks 2, 3 mod 4: one extra
    # cycle per group, two per instruction, whatever the plane stride (profiles/winof4_halo16.md)
    assert worst[16] == 0
    assert worst[8] == (2 if info[H16] else 0)
