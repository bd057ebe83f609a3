"""Host side of the F(4x4,3x3) kernel's 32-cout instance (csrc/conv3x3_winof4.hip, option fp32_winof4_c32): its weight packer, the
selector's row for it (csrc/conv_f32_select.hip through pnpx_conv_f32_forward_plan), the probe plan of kind 12, and the per-layer error
bar with the proof that it catches subtle errors (tests/winof4_c32_cases.py).  No GPU."""
import numpy as np
import pytest

from tests import conv_layer_cases as CL
from tests import winof4_c32_cases as C32
from tfpnp_amd import _lib


def _matrices():
    g, bt, at = np.zeros((6, 3)), np.zeros((6, 6)), np.zeros((4, 6))
    _lib.lib().pnpx_winof4_matrices(g.ctypes.data, bt.ctypes.data, at.ctypes.data)
    return g, bt, at


def _pack(w):
    cout, cin = w.shape[:2]
    dst = np.full(36 * cout * cin, np.nan, np.float32)
    assert _lib.lib().pnpx_winof4_c32_pack(w.ctypes.data, cout, cin, dst.ctypes.data) == 0
    return dst


def _operand(dst, cin, ct, chunk, stage, q, block, lane):
    """The 16 bytes the kernel's lane reads as its A operand: weight stage (ct, chunk, stage) of 12 KiB, + q * 2048 (q = 3 * row in stage +
    column pair) + cout block * 1024 + lane * 16 -> [k-step 2][column in pair 2]"""
    base = ((ct * (cin // 8) + chunk) * 3 + stage) * 3072 + q * 512 + block * 256 + lane * 4
    return dst[base:base + 4].reshape(2, 2)


@pytest.mark.parametrize("cout,cin", [(32, 24), (96, 16)])
def test_packer_through_the_transform_domain_product(cout, cin):
    """U read back the way the kernel's MFMA lanes address it (lane = 16 x channel group + cout, register pair = k-step, channel = 8 chunk
    + 2 group + k-step), multiplied with B^T d B in float64 and transformed back: the direct float64 convolution, to the one rounding of U."""
    g, bt, at = _matrices()
    rng = np.random.default_rng(11)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    dst = _pack(w)
    assert np.isfinite(dst).all()                                    # every slot written
    u = np.zeros((cout, cin, 6, 6))
    for ct in range(cout // 32):
        for chunk in range(cin // 8):
            for stage in range(3):
                for q in range(6):
                    for block in range(2):
                        for lane in range(64):
                            op = _operand(dst, cin, ct, chunk, stage, q, block, lane)
                            for ks in range(2):
                                for col in range(2):
                                    u[32 * ct + 16 * block + lane % 16, 8 * chunk + 2 * (lane // 16) + ks, 2 * stage + q // 3, 2 * (q % 3) + col] = op[ks, col]
    # rounded once from G g G^T in double
    want = np.einsum("ia,kcab,jb->kcij", g, w.astype(np.float64), g)
    np.testing.assert_allclose(u, want.astype(np.float32), rtol=1.2e-7, atol=1e-30)
    H, W = 8, 12
    x = rng.standard_normal((cin, H, W))
    xp = np.zeros((cin, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((cout, H, W))
    for ty in range(H // 4):
        for tx in range(W // 4):
            v = np.einsum("ia,cab,jb->cij", bt, xp[:, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6], bt)
            out[:, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = np.einsum("pi,kij,qj->kpq", at, np.einsum("kcij,cij->kij", u, v), at)
    ref = np.zeros((cout, H, W))
    for dy in range(3):
        for dx in range(3):
            ref += np.einsum("kc,chw->khw", w[:, :, dy, dx].astype(np.float64), xp[:, dy:dy + H, dx:dx + W])
    assert np.abs(out - ref).max() / np.abs(ref).max() < 2e-6       # fp32 U: 36 roundings of 6e-8 each on sums of cin terms
    # shapes the packer does not take
    assert _lib.lib().pnpx_winof4_c32_pack(w.ctypes.data, 48, cin, dst.ctypes.data) != 0
    assert _lib.lib().pnpx_winof4_c32_pack(w.ctypes.data, cout, 12, dst.ctypes.data) != 0
    assert _lib.lib().pnpx_winof4_c32_pack(None, cout, cin, dst.ctypes.data) != 0


# pnpx_conv_f32_forward_plan's opts
WINOGRAD, WINO8, F4_BIT, C32_BIT, U, U_F4, U_C32, LAST = (1 << i for i in range(8))
DIRECT_K, WINO4_K, WINO8_K, WINOF4_K, WINOF4_C32_K = range(5)
ON = WINOGRAD | WINO8 | C32_BIT | U | U_C32


def _plan(opts, C0, C1, cout, H, W, B=48, ksplit=1, rule=1):
    v = _lib.lib().pnpx_conv_f32_forward_plan(opts, ksplit, rule, C0, C1, cout, H, W, B)
    assert v >= 0
    return v & 15, (v >> 4) & 15, v >> 8


def test_selector_truth_table():
    g = (32, 0, 32, 256, 256)
    assert _plan(ON, *g) == (WINOF4_C32_K, 1, 1)                       # the layer as the benchmark runs it; the fused pool is available
    assert _plan(ON & ~C32_BIT, *g) == (WINO8_K, 1, 1)                 # bit off: the 8-wave F(2x2) kernel, as before the option
    assert _plan(ON & ~U_C32, *g) == (WINO8_K, 1, 1)                   # weights missing
    assert _plan(ON & ~WINO8, *g) == (WINO4_K, 1, 1)                   # the layer's 8-wave bit cleared: neither
    assert _plan(ON & ~WINOGRAD, *g) == (DIRECT_K, 1, 0) and _plan(ON & ~U, *g) == (DIRECT_K, 1, 0)
    assert _plan(ON | F4_BIT | U_F4, *g) == (WINOF4_C32_K, 1, 1)       # fp32_winof4_layers has no say on a 32-cout layer
    assert _plan(ON, 32, 64, 32, 256, 256)[0] == WINO8_K               # two sources (entry 24's geometry on an up-sampled tensor)
    for ksplit in (0, 1, 2):                                           # the K-split modes never name a 32-cout layer
        for B in (1, 48):
            assert _plan(ON, *g, B=B, ksplit=ksplit) == (WINOF4_C32_K, 1, 1), (ksplit, B)
            assert _plan(ON, 16, 0, 32, 16, 64, B=B, ksplit=ksplit) == (WINOF4_C32_K, 1, 1)
    for W in (32, 96, 160):                                            # W not a multiple of the region width
        assert _plan(ON, 32, 0, 32, 64, W)[0] == WINO8_K, W
    assert _plan(ON, 32, 0, 32, 24, 64)[0] == DIRECT_K                 # H % 16: no Winograd kernel at all
    assert _plan(ON, 8, 0, 32, 64, 64)[0] == WINO4_K                   # one chunk: the pipeline needs two (the 8-wave kernel too)
    assert _plan(ON, 32, 0, 64, 64, 64)[0] == WINO8_K                  # cout 64 belongs to the 64-cout instances and their mask ...
    assert _plan(ON | F4_BIT | U_F4, 32, 0, 64, 64, 64)[0] == WINOF4_K
    assert _plan(ON, 32, 0, 96, 64, 64)[0] == WINOF4_C32_K             # three 32-cout tiles
    # the last layer never: fused out-conv epilogue on the F(2x2) kernels, whatever the new option says
    assert _plan(ON | LAST, *g) == (WINO8_K, 1, 1) and _plan((ON | LAST) & ~WINO8, *g) == (WINO4_K, 1, 1)
    assert _lib.lib().pnpx_conv_f32_forward_plan(ON, 1, 1, 0, 0, 32, 64, 64, 1) == -1
    assert _lib.lib().pnpx_conv_f32_forward_plan(ON | LAST, 1, 1, 32, 32, 32, 64, 64, 1) == -1


def test_probe_plan_of_kind_12():
    P = lambda *g: _lib.lib().pnpx_conv3x3_probe_plan(C32.WINOF4_C32, *g, 1)
    for _, c in C32.CASES:
        assert P(c.C0, c.C1, c.cout, c.H, c.W) == 32, c.name
    for g in C32.REFUSED:
        assert P(*g) == 0, g
    # the kinds around it stay what they were: 9 refuses everything, 10 is unknown
    assert _lib.lib().pnpx_conv3x3_probe_plan(9, 32, 64, 64, 32, 32, 1) == 0 and _lib.lib().pnpx_conv3x3_probe_plan(10, 32, 0, 32, 16, 64, 1) == 0


def test_recorded_bar_is_eight_times_the_emulation_maximum():
    mx, b = C32.recorded_bar()
    emu, where = C32.emulation_maximum()
    print(f"fp32 F(4x4) emulation maximum {emu:.4e} at {where}; bar {CL.BAR_FACTOR * emu:.4e}")
    assert emu == pytest.approx(mx, rel=1e-4), (emu, where)          # the file holds 5 significant digits
    assert b == pytest.approx(CL.BAR_FACTOR * emu, rel=1e-4)
    assert 1e-7 < mx < 1e-5                                           # the F(4x4) accuracy class (profiles/conv_layer_probe.md)


def test_bar_catches_every_mutant():
    for _, c in C32.CASES:
        ref, den = C32.case_reference(c.name)
        got = C32.mutants(c.name)
        assert {n for n, _ in got} == {"weight_zeroed", "tile_shifted", "cout_block_swapped"}
        for n, m in got:
            assert CL.measure(m, ref, den) > C32.bar(), (c.name, n)
