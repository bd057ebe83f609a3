"""CPU side of the decoder entries on the Winograd F(4x4,3x3) kernel (option fp32_winof4_entries): the selector's rows for a decoder entry
(pnpx_conv_f32_entry_plan = csrc/conv_f32_select.hip conv_f32_entry) against a plain restatement, the option's table row and
documentation, the probe plan of the two new kinds, and the bar of tests/test_gpu_winof4_entry.py re-derived from the emulation
(tests/winof4_entry_cases.py).  No GPU."""
import itertools
import os
import re

import pytest

from tests import conv_layer_cases as CL
from tests import winof4_entry_cases as EC

ROOT = CL.ROOT
DIRECT, WINO4, WINO8, WINOF4 = range(4)                      # ConvF32Kernel
WINOGRAD, BIT8, BITF4, BITENTRY, FUSE_UP, PACKED2, PACKED4 = (1 << i for i in range(7))
ALL_ON = WINOGRAD | BIT8 | BITENTRY | FUSE_UP | PACKED2 | PACKED4

# (C0, C1, cout, H, W): the network's four entries at 256 x 256 and at 64 x 128; the smallest accepted geometry and what lies around it
GEOMS = ((256, 512, 256, 32, 32), (128, 256, 128, 64, 64), (64, 128, 64, 128, 128), (32, 64, 32, 256, 256),
         (256, 512, 256, 8, 16), (128, 256, 128, 16, 32), (64, 128, 64, 32, 64),
         (8, 8, 64, 16, 32), (16, 16, 64, 16, 32), (24, 40, 128, 32, 64), (64, 128, 64, 16, 16), (64, 128, 64, 16, 48),
         (64, 128, 64, 24, 32), (64, 12, 64, 16, 32), (12, 64, 64, 16, 32), (64, 128, 96, 16, 32), (48, 16, 64, 32, 32))
BATCHES = (1, 6, 48)


def entry_ok(C0, C1, cout, H, W):
    """conv3x3_winof4_entry_ok restated."""
    return (cout % 64 == 0 and H >= 16 and H % 16 == 0 and W >= 32 and W % 32 == 0 and C0 >= EC.MIN_C0 and C0 % 8 == 0
            and C1 >= 8 and C1 % 8 == 0)


def expected(opts, ksplit, geom, B):
    """(kernel, pieces, fused) of DESIGN.md's entry table."""
    C0, C1, cout, H, W = geom
    c = CL.Case("g", "fwd", C0, C1, cout, H, W, False, False)
    if not (opts & WINOGRAD and opts & PACKED2 and CL.accepts(CL.WINO4, c)):
        return DIRECT, 1, False
    if not (opts & BIT8 and CL.accepts(CL.WINO8, c)):
        return WINO4, 1, False
    pieces = 1
    if ksplit == 2 or (ksplit == 1 and (H // 16) * (W // 16) * (cout // 64) * B < 256):
        pieces = CL.ksplit_pieces(c)
    if pieces == 1 and opts & BITENTRY and opts & PACKED4 and entry_ok(*geom):
        return WINOF4, 1, False
    return WINO8, pieces, bool(pieces == 1 and opts & FUSE_UP and CL.accepts(CL.WINO8_UPS, c._replace(op="ups")))


def plan(opts, ksplit, geom, B, rule=1):
    from tfpnp_amd import _lib
    v = _lib.lib().pnpx_conv_f32_entry_plan(opts, ksplit, rule, *geom, B)
    assert v >= 0
    return v & 15, (v >> 4) & 15, bool(v >> 8)


def test_selector_rows_for_the_entries():
    seen = set()
    for geom, B, ksplit in itertools.product(GEOMS, BATCHES, (0, 1, 2)):
        for opts in range(128):
            got = plan(opts, ksplit, geom, B)
            assert got == expected(opts, ksplit, geom, B), (geom, B, ksplit, bin(opts), got)
            seen.add(got)
            # the layer's fp32_winof4_layers bit changes no decision about an entry
            if opts & BITF4:
                assert got == plan(opts & ~BITF4, ksplit, geom, B), (geom, B, ksplit, bin(opts))
    # every kind of row occurred: direct, 4-wave, 8-wave fused / unfused / split, F(4x4)
    assert {(DIRECT, 1, False), (WINO4, 1, False), (WINO8, 1, True), (WINO8, 1, False), (WINO8, 2, False), (WINO8, 4, False),
            (WINOF4, 1, False)} <= seen, seen
    from tfpnp_amd import _lib
    assert _lib.lib().pnpx_conv_f32_entry_plan(ALL_ON, 1, 1, 64, 0, 64, 16, 32, 1) == -1


def test_the_headline_shape_and_its_neighbours():
    """48 x 256^2: the three entries of levels 1-3 run F(4x4) unsplit and behind the separate up-sampling kernel; level 0's stays on the
    8-wave kernel's fused instance.  Below the K-split's batch threshold the 32 x 32 entry splits on the 8-wave kernel as before."""
    for geom in GEOMS[:3]:
        assert plan(ALL_ON, 1, geom, 48) == (WINOF4, 1, False)
        assert plan(ALL_ON & ~BITENTRY, 1, geom, 48) == (WINO8, 1, True)          # the option off: today's row
        assert plan(ALL_ON & ~BITENTRY | BITF4, 1, geom, 48) == (WINO8, 1, True)   # fp32_winof4_layers does not stand in for it
        assert plan(ALL_ON & ~PACKED4, 1, geom, 48) == (WINO8, 1, True)
        assert plan(ALL_ON & ~BIT8, 1, geom, 48) == (WINO4, 1, False)              # the wino8 bit switches the entry off F(4x4)
        assert plan(ALL_ON & ~FUSE_UP, 1, geom, 48) == (WINOF4, 1, False)
        assert plan(ALL_ON & ~WINOGRAD, 1, geom, 48) == (DIRECT, 1, False)
    assert plan(ALL_ON, 1, GEOMS[3], 48) == (WINO8, 1, True)
    assert plan(ALL_ON, 1, GEOMS[0], 6) == (WINO8, 2, False) and plan(ALL_ON, 0, GEOMS[0], 6) == (WINOF4, 1, False)
    assert plan(ALL_ON, 2, GEOMS[0], 48) == (WINO8, 2, False)
    # the test shapes of tests/test_gpu_winof4_entry.py: 3 x 64 x 128 splits both eligible entries under fp32_ksplit 1
    assert plan(ALL_ON, 1, (64, 128, 64, 32, 64), 3)[:2] == (WINO8, 2) and plan(ALL_ON, 1, (128, 256, 128, 16, 32), 3)[:2] == (WINO8, 4)
    assert plan(ALL_ON, 0, (64, 128, 64, 32, 64), 3) == plan(ALL_ON, 0, (128, 256, 128, 16, 32), 3) == (WINOF4, 1, False)
    assert plan(ALL_ON, 0, (256, 512, 256, 8, 16), 3)[0] == DIRECT                  # H = 8: no Winograd kernel


def test_option_row_and_documentation():
    api = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "api.hip")).read()
    assert re.search(r'\{"fp32_winof4_entries", &pnpx_ctx::opt_fp32_winof4_entries, 0, \(1 << 27\) - 1\}', api)
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    doc = header[header.index('"fp32_winof4_entries"'):header.index('"fp32_chains"')]
    for word in ("15, 18 and 21", "fp32_wino8_layers", "K-split", "up-sampling kernel", '"fp32_winof4_layers" never'):
        assert word in doc, word
    common = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "common.h")).read()
    m = re.search(r"int opt_fp32_winof4_entries = ([^;]+);", common)
    default = eval(m.group(1), {})
    assert default & ~((1 << 15) | (1 << 18) | (1 << 21)) == 0
    for name in ("PNPX_PROBE_WINOF4_2SRC = 8", "PNPX_PROBE_WINOF4_UPS = 9", "PNPX_PROBE_WINO8_GRAD = 7", "PNPX_PROBE_WINOF4 = 4"):
        assert name in header, name


def test_probe_plan_of_the_new_kinds():
    P = lambda kind, *g: CL.plan(kind, g)
    for B, c in EC.ENTRY_CASES:
        assert CL.plan(EC.WINOF4_2SRC, c) == (64, 1), c.name
        assert CL.plan(CL.WINOF4, c) == (0, 0)                                    # the single-source kind still refuses a second source
    for g in GEOMS[:3] + ((8, 8, 64, 16, 32), (8, 128, 64, 16, 32)):
        assert P(EC.WINOF4_2SRC, *g) == (64, 1), g
    # refused: no second source, no first source, ragged chunks, a 32-cout tile, W % 32, H % 16, odd sizes
    for g in ((64, 0, 64, 16, 32), (0, 64, 64, 16, 32), (64, 12, 64, 16, 32), (12, 64, 64, 16, 32), (64, 4, 64, 16, 32), (32, 64, 32, 16, 32),
              (64, 128, 96, 16, 32), (64, 128, 64, 16, 16), (64, 128, 64, 16, 48), (64, 128, 64, 24, 32), (64, 128, 64, 17, 32),
              (64, 128, 64, 16, 33), (64, 128, 64, 8, 32)):
        assert P(EC.WINOF4_2SRC, *g) == (0, 0), g
        assert not entry_ok(*g) or g[1] == 0
    # the F(4x4) kernel has no up-sampling instance: its kind refuses everything, the network's own entries included
    for g in GEOMS:
        assert P(EC.WINOF4_UPS, *g) == (0, 0), g
    assert P(10, 64, 128, 64, 16, 32) == (0, 0)


def test_bar_is_eight_times_the_emulation_maximum():
    mx, b = EC.recorded_bar()
    emu, where = EC.emulation_maximum()
    assert emu == pytest.approx(mx, rel=1e-4), (emu, where)                      # the file holds 5 significant digits
    assert b == pytest.approx(CL.BAR_FACTOR * emu, rel=1e-4) and EC.bar() == b
    assert 1e-7 < mx < 1e-5                                                       # the F(4x4) accuracy class (conv_layer_cases: f4)
    # the emulation of the two steps the kernels take: up-sampling in fp32, then F(4x4) over both sources = the "fwd" emulation on the
    # up-sampled operand
    for i, (B, c) in enumerate(EC.ENTRY_CASES):
        cf, df = EC.full_res(c, EC.inputs(i))
        assert (CL.emulate32(cf, df, "f4") == CL.emulate32(c, EC.inputs(i), "f4")).all()


def test_bar_catches_every_mutant():
    b = EC.bar()
    for i, (B, c) in enumerate(EC.ENTRY_CASES):
        ref, den = EC.case_reference(i)
        got = EC.mutants(i)
        assert [n for n, _ in got] == ["weight_zeroed", "input_zeroed", "tile_shifted", "low_source_shifted"]
        for n, m in got:
            assert CL.measure(m[:B], ref[:B], den[:B]) > b, (c.name, n)
