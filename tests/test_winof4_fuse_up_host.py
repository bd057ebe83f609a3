"""CPU side of the F(4x4,3x3) kernel's up-sampling instance (option fp32_winof4_fuse_up): the selector's rows with the option's bit
(pnpx_conv_f32_entry_plan, opts bit 7) against a plain restatement, the probe plan of kind PNPX_PROBE_WINOF4_FUSE_UP, the option's table
row and documentation, and the restatement of the kernel's window-and-table interpolation (tests/winof4_fuse_up_cases.py) against the
separate up-sampling kernel's, with the mutants that must break their equality.  No GPU."""
import itertools
import os
import re

import numpy as np

from tests import conv_layer_cases as CL
from tests import winof4_entry_cases as EC
from tests import winof4_fuse_up_cases as FU
from tests.test_winof4_entry_host import ALL_ON, BATCHES, BIT8, BITENTRY, BITF4, FUSE_UP, GEOMS, PACKED4, ROOT, WINO8, WINOF4, WINOGRAD, expected, plan

BITFUSE = 1 << 7                                           # the layer's fp32_winof4_fuse_up bit
EVERYTHING = ALL_ON | BITFUSE
# beside the entry grid: the fused instance's own boundary (one and two chunks of the first source) and the cases of the GPU test
MORE_GEOMS = ((8, 16, 64, 16, 32), (16, 8, 64, 16, 32), (16, 16, 64, 48, 96), (24, 8, 64, 16, 32))


def expected_fused(opts, ksplit, geom, B):
    """DESIGN.md's entry table with the option's bit: only an F(4x4) row can change, and only its `fused`."""
    k, pieces, fused = expected(opts & 127, ksplit, geom, B)
    if k == WINOF4:
        fused = bool(opts & BITFUSE and FU.ups_ok(*geom))
    return k, pieces, fused


def test_selector_rows_with_the_option():
    seen = set()
    for geom, B, ksplit in itertools.product(GEOMS + MORE_GEOMS, BATCHES, (0, 1, 2)):
        for low in range(128):
            base = plan(low, ksplit, geom, B)
            assert base == expected(low, ksplit, geom, B), (geom, B, ksplit, bin(low))     # bit 7 clear: today's plan
            got = plan(low | BITFUSE, ksplit, geom, B)
            assert got == expected_fused(low | BITFUSE, ksplit, geom, B), (geom, B, ksplit, bin(low), got)
            assert got[:2] == base[:2]                                                     # the bit never moves a layer to another kernel
            if got != base:
                assert base == (WINOF4, 1, False) and got == (WINOF4, 1, True)
            seen.add(got)
    # (with the bit set no F(4x4) row stays unfused in the selector: a 64-cout entry reaches it through the 8-wave kernel's rule, whose
    # sources are multiples of 16 channels, so it always has its two chunks; the one-chunk refusal shows in the probe plan)
    assert {(WINOF4, 1, True), (WINO8, 1, True), (WINO8, 1, False), (WINO8, 2, False), (WINO8, 4, False)} <= seen, seen
    assert (WINOF4, 1, False) not in seen


def test_the_headline_shape_and_its_neighbours():
    for geom in GEOMS[:3]:
        assert plan(EVERYTHING, 1, geom, 48) == (WINOF4, 1, True)
        assert plan(EVERYTHING & ~BITFUSE, 1, geom, 48) == (WINOF4, 1, False)              # the option off: the two-launch form
        assert plan(EVERYTHING & ~FUSE_UP, 1, geom, 48) == (WINOF4, 1, True)               # fp32_fuse_up has no say
        assert plan(EVERYTHING & ~BITENTRY, 1, geom, 48) == (WINO8, 1, True)               # the bit alone puts no entry on the kernel
        assert plan(EVERYTHING & ~BITENTRY | BITF4, 1, geom, 48) == (WINO8, 1, True)
        assert plan(EVERYTHING & ~PACKED4, 1, geom, 48) == (WINO8, 1, True)
        assert plan(EVERYTHING & ~BIT8, 1, geom, 48)[2] is False and plan(EVERYTHING & ~WINOGRAD, 1, geom, 48)[2] is False
    assert plan(EVERYTHING, 1, GEOMS[3], 48) == (WINO8, 1, True)                           # level 0's entry stays on the 8-wave kernel
    # K-split calls are unchanged
    assert plan(EVERYTHING, 1, GEOMS[0], 6) == plan(ALL_ON, 1, GEOMS[0], 6) == (WINO8, 2, False)
    assert plan(EVERYTHING, 2, GEOMS[0], 48) == plan(ALL_ON, 2, GEOMS[0], 48) == (WINO8, 2, False)
    assert plan(EVERYTHING, 0, GEOMS[0], 6) == (WINOF4, 1, True)
    # the shapes of tests/test_gpu_winof4_fuse_up.py's forward checks: fused without the K-split, untouched with it
    for geom, B in (((64, 128, 64, 16, 32), 1), ((64, 128, 64, 32, 64), 3), ((128, 256, 128, 16, 32), 3), ((256, 512, 256, 16, 32), 1)):
        assert plan(EVERYTHING, 0, geom, B) == (WINOF4, 1, True), geom
        assert plan(EVERYTHING, 1, geom, B) == plan(ALL_ON, 1, geom, B) and plan(EVERYTHING, 1, geom, B)[0] == WINO8, geom
    # one chunk of either source: no Winograd kernel of the forward takes the entry, with or without the bit
    for geom in ((8, 16, 64, 16, 32), (16, 8, 64, 16, 32)):
        assert plan(EVERYTHING, 0, geom, 48) == plan(ALL_ON, 0, geom, 48) and plan(EVERYTHING, 0, geom, 48)[0] not in (WINO8, WINOF4), geom


def test_probe_plan_of_the_fused_kind():
    P = lambda kind, *g: CL.plan(kind, g)
    for B, c in FU.CASES:
        assert CL.plan(FU.FUSE_UP, c) == (64, 1), c.name
    for g in GEOMS[:3] + ((16, 8, 64, 16, 32), (16, 128, 64, 16, 32)):
        assert P(FU.FUSE_UP, *g) == (64, 1), g
    # refused: whatever the two-source kind refuses (tests/test_winof4_entry_host.py's list), odd targets, too few first-source chunks
    for g in ((64, 0, 64, 16, 32), (0, 64, 64, 16, 32), (64, 12, 64, 16, 32), (12, 64, 64, 16, 32), (64, 4, 64, 16, 32), (32, 64, 32, 16, 32),
              (64, 128, 96, 16, 32), (64, 128, 64, 16, 16), (64, 128, 64, 16, 48), (64, 128, 64, 24, 32), (64, 128, 64, 17, 32),
              (64, 128, 64, 16, 33), (64, 128, 64, 8, 32), (64, 128, 64, 18, 34), (8, 16, 64, 16, 32), (8, 128, 64, 32, 64)):
        assert P(FU.FUSE_UP, *g) == (0, 0), g
        assert not FU.ups_ok(*g) or g[1] == 0
    assert P(EC.WINOF4_2SRC, 8, 16, 64, 16, 32) == (64, 1)                          # (the two-source kind takes one chunk)
    for g in GEOMS + MORE_GEOMS:
        assert P(FU.FUSE_UP, *g) == ((64, 1) if FU.ups_ok(*g) else (0, 0)), g
        assert P(EC.WINOF4_UPS, *g) == (0, 0) and P(10, *g) == (0, 0), g            # 9 stays reserved, 10 stays unknown


def test_option_row_and_documentation():
    api = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "api.hip")).read()
    assert re.search(r'\{"fp32_winof4_fuse_up", &pnpx_ctx::opt_fp32_winof4_fuse_up, 0, \(1 << 27\) - 1\}', api)
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    doc = header[header.index('"fp32_winof4_fuse_up" (layer mask'):header.index('"fp32_chains"')]
    for word in ("15, 18 and 21", "fp32_winof4_entries", "K-split", "up-sampling kernel", "bit-identical", "C0 >= 16"):
        assert word in doc, word
    for name in ("PNPX_PROBE_WINOF4_FUSE_UP = 11", "PNPX_PROBE_WINOF4_UPS = 9", "PNPX_PROBE_WINOF4_2SRC = 8"):
        assert name in header, name
    assert "bit 7" in header[header.index("Host-only, for tests: which kernel a UNet decoder entry"):]
    common = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "common.h")).read()
    default = eval(re.search(r"int opt_fp32_winof4_fuse_up = ([^;]+);", common).group(1), {})
    assert default & ~((1 << 15) | (1 << 18) | (1 << 21)) == 0


def _same(a, b):
    return bool((a.view(np.int32) == b.view(np.int32)).all())


def test_window_form_equals_the_separate_kernel_and_mutants_break_it():
    """The equality tests/test_gpu_winof4_fuse_up.py asserts on the GPU can fail: on every case's own low-resolution source the window
    form restated on the CPU gives the separate kernel's bits, and a window whose origin is off by one or tables with h and l swapped do
    not.  The UNCLAMPED second tap is a different matter: at exactly twice the size with align_corners, s * (2n - 1) rounds to n - 1
    exactly for every n, so the one index whose second tap the clamp moves carries l = 0, and on the layout's zero border the unclamped
    tap adds 0 * 0.  The mutant therefore cannot change a finite result (shown here); it does once the border cell holds anything that
    0 does not annihilate, which the clamped form never reads (shown with an infinite border)."""
    for n in range(2, 4097):
        s = np.float32(n - 1) / np.float32(2 * n - 1)
        assert np.float32(s * np.float32(2 * n - 1)) == np.float32(n - 1), n
    for i, (B, c) in enumerate(FU.CASES):
        low = FU.inputs(i)["in1"][:B, :8].numpy()
        sep = FU.upsample_separate(low)
        assert _same(FU.upsample_windowed(low), sep), c.name
        assert _same(FU.upsample_windowed(low, border=np.inf), sep), c.name                  # no border cell is ever a tap
        for m in ("origin", "swapped"):
            assert not _same(FU.upsample_windowed(low, m), sep), (c.name, m)
        assert _same(FU.upsample_windowed(low, "unclamped"), sep), c.name
        assert not _same(FU.upsample_windowed(low, "unclamped", border=np.inf), sep), c.name
        # the restated separate kernel is the bilinear x2 of the float64 reference, to fp32 rounding: the position f = s * index < 48
        # carries up to 2 x 2^-24 f = 6e-6 (s rounded, the product rounded), times a neighbour difference below 10 for these inputs
        assert float(np.abs(sep - CL.upsample64(FU.inputs(i)["in1"][:B, :8]).numpy()).max()) < 6e-5
