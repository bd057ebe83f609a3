"""CPU side of the per-layer convolution probe: the host-only plan (pnpx_conv3x3_probe_plan), the float64 reference helper, the fp32
emulations the bars come from, and the proof that those bars catch subtle errors (tests/conv_layer_cases.py).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_layer_cases as CL


def test_plan_table():
    """The plan agrees with the plain restatement the GPU suite is parametrised by, on every (kind, case), and refuses the refused."""
    for c in CL.CASES:
        for kind in range(8):
            ct, pieces = CL.plan(kind, c)
            assert ct == CL.accepts(kind, c), (CL.KIND_NAMES[kind], c.name)
            if kind == CL.WINO8_KSPLIT and ct:
                assert pieces == CL.ksplit_pieces(c), c.name
    for kind, *geom in CL.REFUSED:
        assert CL.plan(kind, tuple(geom)) == (0, 0), (CL.KIND_NAMES[kind], geom)
    # every kind runs somewhere, with both tile widths where it has both
    tiles = {k: {CL.accepts(k, c) for kk, c in CL.runs() if kk == k} for k in range(8)}
    assert all(tiles[k] == ({64} if k == CL.WINOF4 else {32, 64}) for k in range(8)), tiles
    assert CL.plan(99, (64, 0, 64, 16, 32)) == (0, 0)


def test_plan_tile_widths_and_ksplit_pieces():
    P = lambda kind, *g: CL.plan(kind, g)
    assert P(CL.WINO8, 32, 0, 32, 16, 32) == (32, 1) and P(CL.WINO8, 32, 0, 64, 16, 16) == (64, 1)
    assert P(CL.WINO8_GRAD, 32, 0, 96, 16, 32) == (32, 1) and P(CL.DIRECT_GRAD, 32, 0, 96, 16, 32) == (32, 1)   # three 32-wide tiles
    assert P(CL.WINO8_GRAD, 256, 0, 768, 16, 16) == (64, 1)
    assert P(CL.WINOF4, 24, 0, 64, 16, 32) == (64, 1)            # an odd chunk count is accepted
    # the K-split cases really split
    for name, pieces in CL.KSPLIT_PIECES.items():
        assert CL.plan(CL.WINO8_KSPLIT, CL.CASE_BY_NAME[name]) == (64, pieces), name
    # conv3x3_wino8.hip's comment: the 16 x 16 level of a 256 x 256 input (256 -> 512, 512 -> 512) splits in 4, the 32 x 32 level
    # (128 -> 256, 256 -> 256) in 2
    assert P(CL.WINO8_KSPLIT, 256, 0, 512, 16, 16) == (64, 4) and P(CL.WINO8_KSPLIT, 512, 0, 512, 16, 16) == (64, 4)
    assert P(CL.WINO8_KSPLIT, 128, 0, 256, 32, 32) == (64, 2) and P(CL.WINO8_KSPLIT, 256, 0, 256, 32, 32) == (64, 2)
    assert P(CL.WINO8_KSPLIT, 64, 0, 64, 64, 64)[1] == 1         # enough tiles: no split
    # a tuning rule: pieces for <= 8 tiles in bits 0-3, for <= 16 in bits 4-7
    assert P(CL.WINO8_KSPLIT, 256, 0, 256, 16, 16) == (64, 4)
    assert CL.plan(CL.WINO8_KSPLIT, (256, 0, 256, 16, 16), ks_rule=0x12) == (64, 2)
    assert CL.plan(CL.WINO8_KSPLIT, (256, 0, 256, 16, 16), ks_rule=0) == (64, 1)
    # fused up-sampling: the smallest accepted geometries and what lies just below them
    assert P(CL.WINO8_UPS, 48, 16, 64, 32, 16) == (64, 1) and P(CL.WINO8_UPS, 32, 16, 64, 32, 16) == (0, 0)
    assert P(CL.WINO8_UPS, 48, 16, 64, 16, 16) == (0, 0)
    assert P(CL.WINO8_UPS, 32, 64, 32, 32, 32) == (32, 1) and P(CL.WINO8_UPS, 24, 64, 32, 32, 32) == (0, 0)
    assert P(CL.WINO8_UPS, 32, 64, 32, 16, 32) == (0, 0)


def test_case_table_covers_both_networks_layer_shapes():
    names = set(CL.CASE_BY_NAME)
    geoms = {(c.op, c.C0, c.C1, c.cout) for c in CL.CASES}
    for g in (("fwd", 32, 0, 32), ("fwd", 32, 0, 64), ("fwd", 64, 0, 64), ("fwd", 128, 0, 256), ("fwd", 512, 0, 512), ("fwd", 32, 64, 32),
              ("fwd", 64, 128, 64), ("fwd", 256, 512, 256), ("adj", 64, 0, 32), ("adj", 512, 0, 256), ("adj", 256, 0, 768), ("adj", 32, 0, 96)):
        assert g in geoms, g
    sizes64 = {(c.H, c.W) for c in CL.CASES if c.cout % 64 == 0}
    assert {(16, 16), (16, 32), (32, 16), (32, 48)} <= sizes64
    assert {(16, 32), (32, 64)} <= {(c.H, c.W) for c in CL.CASES if c.cout in (32, 96)}
    assert set(CL.KSPLIT_PIECES) <= names
    f4 = [c for k, c in CL.runs() if k == CL.WINOF4]
    assert {16, 24} <= {c.C0 for c in f4} and {64, 128} <= {c.cout for c in f4 if c.pool}


def test_reference_helper_against_torch_fp32():
    """The float64 reference, its padding helpers and the emulations' plumbing against torch's own fp32 convolution."""
    for name in ("fwd_64to64_32x48_res", "fwd_32+64to32_16x32", "ups_32+64to32_32x32", "adj_32to96_16x32"):
        c, d = CL.CASE_BY_NAME[name], CL.inputs(name)
        for masked in ((False, True) if c.op == "adj" else (False,)):
            ref, den = CL.case_reference(name, masked)
            if c.op == "adj":
                y = F.conv_transpose2d(d["in0"], d["w"], padding=1)
                y = y * torch.where(d["mask"] > 0, 1.0, CL.SLOPE) if masked else y
            else:
                x = d["in0"]
                if c.C1:
                    x = torch.cat([x, F.interpolate(d["in1"], scale_factor=2, mode="bilinear", align_corners=True) if c.op == "ups" else d["in1"]], 1)
                y = F.leaky_relu(F.conv2d(x, d["w"], d["bias"], padding=1), CL.SLOPE)
                y = y + d["res"] if c.res else y
            assert ref.dtype == torch.float64 and ref.shape == y.shape == den.shape
            assert bool((den > 0).all())
            assert CL.measure(y, ref, den) < 1e-6, name
            assert CL.measure(ref, ref, den) == 0.0
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).view(2, 3, 4, 5) + 1
    xp = CL.pad(x)
    assert xp.shape == (2, 3, 6, 5 + 2 * CL.PADL) and torch.equal(CL.interior(xp), x) and float(CL.border_cells(xp).abs().sum()) == 0.0
    assert CL.border_cells(xp).numel() > xp.numel() - x.numel() - 1      # corners counted twice, nothing left out
    bad = torch.full((1, 1, 2, 2), float("nan"), dtype=torch.float64)
    assert CL.measure(bad, bad, torch.ones_like(bad)) == float("inf")


def test_adjoint_mask_zero_cells():
    """Exact +0.0 and -0.0 mask cells take the factor `slope` (torch's convention: LeakyReLU'(0) = slope), both signs are present."""
    d = CL.inputs("adj_64to32_16x32")
    flat = d["mask"].reshape(-1)
    z = flat[d["zero_cells"]]
    assert bool((z == 0).all()) and bool(torch.signbit(z).any()) and not bool(torch.signbit(z).all())
    assert float(flat[flat != 0].abs().min()) >= 0.1
    ref, _ = CL.case_reference("adj_64to32_16x32", True)
    lin, _ = CL.case_reference("adj_64to32_16x32", False)
    assert torch.equal(ref.reshape(-1)[d["zero_cells"]], lin.reshape(-1)[d["zero_cells"]] * torch.tensor(CL.SLOPE, dtype=torch.float32).double())


def test_emulations_are_the_algorithms():
    """The transform-domain emulations compute the convolution (to fp32 accuracy) and the kernel-arithmetic up-sampling is the bilinear one."""
    d = CL.inputs("fwd_64to64_16x32")
    ref = F.conv2d(d["in0"].double(), d["w"].double(), padding=1)
    for cls, tol in (("f2", 1e-5), ("f4", 1e-4)):
        y = CL.winograd32(d["in0"], d["w"], cls)
        assert y.shape == ref.shape and float((y.double() - ref).abs().max()) < tol * float(ref.abs().max()), cls
    low = CL.inputs("ups_32+64to32_32x32")["in1"]
    up = CL.upsample32(low, 32, 32)
    assert float((up.double() - CL.upsample64(low)).abs().max()) < 1e-5
    w = CL.inputs("adj_32to96_16x32")["w"]
    g = CL.inputs("adj_32to96_16x32")["in0"].double()
    assert torch.allclose(F.conv2d(g, CL.adjoint_weights(w).double(), padding=1), F.conv_transpose2d(g, w.double(), padding=1), rtol=0, atol=1e-12)


def test_recorded_bars_are_eight_times_the_emulation_maxima():
    rec = CL.recorded_bars()
    emu = CL.emulation_maxima()
    for cls in CL.CLASSES:
        mx, b = rec[cls]
        assert emu[cls][0] == pytest.approx(mx, rel=1e-4), (cls, emu[cls])          # the file holds 5 significant digits
        assert b == pytest.approx(CL.BAR_FACTOR * emu[cls][0], rel=1e-4), cls
        assert CL.bar(cls) == b
    # same accuracy classes as a quick trial with random inputs gave: 3e-7 direct, 1.2e-7 F(2x2), 2e-6 F(4x4)
    assert 1e-8 < rec["direct"][0] < 1e-6 and 1e-8 < rec["f2"][0] < 1e-6 and 1e-7 < rec["f4"][0] < 1e-5


def test_bars_catch_every_mutant():
    """One zeroed weight, one zeroed input element, one flipped mask sign, one tile shifted by a pixel: each beyond EVERY class's bar at
    EVERY case."""
    widest = max(CL.bar(cls) for cls in CL.CLASSES)
    for c in CL.CASES:
        for masked in ((False, True) if c.op == "adj" else (False,)):
            ref, den = CL.case_reference(c.name, masked)
            got = CL.mutants(c, CL.inputs(c.name), masked)
            assert {n for n, _ in got} == {"weight_zeroed", "input_zeroed", "tile_shifted"} | ({"mask_flipped"} if masked else set())
            for n, m in got:
                assert CL.measure(m, ref, den) > widest, (c.name, masked, n)


def test_impulse_cases():
    """Distinct dyadic weights, one site per image, sites on both sides of every tile and region boundary, channels of every chunk class."""
    for c in CL.IMPULSE_CASES:
        w = CL.impulse_weights(c)
        assert w.unique().numel() == w.numel() and float(w.abs().max()) < 4.0
        assert torch.equal((w.double() * 2.0 ** 22).round(), w.double() * 2.0 ** 22)
        chunk = 16 if c.cout % 64 == 0 else 8
        sites = CL.impulse_sites(c, chunk)
        xs, ys = {s[3] for s in sites}, {s[2] for s in sites}
        assert {0, 1, 15, c.W - 1} <= xs and {0, 1, 15, c.H - 1} <= ys
        assert ({16, 17, 31} <= xs) == (c.W >= 32) and ({16, 17, 31} <= ys) == (c.H >= 32) and ((32 in xs) == (c.W > 32))
        assert {(0, 0), (0, c.W - 1), (c.H - 1, 0), (c.H - 1, c.W - 1)} <= {(s[2], s[3]) for s in sites}
        ch0 = {s[1] for s in sites if s[0] == "in0"}
        assert {0, chunk - 1, c.C0 - chunk, c.C0 - 1} <= ch0
        if c.C1 and c.op != "ups":
            assert {0, c.C1 - 1} <= {s[1] for s in sites if s[0] == "in1"}
        d = CL.impulse_inputs(c, sites, CL.impulse_planes(c))
        assert float(d["in0"].sum() + (d["in1"][:len(sites)].sum() if c.C1 else 0)) == len(sites)
        # the reference of an impulse is the flipped stencil, exactly
        if c.op == "fwd" and not c.C1:
            ref, _ = CL.reference(c, d, slope=CL.IMPULSE_SLOPE)
            src, ch, y, x = sites[0]
            assert (y, x) == (0, 0)
            want = F.leaky_relu(w[:, ch, :2, :2].double(), CL.IMPULSE_SLOPE).flip(1, 2)
            assert torch.equal(ref[0, :, :2, :2], want) and float(ref[0].abs().sum()) == float(want.abs().sum())
