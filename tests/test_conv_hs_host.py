"""CPU side of the half-split single-layer probe: the host-only plan (pnpx_conv_hs_probe_plan) against the case table and over the coverage
sweep, the HS8 codec, the float64 reference against torch's own convolution, the fp32 emulation the bars come from, and the proof that
those bars catch subtle errors (tests/conv_hs_cases.py).  No GPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import conv_hs_cases as HS


def test_every_case_runs_the_instance_the_table_expects():
    for c in HS.CASES:
        p = HS.plan(c)
        assert p is not None and HS.expected(p) == c.expect, (c.name, p, c.expect)
        mt, nbw, mbw, nw = p[:4]
        tw, th = mbw, nw * nbw * (32 // mbw)
        tiles = (c.cout // mt) * -(-c.W // tw) * -(-c.H // th) * c.B
        assert p[10] == tiles and p[9] == (tiles if p[11] else p[9]) and (p[11] == 1) == (tiles <= 256), (c.name, p)
    # the walks nothing else reaches: nct = 3 rounds the persistent grid down to a multiple of 8 * nct; a persistent launch with fewer than 32
    # regions; a persistent 16-pixel block with a partial last tile
    p = HS.plan(HS.CASE_BY_NAME["act1ff_16to192_64x40_B32"])
    assert (p[0], p[9], p[10], p[11]) == (64, 240, 768, 0) and 192 // p[0] == 3
    p = HS.plan(HS.CASE_BY_NAME["act1ff_16to1024_4x4_B17"])
    assert p[11] == 0 and p[10] > 256 and p[10] // (1024 // p[0]) < 32
    p = HS.plan(HS.CASE_BY_NAME["act1ff_16to512_4x24_B32"])
    assert p[2] == 16 and p[11] == 0 and 24 % 16 != 0


def test_the_table_holds_the_edges_of_every_operand():
    cs = HS.CASES
    assert {0.0, 0.2, 1.0} <= {c.slope for c in cs if c.epi in ("act", "dmask", "res")}
    for epi in ("trelu", "dthr"):
        al = {c.alpha for c in cs if c.epi == epi}
        assert min(al) < 0 and 0.0 in al and max(al) > 0
    assert any(c.epi == "dthr" and c.res and 0 < c.res_groups < c.cout // 8 for c in cs)
    assert any(c.epi == "dthr" and not c.dmask for c in cs) and any(c.epi == "trelu" and c.res for c in cs)
    assert any(c.G1 and c.G0 > c.G1 and not c.ups for c in cs) and any(c.G1 and c.G0 < c.G1 for c in cs)
    assert any(c.in0_groups > c.G0 for c in cs) and any(c.cin % 16 for c in cs)
    assert any(c.W == 40 and c.H % 2 and c.H < 8 for c in cs)
    assert {(c.expect[0], c.expect[8]) for c in cs if c.cin == 512 and (c.H, c.W, c.B) == (8, 8, 1)} == {(32, 32), (32, 64)}
    # the four weights-in-registers instances, the folded first convolution, both up-sampling instances (one with a partial last tile)
    wr = {(c.expect[1], c.expect[3], c.expect[4], c.expect[6]) for c in cs if c.expect[6]}
    assert wr == {(2, 8, 0, 1), (4, 4, 0, 1), (2, 8, 1, 1), (4, 4, 1, 1), (2, 8, 0, 2)}, wr
    ups = [c for c in cs if c.ups]
    assert {c.expect[0] for c in ups} == {32, 64} and any(c.W % 32 and c.H % 16 for c in ups)
    # fused pool under every (NBW, NW) it can run with
    assert {(c.expect[1], c.expect[3]) for c in cs if c.pool and not c.expect[6]} == {(2, 4), (4, 4), (2, 8)}


@functools.lru_cache(maxsize=None)
def _sweep():
    """{instance: a geometry that selects it} and the (instance, packing tile, walk) combinations, over the coverage grid."""
    inst, full = {}, set()
    for c in HS.sweep_grid():
        p = HS.plan(c)
        if p is not None:
            inst.setdefault(p[:8], c.name)
            full.add(HS.expected(p))
    return inst, full


def test_every_instance_the_sweep_finds_is_run():
    inst, full = _sweep()
    assert len(inst) > 100            # "more than a hundred compiled instances"
    run = {c.expect[:8] for c in HS.CASES}
    missing = {k: v for k, v in inst.items() if k not in run and k not in HS.EXEMPT}
    assert not missing, missing
    assert not (set(HS.EXEMPT) & run), "an exempted instance is selected by a case"
    # the plain convolution also under every (instance, packing tile, walk) combination the launcher produces on the grid
    plain = {k for k in full if k[4:8] == (0, 0, 0, 0x1FF)}
    assert plain <= {c.expect for c in HS.CASES}, plain - {c.expect for c in HS.CASES}


def test_refused_combinations_have_no_plan():
    for name, kw, _ in HS.REFUSED:
        assert HS.plan(HS.refused_case(kw)) is None, name
    # operands the selected path has no place for: refused by the probe, never dropped
    c = HS.CASE_BY_NAME["act1ff_16to32_4x32_B1_pool"]
    assert HS.plan(c) is not None
    assert HS.plan(c._replace(H=5)) is None and HS.plan(c._replace(W=16)) is None          # no pool is fused there
    assert HS.plan(c._replace(epi="dmask", dmask=True)) is None and HS.plan(c._replace(epi="res", res=True)) is None
    assert HS.plan(c._replace(pool=False, res_groups=2)) is None and HS.plan(c._replace(pool=False, alpha=0.5)) is None
    assert HS.plan(c._replace(pool=False, in0_groups=1)) is None
    assert HS.plan(HS.CASE_BY_NAME["dmask1ff_16to32_7x40_B2"]._replace(res=True)) is None   # res beside dmask
    assert HS.plan(HS.CASE_BY_NAME["act1ff_32to32_20x40_B64_first"]._replace(B=8)) is None  # too few tiles to fold the first layer


def test_hs8_codec():
    x = torch.randn(2, 16, 3, 5, generator=torch.Generator().manual_seed(1))
    r = HS.hs8_encode(x)
    assert r.dtype == torch.float16 and r.shape == (2, 2, 5, 7, 16)
    assert bool((HS.hs8_border(r).view(torch.int16) == 0).all()) and HS.hs8_border(r).numel() >= r.numel() - 2 * 2 * 3 * 5 * 16
    # record (b, g, y + 1, x + 1): hi of channels 8 g .. 8 g + 7, then their lo; hi = f16(16 v), lo = f16(16 v - hi)
    v = 16.0 * x[1, 11, 2, 4]
    hi = v.half()
    assert r[1, 1, 3, 5, 3] == hi and r[1, 1, 3, 5, 11] == (v - hi.float()).half()
    back = HS.hs8_decode(r)
    assert back.dtype == torch.float64 and torch.equal(back, HS.quantize(x))
    assert float((back - x.double()).abs().max() / x.abs().max()) < 2.0 ** -21
    one = torch.zeros(1, 8, 1, 1)
    one[0, 3] = 1.0
    assert float(HS.hs8_encode(one)[0, 0, 1, 1, 3]) == 16.0
    assert HS.threshold(0.3) == float(HS.hs8_decode(HS.hs8_encode(torch.full((1, 8, 1, 1), 0.3)))[0, 0, 0, 0])


def _torch_reference(c, d):
    """The case by torch's own float64 convolution, written without the helpers of the module under test."""
    mask = torch.tensor([[float((c.taps >> (3 * i + j)) & 1) for j in range(3)] for i in range(3)], dtype=torch.float64)
    w = d["w"].double() * mask
    if c.first:
        xs = torch.stack([d["first_x"], d["first_sigma"].view(-1, 1, 1).expand(-1, c.H, c.W)], 1).double()
        x = F.leaky_relu(F.conv2d(xs, d["first_w"].double(), d["first_b"].double(), padding=1), HS.FIRST_SLOPE)
    else:
        x = HS.hs8_decode(HS.hs8_encode(d["in0"]))[:, :8 * c.G0]
    if c.G1:
        x1 = HS.hs8_decode(HS.hs8_encode(d["in1"]))
        x = torch.cat([x, F.interpolate(x1, scale_factor=2, mode="bilinear", align_corners=True) if c.ups else x1], 1)
    t = F.conv2d(x[:, :c.cin], w, d["bias"].double() if "bias" in d else None, padding=1)
    if c.res:
        r = HS.hs8_decode(HS.hs8_encode(d["res"]))
        t[:, :r.shape[1]] += r
    sl = float(torch.tensor(c.slope, dtype=torch.float32))
    if c.epi in ("act", "res"):
        return {"out": F.leaky_relu(t, sl)}
    if c.epi == "trelu":
        a = float(torch.tensor(c.alpha, dtype=torch.float32))
        return {"out": F.relu(t - a) + a}
    m = HS.hs8_decode(HS.hs8_encode(d["dmask"])) if c.dmask else None
    if c.epi == "dmask":
        return {"out": t * torch.where(m > 0, 1.0, sl)}
    if c.epi == "dthr":
        return {"out": t * (m > HS.threshold(c.alpha)) if c.dmask else t}
    pre = d["x_in"].double() + F.conv2d(F.leaky_relu(t, sl), d["outc_w"].double().view(1, 32, 1, 1), d["outc_b"].double())[:, 0]
    return {"pre": pre, "img": pre.clamp(0, 1)}


CHECKED = ("act01b_16to64_4x16_B1", "act010_16to32_4x4_B1", "outc1ff_16to32_5x40_B2", "dmask1ff_16to32_7x40_B2_sl0", "res1ff_16to64_5x40_B2_res",
           "trelu01b_16to128_9x40_B2_res_a-0.25", "dthr1b0_16to128_9x40_B2_res_rg4_a-0.25", "dthr1ff_16to64_6x24_B2_a0.3_nomask",
           "act1ff_48+16to32_8x40_B2", "act1ff_48+32to64_8x24_B2", "act1ff_24to32_8x40_B2", "act1ff_16to32_8x40_B2_g4",
           "act1ff_64+32to64_10x40_B2_ups", "act1ff_32to32_20x40_B64_first")


@pytest.mark.parametrize("name", CHECKED)
def test_reference_against_torch_float64(name):
    c = HS.CASE_BY_NAME[name]
    d = HS.take(HS.inputs(c), 0, 2)
    ref, want = HS.reference(c, d), _torch_reference(c, d)
    for k, v in want.items():
        assert ref[k].dtype == torch.float64 and ref[k].shape == v.shape
        assert float((ref[k] - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), (name, k)
    den = ref["den_img" if c.epi == "outc" else "den"]
    assert bool((den > 0).all()) and bool((den >= ref["pre" if c.epi == "outc" else "out"].abs() * (1 - 1e-12)).all())
    assert HS.case_measure(c, ref, ref) == 0.0
    bad = {k: torch.full_like(v, float("nan")) for k, v in want.items()}
    assert HS.case_measure(c, bad, ref) == float("inf")


def test_mask_cells_sit_on_the_decision():
    for name in ("dmask1ff_16to32_7x40_B2", "dthr1ff_16to64_6x24_B2_a0.3", "dthr1ff_16to64_6x24_B2_a-0.25", "dthr1ff_16to64_6x24_B2_a0"):
        c = HS.CASE_BY_NAME[name]
        d = HS.inputs(c)
        m = HS.quantize(d["dmask"]).view(c.B, -1)
        centre = HS.threshold(c.alpha) if c.epi == "dthr" else 0.0
        for b in range(c.B):
            assert float(m[b, 0]) == centre and float(m[b, 1]) == 0.0 and float(m[b, 2]) == 0.0 and bool(torch.signbit(d["dmask"].view(c.B, -1)[b, 2]))
        off = (m - centre).abs()
        assert float(off[off > 0].min()) > 0.09
        # a cell exactly at the threshold is masked out, and takes the slope in the LeakyReLU gradient
        ref = HS.reference(c, d)
        lin = HS.reference(c._replace(dmask=False), d)["out"] if c.epi == "dthr" else None
        at = (m == centre).view(ref["out"].shape)
        assert int(at.sum()) >= c.B
        if c.epi == "dthr":
            assert bool((ref["out"][at] == 0).all()) and bool((ref["out"][~at & (m.view(at.shape) > centre)] == lin[~at & (m.view(at.shape) > centre)]).all())


def test_emulation_is_the_half_split_arithmetic():
    """Three products of f16 halves per operand pair: the emulation is within 1e-6 of the reference, its dropped w_lo x_lo term shows."""
    c = HS.CASE_BY_NAME["act1ff_16to32_5x40_B2"]
    d = HS.inputs(c)
    s, wh, wl = HS.weight_halves(d["w"])
    assert 2.0 ** 13 <= s * float(d["w"].abs().max()) < 2.0 ** 14
    assert float(((wh.double() + wl.double()) / s - d["w"].double()).abs().max()) <= 2.0 ** -21 * float(d["w"].abs().max())
    e = HS.case_measure(c, HS.emulate32(c, d), HS.reference(c, d))
    assert 1e-9 < e < 1e-6


def test_recorded_bars_are_eight_times_the_emulation_maxima():
    rec = HS.recorded_bars()
    emu = HS.emulation_maxima()
    for cls in HS.CLASSES:
        mx, b = rec[cls]
        assert emu[cls][0] == pytest.approx(mx, rel=1e-4), (cls, emu[cls])          # the file holds 5 significant digits
        assert b == pytest.approx(HS.BAR_FACTOR * emu[cls][0], rel=1e-4), cls
        assert HS.bar(cls) == b
        assert 1e-9 < mx < 1e-6, cls                                               # an fp32-class accuracy


def test_bars_catch_every_mutant():
    """A dropped cross term, one tap shifted by a pixel, two weight rows exchanged against hs_row_channel: each beyond its class's bar."""
    assert set(HS.MUTANT_CASES) == set(HS.CLASSES)
    for cls, name in HS.MUTANT_CASES.items():
        c = HS.CASE_BY_NAME[name]
        assert c.cls == cls
        d = HS.take(HS.inputs(c), 0, HS.EMU_IMAGES)
        ref = HS.reference(c, d)
        got = HS.mutants(c, d)
        assert [n for n, _ in got] == ["cross_term_dropped", "tap_shifted", "rows_exchanged"]
        for n, m in got:
            assert HS.case_measure(c, m, ref) > HS.bar(cls), (name, n)
