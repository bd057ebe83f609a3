"""CPU side of the probe of the launches between the denoisers' forward convolutions (tests/fwd_glue_cases.py): the host-only plan
(pnpx_fwd_glue_probe_plan) against a plain restatement of every form decision, refusal and launch count; the case table against the
forms; the restatements and emulations against the float64 references; the derived bars against profiles/fwd_glue_probe.md; and the
mutants each bar must catch.  No GPU."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import fwd_glue_cases as FG

ROOT = FG.ROOT


def test_symbols_are_declared_and_bound():
    from tfpnp_amd import _lib
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    for name in ("pnpx_fwd_glue_probe", "pnpx_fwd_glue_probe_plan"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name), name
    body = re.search(r"typedef struct pnpx_fwd_glue_probe_desc \{(.*?)\} pnpx_fwd_glue_probe_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?(unsigned|void|float|int)\s*", "", decl.strip())
        names += [n.strip(" *\n") for n in decl.split(",") if n.strip()]
    assert names == [f[0] for f in _lib.FwdGlueProbeDesc._fields_], names
    ops = re.search(r"enum pnpx_fwd_glue_op \{(.*?)\};", header, flags=re.S).group(1)
    assert [n for n, _ in re.findall(r"PNPX_FWD_(\w+) = (\d+)", ops)] == list(FG.OP_NAMES)


def test_walks_launch_through_the_shared_launchers():
    """No glue kernel of the list is launched outside its launcher: each kernel's name appears in one hipLaunchKernelGGL of its file."""
    csrc = os.path.join(ROOT, "tfpnp_amd", "csrc")
    kernels = {"unet.hip": ("prep_input_kernel", "prep_input_hs_kernel", "maxpool2_kernel", "maxpool2_hs_kernel", "upsample2x_kernel", "upsample2x_v4_kernel",
                            "(upsample2x_hs_kernel<64, 4>)", "(upsample2x_hs_kernel<32, 2>)", "outc_residual_kernel", "outc_residual_hs_kernel",
                            "conv_first_f32_kernel", "conv_first_hs_kernel"),
               "drunet_f32.hip": ("f32_s2d_kernel", "f32_d2s_kernel", "f32_add_kernel", "f32_out_kernel", "f32_tail_mask_kernel", "f32_input_grad_kernel"),
               "drunet.hip": ("dru_add_kernel", "dru_tail_mask_kernel", "hs_s2d_kernel", "hs_d2s_kernel")}
    for name, ks in kernels.items():
        src = open(os.path.join(csrc, name)).read()
        for k in ks:
            assert src.count("hipLaunchKernelGGL(%s," % k) == 1, (name, k)
    both = open(os.path.join(csrc, "drunet.hip")).read() + open(os.path.join(csrc, "drunet_f32.hip")).read()
    assert '"conv_first.h"' not in both and "f32_prep_kernel" not in both      # one copy of each: unet.hip's


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan

def test_plan_against_the_restated_predicates():
    sweeps = 0
    for fam in (0, 1):
        for w in range(1, 71):                                   # every width: the 16-byte form, the half-split tile boundary at 2w = 32
            for B, C in ((1, 8), (3, 16), (8191, 8), (8192, 8), (65535, 8), (65536, 8), (1023, 512), (1024, 512), (8193, 64)):
                for odd in (0, 1):
                    kw = dict(B=B, C=C, H=2, W=w, Ht=4 + odd, Wt=2 * w + odd)
                    for form in (0, 1, 2, 3):
                        assert FG.plan(FG.UPSAMPLE2X, fam, form, **kw) == FG.plan_restated(FG.UPSAMPLE2X, fam, form, **kw), (fam, form, kw)
                        sweeps += 1
            assert FG.plan(FG.UPSAMPLE2X, fam, B=3, C=8, H=2, W=w, Ht=4, Wt=2 * w)[0] == FG.ups_form(fam, 3 if fam else 24, w)
            kw = dict(B=2, C=32, H=5, W=w, sigma_stride=1, slope=0.2)
            assert FG.plan(FG.CONV_FIRST, fam, **kw) == FG.plan_restated(FG.CONV_FIRST, fam, **kw) == ((1, 1) if fam or w % 4 == 0 else (0, 0)), (fam, w)
    assert sweeps == 2 * 70 * 9 * 2 * 4
    # plane counts around the limit: fp32 takes the scalar form above 65535 planes, half-split slices over whole images
    for planes in (65534, 65535, 65536, 65537):
        assert FG.plan(FG.UPSAMPLE2X, 0, B=1, C=planes, H=1, W=2, Ht=2, Wt=4) == ((FG.UPS_V4 if planes <= 65535 else FG.UPS_SCALAR), 1)
        assert FG.plan(FG.UPSAMPLE2X, 0, FG.UPS_V4, B=1, C=planes, H=1, W=2, Ht=2, Wt=4) == ((FG.UPS_V4, 1) if planes <= 65535 else (0, 0))
        assert FG.plan(FG.UPSAMPLE2X, 1, B=planes, C=8, H=1, W=1, Ht=2, Wt=2) == (FG.UPS_HS32, 1 if planes <= 65535 else 2)
    for B, G in ((128, 64), (1023, 64), (1024, 64), (5000, 64), (8193, 8), (70000, 3)):
        form, n = FG.plan(FG.UPSAMPLE2X, 1, B=B, C=8 * G, H=1, W=1, Ht=2, Wt=2)
        per = FG.GRID_Z_MAX // G
        assert form == FG.UPS_HS32 and n == -(-B // per) and per * G <= FG.GRID_Z_MAX and n * per >= B > (n - 1) * per, (B, G)
    assert FG.plan(FG.UPSAMPLE2X, 1, B=2, C=8 * 65536, H=1, W=1, Ht=2, Wt=2) == (0, 0)        # one image alone is over the limit
    c = FG.UPS_HS_SLICED
    assert FG.plan(FG.UPSAMPLE2X, 1, B=c.B, C=c.C, H=c.h, W=c.w, Ht=c.Ht, Wt=c.Wt) == (FG.UPS_HS32, 2)


def test_plan_of_every_op_and_its_refusals():
    shapes = (dict(B=1, C=0, H=4, W=4), dict(B=2, C=8, H=4, W=4), dict(B=2, C=32, H=4, W=8), dict(B=2, C=32, H=5, W=7), dict(B=2, C=12, H=4, W=4),
              dict(B=2, C=64, H=4, W=8, k=2, slope=0.2, sigma_stride=1), dict(B=2, C=64, H=4, W=8, k=25, slope=1.0), dict(B=2, C=8, H=4, W=4, Ht=8, Wt=9),
              dict(B=0, C=8, H=4, W=4), dict(B=2, C=8, H=1, W=4), dict(B=65536, C=32, H=4, W=4), dict(B=2, C=0, H=3, W=3, sigma_stride=3),
              dict(B=2, C=2, H=3, W=3), dict(B=2, C=1, H=3, W=3))
    ran = set()
    for op in range(-1, 12):
        for fam in (0, 1, 2):
            for kw in shapes:
                for form in (0, 1, 2):
                    got = FG.plan(op, fam, form, **kw)
                    assert got == FG.plan_restated(op, fam, form, **kw), (op, fam, form, kw)
                    if got != (0, 0):
                        ran.add((op, fam, got[0]))
    assert ran == FG.all_forms()              # every op runs in every family that has it, and nothing else does


def test_case_table_reaches_every_form_of_every_op_in_both_families():
    assert FG.reached_forms() == FG.all_forms()
    # ... and each case is admitted by the plan with the form the tables expect
    for c in FG.FIRST_CASES:
        assert FG.plan(FG.CONV_FIRST, c.family, B=c.B, C=c.cout, H=c.H, W=c.W, sigma_stride=c.sigma_stride, k=c.k, slope=c.slope) == (1, 1), c.name
    for c in FG.UPS_CASES:
        for fam in (0, 1):
            planes = c.B * (c.C // 8 if fam else c.C)
            for f in (1, 2):
                want = (f, 1) if f in FG.ups_forms_admitted(fam, planes, c.w) else (0, 0)
                assert FG.plan(FG.UPSAMPLE2X, fam, f, B=c.B, C=c.C, H=c.h, W=c.w, Ht=c.Ht, Wt=c.Wt) == want, (c.name, fam, f)
    # the branches the sizes were chosen for
    w_of = lambda fam, f: {c.w for c in FG.UPS_CASES if f in FG.ups_forms_admitted(fam, 3, c.w)}
    assert {8, 16, 17} <= {c.w for c in FG.UPS_CASES} and FG.ups_form(1, 3, 16) == FG.UPS_HS32 and FG.ups_form(1, 3, 17) == FG.UPS_HS64
    assert 17 not in w_of(0, FG.UPS_V4) and {2, 66, 130} <= w_of(0, FG.UPS_V4)
    assert any(c.Ht == 2 * c.h + 1 for c in FG.UPS_CASES) and any(2 * c.h % 4 for c in FG.UPS_CASES if c.w % 2 == 0)
    assert any(H * (W // 4) > 256 for _, H, W in FG.QUAD_SHAPES) and any(W > 64 for _, _, W in FG.IMAGE_SHAPES)
    assert {c.sigma_stride for c in FG.PREP_CASES} == {0, 1, 3} and {c.sigma_stride for c in FG.FIRST_CASES} == {0, 1, 3}
    assert {(c.H * c.W) for c in FG.INGRAD_CASES} == {5, 64, 65, 50 * 39}


# ---------------------------------------------------------------------------------------------------------------------------------
# exact ops: the restatements against plain float64 torch, and their mutants

@pytest.mark.parametrize("case", FG.PREP_CASES, ids=lambda c: c.name)
def test_prep_restatement_and_the_border_mutant(case):
    c, d = case, FG.prep_inputs(case.name)
    y = FG.prep_restate(c, d)
    s = FG.sigma_of(d, c.B, c.sigma_stride)
    assert torch.equal(FG.interior(y)[:, 0], d["x"]) and torch.equal(FG.interior(y)[:, 1], s.view(-1, 1, 1).expand(c.B, c.H, c.W))
    assert bool((FG.border_cells(y) == 0).all()) and not bool((s == 777.0).any())
    prefill = torch.zeros(c.B, 2, c.H + 2, c.W + 2, 16, dtype=torch.float16)
    prefill[:, :, 1:-1, 1:-1] = float("nan")
    yh = FG.prep_restate_hs(c, d, prefill)
    assert torch.equal(FG.hs8_decode(yh[:, :1])[:, :2], FG.decoded(FG.interior(y)).double()) and FG.bits_equal(yh[:, 1], prefill[:, 1])
    if c.sigma_stride:            # sigma written into the border: the whole-tensor comparison sees it
        assert not FG.bits_equal(FG.prep_restate(c, d, sigma_in_border=True), y)
        assert not FG.bits_equal(FG.prep_restate_hs(c, d, prefill, sigma_in_border=True), yh)


@pytest.mark.parametrize("case", FG.POOL_CASES, ids=lambda c: c.name)
def test_pool_restatement_ties_and_the_ceil_mutant(case):
    c = case
    for fam in FG.pool_families(c):
        x = FG.pool_inputs(c.name, fam)["x"]
        y = FG.pool_restate(x)
        assert torch.equal(y, F.max_pool2d(x, 2)) and torch.equal(y.double(), F.max_pool2d(x.double(), 2))       # values; the zeros' signs below
        Ho, Wo = c.H // 2, c.W // 2
        win = x[..., :2 * Ho, :2 * Wo].reshape(c.B, c.C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        zero_max = win.max(1).values == 0
        if win.shape[0] > 3:
            assert bool(zero_max.any()) and bool(((win == win.max(1, keepdim=True).values).sum(1) > 1).any()), "no tie in the case"
        assert bool((torch.signbit(y.reshape(-1)[zero_max]) == torch.signbit(win[zero_max]).all(1)).all())        # -0 only where every zero is -0
        if c.W % 2:
            m = FG.pool_restate(x, ceil_index=True)
            assert m.shape == y.shape and not torch.equal(m, y)
    assert torch.equal(FG.pool_restate(torch.tensor([[[[0.0, -0.0], [-0.0, -1.0]]]])), torch.zeros(1, 1, 1, 1))
    assert bool(torch.signbit(FG.pool_restate(torch.tensor([[[[-0.0, -0.0], [-0.0, -1.0]]]]))).all())


@pytest.mark.parametrize("case", FG.RELAYOUT_CASES, ids=lambda c: c.name)
def test_relayout_restatements_and_the_swapped_phase_mutant(case):
    c = case
    x = FG.relayout_inputs(c.name)["x"]
    y = FG.s2d_restate(x)
    for dy in (0, 1):
        for dx in (0, 1):
            for ch in (0, c.C - 1):
                assert torch.equal(y[:, (2 * dy + dx) * c.C + ch], x[:, ch, dy::2, dx::2])
    assert FG.bits_equal(FG.d2s_restate(y), x)
    # pixel_unshuffle orders c * 4 + phase: the same values, another channel order
    pu = F.pixel_unshuffle(x, 2)
    assert torch.equal(pu.view(c.B, c.C, 4, c.h // 2, c.w // 2).transpose(1, 2).reshape(y.shape), y) and not torch.equal(pu, y)
    assert not torch.equal(FG.s2d_restate(x, swapped=True), y) and not torch.equal(FG.d2s_restate(y, swapped=True), x)
    assert FG.bits_equal(FG.d2s_restate(FG.s2d_restate(x, swapped=True), swapped=True), x)       # the round trip alone does not catch it
    # half-split: phase-major over groups of 8 channels is the same channel order, so whole records move
    G = c.C // 8
    rec, rec_y = FG.hs8_encode(x)[:, :, 1:-1, 1:-1], FG.hs8_encode(y)[:, :, 1:-1, 1:-1]
    for dy in (0, 1):
        for dx in (0, 1):
            assert FG.bits_equal(rec_y[:, (2 * dy + dx) * G:(2 * dy + dx + 1) * G].contiguous(), rec[:, :, dy::2, dx::2].contiguous())
    # the skip sum: one fp32 addition of the decoded values
    a, b = FG.relayout_inputs(c.name, 1)["x"], FG.relayout_inputs(c.name, 1)["y"]
    assert FG.measure(a + b, a.double() + b.double(), a.double().abs() + b.double().abs()) <= FG.U


@pytest.mark.parametrize("shape", FG.TAIL_SHAPES, ids=str)
def test_tail_restatements_and_the_exclusive_mask_mutant(shape):
    B, H, W = shape
    d = FG.tail_mask_inputs(B, H, W)
    p = d["pre"]
    n = min(H * W, 6)
    assert FG.bits_equal(p.view(B, -1)[0, :n], torch.tensor(FG.EDGES_IN + FG.EDGES_OUT + (float("nan"),))[:n])
    for scale in (None, FG.HS_SC[0]):
        y = FG.tail_mask_restate(d, scale)
        # float64 autograd of clamp at pre: the inclusive mask
        z = torch.nan_to_num(p.double(), nan=5.0).requires_grad_(True)
        (z.clamp(0.0, 1.0) * d["g"].double() * (scale or 1.0)).sum().backward()
        assert torch.equal(y.double(), z.grad), shape
        if H * W >= 3:            # the cell holding exactly 1.0 tells `<= 1` from `< 1`
            assert not FG.bits_equal(FG.tail_mask_restate(d, scale, exclusive_one=True), y)
    t = FG.tail_out_inputs(B, H, W)
    pre, out = FG.tail_out_restate(t)
    assert FG.bits_equal(pre, t["t32"][:, 0].contiguous()) and torch.equal(out, pre.clamp(0, 1)) and float(out.min()) >= 0 and float(out.max()) <= 1
    assert FG.bits_equal(FG.unsigned_zeros(torch.tensor([-0.0, 0.0, 1.0])), torch.tensor([0.0, 0.0, 1.0]))


@pytest.mark.parametrize("case", FG.INGRAD_CASES, ids=lambda c: c.name)
def test_input_gradient_chunks_and_sum_depth(case):
    c, d = case, FG.ingrad_inputs(case.name)
    gx, part64, part_abs, gs64, gs_abs = FG.ingrad_reference(c, d)
    assert FG.bits_equal(gx, d["g"][:, 0].contiguous())
    n = c.H * c.W
    per = (n + 63) // 64
    kp, kf = FG.sigma_depth(c.H, c.W)
    assert (kp, kf) == ((per + 255) // 256 + 8, (per + 255) // 256 + 72)
    full = n // per
    assert bool((part_abs[:, :full] > 0).all()) and bool((part_abs[:, -(-n // per):] == 0).all())
    assert torch.allclose(part64.sum(1), gs64, rtol=1e-12, atol=0) and torch.allclose(gs64, d["g"][:, 1].double().sum((1, 2)), rtol=1e-12, atol=1e-300)
    s32 = d["g"][:, 1].reshape(c.B, -1).sum(1)
    assert bool(((s32.double() - gs64).abs() <= kf * FG.U * gs_abs).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# measured ops: the emulations under their bars, the mutants above them

def test_conv_first_emulation_and_the_unmasked_noise_map_mutant():
    caught = 0
    for c in FG.FIRST_CASES:
        key = "first_hs" if c.family else "first_f32"
        d = FG.first_inputs(c.name)
        ref, den = FG.first_reference(c, d)
        # the reference is conv2d of the zero-padded [x | sigma map]
        inp = torch.stack([d["x"].double(), FG.sigma_of(d, c.B, c.sigma_stride).double().view(-1, 1, 1).expand(c.B, c.H, c.W)], 1)
        conv = F.leaky_relu(F.conv2d(inp, d["w"].double().view(c.cout, 2, 3, 3), d["bias"].double(), padding=1), c.slope)
        assert torch.allclose(ref, conv, rtol=1e-12, atol=1e-14), c.name
        e = FG.measure(FG.first_emulate32(c, d), ref, den)
        assert e <= FG.bar(key) / FG.BAR_FACTOR * (1 + 1e-4), (c.name, e)
        m = FG.first_emulate32(c, d, unmasked=True)
        inner = (slice(None), slice(None), slice(1, -1), slice(1, -1))
        if c.sigma_stride and c.H > 2 and c.W > 2:         # differs only on border pixels, and fails there
            assert FG.bits_equal(m[inner].contiguous(), FG.first_emulate32(c, d)[inner].contiguous())
            assert FG.measure(m, ref, den) > FG.bar(key), c.name
            caught += 1
    assert caught >= 6


@pytest.mark.parametrize("family", [0, 1])
def test_outc_emulation_clamp_and_the_zeroed_weight_mutant(family):
    key = "outc_hs" if family else "outc_f32"
    for c in FG.OUTC_CASES:
        d = FG.outc_inputs(c.name, family)
        ref, den = FG.outc_reference(c, d)
        pre, out = FG.outc_emulate32(c, d, family)
        if c.H * c.W >= 35:
            assert FG.straddles(ref), c.name
        assert FG.measure(pre, ref, den) <= FG.bar(key) / FG.BAR_FACTOR * (1 + 1e-4), c.name
        assert FG.measure(out, ref.clamp(0.0, 1.0), den) <= FG.measure(pre, ref, den)            # the clamp is a contraction
        for ch in (0, 17, 31):
            mp, mo = FG.outc_emulate32(c, d, family, zeroed=ch)
            assert FG.measure(mp, ref, den) > FG.bar(key), (c.name, ch)
            if c.H * c.W >= 35:
                assert FG.measure(mo, ref.clamp(0.0, 1.0), den) > FG.bar(key), (c.name, ch)


@pytest.mark.parametrize("family", [0, 1])
def test_upsample_emulation_holds_both_tiers_and_the_unclamped_mutant_fails(family):
    key = "ups_hs" if family else "ups_f32"
    tier_a = FG.UPS_TIER_A_HS if family else FG.UPS_TIER_A
    other_table_fails = 0
    for c in FG.UPS_CASES:
        x = FG.ups_inputs(c.name, family)["x"]
        rb = FG.ups_reference_b(x)
        for form in FG.ups_forms_admitted(family, c.B * (c.C // 8 if family else c.C), c.w):
            con = FG.ups_contracted(family, form)
            ra, den = FG.ups_reference_a(x, con)
            y = FG.ups_emulate32(x, family, contracted=con)
            assert FG.measure(y, ra, den) <= tier_a, (c.name, form)
            assert FG.measure(y, rb, den) <= FG.bar(key) / FG.BAR_FACTOR * (1 + 1e-4), (c.name, form)
            assert FG.measure(ra, rb, den) <= FG.bar(key), (c.name, form)      # tier (a)'s reference sits within the weights' own error of tier (b)'s
            other_table_fails += FG.measure(y, FG.ups_reference_a(x, not con)[0], den) > tier_a      # the other weight arithmetic shows
            if not con:      # the uncontracted emulation is the one the fp32 convolution tests already use (tests/conv_layer_cases.py)
                assert FG.bits_equal(y, FG.upsample32(x, 2 * c.h, 2 * c.w)), c.name
            # without the `x0 < w - 1` clamp the last destination reads the (NaN) border: its row and column fail every bar
            m = FG.ups_emulate32(x, family, clamp=False, contracted=con)
            assert FG.measure(m, rb, den) == float("inf") and bool(torch.isnan(m[..., -1, :]).all()) and bool(torch.isnan(m[..., :, -1]).all()), c.name
            if c.h > 1 and c.w > 1:            # ... and nothing else moves (a 1-wide source takes every tap from beyond)
                assert torch.equal(m[..., :-1, :-1].double(), y[..., :-1, :-1].double()), c.name
        src = FG.nan_border(FG.hs8_encode(x) if family else FG.pad(x), family)
        assert bool(torch.isnan(FG.hs8_border(src).float()).all() if family else torch.isnan(FG.border_cells(src)).all())
    assert other_table_fails >= 8
    # the impulse launches hold the indices: a table shifted by one destination moves the support
    for c in FG.UPS_CASES:
        sites = FG.ups_impulse_sites(c, family)
        assert {(0, 0), (c.h - 1, c.w - 1), (0, c.w - 1), (c.h - 1, 0)} <= set(sites)
        xi = FG.ups_impulse_input(c, sites)
        for con in ((True,) if family else (True, False)):
            want = FG.ups_impulse_expected(c, sites, xi.shape[1], con)
            y = FG.ups_emulate32(xi, family, contracted=con).double()
            zeros_ok, e = FG.impulse_measure(y, want, family)
            assert zeros_ok and e <= (FG.IMPULSE_BAR_HS if family else FG.IMPULSE_BAR), (c.name, e)
            if c.w > 2:
                zeros_ok, e = FG.impulse_measure(torch.roll(y, 1, -1), want, family)
                assert not zeros_ok and e > 0.1, c.name
    c = FG.UPS_BY_NAME["ups_5x130_to10x260"]
    assert any(abs(sx - int(129 / 259 * 64)) <= 1 for _, sx in FG.ups_impulse_sites(c, 1)) and any(abs(sx - int(129 / 259 * 256)) <= 1 for _, sx in FG.ups_impulse_sites(c, 0))


def test_recorded_bars_are_eight_times_the_emulation_maxima():
    rec, emu = FG.recorded_bars(), FG.emulation_maxima()
    for k in FG.BAR_KEYS:
        mx, b = rec[k]
        assert emu[k][0] == pytest.approx(mx, rel=1e-4), (k, emu[k])          # the file holds 5 significant digits
        assert b == pytest.approx(FG.BAR_FACTOR * emu[k][0], rel=1e-4), k
        assert FG.bar(k) == b
    # what sets them: an fp32 fma chain of 19 / 33 terms sits a few 2^-24 of sum |terms| from the exact sum; the up-sampling's scale s is
    # itself rounded (2^-25 relative), so l carries an absolute 2^-25 per unit of the index, over a denominator that can be 20 x smaller
    # than |v1 - v0|
    for k in ("first_f32", "first_hs", "outc_f32", "outc_hs"):
        assert FG.U < rec[k][0] < 12 * FG.U, k
    assert 1e-6 < rec["ups_f32"][0] < 5e-5 and 1e-6 < rec["ups_hs"][0] < 5e-5
    assert FG.UPS_TIER_A == 6 * 2.0 ** -24 and FG.UPS_TIER_A_HS == 11 * 2.0 ** -24
