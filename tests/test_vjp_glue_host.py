"""CPU side of the probe of the launches between the UNet VJP's adjoint convolutions (tests/vjp_glue_cases.py): the fp32 restatements
against the float64 autograd references, the mutants each bar must catch, the derived bars against profiles/vjp_glue_probe.md, and the
host-only plan (pnpx_vjp_glue_probe_plan) against a plain restatement of the launchers' predicates.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import vjp_glue_cases as VG

ROOT = VG.ROOT


def test_symbols_are_declared_and_bound():
    from tfpnp_amd import _lib
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    for name in ("pnpx_vjp_glue_probe", "pnpx_vjp_glue_probe_plan"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name), name
    # the python descriptor mirrors the header's field for field
    body = re.search(r"typedef struct pnpx_vjp_glue_probe_desc \{(.*?)\} pnpx_vjp_glue_probe_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?(unsigned|void|float|int)\s*", "", decl.strip())
        names += [n.strip(" *\n") for n in decl.split(",") if n.strip()]
    assert names == [f[0] for f in _lib.VjpGlueProbeDesc._fields_], names


# ---------------------------------------------------------------------------------------------------------------------------------
# single-product ops: the restatement within 3 * 2^-24 of float64 autograd, per element

@pytest.mark.parametrize("family", [0, 1])
@pytest.mark.parametrize("case", VG.OUTC_CASES, ids=lambda c: c.name)
def test_outc_restatement_against_autograd(case, family):
    d = VG.outc_inputs(case.name, family)
    scale = VG.HS_SC[0] if family else None
    gf, gr = VG.outc_restate32(case, d, scale)
    rf, rr = VG.outc_reference(case, d, scale or 1.0)
    assert VG.rel_err(gf, rf) <= VG.SINGLE_BAR and VG.rel_err(gr, rr) <= VG.SINGLE_BAR
    # the edge cells: the inclusive ends pass the gradient, the values just outside do not
    assert bool((gr[:, 0, :3] == d["g"][:, 0, :3] * (scale or 1.0)).all()) and bool((gr[:, 0, 3:5] == 0).all())
    # +0 and -0 feat cells take the slope
    assert bool((gf[:, :2, 0, :3] == d["w"][:2].view(1, 2, 1) * gr[:, None, 0, :3] * np.float32(0.2)).all())
    # mutants
    for kw in ({"exclusive": True}, {"unit_at_plus_zero": True}):
        mf, mr = VG.outc_restate32(case, d, scale, **kw)
        assert VG.rel_err(mf, rf) > VG.SINGLE_BAR, kw
        assert not VG.bits_equal(mf, gf)
    assert VG.rel_err(VG.outc_restate32(case, d, scale, exclusive=True)[1], rr) > VG.SINGLE_BAR


@pytest.mark.parametrize("family", [0, 1])
@pytest.mark.parametrize("case", VG.SPM_CASES, ids=lambda c: c.name)
def test_skip_pool_restatement_against_autograd(case, family):
    d = VG.spm_inputs(case.name, family)
    y, ref = VG.spm_restate32(case, d), VG.spm_reference(case, d)
    assert VG.rel_err(y, ref) <= VG.SINGLE_BAR
    if case.pool and (case.H % 2 or case.W % 2):        # the dropped last row / column: the skip gradient alone
        skip = d["g"][:, :case.C] * VG.dlrelu(d["act"])
        if case.H % 2:
            assert VG.bits_equal(y[..., -1, :], skip[..., -1, :])
        if case.W % 2:
            assert VG.bits_equal(y[..., :, -1].contiguous(), skip[..., :, -1].contiguous())
    if case.ties:                                       # the last-maximum rule fails the bar where windows tie
        m = VG.spm_restate32(case, d, last_max=True)
        assert VG.rel_err(m, ref) > VG.SINGLE_BAR and not VG.bits_equal(m, y)


def test_tie_cases_hold_every_tie_pattern():
    for c in VG.SPM_CASES:
        if not c.ties:
            continue
        a = VG.spm_inputs(c.name)["act"]
        Ho, Wo = c.H // 2, c.W // 2
        win = a[..., :2 * Ho, :2 * Wo].reshape(c.B, c.C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        have = {tuple(np.copysign(1, w) * (abs(w) + 1) for w in row) for row in win.tolist()}     # +-0 told apart
        want = {tuple(np.copysign(1, w) * (abs(w) + 1) for w in row) for row in VG.TIE_WINDOWS}
        n = min(len(VG.TIE_WINDOWS), (win.shape[0] + 2) // 3)
        assert len(want & have) >= n, c.name


@pytest.mark.parametrize("family", [0, 1])
@pytest.mark.parametrize("case", VG.INGRAD_CASES, ids=lambda c: c.name)
def test_input_gradient_restatement_and_sum_depth(case, family):
    d = VG.ingrad_inputs(case.name, family)
    m = VG.HS_SC[1] if family else None
    gx64, part64, part_abs, gs64, gs_abs = VG.ingrad_reference(case, d, m or 1.0)
    assert VG.rel_err(VG.ingrad_restate32(case, d, m), gx64) <= VG.SINGLE_BAR
    kp, kf = VG.sigma_depth(case.H, case.W)
    per = (case.H * case.W + 63) // 64
    assert (kp, kf) == ((per + 255) // 256 + 8, (per + 255) // 256 + 72)
    if case.name == "ingrad_17x23":                     # the last chunks are empty
        assert per == 7 and bool((part_abs[:, 56:] == 0).all()) and bool((part_abs[:, :55] > 0).all())
    # a plain fp32 sum of the same terms stays within the final bound (any order does, to first order)
    s32 = (d["g"][:, 1] * np.float32(m or 1.0)).reshape(case.B, -1).sum(1)
    assert bool(((s32.double() - gs64).abs() <= kf * VG.U * gs_abs).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# up-sampling adjoint

def test_weight_table_is_the_forward_interpolation():
    """Rows of the fp32 table against float64 align_corners weights; every destination's weights sum to 1 within an ulp; all weight sits
    inside the kernels' +-3 window (7 candidates)."""
    for n in (1, 2, 8, 16, 17, 19, 33, 64, 65, 72, 128, 130):
        T = VG.weight_table(n).astype(np.float64)
        assert np.abs(T.sum(0) - 1).max() <= 2.0 ** -23
        s, d = np.nonzero(T)
        assert (np.abs(d - 2 * s) <= 3).all(), n
        x = torch.eye(n, dtype=torch.float64).view(n, 1, n, 1)
        up = torch.nn.functional.interpolate(x.expand(n, 1, n, 2), scale_factor=2, mode="bilinear", align_corners=True)[:, 0, :, 0] if n > 1 else None
        if up is not None:
            assert np.abs(T - up.numpy()).max() <= 4 * n * 2.0 ** -24, n      # f = s * index: two roundings of a number up to n


@pytest.mark.parametrize("family", [0, 1])
def test_upsample_emulation_holds_both_tiers_and_mutants_fail(family):
    key = "ups_hs" if family else "ups_f32"
    b = VG.bar(key)
    caught = {m: 0 for m in VG.UPS_MUTANTS}
    for c in VG.UPS_CASES:
        d = VG.ups_inputs(c.name, family)
        ra, den = VG.ups_reference_a(c, d)
        rb = VG.ups_reference_b(c, d)
        y = VG.ups_emulate32(c, d, family)
        assert VG.measure(y, ra, den) <= VG.UPS_TIER_A, c.name
        assert VG.measure(y, rb, den) <= b / VG.BAR_FACTOR * (1 + 1e-4), c.name
        for m in VG.UPS_MUTANTS:
            if m == "shifted_table" and c.w == 1:
                continue                       # a 1 x 1 source has one weight
            ym = VG.ups_emulate32(c, d, family, mutant=m)
            assert VG.measure(ym, rb, den) > b and VG.measure(ym, ra, den) > VG.UPS_TIER_A, (c.name, m)
            caught[m] += 1
    assert all(v >= len(VG.UPS_CASES) - 2 for v in caught.values()), caught


def test_recorded_bars_are_eight_times_the_emulation_maxima():
    rec, emu = VG.recorded_bars(), VG.emulation_maxima()
    for k in VG.BAR_KEYS:
        mx, b = rec[k]
        assert emu[k][0] == pytest.approx(mx, rel=1e-4), (k, emu[k])          # the file holds 5 significant digits
        assert b == pytest.approx(VG.BAR_FACTOR * emu[k][0], rel=1e-4), k
        assert VG.bar(k) == b
    # what sets them: the scale s is itself rounded to fp32 (2^-25 relative), so the weight l = fma(s, index, -i0) carries an absolute
    # 2^-25 per unit of the index (130 columns: 4e-6); the adjoint identity sums ~1e5 signed terms whose errors average out
    assert 1e-6 < rec["ups_f32"][0] < 5e-5 and 1e-6 < rec["ups_hs"][0] < 5e-5 and 1e-10 < rec["adjoint"][0] < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# gradient scale

def test_gradient_scale_expectations():
    cases = VG.gscale_cases()
    for k in (-20, 0, 7):
        bits, inv, m = VG.gscale_expected(cases[f"gs_pow{k}"])
        assert bits == int(np.float32(2.0 ** k).view(np.uint32))
        assert (inv, m) == (2.0 ** -(k + 1), 2.0 ** (k + 1))          # an exact power of two is NOT its own scale: f in [0.5, 1)
    assert VG.gscale_expected(cases["gs_zeros"]) == (0, 0.0, 0.0)
    assert VG.gscale_expected(cases["gs_inf"]) == (0x7F800000, 1.0, 1.0)
    bits, inv, m = VG.gscale_expected(cases["gs_nan"])                 # fmaxf drops the NaN
    assert 0 < bits < 0x7F800000 and inv * m == 1.0
    bits, inv, m = VG.gscale_expected(cases["gs_denormal"])
    assert bits == 3 << 8 and (inv, m) == (2.0 ** 126, 2.0 ** -126)    # 3 * 2^-141 = 0x300 denormal steps of 2^-149
    bits, inv, m = VG.gscale_expected(cases["gs_generic"])
    mx = float(cases["gs_generic"].abs().max())
    assert m / 2 <= mx < m and inv * m == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan

def test_plan_against_the_restated_predicates():
    for B in (1, 3, 48, 128, 4096, 8191, 8192, 65535, 65536):
        for C in (8, 16, 512):
            for h, w in ((1, 1), (2, 2), (16, 16), (16, 63), (16, 64), (17, 65), (128, 128)):
                kw = dict(B=B, C=C, H=h, W=w, Ccat=C + 8, c_off=8, Ht=2 * h, Wt=2 * w + 1)
                assert VG.plan(VG.UPSAMPLE_BWD, 0, **kw) == (VG.ups_form(B, C, w), 1), kw
                for form in (1, 2, 3):
                    assert VG.plan(VG.UPSAMPLE_BWD, 0, form, **kw) == ((form, 1) if form in VG.ups_forms_admitted(B, C) else (0, 0)), (form, kw)
                n = VG.ups_hs_launches(B, C // 8)
                assert VG.plan(VG.UPSAMPLE_BWD, 1, **kw) == (1, n) and n >= 1, kw
                assert VG.plan(VG.UPSAMPLE_BWD, 1, 2, **kw) == (0, 0)
                kw = dict(B=min(B, 128), C=C, H=h, W=w, Ccat=2 * C)
                assert VG.plan(VG.SKIP_POOL_MERGE, 0, **kw) == (VG.spm_form(h, w), 1), kw
                for form in (1, 2):
                    assert VG.plan(VG.SKIP_POOL_MERGE, 0, form, **kw) == ((form, 1) if form in VG.spm_forms_admitted(h, w) else (0, 0)), (form, kw)
                assert VG.plan(VG.SKIP_POOL_MERGE, 1, **kw) == (1, 1)
    # refusals: the concat too small, Ht off, channels of the half-split family, unknown forms and ops
    ok = dict(B=1, C=8, H=8, W=8, Ccat=16, c_off=8, Ht=16, Wt=17)
    assert VG.plan(VG.UPSAMPLE_BWD, 0, **ok) == (VG.UPS_LDS16, 1)
    for bad in (dict(Ccat=15), dict(c_off=9), dict(Ht=15), dict(Ht=18), dict(Wt=18), dict(B=0), dict(H=0)):
        assert VG.plan(VG.UPSAMPLE_BWD, 0, **dict(ok, **bad)) == (0, 0), bad
    assert VG.plan(VG.UPSAMPLE_BWD, 1, **dict(ok, C=4)) == (0, 0) and VG.plan(VG.UPSAMPLE_BWD, 0, 4, **ok) == (0, 0)
    assert VG.plan(VG.OUTC_BWD, 0, C=32) == (1, 1) and VG.plan(VG.OUTC_BWD, 0, C=16) == (0, 0) and VG.plan(VG.OUTC_BWD, 0, C=32, Ccat=8) == (0, 0)
    assert VG.plan(VG.INPUT_GRAD, 1, C=32) == (1, 1) and VG.plan(VG.INPUT_GRAD, 1, C=8) == (0, 0) and VG.plan(VG.INPUT_GRAD, 0, 2, C=32) == (0, 0)
    assert VG.plan(VG.GRAD_SCALE, 1, C=1) == (1, 1) and VG.plan(VG.GRAD_SCALE, 0, C=1) == (0, 0) and VG.plan(5, 0) == (0, 0)


def test_chain_batches_restate_the_fork():
    """csrc/unet_bwd.hip: `if (ctx->opt_fp32_chains >= 2 && B >= 2) fan_out_chains(ctx, 2, ...)`; csrc/common.h: slice c of n is
    [B c / n, B (c + 1) / n); the option's default is 2."""
    src = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "unet_bwd.hip")).read()
    assert "if (ctx->opt_fp32_chains >= 2 && B >= 2)\n    return fan_out_chains(ctx, 2, B, s," in src
    common = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "common.h")).read()
    assert "int opt_fp32_chains = 2;" in common and "(long long)B * c / chains), hi = (int)((long long)B * (c + 1) / chains)" in common
    assert VG.fp32_chain_batches(1) == [1] and VG.fp32_chain_batches(3) == [1, 2] and VG.fp32_chain_batches(48) == [24, 24]
    assert VG.fp32_chain_batches(128) == [64, 64] and VG.fp32_chain_batches(128, 1) == [128] and VG.fp32_chain_batches(256) == [128, 128]


def test_library_is_built_with_the_default_contraction():
    """tests/vjp_glue_cases.py: weight_table mirrors `sy * yd - y0` fused into one fma, which is what the compiler's default contraction
    mode does; a build that sets another mode computes the other table (weight_table(n, contracted=False))."""
    mk = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "Makefile")).read()
    assert "-ffp-contract" not in mk and "fp-contract" not in mk
    a, b = VG.weight_table(130), VG.weight_table(130, contracted=False)
    assert 0 < np.abs(a.astype(np.float64) - b).max() <= 130 * 2.0 ** -24


def _fp32_forms(B, H, W, fp32_chains=2):
    """Per launch chain of a B x H x W fp32 VJP: the forms of its four up-sampling adjoints (level 0 first), asked with the batch the
    chain hands the launcher."""
    return [[VG.plan(VG.UPSAMPLE_BWD, 0, B=b, C=C, H=h, W=w, Ccat=Cc, c_off=co, Ht=Ht, Wt=Wt)[0] for C, h, w, Cc, co, Ht, Wt in VG.vjp_levels(H, W)]
            for b in VG.fp32_chain_batches(B, fp32_chains)]


def test_forms_of_the_default_workload_and_of_the_whole_network_tests():
    L16, L64, PLAIN = VG.UPS_LDS16, VG.UPS_LDS64, VG.UPS_PLAIN
    # 48 x 256^2 under the default options: two chains of 24 images; every level runs an LDS-window form, the two upper levels (source
    # width 128, 64) the 64-wide one; block merges everywhere.  One chain of 48 (fp32_chains = 1) dispatches the same.
    assert VG.fp32_chain_batches(48) == [24, 24]
    assert _fp32_forms(48, 256, 256) == [[L64, L64, L16, L16]] * 2 and _fp32_forms(48, 256, 256, 1) == [[L64, L64, L16, L16]]
    for b in (24, 48):      # the half-split family has one form per op, whatever slice of the batch a chain takes
        for C, h, w, Cc, co, Ht, Wt in VG.vjp_levels(256, 256):
            assert VG.plan(VG.UPSAMPLE_BWD, 1, B=b, C=C, H=h, W=w, Ccat=Cc, c_off=co, Ht=Ht, Wt=Wt) == (1, 1)
            assert VG.plan(VG.SKIP_POOL_MERGE, 0, B=b, C=C // 2, H=Ht, W=Wt, Ccat=Cc) == (VG.SPM_BLOCK, 1)
            assert VG.plan(VG.SKIP_POOL_MERGE, 1, B=b, C=C // 2, H=Ht, W=Wt, Ccat=Cc) == (1, 1)
    # tests/test_gpu_backward.py before the calls below: only 128 x 128 reaches the 64-wide form (its top level alone), and only under
    # the loose bar; no shape reaches the plain form
    wide = set()
    for B, H, W in ((1, 16, 16), (2, 16, 16), (1, 17, 23), (1, 24, 40), (2, 19, 33), (1, 32, 32), (2, 48, 80), (1, 50, 39), (3, 64, 64), (1, 128, 128),
                    (3, 48, 48)):
        for forms in _fp32_forms(B, H, W):
            assert set(forms) <= {L16, L64}, (B, H, W)
            if L64 in forms:
                wide.add((B, H, W))
    assert wide == {(1, 128, 128)}
    # test_denoiser_vjp_at_65536_upsampling_planes.  B = 128 at 16 x 16 under the default options is two chains of 64 images: 32768
    # planes at the bottom level, an LDS-window form.  As ONE chain (fp32_chains = 1) the level-3 adjoint (512 channels from the 1 x 1
    # bottom) has 65536 planes -> the plain form; so has each chain of a B = 256 call under the default options.
    assert _fp32_forms(128, 16, 16) == [[L16, L16, L16, L16]] * 2
    assert _fp32_forms(128, 16, 16, 1) == [[L16, L16, L16, PLAIN]]
    assert _fp32_forms(256, 16, 16) == [[L16, L16, L16, PLAIN]] * 2
    assert VG.plan(VG.UPSAMPLE_BWD, 1, B=128, C=512, H=1, W=1, Ccat=768, c_off=256, Ht=2, Wt=2) == (1, 1)      # half-split: 8192 groups


def test_half_split_upsampling_adjoint_over_the_grid_limit_is_sliced():
    """B * groups above 65535: consecutive launches over whole images, none above the limit, together all images; nothing is refused up
    to 65535 groups per image (the denoiser has at most 64)."""
    for B, Gs in ((128, 64), (1023, 64), (1024, 64), (5000, 64), (65536, 1), (65535, 1), (70000, 3)):
        form, n = VG.plan(VG.UPSAMPLE_BWD, 1, B=B, C=8 * Gs, H=1, W=1, Ccat=8 * Gs, c_off=0, Ht=2, Wt=2)
        per = VG.GRID_Z_MAX // Gs
        assert form == 1 and n == -(-B // per) and per * Gs <= VG.GRID_Z_MAX and n * per >= B > (n - 1) * per, (B, Gs)
    assert VG.plan(VG.UPSAMPLE_BWD, 1, B=1023, C=512, H=1, W=1, Ccat=512, c_off=0, Ht=2, Wt=2) == (1, 1)
    assert VG.plan(VG.UPSAMPLE_BWD, 1, B=1024, C=512, H=1, W=1, Ccat=512, c_off=0, Ht=2, Wt=2) == (1, 2)
    assert VG.plan(VG.UPSAMPLE_BWD, 1, B=2, C=8 * 65536, H=1, W=1, Ccat=8 * 65536, c_off=0, Ht=2, Wt=2) == (0, 0)
    assert VG.plan(*((VG.UPSAMPLE_BWD, 1)), **dict(B=VG.UPS_HS_SLICED.B, C=8, H=1, W=1, Ccat=8, c_off=0, Ht=2, Wt=2)) == (1, 2)
