"""Every launch between the convolutions of the two denoisers' forward passes, and the DRUNet VJP's own glue, one launcher call at a time
(pnpx_fwd_glue_probe), against float64 references (cases, references, restatements, emulations and bars: tests/fwd_glue_cases.py; derived
bars: profiles/fwd_glue_probe.md).

Per (case, family, form): the bar, or bit identity with the restatement; every output pre-filled (interior NaN, border zero) and compared
WHOLE, so a skipped pixel, a written border cell or a written extra row / column of an odd target shows; 1 MiB of a fixed bit pattern
before and after every output untouched; image 0 of the batched launch bit-identical to the image launched alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fwd_glue_cases as FG
from tests.test_gpu_vjp_glue import PNPX_ERR_ARG, PNPX_ERR_HIP, PNPX_ERR_SHAPE, Slab, _decode, plain_out, planar, planar_out, records, records_out

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


def probe(ctx, op, family, form, sizes, outs, expect=0, host=None, **operands):
    """One pnpx_fwd_glue_probe call; operands / outs: {descriptor field: Slab}, host: {field: fp32 numpy array}.  The outputs' guards are
    checked."""
    from tfpnp_amd import _lib
    D = _lib.FwdGlueProbeDesc(op=op, family=family, form=form, **sizes)
    for k, v in list(operands.items()) + list(outs.items()):
        setattr(D, k, v.ptr())
    host = {k: np.ascontiguousarray(v, np.float32) for k, v in (host or {}).items()}
    for k, v in host.items():
        setattr(D, k, v.ctypes.data)
    torch.cuda.synchronize()
    st = _lib.lib().pnpx_fwd_glue_probe(ctx.handle, C.byref(D), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if st == PNPX_ERR_HIP:                 # a HIP runtime error: nothing more may be started on this device
        pytest.exit("pnpx_fwd_glue_probe: " + _lib.lib().pnpx_last_error().decode(), returncode=3)
    torch.cuda.synchronize()
    assert st == expect, (st, _lib.lib().pnpx_last_error().decode())
    for k, v in outs.items():
        assert v.guards_intact(), f"the launch wrote outside its output {k}"
    return st


def _region(t, family, H, W):
    """The H x W corner of the interior of a padded tensor (family 1: of a record tensor)."""
    return t[:, :, 1:1 + H, 1:1 + W] if family else t[..., 1:1 + H, FG.PADL:FG.PADL + W]


def _filled(prefill, family, values):
    """`prefill` with `values` ([B][C][H][W]; family 1: records [B][G][H][W][16]) in the corner of its interior: the whole expected tensor."""
    out = prefill.clone()
    H, W = values.shape[2:4]
    _region(out, family, H, W)[...] = values
    return out


def _rest_untouched(got, prefill, family, H, W):
    a, b = got.clone(), prefill.clone()
    _region(a, family, H, W)[...] = 0
    _region(b, family, H, W)[...] = 0
    return FG.bits_equal(a, b)


def _diff(a, b):
    """Where two tensors differ bit for bit: the first few (index, got, want), for an assertion's message."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shapes / types {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    v = torch.int32 if a.dtype == torch.float32 else torch.int16
    idx = torch.nonzero(a.contiguous().view(v) != b.contiguous().view(v))
    return f"{idx.shape[0]} cells differ: " + "; ".join(f"{tuple(i.tolist())}: {a[tuple(i)].item()!r} vs {b[tuple(i)].item()!r}" for i in idx[:5])


def _rec(x):
    """fp32 [B][C][H][W] -> the interior records [B][C/8][H][W][16]."""
    return FG.hs8_encode(x)[:, :, 1:-1, 1:-1].contiguous()


def _mk(family):
    return (records, records_out) if family else (planar, planar_out)


def _first_image(d, shared=()):
    return {k: (v if k in shared else v[:1]) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# input preparation

def _run_prep(ctx, c, family, d, B):
    out = records_out(B, 16, c.H, c.W) if family else planar_out(B, 2, c.H, c.W)
    prefill = out.cpu()
    probe(ctx, FG.PREP_INPUT, family, 0, dict(B=B, H=c.H, W=c.W, sigma_stride=c.sigma_stride), {"out": out}, x=Slab(d["x"]), sigma=Slab(d["sigma"]))
    return out.cpu(), prefill


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", FG.PREP_CASES, ids=lambda c: c.name)
def test_prep_input(ctx, case, family):
    c, d = case, FG.prep_inputs(case.name)
    got, prefill = _run_prep(ctx, c, family, d, c.B)
    want = FG.prep_restate_hs(c, d, prefill) if family else FG.prep_restate(c, d)
    if family:      # the sign of a ZERO lo half is the compiler's: lo = v - hi is fused with the x 16 (v_fma_mixlo_f16), which gives -0 for the
        # -0.0 pixel where hs8_encode gives +0; hi carries the value's sign either way (hs_pack after a product)
        got, want = got.clone(), want.clone()
        got[..., 8:], want[..., 8:] = FG.unsigned_zeros(got[..., 8:]), FG.unsigned_zeros(want[..., 8:])
    assert FG.bits_equal(got, want), (c.name, _diff(got, want))      # interior, border and (half-split) the unwritten second group alike
    one, _ = _run_prep(ctx, c, family, d, 1)
    assert FG.bits_equal(one, _run_prep(ctx, c, family, d, c.B)[0][:1].contiguous()), "image 0 alone differs from image 0 of the batch"


# ---------------------------------------------------------------------------------------------------------------------------------
# first convolution

def _run_first(ctx, c, d, B, expect=0):
    out = _mk(c.family)[1](B, c.cout, c.H, c.W)
    prefill = out.cpu()
    probe(ctx, FG.CONV_FIRST, c.family, 0, dict(B=B, C=c.cout, H=c.H, W=c.W, sigma_stride=c.sigma_stride, k=c.k, slope=c.slope), {"out": out},
          expect=expect, host={"w": d["w"].numpy(), "bias": d["bias"].numpy()}, x=Slab(d["x"]), sigma=Slab(d["sigma"]))
    return out.cpu(), prefill


@pytest.mark.parametrize("case", FG.FIRST_CASES, ids=lambda c: c.name)
def test_conv_first(ctx, case):
    c, d = case, FG.first_inputs(case.name)
    key = "first_hs" if c.family else "first_f32"
    got, prefill = _run_first(ctx, c, d, c.B)
    assert _rest_untouched(got, prefill, c.family, c.H, c.W), "a border cell was written"
    y = _region(got, c.family, c.H, c.W).contiguous()
    v = _decode(y) * 2.0 ** c.k if c.family else y
    ref, den = FG.first_reference(c, d)
    e = FG.measure(v, ref, den)
    print(f"\nfwd_glue_probe {key} {c.name} measure {e:.4e} bar {FG.bar(key):.4e}")
    assert e <= FG.bar(key), (c.name, e)
    one, _ = _run_first(ctx, c, _first_image(d, ("w", "bias", "sigma")), 1)
    assert FG.bits_equal(one, got[:1].contiguous()), "image 0 alone differs from image 0 of the batch"


@pytest.mark.parametrize("shape", FG.FIRST_REFUSED_F32, ids=str)
def test_fp32_conv_first_refuses_widths_that_are_no_multiple_of_four(ctx, shape):
    B, H, W = shape
    c = FG.FirstCase("refused", 0, B, H, W, 32, 0.2, 0, 1)
    assert FG.plan(FG.CONV_FIRST, 0, B=B, C=32, H=H, W=W, sigma_stride=1, slope=0.2) == (0, 0)
    g = torch.Generator().manual_seed(1)
    d = {"x": torch.randn(B, H, W, generator=g), "sigma": torch.rand(B, generator=g), "w": torch.randn(32, 2, 9, generator=g), "bias": torch.zeros(32)}
    got, prefill = _run_first(ctx, c, d, B, expect=PNPX_ERR_SHAPE)
    assert FG.bits_equal(got, prefill), "a refused call wrote its output"


# ---------------------------------------------------------------------------------------------------------------------------------
# pooling

def _run_pool(ctx, c, family, x, B):
    mk, mko = _mk(family)
    out = mko(B, c.C, c.H // 2, c.W // 2)
    prefill = out.cpu()
    probe(ctx, FG.MAXPOOL2, family, 0, dict(B=B, C=c.C, H=c.H, W=c.W), {"out": out}, src=mk(x))
    return out.cpu(), prefill


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", FG.POOL_CASES, ids=lambda c: c.name)
def test_maxpool(ctx, case, family):
    c = case
    if family not in FG.pool_families(c):
        assert FG.plan(FG.MAXPOOL2, 1, B=c.B, C=c.C, H=c.H, W=c.W) == (0, 0)      # C no multiple of 8: no half-split tensor
        return
    x = FG.pool_inputs(c.name, family)["x"]
    got, prefill = _run_pool(ctx, c, family, x, c.B)
    Ho, Wo = c.H // 2, c.W // 2
    if family:            # decoded values: re-encoding a decoded tie need not give the same pair of halves
        assert _rest_untouched(got, prefill, 1, Ho, Wo), "a border record was written"
        assert torch.equal(_decode(_region(got, 1, Ho, Wo).contiguous()), torch.nn.functional.max_pool2d(x.double(), 2)), c.name
    else:
        assert FG.bits_equal(got, _filled(prefill, 0, FG.pool_restate(x))), c.name
    one, _ = _run_pool(ctx, c, family, x[:1], 1)
    assert FG.bits_equal(one, got[:1].contiguous()), "image 0 alone differs from image 0 of the batch"


# ---------------------------------------------------------------------------------------------------------------------------------
# up-sampling

def _run_ups(ctx, c, family, form, x, expect=0):
    B, Cn = x.shape[:2]
    out = _mk(family)[1](B, Cn, c.Ht, c.Wt)
    prefill = out.cpu()
    src = Slab(FG.nan_border(FG.hs8_encode(x) if family else FG.pad(x), family))      # a correct kernel never reads the source's border
    probe(ctx, FG.UPSAMPLE2X, family, form, dict(B=B, C=Cn, H=c.h, W=c.w, Ht=c.Ht, Wt=c.Wt), {"out": out}, expect=expect, src=src)
    return out.cpu(), prefill


def _ups_values(c, family, got):
    y = _region(got, family, 2 * c.h, 2 * c.w).contiguous()
    return _decode(y) if family else y


def _check_ups(ctx, c, family, x, forms, what):
    key = "ups_hs" if family else "ups_f32"
    tier_a = FG.UPS_TIER_A_HS if family else FG.UPS_TIER_A
    rb = FG.ups_reference_b(x)
    planes = x.shape[0] * (x.shape[1] // 8 if family else x.shape[1])
    got = {}
    for form in forms:
        con = FG.ups_contracted(family, form or FG.ups_form(family, planes, c.w))       # the form's own weight arithmetic
        ra, den = FG.ups_reference_a(x, con)
        full, prefill = _run_ups(ctx, c, family, form, x)
        assert _rest_untouched(full, prefill, family, 2 * c.h, 2 * c.w), f"{what}: the border or the extra row / column of an odd target was written"
        v = _ups_values(c, family, full)
        ea, eb = FG.measure(v, ra, den), FG.measure(v, rb, den)
        fname = FG.UPS_FORM_NAMES[family][form]
        print(f"\nfwd_glue_probe {key}_a {c.name} {fname} measure {ea:.4e} bar {tier_a:.4e}")
        print(f"fwd_glue_probe {key} {c.name} {fname} measure {eb:.4e} bar {FG.bar(key):.4e}")
        if ea > tier_a:      # is it the weight arithmetic (the compiler fusing, or no longer fusing, s * d - i0) or the kernel?
            other = FG.measure(v, FG.ups_reference_a(x, not con)[0], den)
            raise AssertionError(f"{c.name} {fname}: tier (a) {ea:.3e} > {tier_a:.3e}; against the {'un' if con else ''}contracted weight table {other:.3e}")
        assert eb <= FG.bar(key), (c.name, fname, eb)
        got[form] = full
    return got


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", FG.UPS_CASES, ids=lambda c: c.name)
def test_upsample(ctx, case, family):
    c = case
    x = FG.ups_inputs(c.name, family)["x"]
    planes = c.B * (c.C // 8 if family else c.C)
    admitted = FG.ups_forms_admitted(family, planes, c.w)
    got = _check_ups(ctx, c, family, x, (0,) + admitted, c.name)
    auto = FG.ups_form(family, planes, c.w)
    assert FG.plan(FG.UPSAMPLE2X, family, B=c.B, C=c.C, H=c.h, W=c.w, Ht=c.Ht, Wt=c.Wt) == (auto, 1)
    assert FG.bits_equal(got[0], got[auto]), "form 0 is not the form the plan names"
    if not family and FG.UPS_V4 not in admitted:          # odd w: the 16-byte form is refused and launches nothing
        full, prefill = _run_ups(ctx, c, 0, FG.UPS_V4, x, expect=PNPX_ERR_SHAPE)
        assert FG.bits_equal(full, prefill)
    for form in admitted:
        one, _ = _run_ups(ctx, c, family, form, x[:1])
        assert FG.bits_equal(one, got[form][:1].contiguous()), f"form {form}: image 0 alone differs from image 0 of the batch"


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", FG.UPS_CASES, ids=lambda c: c.name)
def test_upsample_impulses_give_the_weight_tables(ctx, case, family):
    """One 1.0 per plane, at the corners and on both sides of every tile and window boundary: the output is the outer product of the two
    1-D weight tables' rows -- exact zeros where a table holds a zero, which holds the indices."""
    c = case
    sites = FG.ups_impulse_sites(c, family)
    x = FG.ups_impulse_input(c, sites)
    b = FG.IMPULSE_BAR_HS if family else FG.IMPULSE_BAR
    for form in FG.ups_forms_admitted(family, x.shape[1] // (8 if family else 1), c.w):
        want = FG.ups_impulse_expected(c, sites, x.shape[1], FG.ups_contracted(family, form))
        full, prefill = _run_ups(ctx, c, family, form, x)
        assert _rest_untouched(full, prefill, family, 2 * c.h, 2 * c.w)
        zeros_ok, e = FG.impulse_measure(_ups_values(c, family, full), want, family)
        assert zeros_ok, (c.name, form, "a weight sits where the table has none, or is missing")
        print(f"\nfwd_glue_probe impulse_{'hs' if family else 'f32'} {c.name} {FG.UPS_FORM_NAMES[family][form]} measure {e:.4e} bar {b:.4e}")
        assert e <= b, (c.name, form, e)


def test_fp32_upsample_at_the_plane_limit(ctx):
    """65535 planes: the 16-byte form still runs (gridDim.z at its limit); 65536: the forward falls back to the scalar form and the
    16-byte form is refused."""
    c = FG.UPS_F32_65535
    assert FG.plan(FG.UPSAMPLE2X, 0, B=c.B, C=c.C, H=c.h, W=c.w, Ht=c.Ht, Wt=c.Wt) == (FG.UPS_V4, 1)
    got = _check_ups(ctx, c, 0, FG.ups_inputs(c.name)["x"], (0, FG.UPS_SCALAR), c.name)
    # the planes at the far end of gridDim.z are what they are in a launch of their own
    assert FG.bits_equal(got[0][:, -8:].contiguous(), _run_ups(ctx, c, 0, FG.UPS_V4, FG.ups_inputs(c.name)["x"][:, -8:])[0])
    c = FG.UPS_F32_OVER_LIMIT
    x = FG.ups_inputs(c.name)["x"]
    assert c.B * c.C == 65536 and FG.plan(FG.UPSAMPLE2X, 0, B=c.B, C=c.C, H=c.h, W=c.w, Ht=c.Ht, Wt=c.Wt) == (FG.UPS_SCALAR, 1)
    _check_ups(ctx, c, 0, x, (0,), c.name)
    full, prefill = _run_ups(ctx, c, 0, FG.UPS_V4, x, expect=PNPX_ERR_SHAPE)
    assert FG.bits_equal(full, prefill), "a refused call wrote its output"


def test_half_split_upsample_over_the_grid_limit_runs_in_slices(ctx):
    """65544 (image, group) planes: two launches over whole images, none above the limit; every image is bit for bit what it is in a
    launch below the limit."""
    c = FG.UPS_HS_SLICED
    assert c.B * (c.C // 8) == 65544
    assert FG.plan(FG.UPSAMPLE2X, 1, B=c.B, C=c.C, H=c.h, W=c.w, Ht=c.Ht, Wt=c.Wt) == (FG.UPS_HS32, 2)
    few = FG.ups_inputs(c.name, 1)["x"][:3]
    x = few.repeat((c.B + 2) // 3, 1, 1, 1)[:c.B]          # images 0, 1, 2 in turn: the image at the seam (8191) is image 1
    small = _check_ups(ctx, c, 1, few, (0,), c.name + "/3 images")[0]
    for form in (0, FG.UPS_HS64):
        full, prefill = _run_ups(ctx, c, 1, form, x)
        assert FG.bits_equal(full, small.repeat((c.B + 2) // 3, 1, 1, 1, 1)[:c.B].contiguous()), f"form {form}: an image of the sliced launch differs"


# ---------------------------------------------------------------------------------------------------------------------------------
# out-conv + residual + clamp

def _run_outc(ctx, c, family, d, B, with_pre=True):
    out, pre = plain_out(B, c.H, c.W), plain_out(B, c.H, c.W)
    outs = {"out": out, "out_pre": pre} if with_pre else {"out": out}
    probe(ctx, FG.OUTC_RESIDUAL, family, 0, dict(B=B, C=32, H=c.H, W=c.W), outs, host={"w": d["w"].numpy(), "bias": d["bias"].numpy()},
          src=_mk(family)[0](d["feat"]), x=Slab(d["x"]))
    return out.cpu(), pre.cpu()


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", FG.OUTC_CASES, ids=lambda c: c.name)
def test_outc_residual(ctx, case, family):
    c, d = case, FG.outc_inputs(case.name, family)
    key = "outc_hs" if family else "outc_f32"
    ref, den = FG.outc_reference(c, d)
    out, pre = _run_outc(ctx, c, family, d, c.B)
    e_pre, e_out = FG.measure(pre, ref, den), FG.measure(out, ref.clamp(0.0, 1.0), den)
    print(f"\nfwd_glue_probe {key} {c.name} pre measure {e_pre:.4e} bar {FG.bar(key):.4e}")
    print(f"fwd_glue_probe {key} {c.name} out measure {e_out:.4e} bar {FG.bar(key):.4e}")
    assert e_pre <= FG.bar(key) and e_out <= FG.bar(key), (c.name, e_pre, e_out)
    assert FG.bits_equal(FG.unsigned_zeros(out), FG.unsigned_zeros(pre.clamp(0.0, 1.0))), "out is not the clamp of out_pre"
    out2, untouched = _run_outc(ctx, c, family, d, c.B, with_pre=False)       # out_pre may be null
    assert FG.bits_equal(out2, out) and bool(torch.isnan(untouched).all())
    one = _run_outc(ctx, c, family, _first_image(d, ("w", "bias")), 1)
    assert FG.bits_equal(one[0], out[:1].contiguous()) and FG.bits_equal(one[1], pre[:1].contiguous()), "image 0 alone differs"


# ---------------------------------------------------------------------------------------------------------------------------------
# re-layouts, skip sum

def _run_relayout(ctx, op, family, x, out_shape):
    mk, mko = _mk(family)
    B, Cin, h, w = x.shape
    out = mko(*out_shape)
    prefill = out.cpu()
    C_arg = Cin if op == FG.S2D else Cin // 4
    probe(ctx, op, family, 0, dict(B=B, C=C_arg, H=h, W=w), {"out": out}, src=mk(x))
    return out.cpu(), prefill


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", FG.RELAYOUT_CASES, ids=lambda c: c.name)
def test_s2d_d2s(ctx, case, family):
    c = case
    x = FG.relayout_inputs(c.name, family)["x"]
    enc = _rec if family else (lambda t: t)
    want = FG.s2d_restate(x)
    got, prefill = _run_relayout(ctx, FG.S2D, family, x, (c.B, 4 * c.C, c.h // 2, c.w // 2))
    assert FG.bits_equal(got, _filled(prefill, family, enc(want))), "space-to-depth differs from the phase-major restatement"
    back, prefill_b = _run_relayout(ctx, FG.D2S, family, want, (c.B, c.C, c.h, c.w))
    assert FG.bits_equal(back, _filled(prefill_b, family, enc(FG.d2s_restate(want)))), "depth-to-space differs from the restatement"
    assert FG.bits_equal(back, _filled(prefill_b, family, enc(x))), "d2s(s2d(x)) != x"
    for op, src, full, shape in ((FG.S2D, x, got, (1, 4 * c.C, c.h // 2, c.w // 2)), (FG.D2S, want, back, (1, c.C, c.h, c.w))):
        one, _ = _run_relayout(ctx, op, family, src[:1], shape)
        assert FG.bits_equal(one, full[:1].contiguous()), "image 0 alone differs from image 0 of the batch"


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", FG.RELAYOUT_CASES, ids=lambda c: c.name)
def test_add(ctx, case, family):
    c, d = case, FG.relayout_inputs(case.name, family)
    mk, mko = _mk(family)

    def run(a, b):
        out = mko(a.shape[0], c.C, c.h, c.w)
        prefill = out.cpu()
        probe(ctx, FG.ADD, family, 0, dict(B=a.shape[0], C=c.C, H=c.h, W=c.w), {"out": out}, src=mk(a), src2=mk(b))
        return out.cpu(), prefill
    got, prefill = run(d["x"], d["y"])
    s = d["x"] + d["y"]
    assert FG.bits_equal(got, _filled(prefill, family, _rec(s) if family else s)), c.name
    assert FG.bits_equal(run(d["x"][:1], d["y"][:1])[0], got[:1].contiguous()), "image 0 alone differs from image 0 of the batch"


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp32 DRUNet's tail, the tail masks, the fp32 input gradient

@pytest.mark.parametrize("shape", FG.TAIL_SHAPES, ids=str)
def test_tail_out(ctx, shape):
    B, H, W = shape
    d = FG.tail_out_inputs(B, H, W)

    def run(t, with_pre=True):
        out, pre = plain_out(t.shape[0], H, W), plain_out(t.shape[0], H, W)
        probe(ctx, FG.TAIL_OUT, 0, 0, dict(B=t.shape[0], C=32, H=H, W=W), {"out": out, "out_pre": pre} if with_pre else {"out": out}, src=planar(t))
        return out.cpu(), pre.cpu()
    out, pre = run(d["t32"])
    want_pre, want_out = FG.tail_out_restate(d)
    assert FG.bits_equal(pre, want_pre), "out_pre is not channel 0"
    assert FG.bits_equal(FG.unsigned_zeros(out), FG.unsigned_zeros(want_out)), "out is not its clamp"
    out2, untouched = run(d["t32"], with_pre=False)
    assert FG.bits_equal(out2, out) and bool(torch.isnan(untouched).all())
    assert FG.bits_equal(run(d["t32"][:1])[0], out[:1].contiguous())


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("shape", FG.TAIL_SHAPES, ids=str)
def test_tail_mask(ctx, shape, family):
    B, H, W = shape
    d = FG.tail_mask_inputs(B, H, W)

    def run(g, p):
        out = plain_out(g.shape[0], H, W)
        ops = {"x": Slab(g), "pre": Slab(p)}
        if family:
            ops["sc"] = Slab(torch.tensor(FG.HS_SC, dtype=torch.float32))
        probe(ctx, FG.TAIL_MASK, family, 0, dict(B=g.shape[0], H=H, W=W), {"out": out}, **ops)
        return out.cpu()
    got = run(d["g"], d["pre"])
    assert FG.bits_equal(got, FG.tail_mask_restate(d, FG.HS_SC[0] if family else None)), (shape, family)
    assert FG.bits_equal(run(d["g"][:1], d["pre"][:1]), got[:1].contiguous())


@pytest.mark.parametrize("case", FG.INGRAD_CASES, ids=lambda c: c.name)
def test_dru_input_gradient_and_sigma_sums(ctx, case):
    c, d = case, FG.ingrad_inputs(case.name)

    def run(g):
        B = g.shape[0]
        gx, part, gs = plain_out(B, c.H, c.W), plain_out(B, FG.SIG_CHUNKS), plain_out(B)
        probe(ctx, FG.DRU_INPUT_GRAD, 0, 0, dict(B=B, C=c.C, H=c.H, W=c.W), {"out": gx, "part": part, "gsigma": gs}, src=planar(g))
        return gx.cpu(), part.cpu(), gs.cpu()
    gx, part, gs = first = run(d["g"])
    gx_want, part64, part_abs, gs64, gs_abs = FG.ingrad_reference(c, d)
    assert FG.bits_equal(gx, gx_want), "gx is not channel 0"
    kp, kf = FG.sigma_depth(c.H, c.W)
    ep, ef = (part.double() - part64).abs(), (gs.double() - gs64).abs()
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(gs).all())
    rp = float((ep / (kp * FG.U * part_abs).clamp_min(1e-300)).max())
    rf = float((ef / (kf * FG.U * gs_abs)).max())
    print(f"\nfwd_glue_probe sigma_part {c.name} k {kp} measure {rp:.4e} bar 1.0")
    print(f"fwd_glue_probe sigma_final {c.name} k {kf} measure {rf:.4e} bar 1.0")
    assert bool((ep <= kp * FG.U * part_abs).all()), (c.name, rp)          # an empty chunk: exactly 0
    assert bool((ef <= kf * FG.U * gs_abs).all()), (c.name, rf)
    for a, b in zip(run(d["g"][:1]), first):
        assert FG.bits_equal(a, b[:1].contiguous()), "image 0 alone differs from image 0 of the batch"


# ---------------------------------------------------------------------------------------------------------------------------------
# operands and shapes

def test_misplaced_and_missing_operands_and_bad_shapes_are_refused(ctx):
    c = FG.RELAYOUT_BY_NAME["relayout_2x8x4x6"]
    d = FG.relayout_inputs(c.name)
    sizes = dict(B=c.B, C=c.C, H=c.h, W=c.w)
    out = planar_out(c.B, c.C, c.h, c.w)
    prefill = out.cpu()
    a, b = planar(d["x"]), planar(d["y"])
    img = Slab(torch.zeros(c.B, c.h, c.w))
    probe(ctx, FG.ADD, 0, 0, sizes, {"out": out}, expect=PNPX_ERR_ARG, src=a)                       # no second addend
    probe(ctx, FG.ADD, 0, 0, sizes, {"out": out}, expect=PNPX_ERR_ARG, src=a, src2=b, x=img)        # no place for an image
    probe(ctx, FG.MAXPOOL2, 0, 0, sizes, {"out": out}, expect=PNPX_ERR_ARG, src=a, src2=b)
    probe(ctx, FG.ADD, 0, 0, dict(sizes, Ht=8), {"out": out}, expect=PNPX_ERR_ARG, src=a, src2=b)
    probe(ctx, FG.ADD, 0, 0, dict(sizes, sigma_stride=1), {"out": out}, expect=PNPX_ERR_ARG, src=a, src2=b)
    probe(ctx, FG.TAIL_OUT, 1, 0, dict(sizes, C=32), {"out": out}, expect=PNPX_ERR_ARG, src=a)     # an fp32-only op
    probe(ctx, FG.TAIL_MASK, 0, 0, dict(B=c.B, H=c.h, W=c.w), {"out": out}, expect=PNPX_ERR_ARG, x=img, pre=img, sc=img)
    probe(ctx, FG.ADD, 0, 2, sizes, {"out": out}, expect=PNPX_ERR_SHAPE, src=a, src2=b)            # one form only
    probe(ctx, FG.S2D, 0, 0, dict(sizes, H=3), {"out": out}, expect=PNPX_ERR_SHAPE, src=a)          # odd size
    probe(ctx, FG.MAXPOOL2, 0, 0, dict(sizes, H=1), {"out": out}, expect=PNPX_ERR_SHAPE, src=a)
    probe(ctx, FG.UPSAMPLE2X, 0, 0, dict(sizes, Ht=2 * c.h + 2, Wt=2 * c.w), {"out": out}, expect=PNPX_ERR_SHAPE, src=a)
    probe(ctx, FG.UPSAMPLE2X, 1, 3, dict(sizes, Ht=2 * c.h, Wt=2 * c.w), {"out": out}, expect=PNPX_ERR_SHAPE, src=a)
    probe(ctx, FG.OUTC_RESIDUAL, 0, 0, sizes, {"out": out}, expect=PNPX_ERR_SHAPE, host={"w": np.zeros(32), "bias": np.zeros(1)}, src=a, x=img)
    assert FG.bits_equal(out.cpu(), prefill), "a refused call wrote its output"
