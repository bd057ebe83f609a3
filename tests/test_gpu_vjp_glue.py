"""Every launch between the UNet VJP's adjoint convolutions, one launcher call at a time (pnpx_vjp_glue_probe), against float64 references
(cases, references, restatements, emulations and bars: tests/vjp_glue_cases.py; derived bars: profiles/vjp_glue_probe.md).

Per (case, family, form): the bar; the output's border cells still zero and 1 MiB of a fixed bit pattern before and after every output
untouched; the output interior pre-filled with NaN, so a skipped pixel shows; image i of a B = 3 launch bit-identical to the image
launched alone; a second launch bit-identical."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import vjp_glue_cases as VG
from tests.conv_hs_cases import hs8_border

pytestmark = pytest.mark.gpu

GUARD = 1 << 20                       # bytes on either side of every tensor
PATTERN = 0x5A5AA5A5                  # as a float: 1.5e16, finite
PNPX_ERR_ARG, PNPX_ERR_SHAPE, PNPX_ERR_HIP = 1, 2, 5
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


class Slab:
    """A device tensor (any 2- or 4-byte type) inside a larger buffer: GUARD bytes of PATTERN, the tensor, GUARD bytes of PATTERN."""

    def __init__(self, cpu):
        cpu = cpu.contiguous()
        nbytes = (cpu.numel() * cpu.element_size() + 3) // 4 * 4
        self.buf = torch.empty(2 * GUARD + nbytes, dtype=torch.uint8, device="cuda")
        self.buf.view(torch.int32).fill_(PATTERN)
        self.t = self.buf[GUARD:GUARD + cpu.numel() * cpu.element_size()].view(cpu.dtype).view(cpu.shape)
        self.t.copy_(cpu)

    def guards_intact(self):
        g = self.buf.view(torch.int32)
        return bool((g[:GUARD // 4] == PATTERN).all()) and bool((g[-(GUARD // 4):] == PATTERN).all())

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        return self.t.cpu()


def planar(x):
    return Slab(VG.pad(x))


def planar_out(B, Cn, H, W):
    t = torch.zeros(B, Cn, H + 2, W + 2 * VG.PADL)
    VG.interior(t).fill_(NAN)
    return Slab(t)


def records(x):
    return Slab(VG.hs8_encode(x))


def records_out(B, Cn, H, W):
    t = torch.zeros(B, Cn // 8, H + 2, W + 2, 16, dtype=torch.float16)
    t[:, :, 1:-1, 1:-1] = NAN
    return Slab(t)


def plain_out(*shape):
    return Slab(torch.full(shape, NAN))


def probe(ctx, op, family, form, sizes, outs, expect=0, **operands):
    """One pnpx_vjp_glue_probe call; operands / outs: {descriptor field: Slab}.  The outputs' guards are checked."""
    from tfpnp_amd import _lib
    D = _lib.VjpGlueProbeDesc(op=op, family=family, form=form, **sizes)
    for k, v in list(operands.items()) + list(outs.items()):
        setattr(D, k, v.ptr())
    torch.cuda.synchronize()
    st = _lib.lib().pnpx_vjp_glue_probe(ctx.handle, C.byref(D), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if st == PNPX_ERR_HIP:                 # a HIP runtime error: nothing more may be started on this device
        pytest.exit("pnpx_vjp_glue_probe: " + _lib.lib().pnpx_last_error().decode(), returncode=3)
    torch.cuda.synchronize()
    assert st == expect, (st, _lib.lib().pnpx_last_error().decode())
    for k, v in outs.items():
        assert v.guards_intact(), f"the launch wrote outside its output {k}"
    return st


def _out_tensor(family, slab, what):
    """The interior of a padded output on the CPU (family 1: the records [B][G][H][W][16]); the border must still be +0."""
    t = slab.cpu()
    if family:
        assert bool((hs8_border(t).view(torch.int16) == 0).all()), f"{what}: a border record of the output is no longer zero"
        return t[:, :, 1:-1, 1:-1].contiguous()
    assert bool((VG.border_cells(t).view(torch.int32) == 0).all()), f"{what}: a border cell of the padded output is no longer +0.0"
    return VG.interior(t).contiguous()


def _records_interior(x):
    return VG.hs8_encode(x)[:, :, 1:-1, 1:-1].contiguous()


def _decode(rec):
    """[B][G][H][W][16] f16 records -> float64 values [B][8 G][H][W]."""
    v = (rec[..., :8].double() + rec[..., 8:].double()) / VG.ASCALE
    B, G, H, W, _ = v.shape
    return v.permute(0, 1, 4, 2, 3).reshape(B, G * 8, H, W)


def _sub(d, lo, hi):
    """Images [lo, hi) of a case's operands (the out-conv weights belong to no image)."""
    return {k: (v if k == "w" else v[lo:hi]) for k, v in d.items()}


def _image_and_repeat_checks(run, d, B, first, what):
    """`run(d, B)` -> tuple of CPU outputs.  A second launch is bit-identical; every image alone is bit-identical to its place in the batch."""
    again = run(d, B)
    for a, b in zip(first, again):
        assert VG.bits_equal(a, b), f"{what}: second launch differs"
    for i in range(B):
        one = run(_sub(d, i, i + 1), 1)
        for a, b in zip(first, one):
            assert VG.bits_equal(a[i:i + 1].contiguous(), b), f"{what}: image {i} alone differs from image {i} of the batch"


# ---------------------------------------------------------------------------------------------------------------------------------
# up-sampling adjoint

def _run_ups(ctx, c, family, form):
    def run(d, B):
        sizes = dict(B=B, C=c.C, H=c.h, W=c.w, Ccat=c.Ccat, c_off=c.c_off, Ht=c.Ht, Wt=c.Wt)
        mk, mko = (records, records_out) if family else (planar, planar_out)
        out = mko(B, c.C, c.h, c.w)
        probe(ctx, VG.UPSAMPLE_BWD, family, form, sizes, {"out": out}, g=mk(d["g"]), act=mk(d["act"]))
        return (_out_tensor(family, out, c.name),)
    return run


def _ups_forms(c, family):
    return (0,) if family else (0,) + VG.ups_forms_admitted(c.B, c.C)


def _check_ups(ctx, c, family, images=True):
    key = "ups_hs" if family else "ups_f32"
    d = VG.ups_inputs(c.name, family)
    ra, den = VG.ups_reference_a(c, d)
    rb = VG.ups_reference_b(c, d)
    got = {}
    for form in _ups_forms(c, family):
        run = _run_ups(ctx, c, family, form)
        (y,) = first = run(d, c.B)
        v = _decode(y) if family else y
        ea, eb = VG.measure(v, ra, den), VG.measure(v, rb, den)
        fname = "auto" if not form else VG.UPS_FORM_NAMES[form]
        print(f"\nvjp_glue_probe {key}_a {c.name} {fname} measure {ea:.4e} bar {VG.UPS_TIER_A:.4e}")
        print(f"vjp_glue_probe {key} {c.name} {fname} measure {eb:.4e} bar {VG.bar(key):.4e}")
        if ea > VG.UPS_TIER_A:      # is it the weight arithmetic (a build that no longer contracts s * d - i0 into an fma) or the kernel?
            plain = VG.measure(v, VG.ups_reference_a(c, d, VG.weight_table(c.h, False), VG.weight_table(c.w, False))[0], den)
            raise AssertionError(f"{c.name} {fname}: tier (a) {ea:.3e} > {VG.UPS_TIER_A:.3e}; against the uncontracted weight table {plain:.3e}")
        assert eb <= VG.bar(key), (c.name, fname, eb)
        if images:
            _image_and_repeat_checks(run, d, c.B, first, f"{c.name} {fname}")
        got[form] = y
    if not family:      # every forced form the geometry admits is the plain form bit for bit, and auto is the form the plan names
        for form, y in got.items():
            assert VG.bits_equal(y, got[VG.UPS_PLAIN]), (c.name, form)
        assert VG.plan(VG.UPSAMPLE_BWD, 0, B=c.B, C=c.C, H=c.h, W=c.w, Ccat=c.Ccat, c_off=c.c_off, Ht=c.Ht, Wt=c.Wt) == (VG.ups_form(c.B, c.C, c.w), 1)


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", VG.UPS_CASES, ids=lambda c: c.name)
def test_upsample_adjoint(ctx, case, family):
    _check_ups(ctx, case, family)


def test_upsample_adjoint_at_65536_planes_takes_the_plain_form(ctx):
    c = VG.UPS_MANY_PLANES
    assert c.B * c.C == 65536 and VG.plan(VG.UPSAMPLE_BWD, 0, B=c.B, C=c.C, H=c.h, W=c.w, Ccat=c.Ccat, c_off=0, Ht=c.Ht, Wt=c.Wt) == (VG.UPS_PLAIN, 1)
    _check_ups(ctx, c, 0, images=False)
    # the LDS-window forms refuse it and launch nothing
    d = VG.ups_inputs(c.name, 0)
    out = planar_out(c.B, c.C, c.h, c.w)
    probe(ctx, VG.UPSAMPLE_BWD, 0, VG.UPS_LDS16, dict(B=c.B, C=c.C, H=c.h, W=c.w, Ccat=c.Ccat, c_off=0, Ht=c.Ht, Wt=c.Wt), {"out": out},
          expect=PNPX_ERR_SHAPE, g=planar(d["g"]), act=planar(d["act"]))
    assert bool(torch.isnan(VG.interior(out.cpu())).all())


def test_half_split_upsample_adjoint_over_the_grid_limit_runs_in_slices(ctx):
    c = VG.UPS_HS_SLICED
    assert VG.plan(VG.UPSAMPLE_BWD, 1, B=c.B, C=c.C, H=c.h, W=c.w, Ccat=c.Ccat, c_off=0, Ht=c.Ht, Wt=c.Wt) == (1, 2)      # no launch above 65535
    _check_ups(ctx, c, 1, images=False)


@pytest.mark.parametrize("case", VG.UPS_ADJOINT_CASES, ids=lambda c: c.name)
def test_upsample_adjoint_identity_against_the_forward_kernel(ctx, case):
    """<up(x), g> = <x, up_bwd(g)> with up = the library's own forward up-sampling launch and LeakyReLU' = 1 everywhere."""
    from tfpnp_amd import _lib
    c = case
    d = VG.ups_inputs(c.name, 0, True)
    assert bool((d["act"] > 0).all()) and c.c_off == 0 and c.Ccat == c.C and (c.Ht, c.Wt) == (2 * c.h, 2 * c.w)
    x = VG.adjoint_x(c)
    src, dst = planar(x), Slab(torch.zeros(c.B, c.C, c.Ht + 2, c.Wt + 2 * VG.PADL))
    torch.cuda.synchronize()
    st = _lib.lib().pnpx_upsample2x_probe(ctx.handle, C.c_void_p(src.ptr()), C.c_void_p(dst.ptr()), c.B * c.C, c.h, c.w,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, _lib.lib().pnpx_last_error().decode()
    torch.cuda.synchronize()
    assert dst.guards_intact()
    up = VG.interior(dst.cpu())
    b = VG.bar("adjoint")
    for form in VG.ups_forms_admitted(c.B, c.C):
        (y,) = _run_ups(ctx, c, 0, form)(d, c.B)
        gap = VG.adjoint_gap(up, d["g"], x, y)
        print(f"\nvjp_glue_probe adjoint {c.name} {VG.UPS_FORM_NAMES[form]} measure {gap:.4e} bar {b:.4e}")
        assert gap <= b, (c.name, form, gap)


# ---------------------------------------------------------------------------------------------------------------------------------
# skip / pool merge

def _run_spm(ctx, c, family, form):
    def run(d, B):
        mk, mko = (records, records_out) if family else (planar, planar_out)
        out = mko(B, c.C, c.H, c.W)
        ops = {"g": mk(d["g"]), "act": mk(d["act"])}
        if c.pool:
            ops["g_pool"] = mk(d["g_pool"])
        probe(ctx, VG.SKIP_POOL_MERGE, family, form, dict(B=B, C=c.C, H=c.H, W=c.W, Ccat=c.Ccat), {"out": out}, **ops)
        return (_out_tensor(family, out, c.name),)
    return run


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", VG.SPM_CASES, ids=lambda c: c.name)
def test_skip_pool_merge(ctx, case, family):
    c = case
    d = VG.spm_inputs(c.name, family)
    want = VG.spm_restate32(c, d)
    want = _records_interior(want) if family else want
    forms = (0,) if family else (0,) + VG.spm_forms_admitted(c.H, c.W)
    for form in forms:
        run = _run_spm(ctx, c, family, form)
        first = run(d, c.B)
        assert VG.bits_equal(first[0], want), (c.name, form, "differs from the fp32 restatement")     # so both fp32 forms are torch.equal
        _image_and_repeat_checks(run, d, c.B, first, f"{c.name} form {form}")
    if not family:
        assert VG.plan(VG.SKIP_POOL_MERGE, 0, B=c.B, C=c.C, H=c.H, W=c.W, Ccat=c.Ccat) == (VG.spm_form(c.H, c.W), 1)
        if c.H % 2 or c.W % 2:             # the 2 x 2-block form refuses odd sizes and launches nothing
            out = planar_out(c.B, c.C, c.H, c.W)
            probe(ctx, VG.SKIP_POOL_MERGE, 0, VG.SPM_BLOCK, dict(B=c.B, C=c.C, H=c.H, W=c.W, Ccat=c.Ccat), {"out": out}, expect=PNPX_ERR_SHAPE,
                  g=planar(d["g"]), act=planar(d["act"]))
            assert bool(torch.isnan(VG.interior(out.cpu())).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# out-conv tail

def _run_outc(ctx, c, family):
    def run(d, B):
        out = (records_out if family else planar_out)(B, 32, c.H, c.W)
        res = plain_out(B, c.H, c.W)
        ops = {"g": Slab(d["g"]), "pre": Slab(d["pre"]), "w": Slab(d["w"]), "act": (records if family else planar)(d["act"])}
        if family:
            ops["sc"] = Slab(torch.tensor(VG.HS_SC, dtype=torch.float32))
        probe(ctx, VG.OUTC_BWD, family, 0, dict(B=B, C=32, H=c.H, W=c.W), {"out": out, "out_res": res}, **ops)
        return _out_tensor(family, out, c.name), res.cpu()
    return run


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", VG.OUTC_CASES, ids=lambda c: c.name)
def test_outc_tail(ctx, case, family):
    d = VG.outc_inputs(case.name, family)
    gf, gr = VG.outc_restate32(case, d, VG.HS_SC[0] if family else None)
    run = _run_outc(ctx, case, family)
    first = run(d, case.B)
    assert VG.bits_equal(first[1], gr), "g_res differs from the fp32 restatement"
    assert VG.bits_equal(first[0], _records_interior(gf) if family else gf), "g_feat differs from the fp32 restatement"
    _image_and_repeat_checks(run, d, case.B, first, case.name)


# ---------------------------------------------------------------------------------------------------------------------------------
# input gradient, sigma sums

def _run_ingrad(ctx, c, family):
    def run(d, B):
        gx, part, gs = plain_out(B, c.H, c.W), plain_out(B, VG.SIG_CHUNKS), plain_out(B)
        ops = {"g": (records if family else planar)(d["g"]), "g_res": Slab(d["g_res"])}
        if family:
            ops["sc"] = Slab(torch.tensor(VG.HS_SC, dtype=torch.float32))
        probe(ctx, VG.INPUT_GRAD, family, 0, dict(B=B, C=c.C, H=c.H, W=c.W), {"out": gx, "part": part, "gsigma": gs}, **ops)
        return gx.cpu(), part.cpu(), gs.cpu()
    return run


@pytest.mark.parametrize("family", [0, 1], ids=["f32", "hs"])
@pytest.mark.parametrize("case", VG.INGRAD_CASES, ids=lambda c: c.name)
def test_input_gradient_and_sigma_sums(ctx, case, family):
    c = case
    d = VG.ingrad_inputs(c.name, family)
    m = VG.HS_SC[1] if family else None
    run = _run_ingrad(ctx, c, family)
    gx, part, gs = first = run(d, c.B)
    assert VG.bits_equal(gx, VG.ingrad_restate32(c, d, m)), "gx differs from the fp32 restatement"
    _, part64, part_abs, gs64, gs_abs = VG.ingrad_reference(c, d, m or 1.0)
    kp, kf = VG.sigma_depth(c.H, c.W)           # k = serial steps of a thread + 6 shuffle steps + 2 (+ 64 for the final sum)
    ep, ef = (part.double() - part64).abs(), (gs.double() - gs64).abs()
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(gs).all())
    rp = float((ep / (kp * VG.U * part_abs).clamp_min(1e-300)).max())
    rf = float((ef / (kf * VG.U * gs_abs)).max())
    print(f"\nvjp_glue_probe sigma_part {c.name} k {kp} measure {rp:.4e} bar 1.0")
    print(f"vjp_glue_probe sigma_final {c.name} k {kf} measure {rf:.4e} bar 1.0")
    assert bool((ep <= kp * VG.U * part_abs).all()), (c.name, rp)          # an empty chunk: exactly 0
    assert bool((ef <= kf * VG.U * gs_abs).all()), (c.name, rf)
    _image_and_repeat_checks(run, d, c.B, first, c.name)


# ---------------------------------------------------------------------------------------------------------------------------------
# gradient scale

@pytest.mark.parametrize("name", sorted(VG.gscale_cases()))
def test_gradient_scale(ctx, name):
    x = VG.gscale_cases()[name]
    B, H, W = VG.GSCALE_N
    bits_want, inv, m = VG.gscale_expected(x)
    for _ in range(2):                       # the second launch: the maximum word is cleared by the launcher itself
        bits = Slab(torch.full((1,), -1, dtype=torch.int32))
        sc = plain_out(2)
        probe(ctx, VG.GRAD_SCALE, 1, 0, dict(B=B, C=1, H=H, W=W), {"out": sc, "bits": bits}, g=Slab(x))
        got = sc.cpu().numpy()
        assert int(bits.cpu()[0]) & 0xFFFFFFFF == bits_want, (name, hex(int(bits.cpu()[0]) & 0xFFFFFFFF), hex(bits_want))
        assert got.view(np.uint32).tolist() == [int(np.float32(inv).view(np.uint32)), int(np.float32(m).view(np.uint32))], (name, got, inv, m)


# ---------------------------------------------------------------------------------------------------------------------------------
# operands

def test_misplaced_and_missing_operands_are_refused(ctx):
    c = VG.SPM_BY_NAME["spm_16x16_nopool"]
    d = VG.spm_inputs(c.name)
    sizes = dict(B=c.B, C=c.C, H=c.H, W=c.W, Ccat=c.Ccat)
    out = planar_out(c.B, c.C, c.H, c.W)
    g, act = planar(d["g"]), planar(d["act"])
    probe(ctx, VG.SKIP_POOL_MERGE, 0, 0, sizes, {"out": out}, expect=PNPX_ERR_ARG, g=g, act=act, pre=act)       # no place for `pre`
    probe(ctx, VG.SKIP_POOL_MERGE, 0, 0, sizes, {"out": out}, expect=PNPX_ERR_ARG, g=g)                         # no activation
    probe(ctx, VG.UPSAMPLE_BWD, 0, 0, dict(B=c.B, C=c.C, H=8, W=8, Ccat=c.Ccat, c_off=8, Ht=16, Wt=16), {"out": out}, expect=PNPX_ERR_ARG,
          g=g, act=act, g_pool=act)
    probe(ctx, VG.SKIP_POOL_MERGE, 0, 0, dict(sizes, c_off=8), {"out": out}, expect=PNPX_ERR_ARG, g=g, act=act)
    assert bool(torch.isnan(VG.interior(out.cpu())).all())
