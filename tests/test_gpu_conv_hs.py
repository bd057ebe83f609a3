"""Every half-split convolution instance, one launch_conv_hs call at a time, against a float64 reference of that layer (the single-layer
probe pnpx_conv_hs_probe; cases, references, emulation and bars: tests/conv_hs_cases.py; bars: profiles/conv_hs_probe.md).

Per case: the plan's instance is the one the table expects; the per-element measure is under the class bar; a second launch is
bit-identical; the first, a middle and the last image of the batch are bit-identical to the image launched alone (every instance of the
family adds its products in the same K order, whatever tile the launcher picks for the smaller launch); every border record of out /
pool_out is still +0; pool_out is max_pool2d of the kernel's own out; 1 MiB of a fixed pattern before and after every output is untouched;
the result is bit-identical whether the 1 MiB behind each input holds zeros or large finite values; the range flag stays 0.
The float64 references are matrix products on the device (torch, no kernel of this library)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_hs_cases as HS

pytestmark = pytest.mark.gpu

GUARD = 1 << 20                       # bytes on either side of every tensor
PATTERN = 0x5A5AA5A5                  # as two f16: 211.25, -0.0222; as a float: 1.5e16 -- finite either way
PNPX_ERR_ARG, PNPX_ERR_SHAPE, PNPX_ERR_HIP = 1, 2, 5
F16_NAN = 0x7E00


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


class Slab:
    """A device tensor inside a larger buffer: GUARD bytes of PATTERN, the tensor, GUARD bytes of PATTERN."""

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        n4 = (n + 3) // 4
        self.buf = torch.empty(2 * (GUARD // 4) + n4, dtype=torch.int32, device="cuda")
        self.buf.fill_(PATTERN)
        self.t = self.buf[GUARD // 4:GUARD // 4 + n4].view(dtype)[:int(np.prod(shape))].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def tail(self):
        return self.buf[-(GUARD // 4):]

    def guards_intact(self):
        g = GUARD // 4
        return bool((self.buf[:g] == PATTERN).all()) and bool((self.buf[-g:] == PATTERN).all())

    def ptr(self):
        return self.t.data_ptr()


def _hs8_output(B, G, H, W):
    """An HS8 output tensor: zero border, NaN interior (a pixel the kernel leaves out shows)."""
    s = Slab((B, G, H + 2, W + 2, 16), torch.float16)
    s.t.zero_()
    s.t[:, :, 1:-1, 1:-1].view(torch.int16).fill_(F16_NAN)
    return s


class Launch:
    """The device operands of images [lo, hi) of a case's inputs d (plain fp32 layouts on the device), and probe launches on them."""

    HS8 = ("in0", "in1", "res", "dmask")
    F32 = ("x_in", "first_x", "first_sigma")
    HOST = ("w", "bias", "outc_w", "outc_b", "first_w", "first_b")

    def __init__(self, ctx, c, d, lo, hi):
        self.ctx, self.c, self.B = ctx, c, hi - lo
        self.ins, self.host = {}, {}
        for k in self.HS8:
            if k in d:
                r = HS.hs8_encode(d[k][lo:hi])
                self.ins[k] = Slab(tuple(r.shape), torch.float16, fill=r)
        for k in self.F32:
            if k in d:
                x = d[k][lo:hi].contiguous()
                self.ins[k] = Slab(tuple(x.shape), torch.float32, fill=x)
        for k in self.HOST:
            if k in d:
                self.host[k] = np.ascontiguousarray(d[k].cpu().numpy(), dtype=np.float32)

    def set_tails(self, garbage):
        for i, s in enumerate(self.ins.values()):
            if garbage:
                g = torch.Generator(device="cuda").manual_seed(77 + i)
                t = s.tail()
                if s.t.dtype == torch.float16:
                    t.view(torch.float16).copy_((1e3 * torch.randn(t.numel() * 2, device="cuda", generator=g)).half())
                else:
                    t.view(torch.float32).copy_(1e3 * torch.randn(t.numel(), device="cuda", generator=g))
            else:
                s.tail().zero_()

    def run(self, c=None, expect=0, want_flag=True):
        """One launch into fresh output slabs -> {"out", "pool": raw records; "pre", "img": fp32; "flag"} on the CPU; guards checked."""
        from tfpnp_amd import _lib
        c = c or self.c
        B, G = self.B, c.cout // 8
        outs = {}
        if c.epi == "outc":
            outs["out_img"] = Slab((B, c.H, c.W), torch.float32, fill=torch.full((B, c.H, c.W), float("nan"), device="cuda"))
            outs["out_pre"] = Slab((B, c.H, c.W), torch.float32, fill=torch.full((B, c.H, c.W), float("nan"), device="cuda"))
        else:
            outs["out"] = _hs8_output(B, G, c.H, c.W)
        if c.pool:
            outs["pool_out"] = _hs8_output(B, G, c.H // 2, c.W // 2)
        ptr = {k: s.ptr() for k, s in self.ins.items()}
        ptr.update({k: s.ptr() for k, s in outs.items()})
        ptr.update({k: a.ctypes.data for k, a in self.host.items()})
        D = HS.descriptor(c, ptr, B)
        flag = C.c_uint(0xFFFFFFFF)
        D.want_range_flag = int(want_flag)
        D.range_flag_out = C.pointer(flag)
        torch.cuda.synchronize()
        st = _lib.lib().pnpx_conv_hs_probe(self.ctx.handle, C.byref(D), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        if st == PNPX_ERR_HIP:                 # a HIP runtime error: nothing more may be started on this device
            pytest.exit("pnpx_conv_hs_probe: " + _lib.lib().pnpx_last_error().decode(), returncode=3)
        assert st == expect, (c.name, st, _lib.lib().pnpx_last_error().decode())
        assert all(s.guards_intact() for s in outs.values()), "the kernel wrote outside an output tensor"
        res = {"flag": flag.value}
        for k, name in (("out", "out"), ("pool_out", "pool"), ("out_pre", "pre"), ("out_img", "img")):
            if k in outs:
                res[name] = outs[k].t.cpu()
        return res


def _same_bits(a, b):
    if a.dtype == torch.float16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _assert_same(a, b, what):
    for k in ("out", "pool", "pre", "img"):
        if k in a:
            assert _same_bits(a[k], b[k]), f"{what}: {k} differs"


def _check_borders(res):
    for k in ("out", "pool"):
        if k in res:
            assert bool((HS.hs8_border(res[k]).view(torch.int16) == 0).all()), f"{k}: a border record is no longer +0"


def _decoded(c, res):
    if c.epi == "outc":
        return {"pre": res["pre"].double(), "img": res["img"].double()}
    return {"out": HS.hs8_decode(res["out"])}


def _device_inputs(c):
    return {k: v.cuda() for k, v in HS.inputs(c).items()}


def _run_case(ctx, c):
    """All the per-case checks; returns the measure."""
    d = _device_inputs(c)
    ref = {k: v.cpu() for k, v in HS.reference(c, d, device="cuda").items()}
    L = Launch(ctx, c, d, 0, c.B)
    L.set_tails(False)
    r1 = L.run()
    _check_borders(r1)
    assert r1["flag"] == 0, "range flag raised on values far inside the range"
    err = HS.case_measure(c, _decoded(c, r1), ref)
    if c.epi == "outc":
        assert torch.equal(r1["img"], r1["pre"].clamp(0.0, 1.0))
    if c.pool:
        assert torch.equal(HS.hs8_decode(r1["pool"]), F.max_pool2d(HS.hs8_decode(r1["out"]), 2)), "fused pool != max_pool2d of the kernel's own output"
    # a second launch on the same operands, then one with large finite garbage behind every input
    _assert_same(r1, L.run(), "second launch")
    L.set_tails(True)
    _assert_same(r1, L.run(), "garbage behind the inputs")
    # images alone (the folded first convolution has no instance for a single image: the launcher refuses it there)
    if not c.first:
        for i in sorted({0, c.B // 2, c.B - 1}):
            if c.B == 1:
                break
            assert HS.plan(c, B=1) is not None
            L1 = Launch(ctx, c, d, i, i + 1)
            L1.set_tails(False)
            a = L1.run()
            one = {k: (v[i:i + 1] if k != "flag" else v) for k, v in r1.items()}
            _assert_same(one, a, f"image {i} alone")
    return err


@pytest.mark.parametrize("case", HS.CASES, ids=[c.name for c in HS.CASES])
def test_layer_against_fp64(ctx, case):
    p = HS.plan(case)
    assert p is not None and HS.expected(p) == case.expect, (p, case.expect)
    b = HS.bar(case.cls)
    err = _run_case(ctx, case)
    print(f"\nconv_hs_probe {case.cls} {case.name} instance {p[:8]} grid {p[9]} tiles {p[10]} measure {err:.4e} bar {b:.4e}")
    assert err <= b, (case.name, err, b)


def test_reference_on_the_device_is_the_reference_on_the_host():
    for name in ("act1ff_16to32_5x40_B2", "dthr1b0_16to128_9x40_B2_res_rg4_a-0.25", "act1ff_64+32to64_10x40_B2_ups"):
        c = HS.CASE_BY_NAME[name]
        d = HS.inputs(c)
        a, b = HS.reference(c, d), HS.reference(c, {k: v.cuda() for k, v in d.items()}, device="cuda")
        for k in a:
            assert float((a[k] - b[k].cpu()).abs().max()) <= 1e-12 * float(a[k].abs().max()), (name, k)


def _variant_bits(ctx, c, variants, want_distinct):
    """The case launched as each variant of itself on the same operands: all bit-identical; the plans must be `want_distinct` apart."""
    d = _device_inputs(c)
    L = Launch(ctx, c, d, 0, c.B)
    L.set_tails(False)
    plans = [HS.plan(v) for v in variants]
    assert all(p is not None for p in plans) and len({want_distinct(p) for p in plans}) == len(variants), plans
    first = L.run(variants[0])
    for v in variants[1:]:
        _assert_same(first, L.run(v), v.name)


@pytest.mark.parametrize("name", ["act1ff_16to32_4x4_B1", "res1ff_16to192_12x24_B32_res", "dthr1ff_16to512_64x4_B32_a0.3", "act1ff_16to32_40x40_B32",
                                  "act1ff_16to64_4x32_B1", "trelu01b_16to192_12x24_B32_a0.3"])
def test_share_does_not_change_a_bit(ctx, name):
    c = HS.CASE_BY_NAME[name]
    _variant_bits(ctx, c, [c, c._replace(share=2)], lambda p: (p[1], p[3], p[11]))


@pytest.mark.parametrize("name", ["act1ff_32to32_20x40_B64", "outc1ff_32to32_20x40_B64"])
def test_weights_in_registers_do_not_change_a_bit(ctx, name):
    c = HS.CASE_BY_NAME[name]
    _variant_bits(ctx, c, [c._replace(wreg=0), c._replace(wreg=1), c], lambda p: (p[1], p[3], p[6]))


@pytest.mark.parametrize("name", ["act1ff_16to64_64x40_B32", "dmask1ff_16to512_64x4_B32", "act1ff_16to128_64x40_B32_pool"])
def test_half_tiles_do_not_change_a_bit(ctx, name):
    """The batch runs the 64-cout instance; a few of its images alone run the 32-cout instance over the same 64-cout packing."""
    c = HS.CASE_BY_NAME[name]
    big, small = HS.plan(c), HS.plan(c, B=2)
    assert (big[0], big[8]) == (64, 64) and (small[0], small[8]) == (32, 64)
    d = _device_inputs(c)
    L = Launch(ctx, c, d, 0, c.B)
    L.set_tails(False)
    r = L.run()
    L2 = Launch(ctx, c, d, 5, 7)
    L2.set_tails(False)
    _assert_same({k: (v[5:7] if k != "flag" else v) for k, v in r.items()}, L2.run(), "half tiles")


@pytest.mark.parametrize("name", ["act1ff_48+16to32_18x40_B2_ups", "act1ff_64+32to64_10x40_B2_ups"])
def test_fused_upsampling_against_the_two_source_launch(ctx, name):
    """The fused bilinear x2 against the same layer launched on a second source that was up-sampled beforehand (in fp32 by the kernels'
    own formula, tests/conv_layer_cases.py upsample32, and split again): two launches within their bars of one reference are within twice
    the bar of each other.  (The network-level test, test_gpu_modes.py, holds the two forms to 1e-6 of each other, not to equal bits: the
    separate up-sampling kernel is another translation unit's arithmetic.)"""
    from tests import conv_layer_cases as CL
    c = HS.CASE_BY_NAME[name]
    d = HS.inputs(c)
    hi, lo = HS.split(d["in1"] * HS.ASCALE)
    up = CL.upsample32(hi.float() + lo.float(), c.H, c.W) / HS.ASCALE
    c2 = c._replace(ups=False, cls="act")
    assert HS.plan(c)[5] == 1 and HS.plan(c2)[5] == 0
    ref = HS.reference(c, d)
    dd = {k: v.cuda() for k, v in d.items()}
    La = Launch(ctx, c, dd, 0, c.B)
    Lb = Launch(ctx, c2, dict(dd, in1=up.cuda()), 0, c.B)
    La.set_tails(False), Lb.set_tails(False)
    ya, yb = HS.hs8_decode(La.run()["out"]), HS.hs8_decode(Lb.run()["out"])
    ea, eb = HS.measure(ya, ref["out"], ref["den"]), HS.measure(yb, ref["out"], ref["den"])
    print(f"\nconv_hs_probe fused up-sampling {name}: fused {ea:.3e} pre-up-sampled {eb:.3e} identical bits {torch.equal(ya, yb)}")
    assert ea <= HS.bar("ups") and eb <= HS.bar("ups") and HS.measure(ya, yb, ref["den"]) <= 2 * HS.bar("ups")


@pytest.mark.parametrize("name", ["act1ff_16to32_5x40_B2", "res1ff_16to64_5x40_B2_res", "trelu1ff_16to64_6x24_B2_a0.3", "dthr1ff_16to64_6x24_B2_a0.3_nomask",
                                  "dmask1ff_16to32_7x40_B2_sl1"])
def test_range_flag(ctx, name):
    """One stored value of magnitude >= 4095 raises the flag, the same case scaled just below leaves it 0, NaN raises it."""
    c = HS.CASE_BY_NAME[name]
    d = HS.inputs(c)
    d["in0"] = torch.zeros_like(d["in0"])
    d["w"] = torch.zeros_like(d["w"])
    d["w"][0, 0, 1, 1] = 2.0                      # out[:, 0] = 2 in0[:, 0] (+ bias / res), every other channel = bias: inputs stay in range
    for k in ("bias", "res"):
        if k in d:
            d[k] = torch.zeros_like(d[k])
    y, x = c.H - 1, c.W - 1                       # the last pixel: in the partial tile
    linear = c.epi in ("dmask", "dthr")           # a rectifier would shrink or clip the negative value
    for value, want in ((4095.0, 1), (-4095.0, 1 if linear else 0), (4094.0, 0), (float("nan"), 1)):
        d["in0"][-1, 0, y, x] = value / 2
        L = Launch(ctx, c, {k: v.cuda() for k, v in d.items()}, 0, c.B)
        L.set_tails(False)
        r = L.run()
        assert r["flag"] == want, (name, value, r["flag"])
        if value == 4094.0:
            assert float(HS.hs8_decode(r["out"])[-1, 0, y, x]) == value
        assert L.run(want_flag=False)["flag"] == 0          # no flag wanted: none handed to the kernel


def test_range_flag_is_not_touched_by_the_out_conv(ctx):
    c = HS.CASE_BY_NAME["outc1ff_16to32_5x40_B2"]
    d = HS.inputs(c)
    d["in0"] = torch.zeros_like(d["in0"])
    d["in0"][0, 0, 2, 3] = 2047.5
    d["w"] = torch.zeros_like(d["w"])
    d["w"][0, 0, 1, 1] = 2.0                      # channel 0 of the 32-channel activation = 4095 at that pixel
    d["bias"] = torch.zeros_like(d["bias"])
    L = Launch(ctx, c, {k: v.cuda() for k, v in d.items()}, 0, c.B)
    L.set_tails(False)
    r = L.run()
    assert r["flag"] == 0
    want = float(d["x_in"][0, 2, 3]) + 4095.0 * float(d["outc_w"][0]) + float(d["outc_b"][0])
    assert abs(float(r["pre"][0, 2, 3]) - want) <= 1e-6 * (abs(want) + 4095.0 * abs(float(d["outc_w"][0])))


@pytest.mark.parametrize("name,kw,message", HS.REFUSED, ids=[r[0] for r in HS.REFUSED])
def test_refused_combinations_launch_nothing(ctx, name, kw, message):
    from tfpnp_amd import _lib
    c = HS.refused_case(kw)
    assert HS.plan(c) is None
    d = HS.inputs(c)
    L = Launch(ctx, c, {k: v.cuda() for k, v in d.items()}, 0, c.B)
    r = L.run(expect=PNPX_ERR_SHAPE)
    assert message in _lib.lib().pnpx_last_error().decode()
    # nothing ran: the outputs' interiors still hold what they were filled with, their borders are still zero
    for k in ("out", "pool"):
        if k in r:
            assert bool((r[k][:, :, 1:-1, 1:-1].view(torch.int16) == F16_NAN).all())
    for k in ("pre", "img"):
        if k in r:
            assert bool(torch.isnan(r[k]).all())
    _check_borders(r)


def test_dropped_operands_are_refused(ctx):
    """An operand the selected path has no place for: PNPX_ERR_ARG, nothing launched."""
    c = HS.CASE_BY_NAME["act1ff_16to32_4x32_B1_pool"]._replace(H=5)      # no pool is fused at an odd height
    d = HS.inputs(c)
    L = Launch(ctx, c, {k: v.cuda() for k, v in d.items()}, 0, c.B)
    r = L.run(expect=PNPX_ERR_ARG)
    assert bool((r["out"][:, :, 1:-1, 1:-1].view(torch.int16) == F16_NAN).all())
