"""Every fp32 3x3 convolution kernel of conv_mode 0, one layer at a time, against a float64 reference of that layer (the single-layer
probe pnpx_conv3x3_probe; cases, references, bars and impulse cases: tests/conv_layer_cases.py; bars: profiles/conv_layer_probe.md).

Per (kind, case): the per-element measure under the class bar; image i of a B = 3 launch bit-identical to the image launched alone; a
second launch bit-identical; every border cell of the padded output still zero; 1 MiB of a fixed bit pattern before and after every
output untouched; the result bit-identical whether the 1 MiB after each input holds zeros or large finite garbage."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import conv_layer_cases as CL

pytestmark = pytest.mark.gpu

GUARD = 1 << 18                       # floats: 1 MiB on either side of every tensor
PATTERN = 0x5A5AA5A5                  # as a float: 1.5e16, finite
PNPX_ERR_SHAPE, PNPX_ERR_HIP = 2, 5


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


class Slab:
    """A padded-planar device tensor inside a larger buffer: GUARD floats of PATTERN, the tensor, GUARD floats of PATTERN."""

    def __init__(self, shape, fill=None, nan_interior=False):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(2 * GUARD + n, dtype=torch.float32, device="cuda")
        self.buf.view(torch.int32).fill_(PATTERN)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.zero_()
        if fill is not None:
            CL.interior(self.t).copy_(fill)
        elif nan_interior:                     # an output: a pixel the kernel leaves out shows
            CL.interior(self.t).fill_(float("nan"))

    def tail(self):
        return self.buf[-GUARD:]

    def guards_intact(self):
        g = self.buf.view(torch.int32)
        return bool((g[:GUARD] == PATTERN).all()) and bool((g[-GUARD:] == PATTERN).all())

    def ptr(self):
        return self.t.data_ptr()


def _hw(c, src):
    return (c.H // 2, c.W // 2) if (c.op == "ups" and src == "in1") else (c.H, c.W)


class Launch:
    """The device operands of one case for images [lo, hi) of its inputs, and launches of one kind on them."""

    def __init__(self, ctx, kind, c, d, lo, hi, masked=False, slope=CL.SLOPE):
        self.ctx, self.kind, self.c, self.d, self.B, self.masked, self.slope = ctx, kind, c, d, hi - lo, masked, slope
        self.ins = {}
        for src in ("in0", "in1", "res", "mask"):
            if src in d and (src != "mask" or masked):
                x = d[src][lo:hi]
                h, w = _hw(c, src)
                self.ins[src] = Slab((hi - lo, x.shape[1], h + 2, w + 2 * CL.PADL), fill=x.cuda())
        self.w = d["w"].contiguous().numpy()
        self.bias = d["bias"].contiguous().numpy() if "bias" in d else None

    def set_tails(self, garbage):
        for i, s in enumerate(self.ins.values()):
            if garbage:
                g = torch.Generator(device="cuda").manual_seed(77 + i)
                s.tail().copy_(1e3 * torch.randn(GUARD, device="cuda", generator=g))
            else:
                s.tail().zero_()

    def run(self, expect=0):
        """One launch into fresh output slabs -> (status, padded out on the CPU, padded pool_out or None); guards checked."""
        from tfpnp_amd import _lib
        c, B = self.c, self.B
        pool = c.pool
        out = Slab((B, c.cout, c.H + 2, c.W + 2 * CL.PADL), nan_interior=True)
        po = Slab((B, c.cout, c.H // 2 + 2, c.W // 2 + 2 * CL.PADL), nan_interior=True) if pool else None
        p = lambda k: C.c_void_p(self.ins[k].ptr()) if k in self.ins else None
        torch.cuda.synchronize()
        st = _lib.lib().pnpx_conv3x3_probe(
            self.ctx.handle, self.kind, self.w.ctypes.data, self.bias.ctypes.data if self.bias is not None else None, c.cout,
            p("in0"), c.C0, p("in1"), c.C1, C.c_void_p(out.ptr()), p("res"), p("mask"), self.slope, C.c_void_p(po.ptr()) if po else None,
            1, B, c.H, c.W, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        if st == PNPX_ERR_HIP:                 # a HIP runtime error: nothing more may be started on this device
            pytest.exit("pnpx_conv3x3_probe: " + _lib.lib().pnpx_last_error().decode(), returncode=3)
        assert st == expect, (st, _lib.lib().pnpx_last_error().decode())
        assert out.guards_intact() and (po is None or po.guards_intact()), "the kernel wrote outside its output tensor"
        return out.t.cpu(), (po.t.cpu() if po else None)


def _check_borders(xp, what):
    b = CL.border_cells(xp)
    assert bool((b.view(torch.int32) == 0).all()), f"{what}: a border cell of the padded output is no longer +0.0"


def _run_case(ctx, kind, c, masked):
    """All the per-case checks of one kind; returns the measure."""
    d = CL.inputs(c.name)
    ref, den = CL.case_reference(c.name, masked)
    L = Launch(ctx, kind, c, d, 0, CL.B_MAX, masked)
    L.set_tails(False)
    out, pool = L.run()
    _check_borders(out, "out")
    err = CL.measure(CL.interior(out), ref, den)
    if pool is not None:
        _check_borders(pool, "pool_out")
        assert torch.equal(CL.interior(pool), F.max_pool2d(CL.interior(out), 2)), "fused pool != max_pool2d of the kernel's own output"
    # a second launch on the same operands, then one with large finite garbage behind every input
    out2, pool2 = L.run()
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), "second launch differs"
    L.set_tails(True)
    out3, pool3 = L.run()
    assert torch.equal(out3.view(torch.int32), out.view(torch.int32)), "result depends on what lies behind the input tensors"
    if pool is not None:
        assert torch.equal(pool2.view(torch.int32), pool.view(torch.int32)) and torch.equal(pool3.view(torch.int32), pool.view(torch.int32))
    # every image alone
    for i in range(CL.B_MAX):
        L1 = Launch(ctx, kind, c, d, i, i + 1, masked)
        L1.set_tails(False)
        o1, p1 = L1.run()
        assert torch.equal(o1[0].view(torch.int32), out[i].view(torch.int32)), f"image {i} alone differs from image {i} of the batch"
        if pool is not None:
            assert torch.equal(p1[0].view(torch.int32), pool[i].view(torch.int32))
    return err, out


RUNS = CL.runs()


@pytest.mark.parametrize("kind,case", RUNS, ids=[f"{CL.KIND_NAMES[k]}-{c.name}" for k, c in RUNS])
def test_layer_against_fp64(ctx, kind, case):
    assert CL.plan(kind, case)[0] == CL.accepts(kind, case) != 0
    b = CL.bar(kind)
    for masked in ((False, True) if case.op == "adj" else (False,)):
        err, _ = _run_case(ctx, kind, case, masked)
        print(f"\nconv_layer_probe {CL.KIND_NAMES[kind]} {case.name}{'_mask' if masked else ''} measure {err:.4e} bar {b:.4e}")
        assert err <= b, (CL.KIND_NAMES[kind], case.name, masked, err, b)


def test_ksplit_really_splits_and_one_piece_is_the_unsplit_result(ctx):
    for name, pieces in CL.KSPLIT_PIECES.items():
        c = CL.CASE_BY_NAME[name]
        assert CL.plan(CL.WINO8_KSPLIT, c) == (64, pieces), name
    # a piece straddles the source boundary: 24 chunks in 4 pieces of 6, the first source holds 8
    c = CL.CASE_BY_NAME["fwd_128+256to256_16x16"]
    assert (c.C0 // 16) % ((c.C0 + c.C1) // 16 // 4) != 0
    # one piece: the launch that was handed the scratch is the unsplit launch
    c = CL.CASE_BY_NAME["fwd_64to64_16x16"]
    d = CL.inputs(c.name)
    outs = []
    for kind in (CL.WINO8, CL.WINO8_KSPLIT):
        L = Launch(ctx, kind, c, d, 0, CL.B_MAX)
        L.set_tails(False)
        outs.append(L.run()[0])
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("name", ["adj_32to96_16x32", "adj_512to256_16x16", "adj_256to768_32x16"])
def test_adjoint_kinds_agree_at_zero_mask_cells(ctx, name):
    """Exact +0.0 and -0.0 mask cells take the factor `slope` in both adjoint kernels (the `> 0.f` test; torch's convention)."""
    c, d = CL.CASE_BY_NAME[name], CL.inputs(name)
    ref, den = CL.case_reference(name, True)
    lin, _ = CL.case_reference(name, False)
    cells = d["zero_cells"]
    assert bool((d["mask"].reshape(-1)[cells] == 0).all())
    got = {}
    for kind in CL.GRAD_KINDS:
        L = Launch(ctx, kind, c, d, 0, CL.B_MAX, masked=True)
        L.set_tails(False)
        y = CL.interior(L.run()[0]).reshape(-1)[cells].double()
        r, dn, l = ref.reshape(-1)[cells], den.reshape(-1)[cells], lin.reshape(-1)[cells]
        assert bool(((y - r).abs() <= CL.bar(kind) * dn).all()), CL.KIND_NAMES[kind]
        # ... which is the slope branch: the other branch is 1 / slope times as large
        assert bool(((y - l).abs() > (y - r).abs()).all() or float(l.abs().max()) == 0.0)
        got[kind] = y
    # two algorithms, each within its bar of the reference: within the sum of the bars of each other
    tol = (CL.bar(CL.DIRECT_GRAD) + CL.bar(CL.WINO8_GRAD)) * den.reshape(-1)[cells]
    assert bool(((got[CL.DIRECT_GRAD] - got[CL.WINO8_GRAD]).abs() <= tol).all())


@pytest.mark.parametrize("geom", CL.REFUSED, ids=[f"{CL.KIND_NAMES[g[0]]}-{g[1]}+{g[2]}to{g[3]}_{g[4]}x{g[5]}" for g in CL.REFUSED])
def test_refused_geometries_launch_nothing(ctx, geom):
    from tfpnp_amd import _lib
    kind, C0, C1, cout, H, W = geom
    op = "ups" if kind == CL.WINO8_UPS else ("adj" if kind in CL.GRAD_KINDS else "fwd")
    c = CL.Case("refused", op, C0, C1, cout, H, W, False, False)
    assert CL.plan(kind, c) == (0, 0)
    d = {"w": torch.zeros((C0, cout, 3, 3) if op == "adj" else (cout, C0 + C1, 3, 3)), "in0": torch.ones(1, C0, H, W)}
    if op != "adj":
        d["bias"] = torch.ones(cout)
    if C1:
        d["in1"] = torch.ones((1, C1) + _hw(c, "in1"))
    L = Launch(ctx, kind, c, d, 0, 1)
    out, _ = L.run(expect=PNPX_ERR_SHAPE)
    msg = _lib.lib().pnpx_last_error().decode()
    assert "unsupported geometry" in msg or "single-source" in msg or "incompatible" in msg, msg
    # nothing ran: the output's interior still holds what it was filled with, its border is still zero
    assert bool(torch.isnan(CL.interior(out)).all())
    _check_borders(out, "out")


IMPULSE_RUNS = [(k, c) for c in CL.IMPULSE_CASES for k in CL.kinds_of(c) if CL.accepts(k, c)]


def _impulse_expected(c, d, sites, planes):
    """float64 output of the impulse operands: per image the flipped 3x3 stencil of w[:, channel] around the site (adjoint: the plain
    stencil of w[channel]), LeakyReLU(0.5) applied; per plane image the sums of the channel's taps that fall inside the image."""
    w = d["w"].double()
    n = len(sites) + len(planes)
    ref = torch.zeros(n, c.cout, c.H, c.W, dtype=torch.float64)
    for i, (src, ch, y, x) in enumerate(sites):
        chan = ch + (c.C0 if src == "in1" else 0)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= y + dy < c.H and 0 <= x + dx < c.W:
                    ref[i, :, y + dy, x + dx] = w[chan, :, 1 + dy, 1 + dx] if c.op == "adj" else w[:, chan, 1 - dy, 1 - dx]
    den = torch.zeros_like(ref)
    for j, ch in enumerate(planes):
        one = torch.ones(1, 1, c.H, c.W, dtype=torch.float64)
        wk = w[:, c.C0 + ch:c.C0 + ch + 1]
        ref[len(sites) + j] = F.conv2d(one, wk, padding=1)[0]
        den[len(sites) + j] = F.conv2d(one, wk.abs(), padding=1)[0]
    return (ref if c.op == "adj" else F.leaky_relu(ref, CL.IMPULSE_SLOPE)), den


@pytest.mark.parametrize("kind,case", IMPULSE_RUNS, ids=[f"{CL.KIND_NAMES[k]}-{c.name}" for k, c in IMPULSE_RUNS])
def test_impulse_responses(ctx, kind, case):
    c = case
    ct = CL.accepts(kind, c)
    chunk = 8 if (kind in (CL.DIRECT, CL.DIRECT_GRAD, CL.WINOF4) or ct == 32) else 16      # channels per K step of the kind
    sites, planes = CL.impulse_sites(c, chunk), CL.impulse_planes(c)
    d = CL.impulse_inputs(c, sites, planes)
    ref, den = _impulse_expected(c, d, sites, planes)
    wmax = float(d["w"].abs().max())
    tol = CL.bar(kind) * wmax
    n = len(sites) + len(planes)
    worst = 0.0
    for lo in range(0, n, 32):
        hi = min(n, lo + 32)
        L = Launch(ctx, kind, c, d, lo, hi, slope=CL.IMPULSE_SLOPE)
        L.set_tails(False)
        out, _ = L.run()
        _check_borders(out, "out")
        e = (CL.interior(out).double() - ref[lo:hi]).abs()
        assert bool(torch.isfinite(e).all())
        for i in range(lo, hi):
            ei = e[i - lo]
            if i < len(sites):
                worst = max(worst, float(ei.max()) / wmax)
                assert float(ei.max()) <= tol, (CL.KIND_NAMES[kind], c.name, sites[i], float(ei.max()), tol)
            else:                              # a constant plane: 9 taps add up, so the per-element measure
                assert bool((ei <= CL.bar(kind) * den[i]).all()), (CL.KIND_NAMES[kind], c.name, "plane", planes[i - len(sites)])
    print(f"\nconv_layer_impulse {CL.KIND_NAMES[kind]} {c.name} worst |y - stencil| / max|w| {worst:.3e} bar {CL.bar(kind):.3e}")
