"""GPU tests of the F(4x4,3x3) kernel's 32-cout instance (csrc/conv3x3_winof4.hip): probe kind 12 against the float64 reference of one
layer (cases, bar and mutants: tests/winof4_c32_cases.py; bar: profiles/winof4_c32.md), and the whole network under option
fp32_winof4_c32 against the fp64 oracle."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import conv_layer_cases as CL
from tests import winof4_c32_cases as C32
from tests.golden_inputs import denoiser_inputs
from tests.test_gpu_conv_layers import PNPX_ERR_SHAPE, Launch, _check_borders
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

BITS = (1, 2, 25)
C32_ALL = sum(1 << li for li in BITS)


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("name", [c.name for _, c in C32.CASES])
def test_kind12_against_float64(ctx, name):
    B, c = C32.CASE_BY_NAME[name]
    d = C32.inputs(name)
    ref, den = C32.case_reference(name)
    L = Launch(ctx, C32.WINOF4_C32, c, d, 0, B)
    L.set_tails(False)
    out, pool = L.run()                                               # (the guard bands around out and pool_out are checked in there)
    _check_borders(out, "out")
    err = CL.measure(CL.interior(out), ref, den)
    print(f"{name}: measure {err:.3e}, bar {C32.bar():.3e}")
    assert err < C32.bar(), err
    if c.pool:
        _check_borders(pool, "pool_out")
        assert torch.equal(CL.interior(pool), F.max_pool2d(CL.interior(out), 2)), "fused pool != max_pool2d of the kernel's own output"
    # a second launch, and one with large finite garbage behind the input
    out2, pool2 = L.run()
    assert torch.equal(_bits(out2), _bits(out)), "second launch differs"
    L.set_tails(True)
    out3, pool3 = L.run()
    assert torch.equal(_bits(out3), _bits(out)), "result depends on what lies behind the input tensor"
    if c.pool:
        assert torch.equal(_bits(pool2), _bits(pool)) and torch.equal(_bits(pool3), _bits(pool))
    # images alone (the first and the last: the last one's regions are the ones a workgroup reaches as its second tile)
    for i in sorted({0, B - 1}) if B > 1 else ():
        L1 = Launch(ctx, C32.WINOF4_C32, c, d, i, i + 1)
        L1.set_tails(False)
        o1, p1 = L1.run()
        assert torch.equal(_bits(o1[0]), _bits(out[i])), f"image {i} alone differs from image {i} of the batch"
        if c.pool:
            assert torch.equal(_bits(p1[0]), _bits(pool[i]))


def test_impulses(ctx):
    """One 1.0 per image at the first and last pixel of a region, a tile and the image, in the first and last channel of the first and last
    chunk; every weight a different dyadic number: each of the 32 couts (both cout blocks) must show the weights the site selects."""
    c = CL._c("fwd", 32, 0, 32, 32, 128)
    xs, ys = (0, 3, 4, 63, 64, 127), (0, 3, 4, 15, 16, 31)
    chans = (0, 7, 24, 31)
    sites = [("in0", chans[i % 4], y, x) for i, (y, x) in enumerate((y, x) for y in ys for x in xs)]
    sites += [("in0", ch, y, x) for ch in chans for y in (0, 31) for x in (0, 127)]
    d = CL.impulse_inputs(c, sites)
    ref, _ = CL.reference(c, d, slope=CL.IMPULSE_SLOPE)
    L = Launch(ctx, C32.WINOF4_C32, c, d, 0, len(sites), slope=CL.IMPULSE_SLOPE)
    L.set_tails(False)
    out, _ = L.run()
    _check_borders(out, "out")
    # the measure's denominator for an impulse is the magnitude of the one weight an output sees: its absolute form keeps a zero output
    # (no tap of the site) in the check, at the scale of the largest weight
    err = float((CL.interior(out).double() - ref).abs().max() / d["w"].double().abs().max())
    print(f"impulses: max |y - ref| / max |w| = {err:.3e}, bar {C32.bar():.3e}")
    assert err < C32.bar(), err


def test_refused_geometries(ctx):
    for C0, C1, cout, H, W in C32.REFUSED:
        c = CL._c("fwd", C0, C1, cout, H, W)
        d = {"w": torch.zeros(cout, C0 + C1, 3, 3), "bias": torch.zeros(cout), "in0": torch.zeros(1, C0, H, W)}
        if C1:
            d["in1"] = torch.zeros(1, C1, H, W)
        Launch(ctx, C32.WINOF4_C32, c, d, 0, 1).run(expect=PNPX_ERR_SHAPE)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole network

def dev():
    return torch.device("cuda:0")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def _params():
    return synth.make_unet_params(0)


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """inputs and the fp64 oracle's pre-clamp output (computed once per shape, never modified)"""
    from oracle import pnp_oracle as O
    x, s = denoiser_inputs(B, H, W, 60 + B)
    p64 = {k: torch.as_tensor(v).double() for k, v in _params().items()}
    with torch.no_grad():
        sig = torch.from_numpy(s).double().view(B, 1, 1, 1).expand(B, 1, H, W)
        ref = O.unet_forward(torch.cat([torch.from_numpy(x).double(), sig], 1), p64)
    return x, s, ref


@pytest.fixture(scope="module")
def den():
    from tfpnp_amd.pnp import UNetDenoiser2D
    d = UNetDenoiser2D(state_dict=_params(), conv_mode=0)
    c = d.context(dev())
    saved = {k: c.get_option(k) for k in ("fp32_winof4_c32", "fp32_wino8_layers", "fp32_chains")}
    yield d
    for k, v in saved.items():
        c.set_option(k, v)


def _run(den, xt, st, mask):
    den.context(dev()).set_option("fp32_winof4_c32", mask)
    out, pre = den.forward_preclamp(xt, st)
    return out.clone(), pre.clone()


# 1 x 32 x 64: level 0 is two regions of 16 x 64 (the smallest image the instance runs on: W = 64); 2 x 64 x 64: the drift test's shape;
# 3 x 64 x 128: regions both ways, odd batch, two launch chains of unequal size
@pytest.mark.parametrize("B,H,W", [(1, 32, 64), (2, 64, 64), (3, 64, 128)])
def test_network_against_oracle(den, B, H, W):
    x, s, ref = _case(B, H, W)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    c = den.context(dev())
    out0, pre0 = _run(den, xt, st, 0)
    out4, pre4 = _run(den, xt, st, C32_ALL)
    assert c.get_option("fp32_winof4_c32") == C32_ALL
    assert not torch.equal(pre4, pre0), "the 32-cout instance did not run"
    e0, e4, e04 = rel(pre0.cpu(), ref), rel(pre4.cpu(), ref), rel(pre4, pre0)
    print(f"{B}x{H}x{W}: without vs fp64 {e0:.2e}, with vs fp64 {e4:.2e}, with vs without {e04:.2e}")
    assert e0 < 3e-6 and e4 < 3e-6 and e04 < 3e-6, (e0, e4, e04)
    assert torch.equal(out4, pre4.clamp(0.0, 1.0))
    # a second call is bit-identical, with the option and without it
    assert torch.equal(_run(den, xt, st, C32_ALL)[1], pre4) and torch.equal(_run(den, xt, st, 0)[1], pre0)
    # each bit alone reaches the kernel and stays within the bar
    for li in BITS:
        _, pre = _run(den, xt, st, 1 << li)
        assert not torch.equal(pre, pre0) and not torch.equal(pre, pre4), li
        assert rel(pre.cpu(), ref) < 3e-6 and rel(pre, pre0) < 3e-6, (li, rel(pre.cpu(), ref), rel(pre, pre0))
    # an image of the batch equals the same image run alone, under every launch-chain setting
    if B == 3:
        for chains in (1, 2):
            c.set_option("fp32_chains", chains)
            _, full = _run(den, xt, st, C32_ALL)
            assert torch.equal(full, pre4), chains
            for i in range(B):
                _, one = _run(den, xt[i:i + 1].contiguous(), st[i:i + 1].contiguous(), C32_ALL)
                assert torch.equal(one[0], full[i]), (chains, i)
        c.set_option("fp32_chains", 2)


def test_option_off_and_ineligible_shapes_take_the_f2_path(den):
    """fp32_winof4_c32 = 0 is the path the library took before the option existed: where no full-resolution layer is eligible (W = 96 is no
    multiple of 64) the option changes no bit, and neither does it with the layers' fp32_wino8_layers bits cleared.  This approximates
    the identity with the parent commit: no parent library exists in the tree, so that the option at 0 gives the parent's bytes at an
    ELIGIBLE shape rests on the selector's truth table (tests/test_winof4_c32_host.py: bit off = the 8-wave kernel, as before) and on the
    recorded `bench.py --dump-outputs` comparison against the parent's tree (profiles/winof4_c32.md), not on this test."""
    x, s = denoiser_inputs(1, 128, 96, 61)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    assert torch.equal(_run(den, xt, st, C32_ALL)[1], _run(den, xt, st, 0)[1])
    x, s, _ = _case(2, 64, 64)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    c = den.context(dev())
    full = (1 << 27) - 1
    c.set_option("fp32_wino8_layers", full & ~C32_ALL)
    a, b = _run(den, xt, st, C32_ALL)[1], _run(den, xt, st, 0)[1]
    c.set_option("fp32_wino8_layers", full)
    assert torch.equal(a, b)


def test_option_setter(den):
    from tfpnp_amd._lib import PnpxError
    c = den.context(dev())
    for bad in (-1, 1, 1 << 24, 1 << 26, C32_ALL | (1 << 3), 1 << 27):
        with pytest.raises(PnpxError):
            c.set_option("fp32_winof4_c32", bad)
    for v in (0, 1 << 1, 1 << 2, 1 << 25, C32_ALL):
        c.set_option("fp32_winof4_c32", v)
        assert c.get_option("fp32_winof4_c32") == v
