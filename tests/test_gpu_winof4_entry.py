"""GPU tests of the decoder entries on the Winograd F(4x4,3x3) kernel (csrc/conv3x3_winof4.hip's two-source instance, option
fp32_winof4_entries).  Per layer through the probe (kind PNPX_PROBE_WINOF4_2SRC) against float64 references built from the LOW-resolution
second source (tests/winof4_entry_cases.py; bar: profiles/winof4_entries.md), and through the whole network (forward_preclamp).

Figures of the first run on an MI355X (measure against the bar 2.6687e-05): see profiles/winof4_entries.md."""
import pytest
import torch

from tests import conv_layer_cases as CL
from tests import winof4_entry_cases as EC
from tests.golden_inputs import denoiser_inputs
from tests.test_gpu_conv_layers import PNPX_ERR_SHAPE, Launch, _check_borders, _impulse_expected
from tests.test_gpu_winof4 import _case, _params      # the shapes' inputs and fp64 oracle forwards, computed once for both files

pytestmark = pytest.mark.gpu

PNPX_ERR_ARG = 1
ALL = (1 << 27) - 1
ENTRIES = (1 << 15) | (1 << 18) | (1 << 21)


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ one layer, through the probe

@pytest.mark.parametrize("i", range(len(EC.ENTRY_CASES)), ids=[c.name for _, c in EC.ENTRY_CASES])
def test_entry_layer_against_fp64(ctx, i):
    B, c = EC.ENTRY_CASES[i]
    assert CL.plan(EC.WINOF4_2SRC, c) == (64, 1)
    cf, df = EC.full_res(c, EC.inputs(i))                 # what the kernel takes: the second source up-sampled in fp32
    ref, den = EC.case_reference(i)                        # what it is held to: float64 from the low-resolution source
    L = Launch(ctx, EC.WINOF4_2SRC, cf, df, 0, B)
    L.set_tails(False)
    out, _ = L.run()
    _check_borders(out, "out")                             # (Launch.run checks the guard bands around the output)
    err = CL.measure(CL.interior(out), ref[:B], den[:B])
    print(f"\nwinof4_entry {c.name} B={B} measure {err:.4e} bar {EC.bar():.4e}")
    assert err <= EC.bar(), (c.name, err, EC.bar())
    # a second launch, and one with large finite garbage behind every input
    out2, _ = L.run()
    assert torch.equal(_bits(out2), _bits(out)), "second launch differs"
    L.set_tails(True)
    out3, _ = L.run()
    assert torch.equal(_bits(out3), _bits(out)), "result depends on what lies behind the input tensors"
    # an image alone = the image in a batch of two
    Lb = Launch(ctx, EC.WINOF4_2SRC, cf, df, 0, EC.B_ALL)
    Lb.set_tails(False)
    both, _ = Lb.run()
    _check_borders(both, "out")
    for b in range(EC.B_ALL):
        L1 = Launch(ctx, EC.WINOF4_2SRC, cf, df, b, b + 1)
        L1.set_tails(False)
        one, _ = L1.run()
        assert torch.equal(_bits(one[0]), _bits(both[b])), f"image {b} alone differs from image {b} of the batch"
    assert torch.equal(_bits(both[:B]), _bits(out))


@pytest.mark.parametrize("i", range(len(EC.ENTRY_CASES)), ids=[c.name for _, c in EC.ENTRY_CASES])
def test_entry_impulse_responses(ctx, i):
    """One 1.0 per image at the region corners, on both sides of every tile and region boundary, in the first and last channel of the
    first, a middle and the last chunk of EITHER source (so on both sides of the source switch): the output is the flipped stencil."""
    c = EC.ENTRY_CASES[i][1]._replace(op="fwd")
    sites = CL.impulse_sites(c, 8)
    assert {("in0", c.C0 - 1), ("in1", 0)} <= {s[:2] for s in sites}
    d = CL.impulse_inputs(c, sites)
    ref, _ = _impulse_expected(c, d, sites, ())
    wmax = float(d["w"].abs().max())
    tol = EC.bar() * wmax
    worst = 0.0
    for lo in range(0, len(sites), 32):
        hi = min(len(sites), lo + 32)
        L = Launch(ctx, EC.WINOF4_2SRC, c, d, lo, hi, slope=CL.IMPULSE_SLOPE)
        L.set_tails(False)
        out, _ = L.run()
        _check_borders(out, "out")
        e = (CL.interior(out).double() - ref[lo:hi]).abs()
        assert bool(torch.isfinite(e).all())
        for k in range(lo, hi):
            worst = max(worst, float(e[k - lo].max()) / wmax)
            assert float(e[k - lo].max()) <= tol, (c.name, sites[k], float(e[k - lo].max()), tol)
    print(f"\nwinof4_entry impulse {c.name} worst |y - stencil| / max|w| {worst:.3e} bar {EC.bar():.3e}")


# odd H, odd W, a ragged second source, a ragged first source, too few first-source chunks (C0 = 0: an argument error of the probe
# itself), and the up-sampling kind, which has no instance
REFUSED = ((EC.WINOF4_2SRC, 64, 128, 64, 17, 32, PNPX_ERR_SHAPE), (EC.WINOF4_2SRC, 64, 128, 64, 16, 33, PNPX_ERR_SHAPE),
           (EC.WINOF4_2SRC, 64, 12, 64, 16, 32, PNPX_ERR_SHAPE), (EC.WINOF4_2SRC, 12, 64, 64, 16, 32, PNPX_ERR_SHAPE),
           (EC.WINOF4_2SRC, 0, 64, 64, 16, 32, PNPX_ERR_ARG), (EC.WINOF4_2SRC, 64, 128, 32, 16, 32, PNPX_ERR_SHAPE),
           (EC.WINOF4_UPS, 64, 128, 64, 32, 32, PNPX_ERR_SHAPE))


@pytest.mark.parametrize("geom", REFUSED, ids=[f"{g[0]}-{g[1]}+{g[2]}to{g[3]}_{g[4]}x{g[5]}" for g in REFUSED])
def test_refused_geometries_launch_nothing(ctx, geom):
    from tfpnp_amd import _lib
    kind, C0, C1, cout, H, W, status = geom
    c = CL.Case("refused", "ups" if kind == EC.WINOF4_UPS else "fwd", C0, C1, cout, H, W, False, False)
    assert CL.plan(kind, c) == (0, 0)
    hw1 = (H // 2, W // 2) if c.op == "ups" else (H, W)
    d = {"w": torch.zeros(cout, C0 + C1, 3, 3), "bias": torch.ones(cout), "in0": torch.ones(1, max(C0, 1), H, W), "in1": torch.ones((1, C1) + hw1)}
    L = Launch(ctx, kind, c, d, 0, 1)
    out, _ = L.run(expect=status)
    msg = _lib.lib().pnpx_last_error().decode()
    assert "unsupported geometry" in msg or "non-positive size" in msg, msg
    assert bool(torch.isnan(CL.interior(out)).all())       # nothing ran: the interior still holds its fill, the border is still zero
    _check_borders(out, "out")


# ------------------------------------------------------------------------------------------------------------ the whole network

def dev():
    return torch.device("cuda:0")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


OPTIONS = ("fp32_winof4_entries", "fp32_winof4_layers", "fp32_wino8_layers", "fp32_fuse_up", "fp32_ksplit")


@pytest.fixture(scope="module")
def den():
    from tfpnp_amd.pnp import UNetDenoiser2D
    d = UNetDenoiser2D(state_dict=_params(), conv_mode=0)
    c = d.context(dev())
    saved = {k: c.get_option(k) for k in OPTIONS}
    yield d
    for k, v in saved.items():
        c.set_option(k, v)


def _run(den, xt, st, **opts):
    """pre-clamp output under the given options; the others at all-F(2x2) entries, default elsewhere"""
    c = den.context(dev())
    base = {"fp32_winof4_entries": 0, "fp32_fuse_up": 1, "fp32_wino8_layers": ALL}
    base.update(opts)
    for k, v in base.items():
        c.set_option(k, v)
    out, pre = den.forward_preclamp(xt, st)
    assert torch.equal(out, pre.clamp(0.0, 1.0))
    return pre.clone()


# (B, H, W): the entries whose geometry the kernel takes -- 1 x 32 x 64: entry 21 (192 -> 64 at 16 x 32, one region); 3 x 64 x 128: entries
# 21 (32 x 64) and 18 (384 -> 128 at 16 x 32, two cout tiles), odd batch.  Under fp32_ksplit 1 the K-split claims all of them at these
# sizes (tests/test_winof4_entry_host.py), under 0 none.
SHAPES = {(1, 32, 64): (21,), (3, 64, 128): (21, 18)}


@pytest.mark.parametrize("B,H,W", list(SHAPES))
def test_each_entry_bit_alone(den, B, H, W):
    x, s, ref = _case(B, H, W)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    c = den.context(dev())
    c.set_option("fp32_ksplit", 0)
    f2 = _run(den, xt, st)
    f2_unfused = _run(den, xt, st, fp32_fuse_up=0)
    e0, eu = rel(f2.cpu(), ref), rel(f2_unfused, f2)
    assert e0 < 3e-6 and 0 < eu < 3e-6, (e0, eu)
    for li in (15, 18, 21):
        pre = _run(den, xt, st, fp32_winof4_entries=1 << li)
        if li not in SHAPES[(B, H, W)]:
            assert torch.equal(pre, f2), li                 # no geometry for the kernel at this size: today's launch
            continue
        assert not torch.equal(pre, f2), f"entry {li} did not reach the F(4x4) kernel"
        e4, e42, e4u = rel(pre.cpu(), ref), rel(pre, f2), rel(pre, f2_unfused)
        print(f"\n{B}x{H}x{W} entry {li}: F(4x4) vs fp64 {e4:.2e} (F(2x2) {e0:.2e}), vs F(2x2) fused {e42:.2e}, unfused {e4u:.2e}")
        assert e4 < 3e-6 and e42 < 3e-6 and e4u < 3e-6, (li, e4, e42, e4u)
        # (the kernel does not up-sample: that fp32_fuse_up leaves its row alone is tests/test_winof4_entry_host.py's check -- here the
        # option would move the other entries)
        assert torch.equal(_run(den, xt, st, fp32_winof4_entries=1 << li), pre)               # a second call
        # fp32_wino8_layers: the layer's bit cleared takes the entry off the kernel
        off = _run(den, xt, st, fp32_winof4_entries=1 << li, fp32_wino8_layers=ALL & ~(1 << li))
        assert torch.equal(off, _run(den, xt, st, fp32_wino8_layers=ALL & ~(1 << li)))
    # all bits but the entries' are ignored; fp32_wino8_layers = 0 switches every entry off
    assert torch.equal(_run(den, xt, st, fp32_winof4_entries=ALL & ~ENTRIES), f2)
    assert torch.equal(_run(den, xt, st, fp32_winof4_entries=ENTRIES, fp32_wino8_layers=0), _run(den, xt, st, fp32_wino8_layers=0))
    # a call of the K-split class keeps the 8-wave pieces
    c.set_option("fp32_ksplit", 1)
    assert torch.equal(_run(den, xt, st, fp32_winof4_entries=ENTRIES), _run(den, xt, st))
    # images of a batch = the images alone
    if B == 3:
        c.set_option("fp32_ksplit", 0)
        full = _run(den, xt, st, fp32_winof4_entries=ENTRIES)
        for k in range(B):
            one = _run(den, xt[k:k + 1].contiguous(), st[k:k + 1].contiguous(), fp32_winof4_entries=ENTRIES)
            assert torch.equal(one[0], full[k]), k
        c.set_option("fp32_ksplit", 1)


def test_the_32x32_level_entry_and_option_range(den):
    """1 x 128 x 256 without the K-split: level 3 is 16 x 32, the smallest size at which entry 15 (768 -> 256, four cout tiles, 96 chunks)
    has a geometry for the kernel.  Against the all-F(2x2) forward (no float64 oracle at this size: it would take minutes on the CPU)."""
    from tfpnp_amd._lib import PnpxError
    c = den.context(dev())
    for bad in (-1, 1 << 27):
        with pytest.raises(PnpxError):
            c.set_option("fp32_winof4_entries", bad)
    for v in (0, 1 << 18, ALL):
        c.set_option("fp32_winof4_entries", v)
        assert c.get_option("fp32_winof4_entries") == v
    x, s = denoiser_inputs(1, 128, 256, 41)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    c.set_option("fp32_ksplit", 0)
    f2 = _run(den, xt, st)
    pre = _run(den, xt, st, fp32_winof4_entries=1 << 15)
    c.set_option("fp32_ksplit", 1)
    assert not torch.equal(pre, f2) and rel(pre, f2) < 3e-6, rel(pre, f2)
