"""GPU tests of the F(4x4,3x3) kernel's up-sampling instance (csrc/conv3x3_winof4.hip, option fp32_winof4_fuse_up, probe kind
PNPX_PROBE_WINOF4_FUSE_UP): it must write, bit for bit, what the separate up-sampling kernel followed by the two-source instance writes.
Per layer through the probes (the up-sampled tensor is the library's own, from pnpx_upsample2x_probe) and against the float64 reference
under the recorded f4_entry bar (profiles/winof4_entries.md); through the whole network with the option's bits on and off.

Figures of the first run on an MI355X: profiles/winof4_fuse_up.md."""
import ctypes as C

import pytest
import torch

from tests import conv_layer_cases as CL
from tests import winof4_entry_cases as EC
from tests import winof4_fuse_up_cases as FU
from tests.golden_inputs import denoiser_inputs
from tests.test_gpu_conv_layers import PNPX_ERR_SHAPE, Launch, Slab, _check_borders
from tests.test_gpu_winof4 import _params

pytestmark = pytest.mark.gpu

ENTRIES = (1 << 15) | (1 << 18) | (1 << 21)
ALL = (1 << 27) - 1
IDS = [c.name + f"_{c.H}x{c.W}" for _, c in FU.CASES]


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


def _bits(t):
    return t.view(torch.int32)


def _library_upsampled(ctx, L):
    """The low-resolution second source of Launch L through the library's separate up-sampling launch -> [B][C1][H][W] on the CPU."""
    from tfpnp_amd import _lib
    src = L.ins["in1"]
    B, C1, hp, wp = src.t.shape
    h, w = hp - 2, wp - 2 * CL.PADL
    dst = Slab((B, C1, 2 * h + 2, 2 * w + 2 * CL.PADL), nan_interior=True)
    st = _lib.lib().pnpx_upsample2x_probe(L.ctx.handle, C.c_void_p(src.ptr()), C.c_void_p(dst.ptr()), B * C1, h, w,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, _lib.lib().pnpx_last_error().decode()
    assert dst.guards_intact()
    up = dst.t.cpu()
    _check_borders(up, "up-sampled")
    assert bool(torch.isfinite(up).all())
    return CL.interior(up).contiguous()


def _both_forms(ctx, c, d, lo, hi, slope=CL.SLOPE, tails=False):
    """(fused launch on the low-resolution in1, two-source launch on the library's up-sampled in1), padded outputs on the CPU."""
    Lf = Launch(ctx, FU.FUSE_UP, c, d, lo, hi, slope=slope)
    Lf.set_tails(tails)
    fused, _ = Lf.run()
    _check_borders(fused, "out")                                      # (Launch.run checks the guard bands around the output)
    up = torch.zeros((d["in1"].shape[0],) + (c.C1, c.H, c.W))
    up[lo:hi] = _library_upsampled(ctx, Lf)
    L2 = Launch(ctx, EC.WINOF4_2SRC, c._replace(op="fwd"), dict(d, in1=up), lo, hi, slope=slope)
    L2.set_tails(False)
    two, _ = L2.run()
    return Lf, fused, two


@pytest.mark.parametrize("i", range(len(FU.CASES)), ids=IDS)
def test_fused_layer_is_the_two_launch_form_bit_for_bit(ctx, i):
    B, c = FU.CASES[i]
    assert CL.plan(FU.FUSE_UP, c) == (64, 1)
    d = FU.inputs(i)
    ref, den = FU.case_reference(i)
    Lf, fused, two = _both_forms(ctx, c, d, 0, B)
    err = CL.measure(CL.interior(fused), ref[:B], den[:B])
    print(f"\nwinof4_fuse_up {c.name} {c.H}x{c.W} B={B} measure {err:.4e} bar {EC.bar():.4e}")
    assert err <= EC.bar(), (c.name, err, EC.bar())
    assert torch.equal(_bits(fused), _bits(two)), f"{int((_bits(fused) != _bits(two)).sum())} elements differ from the two-launch form"
    # a second launch, and one with large finite garbage behind every input
    again, _ = Lf.run()
    assert torch.equal(_bits(again), _bits(fused)), "second launch differs"
    Lf.set_tails(True)
    tails, _ = Lf.run()
    assert torch.equal(_bits(tails), _bits(fused)), "result depends on what lies behind the input tensors"
    # an image alone = the image in a batch of two
    Lb = Launch(ctx, FU.FUSE_UP, c, d, 0, EC.B_ALL)
    Lb.set_tails(False)
    both, _ = Lb.run()
    _check_borders(both, "out")
    for b in range(EC.B_ALL):
        L1 = Launch(ctx, FU.FUSE_UP, c, d, b, b + 1)
        L1.set_tails(False)
        one, _ = L1.run()
        assert torch.equal(_bits(one[0]), _bits(both[b])), f"image {b} alone differs from image {b} of the batch"
    assert torch.equal(_bits(both[:B]), _bits(fused))


@pytest.mark.parametrize("i", range(len(FU.CASES)), ids=IDS)
def test_low_resolution_impulses(ctx, i):
    """One 1.0 per image in the LOW-resolution source: at the first and last source pixel every region's halo taps (the corners of its
    staging window's used part) and at the image's last row and column, in the first and last channel of the second source's first and
    last chunk.  Both forms must give the same bits, and the response must peak where the up-sampled impulse lies."""
    c = FU.CASES[i][1]
    ys, xs = FU.window_corners(c.H, c.W)
    chans = sorted({0, 7, c.C1 - 8, c.C1 - 1})
    sites = [("in1", chans[k % len(chans)], y, x) for k, (y, x) in enumerate((y, x) for y in ys for x in xs)]
    sites += [("in1", ch, c.H // 2 - 1, c.W // 2 - 1) for ch in chans]
    d = CL.impulse_inputs(c, sites)
    d["bias"] = torch.zeros(c.cout)
    for lo in range(0, len(sites), 32):
        hi = min(len(sites), lo + 32)
        _, fused, two = _both_forms(ctx, c, d, lo, hi, slope=CL.IMPULSE_SLOPE)
        assert torch.equal(_bits(fused), _bits(two)), [sites[lo + int(k)] for k in (_bits(fused) != _bits(two)).flatten(1).any(1).nonzero()]
        f = CL.interior(fused)
        assert bool(torch.isfinite(f).all())
        for k in range(lo, hi):      # the impulse arrived: the largest response lies within its up-sampled footprint
            _, _, y, x = sites[k]
            m = f[k - lo].abs().amax(0)
            py, px = divmod(int(m.argmax()), c.W)
            assert float(m.max()) > 0 and abs(py - 2 * y) <= 3 and abs(px - 2 * x) <= 3, (sites[k], py, px)


# too few first-source chunks (one below the minimum), odd targets, ragged sources, a 32-cout tile, no second source; kind 9 stays reserved
REFUSED = ((FU.FUSE_UP, 8, 16, 64, 16, 32), (FU.FUSE_UP, 64, 128, 64, 17, 32), (FU.FUSE_UP, 64, 128, 64, 16, 34), (FU.FUSE_UP, 64, 12, 64, 16, 32),
           (FU.FUSE_UP, 12, 64, 64, 16, 32), (FU.FUSE_UP, 64, 128, 32, 16, 32), (FU.FUSE_UP, 64, 0, 64, 16, 32), (EC.WINOF4_UPS, 64, 128, 64, 32, 32))


@pytest.mark.parametrize("geom", REFUSED, ids=[f"{g[0]}-{g[1]}+{g[2]}to{g[3]}_{g[4]}x{g[5]}" for g in REFUSED])
def test_refused_geometries_launch_nothing(ctx, geom):
    from tfpnp_amd import _lib
    kind, C0, C1, cout, H, W = geom
    c = CL.Case("refused", "ups", C0, C1, cout, H, W, False, False)
    assert CL.plan(kind, c) == (0, 0)
    d = {"w": torch.zeros(cout, C0 + C1, 3, 3), "bias": torch.ones(cout), "in0": torch.ones(1, C0, H, W)}
    if C1:
        d["in1"] = torch.ones(1, C1, H // 2, W // 2)
    L = Launch(ctx, kind, c, d, 0, 1)
    out, _ = L.run(expect=PNPX_ERR_SHAPE)
    assert "unsupported geometry" in _lib.lib().pnpx_last_error().decode()
    assert bool(torch.isnan(CL.interior(out)).all())       # nothing ran: the interior still holds its fill, the border is still zero
    _check_borders(out, "out")


# ------------------------------------------------------------------------------------------------------------ the whole network

def dev():
    return torch.device("cuda:0")


OPTIONS = ("fp32_winof4_fuse_up", "fp32_winof4_entries", "fp32_ksplit", "fuse_outc")


@pytest.fixture(scope="module")
def den():
    from tfpnp_amd.pnp import UNetDenoiser2D
    d = UNetDenoiser2D(state_dict=_params(), conv_mode=0)
    c = d.context(dev())
    saved = {k: c.get_option(k) for k in OPTIONS}
    yield d
    for k, v in saved.items():
        c.set_option(k, v)


def _run(den, xt, st, mask, ksplit=0):
    """pre-clamp output with every entry on the F(4x4) kernel and the given fp32_winof4_fuse_up mask"""
    c = den.context(dev())
    for k, v in (("fp32_winof4_entries", ENTRIES), ("fp32_winof4_fuse_up", mask), ("fp32_ksplit", ksplit)):
        c.set_option(k, v)
    out, pre = den.forward_preclamp(xt, st)
    assert torch.equal(out, pre.clamp(0.0, 1.0))
    return pre.clone()


# (B, H, W): 1 x 32 x 64 reaches entry 21 (192 -> 64 at 16 x 32), 3 x 64 x 128 entries 21 (32 x 64) and 18 (384 -> 128 at 16 x 32),
# 1 x 128 x 256 also entry 15 (768 -> 256 at 16 x 32: four cout tiles, 96 chunks), all with fp32_ksplit 0 (tests/test_winof4_fuse_up_host.py
# checks these rows of the selector)
@pytest.mark.parametrize("B,H,W", [(1, 32, 64), (3, 64, 128), (1, 128, 256)])
def test_forward_is_bit_identical_with_the_mask_on_and_off(den, B, H, W):
    from tfpnp_amd._lib import PnpxError
    x, s = denoiser_inputs(B, H, W, 43)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    c = den.context(dev())
    off = _run(den, xt, st, 0)
    assert bool(torch.isfinite(off).all())
    for mask in (1 << 15, 1 << 18, 1 << 21, ENTRIES, ALL):
        assert torch.equal(_bits(_run(den, xt, st, mask)), _bits(off)), hex(mask)
    assert torch.equal(_bits(_run(den, xt, st, ENTRIES)), _bits(off))                        # a second call
    # a call of the K-split class keeps the 8-wave pieces: the option changes nothing there
    assert torch.equal(_bits(_run(den, xt, st, ENTRIES, ksplit=1)), _bits(_run(den, xt, st, 0, ksplit=1)))
    if B == 3:      # images of a batch = the images alone
        full = _run(den, xt, st, ENTRIES)
        for k in range(B):
            one = _run(den, xt[k:k + 1].contiguous(), st[k:k + 1].contiguous(), ENTRIES)
            assert torch.equal(_bits(one[0]), _bits(full[k])), k
        # a training forward (the activations kept for the VJP) = the inference forward, and the VJP does not miss the up-sampled tensor.
        # (fuse_outc 0: an inference forward then ends in the launches a training forward ends in; its fused out-conv adds the 32
        # channels in another order, which is no business of this option.)
        c.set_option("fuse_outc", 0)
        grads, outs = [], []
        for mask in (ENTRIES, 0):
            c.set_option("fp32_winof4_fuse_up", mask)
            with torch.no_grad():
                inf = den(xt, st).clone()
            xg = xt.clone().requires_grad_(True)
            out = den(xg, st)
            assert torch.equal(_bits(out.detach()), _bits(inf)), (hex(mask), float((out.detach() - inf).abs().max()))
            out.square().sum().backward()
            grads.append(xg.grad.clone())
            outs.append(inf)
        c.set_option("fuse_outc", 1)
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(grads[0]), _bits(grads[1]))
    if (B, H, W) == (1, 32, 64):
        for bad in (-1, 1 << 27):
            with pytest.raises(PnpxError):
                c.set_option("fp32_winof4_fuse_up", bad)
        for v in (0, 1 << 18, ALL):
            c.set_option("fp32_winof4_fuse_up", v)
            assert c.get_option("fp32_winof4_fuse_up") == v
