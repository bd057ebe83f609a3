"""GPU tests of the Winograd F(4x4,3x3) kernel (csrc/conv3x3_winof4.hip, option fp32_winof4_layers): the plain 64-cout layers of the
UNet's forward pass on v_mfma_f32_16x16x4_f32.  Everything goes through UNetDenoiser2D.forward_preclamp; the fp64 oracle forward of
a case is computed once and shared."""
import functools

import pytest
import torch

from tests.golden_inputs import denoiser_inputs
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

ALL = (1 << 27) - 1
# the layers the kernel can take (state_dict order): levels 1-3 of the encoder, the plain layers of the decoder at levels 3, 2, 1
PLAIN = [3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 19, 20, 22, 23]
F4_ALL = sum(1 << li for li in PLAIN)


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
    x, s = denoiser_inputs(B, H, W, 40 + B)
    p64 = {k: torch.as_tensor(v).double() for k, v in _params().items()}
    with torch.no_grad():
        sig = torch.from_numpy(s).double().view(B, 1, 1, 1).expand(B, 1, H, W)
        xin = torch.from_numpy(x).double()
        ref = O.unet_forward(torch.cat([xin, sig], 1), p64)
    return x, s, ref


@pytest.fixture(scope="module")
def den():
    from tfpnp_amd.pnp import UNetDenoiser2D
    d = UNetDenoiser2D(state_dict=_params(), conv_mode=0)
    ctx = d.context(dev())
    saved = {k: ctx.get_option(k) for k in ("fp32_winof4_layers", "fp32_wino8_layers", "fp32_chains", "fp32_ksplit")}
    yield d
    for k, v in saved.items():
        ctx.set_option(k, v)


def _run(den, xt, st, mask):
    den.context(dev()).set_option("fp32_winof4_layers", mask)
    out, pre = den.forward_preclamp(xt, st)
    return out.clone(), pre.clone()


# (B, H, W, fp32_ksplit): 1x32x64 -- level 1 is ONE 16 x 32 region, the smallest shape the kernel runs on (32 -> 64 channels = the fewest
# chunks; level 1's third layer has the fused pool); 2x64x64 -- two regions per image; 3x64x128 -- level 1 is 32 x 64 and level 2 one region
# with 128 couts (two cout tiles), odd batch.  At that size the K-split claims the 128 -> 128 layers of level 2 (and the kernel must
# leave them alone); with fp32_ksplit = 0 the decoder's plain layers of both levels run on the new kernel.
ELIGIBLE = [(1, 32, 64, 1), (2, 64, 64, 1), (3, 64, 128, 1), (3, 64, 128, 0)]


@pytest.mark.parametrize("B,H,W,ksplit", ELIGIBLE)
def test_winof4_matches_f2_and_oracle(den, B, H, W, ksplit):
    x, s, ref = _case(B, H, W)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    ctx = den.context(dev())
    ctx.set_option("fp32_ksplit", ksplit)
    ctx.set_option("fp32_chains", 2)
    out0, pre0 = _run(den, xt, st, 0)
    out4, pre4 = _run(den, xt, st, F4_ALL)
    assert ctx.get_option("fp32_winof4_layers") == F4_ALL
    assert not torch.equal(pre4, pre0), "the F(4x4) kernel did not run"
    e0, e4, e04 = rel(pre0.cpu(), ref), rel(pre4.cpu(), ref), rel(pre4, pre0)
    print(f"{B}x{H}x{W} ksplit={ksplit}: F(2x2) vs fp64 {e0:.2e}, F(4x4) vs fp64 {e4:.2e}, F(4x4) vs F(2x2) {e04:.2e}")
    assert e0 < 3e-6 and e4 < 3e-6 and e04 < 3e-6, (e0, e4, e04)
    assert torch.equal(out4, pre4.clamp(0.0, 1.0))
    # a second call is bit-identical
    out4b, pre4b = _run(den, xt, st, F4_ALL)
    assert torch.equal(pre4b, pre4) and torch.equal(out4b, out4)
    # an image of the batch equals the same image run alone, under every launch-chain setting
    if B == 3:
        for chains in (1, 2):
            ctx.set_option("fp32_chains", chains)
            _, full = _run(den, xt, st, F4_ALL)
            assert torch.equal(full, pre4), chains
            for i in range(B):
                _, one = _run(den, xt[i:i + 1].contiguous(), st[i:i + 1].contiguous(), F4_ALL)
                assert torch.equal(one[0], full[i]), (chains, i)
        ctx.set_option("fp32_chains", 2)


def test_every_layer_bit_reaches_the_kernel(den):
    """3 x 64 x 128 without the K-split: each plain layer of levels 1 and 2 alone changes the result (so the launch, its fused pool -- layers
    5 and 8 feed the next level only through it at their bit -- and both cout tiles of the 128-cout layers ran) and stays within the bar."""
    x, s, ref = _case(3, 64, 128)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    ctx = den.context(dev())
    ctx.set_option("fp32_ksplit", 0)
    _, pre0 = _run(den, xt, st, 0)
    for li in (3, 4, 5, 6, 7, 8, 19, 20, 22, 23):
        _, pre = _run(den, xt, st, 1 << li)
        assert not torch.equal(pre, pre0), li
        assert rel(pre.cpu(), ref) < 3e-6 and rel(pre, pre0) < 3e-6, (li, rel(pre.cpu(), ref), rel(pre, pre0))
    # layers outside the kernel's set are ignored: the 32-cout layers, the decoder entries, the 16 x 16 level (8 x 16 here)
    _, pre = _run(den, xt, st, ALL & ~F4_ALL)
    assert torch.equal(pre, pre0)
    ctx.set_option("fp32_ksplit", 1)


def test_no_eligible_level_is_bit_identical(den):
    x, s, _ = _case(1, 128, 96)        # W / 2 = 48, W / 4 = 24, ...: no level has W % 32 == 0 among the 64-cout layers
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    _, pre0 = _run(den, xt, st, 0)
    _, pre4 = _run(den, xt, st, F4_ALL)
    assert torch.equal(pre4, pre0)


def test_option_range_and_dependence_on_wino8_mask(den):
    from tfpnp_amd._lib import PnpxError
    ctx = den.context(dev())
    for bad in (-1, 1 << 27):
        with pytest.raises(PnpxError):
            ctx.set_option("fp32_winof4_layers", bad)
    for v in (0, 1 << 4, ALL):
        ctx.set_option("fp32_winof4_layers", v)
        assert ctx.get_option("fp32_winof4_layers") == v
    assert ctx.get_option("fp32_wino8_layers") == ALL      # untouched default
    x, s, _ = _case(2, 64, 64)
    xt, st = torch.from_numpy(x).to(dev()), torch.from_numpy(s).to(dev())
    # fp32_wino8_layers = 0 (the 4-wave kernel everywhere) switches the new kernel off whatever its own mask says
    ctx.set_option("fp32_wino8_layers", 0)
    _, w4 = _run(den, xt, st, 0)
    _, w4_f4 = _run(den, xt, st, ALL)
    ctx.set_option("fp32_wino8_layers", ALL)
    _, w8 = _run(den, xt, st, 0)
    assert torch.equal(w4_f4, w4) and not torch.equal(w8, w4)
    # one wino8 bit cleared takes that layer alone off the new kernel
    ctx.set_option("fp32_wino8_layers", ALL & ~(1 << 4))
    _, a = _run(den, xt, st, 1 << 4)
    _, b = _run(den, xt, st, 0)
    ctx.set_option("fp32_wino8_layers", ALL)
    assert torch.equal(a, b)
    # fp32_winograd = 0: the direct kernel everywhere
    ctx.set_option("fp32_winograd", 0)
    _, d0 = _run(den, xt, st, 0)
    _, d4 = _run(den, xt, st, ALL)
    ctx.set_option("fp32_winograd", 1)
    assert torch.equal(d0, d4)
