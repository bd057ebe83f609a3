"""Call sequences on ONE DRUNet context (csrc/drunet_net.h: dru_arena_reserve serves the four arenas -- activations and gradients
of the half-split and of the fp32 family -- under two keep-plane policies).  The other DRUNet tests make one or two calls per
context; here inference and VJP calls of changing batch and shape follow each other, every result is compared bit for bit with
the same single call on a fresh context, and Context.bytes() is watched: arenas only grow, and a call that fits re-lays nothing or
re-lays inside the allocation it has, so the total never falls and repeating a call leaves it where it is."""
import numpy as np
import pytest
import torch

from tests.golden_inputs import denoiser_inputs
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

H, W = 16, 24      # H != W: a transposed dimension shows; 2 x 3 at level 3; B <= 3 keeps the automatic launch chains at one


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.fixture(scope="module")
def params():
    return synth.make_drunet_params(0)


def denoiser(params, conv_mode):
    from tfpnp_amd.pnp import DRUNetDenoiser2D
    return DRUNetDenoiser2D(state_dict=params, conv_mode=conv_mode)


def infer(den, x, s):
    with torch.no_grad():
        return (den(x, s).clone(),)


def vjp(den, x, s, g):
    lx, ls = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
    out = den(lx, ls)
    (out * g).sum().backward()
    return out.detach().clone(), lx.grad.clone(), ls.grad.clone()


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("conv_mode", [1, 0])
def test_drunet_call_sequence_on_one_context(params, conv_mode):
    x3, s3 = map(t, denoiser_inputs(3, H, W, 2101))
    x2, s2 = map(t, denoiser_inputs(2, H, W, 2102))
    xt, st = map(t, denoiser_inputs(2, W, H, 2103))
    g2 = t(np.random.RandomState(2104).standard_normal((2, 1, H, W)).astype(np.float32))
    steps = [(infer, x3, s3),                       # 1
             (vjp, x2, s2, g2),                     # 2
             (infer, x3[:1], s3[:1]),               # 3: the first image of step 1
             (infer, x3, s3),                       # 4 = 1
             (infer, xt, st),                       # 5: 24 x 16
             (vjp, x2, s2, g2),                     # 6 = 2
             (vjp, x2[:1], s2[:1], g2[:1])]         # 7: the first image of step 2
    den = denoiser(params, conv_mode)
    ctx = den.context(dev())
    got, total = [], [ctx.bytes()]
    for i, (call, *args) in enumerate(steps):
        got.append(call(den, *args))
        torch.cuda.synchronize()
        total.append(ctx.bytes())
        assert total[-1] >= total[-2], (i + 1, total)
        again = call(den, *args)
        assert ctx.bytes() == total[-1], (i + 1, total, ctx.bytes())
        assert same(again, got[-1]), i + 1
    print(f"conv_mode {conv_mode}: Context.bytes() after load and after each step: {total}")
    ctx.status()
    assert same(got[3], got[0]) and same(got[5], got[1])
    assert torch.equal(got[2][0], got[0][0][:1])
    for i in (0, 1, 2, 4, 6):        # steps 4 and 6 repeat 1 and 2
        call, *args = steps[i]
        fresh = denoiser(params, conv_mode)
        want = call(fresh, *args)
        torch.cuda.synchronize()
        assert same(got[i], want), i + 1
        fresh.context(dev()).close()


def test_drunet_small_batch_slices_are_bit_identical(params):
    """B = 5 at 16 x 24 in one, two and three launch chains: the slice offsets of the shared walk at a shape where a level is 2 x 3."""
    den = denoiser(params, 1)
    ctx = den.context(dev())
    x, s = map(t, denoiser_inputs(5, H, W, 2105))
    try:
        ctx.set_option("chains", 1)
        ref = infer(den, x, s)
        for c in (2, 3):
            ctx.set_option("chains", c)
            assert same(infer(den, x, s), ref), c
    finally:
        ctx.set_option("chains", 0)
    ctx.status()
