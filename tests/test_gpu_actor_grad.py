"""GPU tests of the actor's parameter gradients through batch-statistics BatchNorm (csrc/policy_grad.hip, pnpx_policy_param_grad)
against autograd through the float64 torch stand-in in `.train()` mode on the CPU (tests/actor_grad_cases.py).  Bounds: the project's
critic-gradient contract on kink-free input, relative L2 <= 1e-3 per tensor and <= 1e-4 on the whole vector; the fp32 stand-in itself
sits at <= 7.0e-6 / 3.4e-6 on these cases, so the bounds leave 30 - 140 x over the reference arithmetic's own error.

Measured on an MI355X (worst tensor / whole vector): c9_4x64x64 5.0e-6 / 2.8e-6, c7_3x32x96 7.8e-6 / 5.0e-6, c17_2x64x64 8.4e-6 /
3.7e-6, spi6_5x64x32 7.5e-6 / 4.8e-6 (profiles/actor_grad.md)."""
import numpy as np
import pytest
import torch

from tests import actor_cases as A
from tests import actor_grad_cases as G
from tests import actor_train_cases as T
from tfpnp_amd import _lib
from tfpnp_amd._lib import PnpxError

pytestmark = pytest.mark.gpu
PNPX_ERR_ARG, PNPX_ERR_NO_WEIGHTS = 1, 3
CASE_PARAMS = [pytest.param(c, s, id=i) for (c, s), i in zip(G.CASES, G.IDS)]
CASE0, SHAPE0 = G.CASES[0]
CASE1, SHAPE1 = G.CASES[1]


def dev():
    return torch.device("cuda:0")


def g(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev())


def fresh(case, **kw):
    from tfpnp_amd import policy
    name, num_aux = A._ACTORS[tuple(case)]
    return getattr(policy, name)(num_aux, 5, state_dict=T.params(case), **kw)


def inputs(case, shape):
    gp, gd = G.upstream(case, shape)
    return g(T.observation(case, shape)), g(gp), g(gd)


def check_parity(flat, ref, case, label):
    worst, key, vec = G.errors(flat, ref["grad"], case)
    w32, _, v32 = G.errors(ref["fp32"], ref["grad"], case)
    print(f"{label}: worst tensor {worst:.2e} ({key})  whole vector {vec:.2e}   (fp32 stand-in {w32:.2e} / {v32:.2e})")
    assert worst <= G.TENSOR_BOUND and vec <= G.VECTOR_BOUND
    stats = flat.cpu()[T.stat_mask(case)]
    assert stats.numel() == 2 * T.N_BN and bool((stats == 0).all())


@pytest.mark.parametrize("case,shape", CASE_PARAMS)
def test_parity_with_float64_autograd(case, shape):
    from tfpnp_amd import ops
    ob, gp, gd = inputs(case, shape)
    flat = ops.policy_param_grad(fresh(case).context(dev()), ob, gp, gd)
    assert flat.dtype == torch.float32 and flat.shape == (A.flat_vector(T.params(case), case).numel(),)
    check_parity(flat, G.reference(case, shape), case, f"{case} {shape}")


def test_nothing_moves():
    from tfpnp_amd import ops
    ob, gp, gd = inputs(CASE0, SHAPE0)
    ctx = fresh(CASE0).context(dev())
    before = ctx.policy_params().clone()
    p0, d0 = ops.policy_forward_train(ctx, ob, update_running=False)
    m0, v0 = (t.clone() for t in ops.policy_bn_stats(ctx))
    other = g(T.observation(CASE0, SHAPE0, "offset"))
    ops.policy_forward_train(ctx, other, update_running=False)       # other statistics in the buffer
    ops.policy_param_grad(ctx, ob, gp, gd)
    m1, v1 = ops.policy_bn_stats(ctx)
    assert torch.equal(m0, m1) and torch.equal(v0, v1)               # those of a train forward on ob, bit for bit
    p1, d1 = ops.policy_forward_train(ctx, ob, update_running=False)
    assert torch.equal(p0, p1) and torch.equal(d0, d1)
    assert torch.equal(before, ctx.policy_params())
    pe, de = ops.policy_forward(ctx, ob)                             # the eval packing is not staled either
    pf, df = ops.policy_forward(fresh(CASE0).context(dev()), ob)
    assert torch.equal(pe, pf) and torch.equal(de, df)


def test_repeatable_and_launch_independent():
    from tfpnp_amd import ops
    ob, gp, gd = inputs(CASE0, SHAPE0)
    ctx = fresh(CASE0).context(dev())
    first = ops.policy_param_grad(ctx, ob, gp, gd)
    assert torch.equal(first, ops.policy_param_grad(ctx, ob, gp, gd))
    big = torch.rand(SHAPE0[0] + 3, CASE0[0], SHAPE0[1], SHAPE0[2], device=dev())      # grows the workspace
    ops.policy_param_grad(ctx, big, torch.randn(big.shape[0], 2, device=dev()), torch.randn(big.shape[0], CASE0[1], device=dev()))
    assert torch.equal(first, ops.policy_param_grad(ctx, ob, gp, gd))
    for s2_hs in (0, 1):                                             # the gradient path ignores the option
        ctx.set_option("policy_s2_hs", s2_hs)
        assert torch.equal(first, ops.policy_param_grad(ctx, ob, gp, gd))
    assert torch.equal(first, ops.policy_param_grad(fresh(CASE0).context(dev()), ob, gp, gd))   # another context


@pytest.mark.parametrize("case,shape", [CASE_PARAMS[1], CASE_PARAMS[3]])
def test_power_of_two_homogeneity(case, shape):
    from tfpnp_amd import ops
    ob, gp, gd = inputs(case, shape)
    ctx = fresh(case).context(dev())
    base = ops.policy_param_grad(ctx, ob, gp, gd)
    assert float(base.abs().max()) > 0
    for f in (2.0, 2.0 ** -20, 2.0 ** 8):
        assert torch.equal(ops.policy_param_grad(ctx, ob, gp * f, gd * f), base * f), f
    zero = ops.policy_param_grad(ctx, ob, gp * 0, gd * 0)
    assert bool(torch.isfinite(zero).all()) and bool((zero == 0).all())


def test_linear_over_the_two_heads():
    from tfpnp_amd import ops
    ob, gp, gd = inputs(CASE0, SHAPE0)
    ctx = fresh(CASE0).context(dev())
    both = ops.policy_param_grad(ctx, ob, gp, gd).double()
    parts = ops.policy_param_grad(ctx, ob, gp, gd * 0).double() + ops.policy_param_grad(ctx, ob, gp * 0, gd).double()
    e = float((parts - both).norm() / both.norm())
    print(f"additivity: {e:.2e}")
    assert e <= 1e-5


def test_fresh_weights_after_load_flat():
    """The adjoint packing is derived again after a reload: the gradient is that of the new weights."""
    from tfpnp_amd import ops, synth
    ob, gp, gd = inputs(CASE1, SHAPE1)
    actor = fresh(CASE1)
    old = ops.policy_param_grad(actor.context(dev()), ob, gp, gd)
    params = synth.make_policy_params(*CASE1, seed=T.WEIGHT_SEED + 1)
    actor.load_flat_(g(A.flat_vector(params, CASE1)))
    new = ops.policy_param_grad(actor.context(dev()), ob, gp, gd)
    assert not torch.equal(old, new)
    ref64, _ = G.autograd_flat(G.stand_in(CASE1, params), torch.from_numpy(T.observation(CASE1, SHAPE1)).double(), gp.cpu().double(),
                               gd.cpu().double())
    ref32, _ = G.autograd_flat(G.stand_in(CASE1, params, torch.float32), torch.from_numpy(T.observation(CASE1, SHAPE1)), gp.cpu(), gd.cpu())
    check_parity(new, {"grad": ref64, "fp32": ref32.double()}, CASE1, "reloaded")


def test_surface():
    from tfpnp_amd import ops, torch_ops
    ob, gp, gd = inputs(CASE1, SHAPE1)
    actor = fresh(CASE1)
    ctx = actor.context(dev())
    a = ops.policy_param_grad(ctx, ob, gp, gd)
    assert "policy_param_grad" in torch_ops.ALL_OPS
    assert torch.equal(a, torch.ops.pnpx.policy_param_grad(ob, gp, gd, ctx.cid))
    assert torch.equal(a, actor.param_grad(ob, gp, gd))
    pr, dr = actor.forward_train_raw(ob)
    pt, dt = ops.policy_forward_train(ctx, ob, update_running=False)
    assert torch.equal(pr, pt) and torch.equal(dr, dt)
    torch.library.opcheck(torch.ops.pnpx.policy_param_grad, (ob, gp, gd, ctx.cid))     # the fake formula: shape, dtype, device
    assert not actor.param_grad(ob.clone().requires_grad_(True), gp, gd).requires_grad


def test_error_returns():
    from tfpnp_amd import ops
    ob, gp, gd = inputs(CASE1, SHAPE1)
    ctx = fresh(CASE1).context(dev())
    n = a_n = ops.policy_flat_size(ctx)
    out = torch.empty(n, device=dev())
    B, H, W = SHAPE1
    call = lambda c, o, nn, b=B, h=H, w=W: _lib.lib().pnpx_policy_param_grad(c.handle, ops._p(ob), ops._p(gp), ops._p(gd), o, nn, b, h, w,
                                                                         ops._stream(ob))
    assert call(ctx, ops._p(out), n - 1) == PNPX_ERR_ARG             # wrong n_params
    assert call(ctx, None, n) == PNPX_ERR_ARG                        # null pointer
    assert call(ctx, ops._p(out), n, 1, 32, 32) == PNPX_ERR_ARG      # B * (H/32) * (W/32) < 2
    empty = ops.Context(dev())
    assert call(empty, ops._p(out), a_n) == PNPX_ERR_NO_WEIGHTS
    with pytest.raises(PnpxError):
        ops.policy_param_grad(empty, ob, gp, gd)
    with pytest.raises(PnpxError):
        ops.policy_param_grad(ctx, ob, gp[:, :1], gd)


def test_one_optimiser_step_end_to_end():
    """The flat parameter takes the native gradient, torch.optim.SGD steps it, load_flat_ takes the result: the toy loss of the float64
    stand-in stepped with its own gradient against the loss of the stand-in loaded from the native actor's state_dict()."""
    case, shape, lr = CASE1, SHAPE1, 1e-3
    ob, gp, gd = inputs(case, shape)
    ob64, gp64, gd64 = (t.cpu().double() for t in (ob, gp, gd))
    actor = fresh(case)
    flat = torch.nn.Parameter(actor.parameters_flat(dev()).clone())
    opt = torch.optim.SGD([flat], lr=lr)
    flat.grad = actor.param_grad(ob, gp, gd)
    opt.step()
    actor.load_flat_(flat.detach())

    def loss_of(module):
        module.train()
        with torch.no_grad():
            p, d = module(ob64)
        return float((gp64 * p).sum() + (gd64 * d).sum())

    ref = G.stand_in(case)
    grad64, loss0 = G.autograd_flat(ref, ob64, gp64, gd64)
    with torch.no_grad():
        named = dict(ref.named_parameters())
        for key, pos, cnt in G.tensors(case):
            named[key] -= lr * grad64[pos:pos + cnt].reshape(named[key].shape)
    want = loss_of(ref)
    native = A.stand_in_actor(*case).double()
    native.load_state_dict({k: v.cpu().double() for k, v in actor.state_dict().items()}, strict=False)
    got = loss_of(native)
    print(f"toy loss {loss0:.6f} -> stepped float64 {want:.6f}, native {got:.6f}")
    assert abs(want - loss0) > 1e-3 * abs(loss0)                     # the step matters
    assert abs(got - want) <= 1e-4 * abs(want)
