"""GPU tests of the critic's parameter gradients (csrc/critic_grad.hip, pnpx_critic_param_grad) -- value_loss.backward() of
tfpnp/trainer/mddpg/trainer.py:198,207 -- against the fp64 leaf restatement of tests/critic_grad_cases.py and the executed
reference's autograd (tests/golden/critic_param_grad.npz).  Every one of the 82 tensors is compared, per tensor:
||got - ref|| / max(||ref||, 1e-6 * largest tensor norm).

Bounds: kink-free cases 1e-3 and arbitrary inputs 2e-2 per tensor, the project's bounds for this chain's input gradient
(test_gpu_critic.py); the K-split case additionally 1e-4 on the whole vector.
"""

import numpy as np
import pytest
import torch

from tests import critic_cases as K
from tests import critic_grad_cases as G
from tests.conftest import golden

pytestmark = pytest.mark.gpu

BOUNDS = {"kf9": 1e-3, "kf17": 1e-3, "arb": 2e-2, "rect": 2e-2}


def dev():
    return torch.device("cuda:0")


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.fixture(scope="module")
def critics():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    made = {}

    def get(num_inputs):
        if num_inputs not in made:
            made[num_inputs] = ResNet_wobn(num_inputs, 18, 1, state_dict=K.critic_params(num_inputs))
        return made[num_inputs]
    return get


@pytest.fixture(scope="module")
def refs():
    """fp64 leaf-restatement gradients per golden case, computed once (CPU)"""
    made = {}
    value = golden("critic_value")

    def get(name):
        if name not in made:
            ob, w = K.case_inputs(name, value[f"{name}_try"])
            made[name] = (ob, w, G.leaf_grads(K.critic_params(K.CASES[name][0]), ob, w, torch.float64)[1])
        return made[name]
    return get


def check_per_tensor(tag, got, ref, bound):
    rel = G.per_tensor_rel(got, ref)
    k, e = G.worst(rel)
    print(f"{tag}: worst tensor {k} {e:.2e} (bound {bound:g}); median {np.median(list(rel.values())):.2e}")
    assert len(rel) == 82
    bad = {q: v for q, v in rel.items() if not v <= bound}
    assert not bad, bad


@pytest.mark.parametrize("name", G.GOLDEN_CASES)
def test_param_grad_vs_restatement_and_reference(critics, refs, name):
    C = K.CASES[name][0]
    ob, w, ref = refs(name)
    flat = critics(C).param_grad(g(ob), g(w))
    assert flat.shape == (sum(int(np.prod(s)) for _, s in K.synth.critic_param_specs(C)),) and flat.dtype == torch.float32
    got = G.split_flat(flat.cpu().numpy(), C)
    check_per_tensor(f"{name} vs fp64 restatement", got, ref, BOUNDS[name])
    print(f"{name}: whole vector {G.whole_rel(got, ref, C):.2e}")
    # the executed reference's autograd: the stored sample of every tensor
    gd = golden("critic_param_grad")
    keys = [k for k, _ in K.synth.critic_param_specs(C)]
    samp_got, samp_ref, pos = {}, {}, 0
    for k in keys:
        idx = G.sample_index(got[k].size)
        samp_got[k] = got[k].reshape(-1)[idx]
        samp_ref[k] = gd[f"{name}_sample"][pos:pos + idx.size]
        pos += idx.size
    assert pos == gd[f"{name}_sample"].size
    check_per_tensor(f"{name} vs reference samples", samp_got, samp_ref, BOUNDS[name])


def test_k_split_case(critics):
    """6 x 9 x 128 x 128: the stage-1 layers (64 x 576 outputs over 6144 pixels = 192 chunks, 4 tiles) run 64 pieces, stage 2
    32, stage 3 eight (critic_wgrad_pieces).  Per tensor 2e-2, whole vector 1e-4 against the fp64 restatement."""
    ob = K.big_inputs(6, 9, 128, 128)
    w = np.array([1.0, -2.0, 0.5, 3.0, 1.5, -1.0], np.float32)
    ref = G.leaf_grads(K.critic_params(9), ob, w, torch.float64)[1]
    got = G.split_flat(critics(9).param_grad(g(ob), g(w)).cpu().numpy(), 9)
    check_per_tensor("6x9x128x128 vs fp64 restatement", got, ref, 2e-2)
    whole = G.whole_rel(got, ref, 9)
    print(f"6x9x128x128: whole vector {whole:.2e} (bound 1e-4)")
    assert whole <= 1e-4
    torch.cuda.synchronize()
    assert not critics(9).context(dev()).range_tripped()


def test_deterministic_linear_and_zero(critics, refs):
    net = critics(9)
    ob, w, _ = refs("rect")
    x, gv = g(ob), g(w)
    a = net.param_grad(x, gv)
    net.param_grad(g(refs("arb")[0]), g(refs("arb")[1]))        # another size in between: the workspace is re-used
    assert torch.equal(net.param_grad(x, gv), a)
    assert torch.equal(net.param_grad(x, gv.view(-1, 1)), a)    # [B, 1] as well as [B]
    assert torch.equal(net.param_grad(x, 2 * gv), 2 * a)
    z = net.param_grad(x, torch.zeros_like(gv))
    assert float(z.abs().max()) == 0.0 and float(a.abs().max()) > 0


def test_additive_over_the_batch(critics, refs):
    """param_grad([x0, x1], [w0, w1]) = param_grad(x0, w0) + param_grad(x1, w1) to 1e-5 per tensor: an image dropped or
    doubled at a piece boundary would show as an O(1) difference."""
    net = critics(9)
    ob, w, _ = refs("arb")
    both = net.param_grad(g(ob), g(w)).double()
    parts = net.param_grad(g(ob[:1]), g(w[:1])).double() + net.param_grad(g(ob[1:]), g(w[1:])).double()
    rel = G.per_tensor_rel(G.split_flat(both.cpu().numpy(), 9), G.split_flat(parts.cpu().numpy(), 9))
    k, e = G.worst(rel)
    print(f"additivity: worst tensor {k} {e:.2e} (bound 1e-5)")
    assert e <= 1e-5


def test_input_gradient_is_unchanged_by_a_param_grad_call(critics, refs):
    from tfpnp_amd import ops
    net = critics(9)
    ctx = net.context(dev())
    ob, w, _ = refs("rect")
    x, gv = g(ob), g(w)
    before_g, before_v = ops.critic_backward(ctx, x, gv), ops.critic_forward(ctx, x)
    net.param_grad(x, gv)
    assert torch.equal(ops.critic_backward(ctx, x, gv), before_g)
    assert torch.equal(ops.critic_forward(ctx, x), before_v)


def test_rejections(critics):
    from tfpnp_amd import _lib, ops
    from tfpnp_amd._lib import PnpxError
    net = critics(9)
    ctx = net.context(dev())
    ob = lambda c, h, w: np.zeros((1, c, h, w), np.float32)
    one = g(np.ones(1, np.float32))
    with pytest.raises(PnpxError, match="multiples of 32"):
        ops.critic_param_grad(ctx, g(ob(9, 48, 64)), one)
    with pytest.raises(PnpxError, match="channel count"):
        ops.critic_param_grad(ctx, g(ob(8, 64, 64)), one)
    with pytest.raises(PnpxError, match="entries"):
        ops.critic_param_grad(ctx, g(ob(9, 32, 32)), g(np.ones(2, np.float32)))
    with pytest.raises(PnpxError):
        net.param_grad(torch.from_numpy(ob(9, 32, 32)), one)                 # CPU observation
    with pytest.raises(PnpxError):
        net.param_grad(g(ob(9, 32, 32)), torch.ones(1))                      # CPU grad_value
    # the library's own checks, past the Python guards
    x = g(ob(9, 32, 32))
    n = int(_lib.lib().pnpx_critic_num_params(9))
    out = torch.empty(n, device=dev())
    call = lambda c, nn: _lib.lib().pnpx_critic_param_grad(c.handle, ops._p(x), ops._p(one), ops._p(out), nn, 1, 32, 32, ops._stream(x))
    assert _lib.lib().pnpx_critic_param_grad(ctx.handle, ops._p(x), ops._p(one), None, n, 1, 32, 32, ops._stream(x)) == 1   # null pointer
    assert call(ctx, n - 1) == 1                                              # PNPX_ERR_ARG
    with pytest.raises(PnpxError, match="parameters"):
        _lib.check(call(ctx, n - 1))                                          # PNPX_ERR_ARG: wrong n_params
    empty = ops.Context(dev())
    with pytest.raises(PnpxError, match="no critic loaded"):
        ops.critic_param_grad(empty, x, one)
    with pytest.raises(PnpxError, match="before pnpx_critic_load"):
        _lib.check(call(empty, n))
    assert call(ctx, n) == 0


def test_opcheck_param_grad(critics, refs):
    from tfpnp_amd import torch_ops
    assert "critic_param_grad" in torch_ops.ALL_OPS
    cid = critics(9).context(dev()).cid
    ob, w, _ = refs("kf9")
    torch.library.opcheck(torch.ops.pnpx.critic_param_grad, (g(ob), g(w), cid))
    # forward stays differentiable with respect to x only: param_grad takes no part in autograd
    x = g(ob).requires_grad_(True)
    assert not critics(9).param_grad(x, g(w)).requires_grad


def _slice_problem():
    rs = np.random.RandomState(4600)
    return rs.uniform(0, 1, (2, 9, 32, 32)).astype(np.float32), rs.standard_normal((2, 1)).astype(np.float32)


SLICE_LR, SLICE_STEPS = 1e-6, 8


def _restatement_loop(dtype):
    ob, Q = _slice_problem()
    P = G.leaves(K.critic_params(9), dtype)
    x, q = torch.from_numpy(ob).to(dtype), torch.from_numpy(Q).to(dtype)
    losses = []
    for it in range(SLICE_STEPS + 1):
        loss = ((G.leaf_forward(P, x) - q) ** 2).mean()
        losses.append(float(loss.detach()))
        if it < SLICE_STEPS:
            grads = torch.autograd.grad(loss, list(P.values()))
            with torch.no_grad():
                for p, d in zip(P.values(), grads):
                    p -= SLICE_LR * d
    return np.array(losses)


def test_training_slice_follows_the_fp64_loop():
    """Eight plain-SGD steps of mean((V(x) - Q)^2) on one fixed 2 x 9 x 32 x 32 batch, step size 1e-6 (chosen on the CPU: the
    fp64 restatement's loss falls monotonically, 21.25 -> 8.98): param_grad with grad_value = 2 (V - Q) / B, then load_flat_.
    The loss must fall at every step and stay within 1.31e-5 (relative, per step) of the same loop driven by the fp64
    restatement's autograd: ten times the spread between the fp32 and the fp64 restatement loops, which measured 1.31e-6
    relative (1.8e-5 absolute at a loss of 13.7) when this test was written."""
    from tfpnp_amd import synth
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    ob, Q = _slice_problem()
    ref = _restatement_loop(torch.float64)
    assert np.all(np.diff(ref) < 0)
    params = K.critic_params(9)
    flat = g(np.concatenate([params[k].reshape(-1) for k, _ in synth.critic_param_specs(9)]).astype(np.float32))
    net = ResNet_wobn(9, 18, 1).load_flat_(flat)
    x, q = g(ob), g(Q)
    losses = []
    for it in range(SLICE_STEPS + 1):
        V = net(x)
        losses.append(float(((V.double() - q.double()) ** 2).mean()))
        if it < SLICE_STEPS:
            flat = flat - SLICE_LR * net.param_grad(x, 2.0 * (V - q) / x.shape[0])
            net.load_flat_(flat)
    losses = np.array(losses)
    spread = np.abs(losses - ref) / ref
    print(f"training slice: loss {losses[0]:.4f} -> {losses[-1]:.4f} (fp64 loop {ref[-1]:.4f}); worst relative distance {spread.max():.2e}")
    assert np.all(np.diff(losses) < 0)
    assert spread.max() <= 1.31e-5
