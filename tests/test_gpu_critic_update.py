"""GPU tests of the critic's live weights (csrc/critic.hip "device-side packing"): the device load against the host load
(bitwise), the in-place refresh, soft_update / hard_update against torch's arithmetic (bitwise), a module source, the input
gradient after a refresh, and the rejections.

"Bitwise" on results is torch.equal on V and on the input gradient of the same observations: both critics run the same
kernels, so equal weight blobs, thresholds and scales give equal bits, and an error in any packed weight that matters shows.
Parameter vectors are compared as int32 words.  Weights: synth.make_critic_params(num_inputs, seed); num_inputs 1 / 9 / 17
cover cin_pad 8 / 16 / 24 and the 32- and 64-row tiles of the stem adjoint.

The two toleranced checks print their figures (run with -s): V of a module-sourced critic against the fp64 restatement
(bound 2e-5 * max(1, |V|), the project's bound) and the input gradient after a refresh against fp64 autograd (bound 1e-3).
"""
import numpy as np
import pytest
import torch

from tests import critic_cases as K
from tests.golden_inputs import KINK_MARGIN
from tfpnp_amd import ops, synth
from tfpnp_amd._lib import PnpxError

pytestmark = pytest.mark.gpu

_params, _flats, _hosts = {}, {}, {}


def dev():
    return torch.device("cuda:0")


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def params(num_inputs, seed):
    if (num_inputs, seed) not in _params:
        _params[num_inputs, seed] = synth.make_critic_params(num_inputs, seed)
    return _params[num_inputs, seed]


def flat_cpu(num_inputs, seed):
    """the flat parameter vector (CPU tensor); shared, never modified"""
    if (num_inputs, seed) not in _flats:
        _flats[num_inputs, seed] = torch.from_numpy(ops.critic_flat_params(params(num_inputs, seed), num_inputs))
    return _flats[num_inputs, seed]


def host_critic(num_inputs, seed):
    """a critic loaded through load_state_dict (host fold and packing); shared, never modified"""
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    if (num_inputs, seed) not in _hosts:
        _hosts[num_inputs, seed] = ResNet_wobn(num_inputs, 18, 1, state_dict=params(num_inputs, seed))
    return _hosts[num_inputs, seed]


def device_critic(num_inputs, seed):
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    return ResNet_wobn(num_inputs, 18, 1).load_flat_(flat_cpu(num_inputs, seed).to(dev()))


def rand_ob(num_inputs, B=2, H=32, W=32, seed=11):
    rs = np.random.RandomState(seed + num_inputs)
    return g(rs.uniform(0, 1, (B, num_inputs, H, W)).astype(np.float32)), g(rs.standard_normal(B).astype(np.float32))


def value_and_grad(net, ob, gv):
    ctx = net.context(dev())
    return ops.critic_forward(ctx, ob), ops.critic_backward(ctx, ob, gv)


def same_results(a, b, ob, gv):
    Va, Ga = value_and_grad(a, ob, gv)
    Vb, Gb = value_and_grad(b, ob, gv)
    return torch.equal(Va, Vb) and torch.equal(Ga, Gb) and bool(torch.isfinite(Va).all()) and float(Ga.abs().max()) > 0


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def formula(t, s, tau):
    """utils/misc.py:81-85 on CPU fp32 tensors"""
    return t * (1.0 - tau) + s * tau


# ------------------------------------------------------------------------------------------------ 1. device load == host load
@pytest.mark.parametrize("num_inputs", [1, 9, 17])
def test_device_load_equals_host_load(num_inputs):
    host, devc = host_critic(num_inputs, 7), device_critic(num_inputs, 7)
    obs = [rand_ob(num_inputs)]
    if num_inputs == 9:
        for name in ("arb", "rect"):
            ob, w = K.case_inputs(name, 0)
            obs.append((g(ob), g(w)))
    for ob, gv in obs:
        assert same_results(host, devc, ob, gv), tuple(ob.shape)
    assert bits_equal(devc.parameters_flat(dev()), flat_cpu(num_inputs, 7))
    assert bits_equal(host.parameters_flat(dev()), flat_cpu(num_inputs, 7))     # the host entry keeps the vector too
    torch.cuda.synchronize()
    assert not devc.context(dev()).range_tripped()


# ------------------------------------------------------------------------------------------------ 2. in-place refresh
def test_refresh_in_place():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    ob, gv = rand_ob(9, B=3, H=64, W=64)
    refs = {s: value_and_grad(host_critic(9, s), ob, gv) for s in (7, 8, 9)}
    flats = {s: flat_cpu(9, s).to(dev()) for s in (7, 8, 9)}
    assert not torch.equal(refs[7][0], refs[8][0]) and not torch.equal(refs[8][0], refs[9][0])
    net = ResNet_wobn(9, 18, 1).load_flat_(flats[7])
    ctx = net.context(dev())
    V, G = value_and_grad(net, ob, gv)           # the arena exists from here on
    assert torch.equal(V, refs[7][0]) and torch.equal(G, refs[7][1])
    free = []
    for s in (8, 9, 8):
        net.load_flat_(flats[s])
        assert net.context(dev()) is ctx
        V, G = value_and_grad(net, ob, gv)
        assert torch.equal(V, refs[s][0]) and torch.equal(G, refs[s][1]), s
        del V, G
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each refresh:", free)
    assert free[1] == free[2]                    # no reallocation, no leak
    assert not ctx.range_tripped()


# ------------------------------------------------------------------------------------------------ 3. soft update arithmetic
@pytest.mark.parametrize("tau", [0.001, 0.5])
def test_soft_update_arithmetic(tau):
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    t, s = flat_cpu(9, 7), flat_cpu(9, 8)
    s_dev = s.to(dev())
    net = device_critic(9, 7)
    ctx = net.context(dev())
    net.soft_update_(s_dev, 0.0)
    assert bits_equal(ctx.critic_params(), t)            # tau = 0 leaves every bit in place
    exp = t
    for it in range(3):
        net.soft_update_(s_dev, tau)
        exp = formula(exp, s, tau)
        assert bits_equal(ctx.critic_params(), exp), it
    assert not bits_equal(exp, t) and not bits_equal(exp, s)
    ob, gv = rand_ob(9)
    sd = net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(sh)) for k, sh in synth.critic_param_specs(9)]
    assert bits_equal(torch.cat([v.reshape(-1) for v in sd.values()]), exp)
    fresh = ResNet_wobn(9, 18, 1, state_dict=sd)         # host fold and packing of the exported weights
    assert same_results(fresh, net, ob, gv)
    assert not torch.equal(value_and_grad(net, ob, gv)[0], value_and_grad(host_critic(9, 7), ob, gv)[0])


def test_soft_update_of_a_host_loaded_critic():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    net = ResNet_wobn(9, 18, 1, state_dict=params(9, 7))
    net.context(dev())
    other = device_critic(9, 7)
    s_dev = flat_cpu(9, 8).to(dev())
    net.soft_update_(s_dev, 0.1)
    other.soft_update_(s_dev, 0.1)
    assert bits_equal(net.parameters_flat(dev()), formula(flat_cpu(9, 7), flat_cpu(9, 8), 0.1))
    assert same_results(net, other, *rand_ob(9))
    assert net._state is None                            # the CPU copy of the load is stale and gone


# ------------------------------------------------------------------------------------------------ 4. module source
def _seeded_module(num_inputs, seed):
    m = K.stand_in_module(num_inputs)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("alpha"):
                p.copy_((torch.rand(1, generator=gen) * 0.1 + 0.02) * (1 if torch.rand(1, generator=gen) < 0.5 else -1))
            elif name.endswith("weight_g") or name.endswith("original0"):
                p.copy_(torch.rand(p.shape, generator=gen) * 1.4 + 0.7)
            elif name.endswith("weight_v") or name.endswith("original1"):
                p.copy_(torch.randn(p.shape, generator=gen) * (2.0 / p[0].numel()) ** 0.5)
            elif name == "fc.weight":
                p.copy_(torch.randn(p.shape, generator=gen) * (1.0 / 512) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    alphas = torch.cat([p.detach().flatten() for n, p in m.named_parameters() if n.endswith("alpha")])
    assert (alphas != 0).all() and (alphas > 0).any() and (alphas < 0).any()
    return m


def test_module_source():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    from tfpnp_amd.utils.misc import hard_update, soft_update
    module = _seeded_module(9, 21).to(dev())
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    native = ResNet_wobn(9, 18, 1)
    hard_update(native, module)
    ob, gv = rand_ob(9)
    host = ResNet_wobn(9, 18, 1, state_dict=sd)
    assert same_results(host, native, ob, gv)
    V = native(ob).cpu().numpy()
    ref = K.restate({k: v.numpy() for k, v in sd.items()}, ob.cpu().numpy(), torch.float64).numpy()
    print(f"module source: V {ref.ravel()}  max|dV| vs fp64 restatement {np.abs(V - ref).max():.2e}")
    assert np.all(np.abs(V - ref) <= 2e-5 * np.maximum(1.0, np.abs(ref)))
    # the module trains on (here: an in-place perturbation by torch ops) and the native target follows
    before = torch.cat([p.detach().reshape(-1) for p in module.parameters()]).cpu()
    with torch.no_grad():
        for i, p in enumerate(module.parameters()):
            p.mul_(1.0 + 0.01 * ((i % 3) - 1)).add_(1e-3)
    after = torch.cat([p.detach().reshape(-1) for p in module.parameters()]).cpu()
    assert not bits_equal(before, after)
    soft_update(native, module, 0.1)
    assert bits_equal(native.parameters_flat(dev()), formula(before, after, 0.1))
    # native -> native
    copy = ResNet_wobn(9, 18, 1)
    hard_update(copy, native)
    assert bits_equal(copy.parameters_flat(dev()), native.parameters_flat(dev()))
    assert same_results(copy, native, ob, gv)
    soft_update(copy, host, 0.5)
    assert bits_equal(copy.parameters_flat(dev()), formula(formula(before, after, 0.1), before, 0.5))


def test_target_critic_example():
    """examples/target_critic.py: the native target follows the torch critic an optimiser steps."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import target_critic
    lines = []
    history, critic, target = target_critic.run(steps=3, B=2, H=32, tau=0.5, log=lines.append)
    assert len(history) == len(lines) == 3 and all(np.isfinite(h).all() for h in history)
    assert history[0] != history[1] != history[2]        # the target moved with every update
    # the example's torch critic is a faithful source: after a hard update the native target computes the module's own V
    # (the project's bound on V against an fp32 evaluation of the same network, test_gpu_critic.py)
    from tfpnp_amd.utils.misc import hard_update
    hard_update(target, critic)
    ob = rand_ob(9)[0]
    with torch.no_grad():
        V_t, V_m = target(ob), critic(ob)
    print(f"example: native target vs its torch source after hard_update: max|dV| {float((V_t - V_m).abs().max()):.2e}")
    assert np.all(np.abs((V_t - V_m).cpu().numpy()) <= 2e-5 * np.maximum(1.0, np.abs(V_m.cpu().numpy())))


# ------------------------------------------------------------------------------------------------ 5. gradient path
def test_autograd_follows_the_refresh():
    """ResNet_wobn.forward under autograd after a refresh: the input gradient of the NEW weights (seed 8) against the fp64
    restatement's autograd, on the first try of case kf9 that keeps every TReLU input KINK_MARGIN away from its threshold
    under the new weights (chosen on the restatement).  Bound: the kink-free bound of test_gpu_critic.py, 1e-3."""
    net = device_critic(9, 7)
    ob0, _ = K.case_inputs("kf9", 0)
    net(g(ob0))
    net.load_flat_(flat_cpu(9, 8).to(dev()))
    for k in range(K.KINKFREE_TRIES):
        ob, w = K.case_inputs("kf9", k)
        V_ref, grad_ref, margin = K.restate_value_and_grad(params(9, 8), ob, w, torch.float64)
        if margin > KINK_MARGIN:
            break
    assert margin > KINK_MARGIN
    x = g(ob).requires_grad_(True)
    V = net(x)
    assert V.requires_grad
    (V[:, 0] * g(w)).sum().backward()
    e = K.rel_l2(x.grad.cpu().numpy(), grad_ref)
    _, grad_old, _ = K.restate_value_and_grad(params(9, 7), ob, w, torch.float64)
    print(f"kf9 try {k} (margin {margin:.2e}): input gradient rel-L2 vs fp64 autograd {e:.2e} (bound 1e-3); "
          f"old weights' gradient is {K.rel_l2(grad_old, grad_ref):.2e} away")
    assert np.all(np.abs(V.detach().cpu().numpy() - V_ref) <= 2e-5 * np.maximum(1.0, np.abs(V_ref)))
    assert e < 1e-3
    assert K.rel_l2(grad_old, grad_ref) > 1e-1           # the check can tell the two weight sets apart


# ------------------------------------------------------------------------------------------------ 6. rejections
def test_rejections():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    from tfpnp_amd.utils.misc import hard_update, soft_update
    good = flat_cpu(9, 7).to(dev())
    net = device_critic(9, 7)
    ctx = net.context(dev())
    ob, gv = rand_ob(9)
    V0 = net(ob)

    def still_works():
        return torch.equal(net(ob), V0) and bits_equal(ctx.critic_params(), flat_cpu(9, 7))

    for call in (net.load_flat_, lambda v: net.soft_update_(v, 0.1), lambda v: ctx.load_critic_device(v, 9),
                 lambda v: ctx.critic_soft_update(v, 0.1)):
        with pytest.raises(PnpxError, match="11177042 parameters, got 11177041"):
            call(good[:-1])                                              # wrong length
        with pytest.raises(PnpxError, match="cpu"):
            call(flat_cpu(9, 7))                                         # CPU tensor
        with pytest.raises(PnpxError, match="float32"):
            call(good.double())                                          # fp64 tensor
        with pytest.raises(PnpxError, match="contiguous"):
            call(torch.stack([good, good], 1)[:, 0])                     # non-contiguous tensor
        assert still_works()
    with pytest.raises(PnpxError, match="parameter count"):
        ctx.load_critic_device(good[:-1], None)
    # a module with a missing layer; a num_inputs mismatch (module and native)
    broken = K.stand_in_module(9)
    del broken.layer3[1].relu_2
    other = K.stand_in_module(17)
    for fn in (hard_update, lambda t, s: soft_update(t, s, 0.1)):
        with pytest.raises(PnpxError, match="81 parameter tensors"):
            fn(net, broken.to(dev()))
        with pytest.raises(PnpxError, match="num_inputs"):
            fn(net, other.to(dev()))
        with pytest.raises(PnpxError, match="num_inputs"):
            fn(net, ResNet_wobn(17, 18, 1))
        with pytest.raises(PnpxError, match="cpu"):
            fn(net, K.stand_in_module(9))
        assert still_works()
    # soft update before any load: the library's own status
    empty = ops.Context(dev())
    with pytest.raises(PnpxError, match=r"status 3\).*before a critic was loaded"):
        empty.critic_soft_update(good, 0.1)
    with pytest.raises(PnpxError, match=r"status 3\)"):
        empty.critic_params()
    # a NaN threshold: PNPX_ERR_ARG, and the critic is unloaded afterwards
    bad = good.clone()
    bad[-1] = float("nan")                                               # relu_1.alpha, the stem's threshold
    victim = device_critic(9, 7)
    vctx = victim.context(dev())
    with pytest.raises(PnpxError, match=r"status 1\).*threshold 0 is not finite"):
        victim.load_flat_(bad)
    with pytest.raises(PnpxError, match="no critic loaded"):
        ops.critic_forward(vctx, ob)
    with pytest.raises(PnpxError, match=r"status 3\)"):
        vctx.critic_params()
    with pytest.raises(PnpxError, match=r"status 1\)"):
        ResNet_wobn(9, 18, 1).load_flat_(bad)                            # the same on a first load
    victim.load_flat_(good)                                              # and it can be loaded again
    assert torch.equal(victim(ob), V0)
    assert still_works()
