"""GPU tests of the actor's live weights (csrc/policy_pack.hip): the device load against the host load (bitwise), the
in-place refresh (of a host-loaded actor too; the retired option policy_s2_hs changes nothing), a module source against the
CPU oracle, state_dict() / native -> native, ordering behind a chained forward, and the rejections.

"Bitwise" on results is torch.equal on probs and det of the same observations: both actors run the same kernels, so equal
packed weights, biases and scales give equal bits, and an error in any packed weight that matters shows.  Parameter vectors
are compared as int32 words.  Weights: synth.make_policy_params(case, seed).  Shapes: B = 2 at 32 x 32 (the smallest image
with five stride-2 levels) and one rectangular B = 3 at 64 x 96.

The one toleranced check prints its figures (run with -s): probs / det of a module-sourced actor against the fp32 CPU oracle on
the module's state dict, bound 2e-5 (the project's actor bound, tests/test_gpu_policy.py).
"""
import numpy as np
import pytest
import torch

from tests import actor_cases as A
from tests.golden_inputs import policy_obs
from tfpnp_amd import ops, synth
from tfpnp_amd._lib import PnpxError

pytestmark = pytest.mark.gpu

_params, _flats, _hosts = {}, {}, {}
ADMM = (9, 10, False)


def dev():
    return torch.device("cuda:0")


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def params(case, seed):
    if (case, seed) not in _params:
        _params[case, seed] = synth.make_policy_params(*case, seed=seed)
    return _params[case, seed]


def flat_cpu(case, seed):
    """the flat parameter vector (CPU tensor); shared, never modified"""
    if (case, seed) not in _flats:
        _flats[case, seed] = A.flat_vector(params(case, seed), case)
    return _flats[case, seed]


def host_actor(case, seed):
    """an actor loaded through load_state_dict (host fold and packing); shared, its weights are never modified"""
    if (case, seed) not in _hosts:
        _hosts[case, seed] = A.native_actor(case, state_dict=params(case, seed))
    return _hosts[case, seed]


def device_actor(case, seed):
    return A.native_actor(case).load_flat_(flat_cpu(case, seed).to(dev()))


def obs(case, B=2, H=32, W=32, seed=23):
    return g(policy_obs(B, case[0], H, W, seed + case[0]))


def forward(actor, ob):
    return ops.policy_forward(actor.context(dev()), ob)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


# ------------------------------------------------------------------------------------------------ 1. device load == host load
@pytest.mark.parametrize("s2_hs", [1])     # the retired option's remaining value: accepted, without effect
@pytest.mark.parametrize("case", A.CASES)
def test_device_load_equals_host_load(case, s2_hs):
    host, devc = host_actor(case, 7), device_actor(case, 7)
    for c in (host.context(dev()), devc.context(dev())):
        c.set_option("policy_s2_hs", s2_hs)
    assert A.same_outputs(host, devc, obs(case))
    assert A.same_outputs(host, devc, obs(case, B=3, H=64, W=96))
    assert bits_equal(devc.parameters_flat(dev()), flat_cpu(case, 7))
    assert bits_equal(host.parameters_flat(dev()), flat_cpu(case, 7))     # the host entry keeps the vector too
    torch.cuda.synchronize()
    assert not devc.context(dev()).range_tripped()


# ------------------------------------------------------------------------------------------------ 2. in-place refresh
def test_refresh_in_place():
    ob = obs(ADMM, B=3, H=64, W=96)
    refs = {s: forward(host_actor(ADMM, s), ob) for s in (7, 8, 9)}
    flats = {s: flat_cpu(ADMM, s).to(dev()) for s in (7, 8, 9)}
    assert not torch.equal(refs[7][1], refs[8][1]) and not torch.equal(refs[8][1], refs[9][1])
    net = A.native_actor(ADMM).load_flat_(flats[7])
    ctx = net.context(dev())
    p, d = forward(net, ob)                      # the arena exists from here on
    assert torch.equal(p, refs[7][0]) and torch.equal(d, refs[7][1])
    free = []
    for s in (8, 9, 8):
        net.load_flat_(flats[s])
        assert net.context(dev()) is ctx
        p, d = forward(net, ob)
        assert torch.equal(p, refs[s][0]) and torch.equal(d, refs[s][1]), s
        del p, d
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each refresh:", free)
    assert free[1] == free[2]                    # no reallocation, no leak
    assert not ctx.range_tripped()


def test_refresh_of_a_host_loaded_actor():
    net = A.native_actor(ADMM, state_dict=params(ADMM, 7))
    ctx = net.context(dev())
    ob = obs(ADMM)
    p7, d7 = forward(net, ob)
    assert torch.equal(d7, forward(host_actor(ADMM, 7), ob)[1])
    net.load_flat_(flat_cpu(ADMM, 8).to(dev()))
    assert net.context(dev()) is ctx and net._state is None          # the CPU copy of the load is stale and gone
    assert A.same_outputs(net, host_actor(ADMM, 8), ob)
    assert bits_equal(net.parameters_flat(dev()), flat_cpu(ADMM, 8))
    net.load_flat_(flat_cpu(ADMM, 7).to(dev()))
    p, d = forward(net, ob)
    assert torch.equal(p, p7) and torch.equal(d, d7)


def test_retired_option_is_inert_and_a_host_load_refreshes_in_place():
    """policy_s2_hs used to select an fp32 kernel for the stem and the stage entries and a second blob layout behind the host
    load.  Now the key is accepted and changes nothing, and a host-loaded actor is refreshed in place like a device-loaded one.
    B = 2 at 32 x 32: the smallest legal image, and the fewest observations the batch statistics accept."""
    ob = obs(ADMM)

    def run(setting):
        ctx = A.native_actor(ADMM, state_dict=params(ADMM, 7)).context(dev())
        ctx.set_option("policy_s2_hs", setting)
        assert ctx.get_option("policy_s2_hs") == 1
        out = [*ops.policy_forward(ctx, ob), *ops.policy_forward_train(ctx, ob), *ops.policy_bn_stats(ctx), ctx.policy_params()]
        used = ctx.bytes()
        ctx.set_option("policy_s2_hs", 0)
        ctx.set_option("policy_s2_hs", 1)
        assert ctx.bytes() == used
        ops.policy_forward_train(ctx, ob, update_running=False)                  # no arena was dropped: nothing is reserved again
        assert ctx.bytes() == used
        return out

    one, zero = run(1), run(0)
    names = ("probs", "det", "train probs", "train det", "batch mean", "batch var", "live vector")
    for name, a, b in zip(names, one, zero):
        assert bits_equal(a, b), name
    assert not bits_equal(one[6], flat_cpu(ADMM, 7))                             # the train forward did move the statistics

    # test_refresh_in_place's check, starting from the host entry
    refs = {s: forward(host_actor(ADMM, s), ob) for s in (8, 9)}
    flats = {s: flat_cpu(ADMM, s).to(dev()) for s in (8, 9)}
    net = A.native_actor(ADMM, state_dict=params(ADMM, 7))
    ctx = net.context(dev())
    forward(net, ob)                                                             # the arena exists from here on
    free = []
    for s in (8, 9, 8):
        net.load_flat_(flats[s])
        assert net.context(dev()) is ctx
        p, d = forward(net, ob)
        assert torch.equal(p, refs[s][0]) and torch.equal(d, refs[s][1]), s
        del p, d
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each refresh of a host-loaded actor:", free)
    assert free[1] == free[2]                                                    # no reallocation, no leak


# ------------------------------------------------------------------------------------------------ 3. module source
def test_module_source_against_the_oracle():
    from oracle import pnp_oracle as O
    from tfpnp_amd.utils.misc import hard_update
    module = A.load_params(A.stand_in_actor(*ADMM), params(ADMM, 21)).to(dev())
    before = A.flat_vector(module.state_dict(), ADMM)
    assert bits_equal(before, flat_cpu(ADMM, 21))
    ob = obs(ADMM)
    # two train-mode passes move the running statistics, one SGD step moves the parameters.  Batch statistics over the two
    # values a channel has at the 1 x 1 stage make gradients of several hundred, so the rate is small: the step has to leave
    # a network whose heads are not saturated, or the comparison below would say nothing
    opt = torch.optim.SGD(module.parameters(), lr=1e-5)
    module.train()
    for k in range(2):
        probs, det = module(obs(ADMM, seed=40 + k))
    opt.zero_grad()
    (det.square().sum() + probs[:, 0].sum()).backward()
    opt.step()
    module.eval()
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    after = A.flat_vector(sd, ADMM)
    o_rv, n_rv = A.offset_of("actor_encoder.layer2.0.bn1.running_var", ADMM)
    o_w, n_w = A.offset_of("actor_encoder.layer3.1.conv2.weight", ADMM)
    assert not bits_equal(before[o_rv:o_rv + n_rv], after[o_rv:o_rv + n_rv])
    assert not bits_equal(before[o_w:o_w + n_w], after[o_w:o_w + n_w])
    native = A.native_actor(ADMM)
    hard_update(native, module)
    assert bits_equal(native.parameters_flat(dev()), after)
    probs, det = forward(native, ob)
    po, do = O.policy_forward(sd, ob.cpu(), False)
    ep, ed = float((probs.cpu() - po).abs().max()), float((det.cpu() - do).abs().max())
    print(f"module source: max|d probs| {ep:.2e}  max|d det| {ed:.2e} against the CPU oracle (bound 2e-5)")
    assert ep < 2e-5 and ed < 2e-5
    assert float(po.min()) > 0.05 and float((do - 0.5).abs().max()) < 0.45 and bool((po[0] != po[1]).any())   # not saturated
    # ... and the module's own eval-mode forward on the GPU is the same network
    with torch.no_grad():
        pm, dm = module(ob)
    print(f"module source: max|d probs| {float((probs - pm).abs().max()):.2e}  max|d det| {float((det - dm).abs().max()):.2e} "
          "against the module's own forward")
    # bitwise: a fresh native actor load_state_dict-ed from that same state dict (host fold and packing)
    fresh = A.native_actor(ADMM, state_dict=sd)
    assert A.same_outputs(fresh, native, ob)


# ------------------------------------------------------------------------------------------------ 4. state_dict, native -> native
@pytest.mark.parametrize("case", [ADMM, (6, 10, True)])
def test_state_dict_round_trip_and_native_hard_update(case):
    from tfpnp_amd.utils.misc import hard_update
    net = device_actor(case, 8)
    ob = obs(case)
    sd = net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in synth.policy_param_specs(*case)]
    assert all(v.device.type == "cuda" and v.dtype == torch.float32 for v in sd.values())
    assert bits_equal(torch.cat([v.reshape(-1) for v in sd.values()]), flat_cpu(case, 8))
    fresh = A.native_actor(case, state_dict=sd)                  # host fold and packing of the exported weights
    assert A.same_outputs(fresh, net, ob)
    assert bits_equal(A.flat_vector(fresh.state_dict(), case), flat_cpu(case, 8))     # ... and from the CPU copy
    copy = A.native_actor(case)
    hard_update(copy, net)
    assert bits_equal(copy.parameters_flat(dev()), flat_cpu(case, 8))
    assert A.same_outputs(copy, net, ob)
    hard_update(copy, host_actor(case, 7))                       # a host-loaded source, onto a loaded target
    assert A.same_outputs(copy, host_actor(case, 7), ob)
    assert copy.device == dev()


def test_follow_actor_example():
    """examples/follow_actor.py: the native actor runs the rollouts of the torch actor an optimiser steps."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import follow_actor
    lines = []
    history, module, native = follow_actor.run(updates=3, B=2, H=64, log=lines.append)
    assert len(history) == len(lines) == 3 and all(np.isfinite(h).all() for h in history)
    assert history[0] != history[1] != history[2]        # the rollout's actions moved with every update
    # after the last hard_update the native actor holds the module's state and computes the module's own eval-mode outputs
    # (the project's actor bound against an fp32 evaluation of the same network, test_gpu_policy.py)
    assert bits_equal(native.parameters_flat(dev()), A.flat_vector(module.state_dict(), ADMM))
    ob = obs(ADMM)
    module.eval()
    with torch.no_grad():
        pm, dm = module(ob)
    p, d = forward(native, ob)
    ep, ed = float((p - pm).abs().max()), float((d - dm).abs().max())
    print(f"example: native actor vs its torch source after hard_update: max|d probs| {ep:.2e}  max|d det| {ed:.2e}")
    assert ep < 2e-5 and ed < 2e-5


# ------------------------------------------------------------------------------------------------ 5. ordering
def test_refresh_is_ordered_behind_a_chained_forward():
    ob = obs(ADMM, B=2)
    refs = {s: forward(host_actor(ADMM, s), ob) for s in (7, 8)}
    assert not torch.equal(refs[7][1], refs[8][1])
    flats = {s: flat_cpu(ADMM, s).to(dev()) for s in (7, 8)}
    net = A.native_actor(ADMM).load_flat_(flats[7])
    ctx = net.context(dev())
    ctx.set_option("chains", 2)
    assert ctx.get_option("chains") == 2
    forward(net, ob)                             # arena allocation (synchronises) out of the way
    torch.cuda.synchronize()
    first = forward(net, ob)                     # two launch chains: one on a side stream
    net.load_flat_(flats[8])                     # same stream: behind both chains
    second = forward(net, ob)
    torch.cuda.synchronize()
    assert torch.equal(first[0], refs[7][0]) and torch.equal(first[1], refs[7][1])
    assert torch.equal(second[0], refs[8][0]) and torch.equal(second[1], refs[8][1])


# ------------------------------------------------------------------------------------------------ 6. rejections
def test_rejections():
    good = flat_cpu(ADMM, 7).to(dev())
    n = good.numel()
    net = device_actor(ADMM, 7)
    ctx = net.context(dev())
    ob = obs(ADMM)
    p0, d0 = forward(net, ob)

    def still_works():
        p, d = forward(net, ob)
        return torch.equal(p, p0) and torch.equal(d, d0) and bits_equal(ctx.policy_params(), flat_cpu(ADMM, 7))

    for call in (net.load_flat_, lambda v: ctx.load_policy_device(v, *ADMM)):
        with pytest.raises(PnpxError, match=f"{n} parameters, got {n - 1}"):
            call(good[:-1])                                              # wrong length
        with pytest.raises(PnpxError, match="cpu"):
            call(flat_cpu(ADMM, 7))                                      # CPU tensor
        with pytest.raises(PnpxError, match="float32"):
            call(good.double())                                          # fp64 tensor
        with pytest.raises(PnpxError, match="contiguous"):
            call(torch.stack([good, good], 1)[:, 0])                     # non-contiguous tensor
        assert still_works()
    with pytest.raises(PnpxError, match="parameters, got"):
        ctx.load_policy_device(good, 9, 15, False)                       # another head: the length no longer fits
    assert still_works()
    # the library's own count check (the Python layer checks first, so call the C entry directly)
    from tfpnp_amd import _lib
    st = _lib.lib().pnpx_policy_load_device(ctx.handle, ops._p(good), n - 1, 9, 10, 0, ops._stream(good))
    assert st == 1 and b"expected" in _lib.lib().pnpx_last_error()
    assert still_works()
    empty = ops.Context(dev())
    with pytest.raises(PnpxError, match=r"status 3\)"):
        empty.policy_params()
    # a NaN running_var: PNPX_ERR_ARG, and the actor is unloaded afterwards
    bad = good.clone()
    o, _ = A.offset_of("actor_encoder.layer2.0.bn1.running_var", ADMM)
    bad[o + 5] = float("nan")
    neg = good.clone()
    neg[o + 5] = -1.0                                                    # sqrt of a negative number
    victim = device_actor(ADMM, 7)
    vctx = victim.context(dev())
    with pytest.raises(PnpxError, match=r"status 1\).*scale of convolution 6 is not finite"):
        victim.load_flat_(bad)
    with pytest.raises(PnpxError, match="no policy loaded"):
        ops.policy_forward(vctx, ob)
    with pytest.raises(PnpxError, match=r"status 3\)"):
        vctx.policy_params()
    with pytest.raises(PnpxError, match=r"status 1\)"):
        A.native_actor(ADMM).load_flat_(neg)                             # the same on a first load
    victim.load_flat_(good)                                              # and it can be loaded again
    p, d = forward(victim, ob)
    assert torch.equal(p, p0) and torch.equal(d, d0)
    assert still_works()
