"""GPU tests of the actor's train-mode forward (pnpx_policy_forward_train): batch-statistics BatchNorm and the running-statistics
update in the live parameter vector, against the torch stand-in of tests/actor_cases.py in `.train()` mode, in float64, on the CPU
(tests/actor_train_cases.py).  Bounds: 2e-5 on probs / det and 2e-5 * max(1, max |ref|) on statistics, the project's bounds for the
eval-mode actor (tests/test_gpu_policy.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import actor_cases as A
from tests import actor_train_cases as T
from tfpnp_amd import _lib
from tfpnp_amd._lib import PnpxError

pytestmark = pytest.mark.gpu
PNPX_ERR_ARG, PNPX_ERR_NO_WEIGHTS = 1, 3
CASE_PARAMS = [pytest.param(c, s, id=i) for (c, s), i in zip(T.CASES, T.IDS)]


def dev():
    return torch.device("cuda:0")


def g(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev())


def fresh(case, **kw):
    """A native actor with the case's weights, loaded from a state_dict (the checkpoint path)."""
    from tfpnp_amd import policy
    name, num_aux = A._ACTORS[tuple(case)]
    return getattr(policy, name)(num_aux, 5, state_dict=T.params(case), **kw)


def err(a, ref):
    return float((a.detach().double().cpu() - ref).abs().max())


def stat_bound(ref):
    return 2e-5 * max(1.0, float(ref.abs().max()))


def running(flat, case):
    flat = flat.cpu()
    return torch.cat([flat[p:p + n] for p, n in T.stat_slices(case)])


@pytest.mark.parametrize("s2_hs", [1])     # the retired option's remaining value: accepted, without effect
@pytest.mark.parametrize("case,shape", CASE_PARAMS)
def test_parity_with_the_float64_stand_in(case, shape, s2_hs):
    from tfpnp_amd import ops
    ref = T.reference(case, shape)
    ctx = fresh(case).context(dev())
    ctx.set_option("policy_s2_hs", s2_hs)
    probs, det = ops.policy_forward_train(ctx, g(T.observation(case, shape)))
    mean, var = ops.policy_bn_stats(ctx)
    moved = running(ctx.policy_params(), case)
    e = {"probs": err(probs, ref["probs1"]), "det": err(det, ref["det1"]), "mean": err(mean, ref["mean"]), "var": err(var, ref["var"]),
         "running": err(moved, ref["running1"])}
    print(f"{case} {shape} s2_hs {s2_hs}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  (fp32 stand-in {ref['fp32_err']:.2e})")
    assert e["probs"] < 2e-5 and e["det"] < 2e-5
    assert e["mean"] <= stat_bound(ref["mean"]) and e["var"] <= stat_bound(ref["var"])
    assert e["running"] <= stat_bound(ref["running1"])
    # the mode matters on these cases: a path that ignores it fails
    pe, de = ops.policy_forward(fresh(case).context(dev()), g(T.observation(case, shape)))
    assert max(float((pe - probs).abs().max()), float((de - det).abs().max())) > 0.02


@pytest.mark.parametrize("case,shape", CASE_PARAMS)
def test_two_train_forwards_then_eval(case, shape):
    from tfpnp_amd import ops
    ref = T.reference(case, shape)
    actor = fresh(case, bn_follows_mode=True)
    ob = g(T.observation(case, shape))
    ctx = actor.context(dev())
    actor.train()
    for it in (1, 2):
        actor(ob, None, True, None)
        assert err(running(actor.parameters_flat(dev()), case), ref[f"running{it}"]) <= stat_bound(ref[f"running{it}"])
    probs, det = ops.policy_forward(ctx, ob)          # re-derives the eval packing from the moved statistics
    e = max(err(probs, ref["probs_eval"]), err(det, ref["det_eval"]))
    print(f"{case} {shape}: eval after two train forwards, max error {e:.2e}")
    assert e < 2e-5
    sd = actor.state_dict()
    assert err(running(A.flat_vector(sd, case), case), ref["running2"]) <= stat_bound(ref["running2"])
    again = A.native_actor(case, state_dict=sd)
    p2, d2 = ops.policy_forward(again.context(dev()), ob)
    assert torch.equal(p2, probs) and torch.equal(d2, det)
    p3, d3 = ops.policy_forward(ctx, ob)              # and the second eval forward re-derives nothing: same bits
    assert torch.equal(p3, probs) and torch.equal(d3, det)


def test_nothing_else_moves():
    from tfpnp_amd import ops
    case, shape = T.CASES[1]
    ctx = fresh(case).context(dev())
    ob = g(T.observation(case, shape))
    before = ctx.policy_params()
    ops.policy_forward_train(ctx, ob, update_running=False)
    assert torch.equal(ctx.policy_params(), before)
    ops.policy_forward_train(ctx, ob, update_running=True)
    after = ctx.policy_params()
    mask = T.stat_mask(case).to(dev())
    assert torch.equal(after[~mask], before[~mask])
    assert not torch.equal(after[mask], before[mask])


def test_determinism_and_chains():
    from tfpnp_amd import ops
    case, shape = T.CASES[0]
    ob = g(T.observation(case, shape))
    runs = []
    for chains in (1, 1, 2):
        ctx = fresh(case).context(dev())
        ctx.set_option("chains", chains)
        out = ops.policy_forward_train(ctx, ob) + ops.policy_bn_stats(ctx) + (ctx.policy_params(),)
        runs.append(out)
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


def test_batch_coupling():
    """Row 0 changes when image 1 changes -- batch statistics couple the images -- and in eval mode it does not."""
    from tfpnp_amd import ops
    case, shape = T.CASES[0]
    ctx = fresh(case).context(dev())
    ob = g(T.observation(case, shape))
    ob2 = ob.clone()
    ob2[1] = 1.0 - ob2[1]
    pa, da = ops.policy_forward_train(ctx, ob, update_running=False)
    pb, db = ops.policy_forward_train(ctx, ob2, update_running=False)
    assert not torch.equal(pa[0], pb[0]) and not torch.equal(da[0], db[0])
    ref = T.reference(case, shape)
    assert err(pa, ref["probs1"]) < 2e-5                    # ... and it is still the right answer
    ea, eb = ops.policy_forward(ctx, ob), ops.policy_forward(ctx, ob2)
    assert torch.equal(ea[0][0], eb[0][0]) and torch.equal(ea[1][0], eb[1][0])


def test_large_mean_against_spread():
    """ob = 0.9 + 0.2 u: the stem's raw outputs carry a mean far above their spread.  Bound: max(2e-5, 8 x the fp32 stand-in's own
    error against float64) -- 4 x for the activation format's 22 bits against fp32's 24, times 2 of headroom."""
    from tfpnp_amd import ops
    case, shape = T.CASES[0]
    ref = T.reference(case, shape, "offset", 1)
    bound = max(2e-5, 8 * ref["fp32_err"])
    ctx = fresh(case).context(dev())
    probs, det = ops.policy_forward_train(ctx, g(T.observation(case, shape, "offset")))
    mean, var = ops.policy_bn_stats(ctx)
    e = max(err(probs, ref["probs1"]), err(det, ref["det1"]))
    print(f"large mean: native {e:.2e}  fp32 stand-in {ref['fp32_err']:.2e}  bound {bound:.2e}  "
          f"mean {err(mean, ref['mean']):.2e}  var {err(var, ref['var']):.2e}")
    assert e <= bound
    assert err(mean, ref["mean"]) <= stat_bound(ref["mean"]) and err(var, ref["var"]) <= stat_bound(ref["var"])


def _heads(actor, probs, det, idx_stop):
    logp = torch.log(probs.clamp_min(torch.finfo(probs.dtype).eps)).gather(1, idx_stop.view(-1, 1))
    entropy = -torch.special.xlogy(probs, probs).sum(dim=1, keepdim=True)
    return actor.action_mapping(det), logp, entropy


def test_module_follows_mode_only_when_asked():
    from tfpnp_amd import ops
    case, shape = T.CASES[1]
    ref = T.reference(case, shape)
    ob = g(T.observation(case, shape))
    idx_stop = torch.tensor([0, 1, 1], device=dev())
    actor = fresh(case, bn_follows_mode=True)
    assert actor.training
    action, logp, entropy, hidden = actor(ob, idx_stop, True, None)
    dist = torch.distributions.Categorical(ref["probs1"])
    want, _, _ = _heads(actor, ref["probs1"], ref["det1"], idx_stop.cpu())
    for k, v in want.items():
        assert err(action[k], v) <= 2e-5 * max(1.0, float(v.abs().max())), k
    assert torch.equal(action["idx_stop"], idx_stop) and hidden is None
    assert err(logp, dist.log_prob(idx_stop.cpu()).unsqueeze(1)) <= 1e-4 and err(entropy, dist.entropy().unsqueeze(1)) <= 1e-4
    assert err(running(actor.parameters_flat(dev()), case), ref["running1"]) <= stat_bound(ref["running1"])
    # .eval(): today's path, bit for bit (on the moved statistics)
    actor.eval()
    probs, det = ops.policy_forward(actor.context(dev()), ob)
    got = actor(ob, idx_stop, False, None)
    want = _heads(actor, probs, det, idx_stop)
    assert all(torch.equal(got[0][k], want[0][k]) for k in want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    # the default: the eval path in either mode, nothing moves
    plain = fresh(case)
    probs, det = ops.policy_forward(fresh(case).context(dev()), ob)
    want = _heads(plain, probs, det, idx_stop)
    for mode in (True, False):
        plain.train(mode)
        got = plain(ob, idx_stop, mode, None)
        assert all(torch.equal(got[0][k], want[0][k]) for k in want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert torch.equal(plain.parameters_flat(dev()).cpu(), A.flat_vector(T.params(case), case))


def test_arguments():
    from tfpnp_amd import ops
    lib = _lib.lib()
    case = (9, 10, False)
    ctx = fresh(case).context(dev())
    before = ctx.policy_params()

    def raw_call(handle, ob, momentum=0.1):
        B, _, H, W = ob.shape
        probs, det = torch.empty(B, 2, device=dev()), torch.empty(B, 10, device=dev())
        return lib.pnpx_policy_forward_train(handle, ob.data_ptr(), probs.data_ptr(), det.data_ptr(), B, H, W, ctypes.c_float(momentum), 1, None)

    with pytest.raises(PnpxError):                              # no train forward has run yet
        ops.policy_bn_stats(ctx)
    one = torch.rand(1, 9, 32, 32, device=dev())                # one value per channel in the last stage: torch raises there
    assert raw_call(ctx.handle, one) == PNPX_ERR_ARG
    with pytest.raises(PnpxError, match="more than 1 value"):
        ops.policy_forward_train(ctx, one)
    two = torch.rand(2, 9, 32, 32, device=dev())
    assert raw_call(ctx.handle, two, momentum=1.5) == PNPX_ERR_ARG
    assert raw_call(ctx.handle, two, momentum=-0.1) == PNPX_ERR_ARG
    with pytest.raises(PnpxError, match="momentum"):
        ops.policy_forward_train(ctx, two, momentum=1.5)
    empty = ops.Context(dev())                                  # before a load
    assert raw_call(empty.handle, two) == PNPX_ERR_NO_WEIGHTS
    with pytest.raises(PnpxError):
        ops.policy_forward_train(empty, two)
    with pytest.raises(PnpxError):
        ops.policy_forward_train(ctx, torch.rand(2, 9, 32, 32))
    with pytest.raises(PnpxError):
        fresh(case, bn_follows_mode=True)(torch.rand(2, 9, 32, 32), None, True, None)
    with pytest.raises(PnpxError):                              # still none: every call above was refused before its first launch
        ops.policy_bn_stats(ctx)
    assert torch.equal(ctx.policy_params(), before)


def test_workspace_regrowth():
    from tfpnp_amd import ops
    case = (6, 10, True)
    ctx = fresh(case).context(dev())
    ops.policy_forward_train(ctx, g(T.observation(case, (2, 64, 32))), update_running=False)
    shape = (5, 64, 32)
    ref = T.reference(case, shape)
    probs, det = ops.policy_forward_train(ctx, g(T.observation(case, shape)), update_running=False)
    assert err(probs, ref["probs1"]) < 2e-5 and err(det, ref["det1"]) < 2e-5
    # a smaller batch in the grown workspace, and the larger one again: same bits
    ops.policy_forward_train(ctx, g(T.observation(case, (3, 64, 32))), update_running=False)
    p2, d2 = ops.policy_forward_train(ctx, g(T.observation(case, shape)), update_running=False)
    assert torch.equal(p2, probs) and torch.equal(d2, det)
