"""GPU tests of the native actor update: pnpx_policy_forward_train_keep (the train-mode forward that keeps its activations),
pnpx_policy_param_grad_kept (the backward pass on what it kept), pnpx_policy_adam_step (clip_grad_norm_ + Adam on the live vector,
the running statistics frozen; csrc/live_optim.hip) and trainer/mddpg/actor_step.py::actor_update -- the actor's half of
tfpnp/trainer/mddpg/trainer.py::_update (:171, :201-204).

Everything the re-computing entries (pnpx_policy_forward_train, pnpx_policy_param_grad) also compute is compared with them bit for
bit.  The optimiser is measured against the fp64 restatement of tests/critic_step_cases.py (bounds: its module docstring; their
soundness: tests/test_critic_step_host.py), evaluated in float64 on the device."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import actor_cases as A
from tests import actor_grad_cases as G
from tests import actor_train_cases as T
from tests import critic_step_cases as S
from tfpnp_amd._lib import PnpxError

pytestmark = pytest.mark.gpu
CASE_PARAMS = [pytest.param(c, s, id=i) for (c, s), i in zip(T.CASES, T.IDS)]
CASE0, SHAPE0 = T.CASES[0]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda:0")


def g(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev())


def fresh(case, flat=None):
    """a native actor with the head of `case`: from the case's parameters, or from a flat vector on the device"""
    from tfpnp_amd import policy
    name, num_aux = A._ACTORS[tuple(case)]
    if flat is None:
        return getattr(policy, name)(num_aux, 5, state_dict=T.params(case))
    return getattr(policy, name)(num_aux, 5).load_flat_(flat)


def inputs(case, shape):
    gp, gd = G.upstream(case, shape)
    return g(T.observation(case, shape)), g(gp), g(gd)


def stat_mask(case):
    return T.stat_mask(case).to(dev())


def step_gradient(case, n, k):
    """critic_step_cases.synthetic_gradient sized to the actor's vector, the running-statistics slots zero (what param_grad writes)"""
    gk = g(S.synthetic_gradient(n, k))
    gk[stat_mask(case)] = 0.0
    return gk


def state(net):
    m, v, t = net.optim_state(dev())
    return net.parameters_flat(dev()), m, v, t


def same_state(a, b):
    return a[3] == b[3] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def example(name):
    spec = importlib.util.spec_from_file_location("example_" + name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------- kept forward
@pytest.mark.parametrize("case,shape", CASE_PARAMS)
def test_kept_forward_and_its_gradient_are_the_recomputing_ones(case, shape):
    from tfpnp_amd import ops
    ob, gp, gd = inputs(case, shape)
    plain, kept, still = (fresh(case).context(dev()) for _ in range(3))
    want = [*ops.policy_forward_train(plain, ob), *ops.policy_bn_stats(plain), plain.policy_params()]
    got = [*ops.policy_forward_train_keep(kept, ob), *ops.policy_bn_stats(kept), kept.policy_params()]
    for name, a, b in zip(("probs", "det", "batch mean", "batch variance", "parameters with the moved running statistics"), got, want):
        assert torch.equal(a, b), name
    mask = stat_mask(case)
    p0 = still.policy_params()
    assert not torch.equal(got[4][mask], p0[mask]) and torch.equal(got[4][~mask], p0[~mask])
    grad = ops.policy_param_grad(plain, ob, gp, gd)
    first = ops.policy_param_grad_kept(kept, gp, gd)
    assert torch.equal(first, grad)
    assert torch.equal(ops.policy_param_grad_kept(kept, gp, gd), grad)               # the backward pass destroys nothing it reads
    assert torch.equal(ops.policy_param_grad_kept(kept, 2.0 * gp, 2.0 * gd), ops.policy_param_grad(plain, ob, 2.0 * gp, 2.0 * gd))
    assert torch.equal(kept.policy_params(), got[4])                                 # ... and moves nothing
    # without the running-statistics update: the same outputs and gradient, the vector untouched
    ps, ds = ops.policy_forward_train_keep(still, ob, update_running=False)
    assert torch.equal(ps, want[0]) and torch.equal(ds, want[1]) and torch.equal(still.policy_params(), p0)
    assert torch.equal(ops.policy_param_grad_kept(still, gp, gd), grad)
    # the dispatcher-registered ops and the module's methods
    assert torch.equal(torch.ops.pnpx.policy_param_grad_kept(gp, gd, kept.cid), grad)
    actor = fresh(case)
    pm, dm = actor.forward_train_keep(ob)
    assert torch.equal(pm, want[0]) and torch.equal(dm, want[1]) and actor.device == dev()
    assert torch.equal(actor.param_grad_kept(gp, gd), grad) and torch.equal(actor.parameters_flat(dev()), got[4])
    assert not pm.requires_grad and not first.requires_grad


def test_opcheck_kept_ops():
    from tfpnp_amd import torch_ops
    assert "policy_forward_train_keep" in torch_ops.ALL_OPS and "policy_param_grad_kept" in torch_ops.ALL_OPS
    case, shape = T.CASES[1]
    ob, gp, gd = inputs(case, shape)
    ctx = fresh(case).context(dev())
    torch.library.opcheck(torch.ops.pnpx.policy_forward_train_keep, (ob, 0.1, False, ctx.cid))
    torch.library.opcheck(torch.ops.pnpx.policy_param_grad_kept, (gp, gd, ctx.cid))


def test_kept_gradient_survives_a_grown_workspace():
    from tfpnp_amd import ops
    ob, gp, gd = inputs(CASE0, SHAPE0)
    ctx = fresh(CASE0).context(dev())
    ops.policy_forward_train_keep(ctx, ob, update_running=False)
    first = ops.policy_param_grad_kept(ctx, gp, gd)
    big = torch.rand(SHAPE0[0] + 3, CASE0[0], SHAPE0[1], SHAPE0[2], device=dev())       # grows the workspace: other plan offsets
    gpb, gdb = torch.randn(big.shape[0], 2, device=dev()), torch.randn(big.shape[0], CASE0[1], device=dev())
    ops.policy_forward_train_keep(ctx, big, update_running=False)
    with pytest.raises(PnpxError, match="one row per observation of the kept forward"):
        ops.policy_param_grad_kept(ctx, gp, gd)                                      # the kept forward is the SECOND one: B + 3 rows
    of_big = ops.policy_param_grad_kept(ctx, gpb, gdb)
    ops.policy_forward_train_keep(ctx, ob, update_running=False)
    assert torch.equal(ops.policy_param_grad_kept(ctx, gp, gd), first)
    assert torch.equal(ops.policy_param_grad(ctx, big, gpb, gdb), of_big)
    assert torch.equal(ops.policy_param_grad(fresh(CASE0).context(dev()), ob, gp, gd), first)


# ------------------------------------------------------------------------------------------------- validity
def test_kept_forward_validity():
    from tfpnp_amd import ops
    case, shape = T.CASES[1]
    ob, gp, gd = inputs(case, shape)
    actor = fresh(case)
    ctx = actor.context(dev())
    n = ops.policy_flat_size(ctx)
    flat = actor.parameters_flat(dev())
    sentinel = torch.full((n,), -7.5, device=dev())
    out = sentinel.clone()

    def refused(reason):
        with pytest.raises(PnpxError, match=reason):
            ops.policy_param_grad_kept(ctx, gp, gd, out=out)
        assert torch.equal(out, sentinel), reason
        with pytest.raises(PnpxError, match=reason):
            actor.param_grad_kept(gp, gd)

    refused("no pnpx_policy_forward_train_keep has run")
    actor.forward_train_keep(ob)
    want = actor.param_grad(ob, gp, gd)                                              # ... which overwrites the workspace
    refused("pnpx_policy_param_grad overwrote")
    actor.forward_train_keep(ob)
    actor.load_flat_(flat)
    refused("pnpx_policy_load_device")
    actor.forward_train_keep(ob)
    actor.forward_train_raw(ob)
    refused("pnpx_policy_forward_train overwrote")
    actor.forward_train_keep(ob)
    actor.adam_step_(torch.zeros(n, device=dev()), 0.0)                              # lr 0, zero gradient: still a step
    refused("pnpx_policy_adam_step")
    assert actor.context(dev()) is ctx
    # what does not end it: an eval forward, reading the vector or the statistics, the optimiser's state, a refused step
    actor.load_flat_(flat)
    actor.forward_train_keep(ob, update_running=False)
    ops.policy_forward(ctx, ob)
    actor.parameters_flat(dev()), ops.policy_bn_stats(ctx), actor.optim_state(dev())
    with pytest.raises(PnpxError, match="not finite"):
        actor.adam_step_(torch.full((n,), float("nan"), device=dev()), 1e-3)
    assert ops.policy_param_grad_kept(ctx, gp, gd, out=out) is out and torch.equal(out, want)
    # a second kept forward replaces the first
    other = g(T.observation(case, shape, "offset"))
    actor.forward_train_keep(other, update_running=False)
    assert torch.equal(actor.param_grad_kept(gp, gd), actor.param_grad(other, gp, gd))
    # wrong sizes: nothing written
    actor.forward_train_keep(ob, update_running=False)
    out.copy_(sentinel)
    from tfpnp_amd import _lib
    assert _lib.lib().pnpx_policy_param_grad_kept(ctx.handle, ops._p(gp), ops._p(gd), ops._p(out), n - 1, ops._stream(gp)) == 1
    assert _lib.lib().pnpx_policy_param_grad_kept(ctx.handle, ops._p(gp), None, ops._p(out), n, ops._stream(gp)) == 1
    torch.cuda.synchronize()
    assert torch.equal(out, sentinel)
    empty = ops.Context(dev())
    assert _lib.lib().pnpx_policy_param_grad_kept(empty.handle, ops._p(gp), ops._p(gd), ops._p(out), n, ops._stream(gp)) == 3


# ------------------------------------------------------------------------------------------------- optimiser
@pytest.mark.parametrize("case", [pytest.param(T.CASES[0][0], id=T.IDS[0]), pytest.param(T.CASES[3][0], id=T.IDS[3])])
def test_adam_steps_follow_the_fp64_restatement(case):
    net, unaligned, twin = fresh(case), fresh(case), fresh(case)
    p0 = net.parameters_flat(dev())
    n = p0.numel()
    mask = stat_mask(case)
    ref = S.Yardstick(p0)
    buf = torch.empty(n + 1, device=dev())
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}
    for k in range(S.STEPS):
        gk = step_gradient(case, n, k)
        assert gk.data_ptr() % 16 == 0
        ref.step(gk)
        norm = net.adam_step_(gk, S.LR, betas=S.BETAS, eps=S.EPS, max_norm=S.MAX_NORM)
        assert norm.shape == () and norm.device.type == "cuda"
        view = buf[1:]
        view.copy_(gk)
        assert view.data_ptr() % 16 == 4                             # 4-byte aligned only: the scalar path throughout
        norm_u = unaligned.adam_step_(view, S.LR)
        norm_t = twin.adam_step_(gk.clone(), S.LR)
        st = state(net)
        assert st[3] == k + 1
        r = ref.ratios(*st[:3])
        r["norm"] = abs(float(norm) - ref.norm) / ref.norm / 1e-5
        print(f"{case}, step {k + 1}: norm {float(norm):.6g} (fp64 {ref.norm:.9g}); |err| / bound", {q: f"{x:.4f}" for q, x in r.items()})
        worst = {q: max(worst[q], r[q]) for q in r}
        assert all(x <= 1.0 for x in r.values()), (k, r)
        assert (ref.norm > S.MAX_NORM) == (k % 2 == 0)
        assert torch.equal(norm_u, norm) and same_state(state(unaligned), st), f"step {k + 1}: the 4-byte path gives other bytes"
        assert torch.equal(norm_t, norm) and same_state(state(twin), st), f"step {k + 1}: two actors fed the same sequence differ"
    print(f"{case}: worst |err| / bound over {S.STEPS} steps", {q: f"{x:.4f}" for q, x in worst.items()})
    p, m, v, _ = state(net)
    assert torch.equal(p[::97], p0[::97])                            # zero gradient entries: nothing moves
    assert torch.equal(p[mask], p0[mask]) and not m[mask].any() and not v[mask].any()
    assert not torch.equal(p[~mask], p0[~mask])


@pytest.mark.parametrize("case", [pytest.param(T.CASES[1][0], id=T.IDS[1]), pytest.param(T.CASES[3][0], id=T.IDS[3])])
def test_frozen_ranges_ignore_what_the_gradient_holds_there(case):
    clean, dirty, dirty_u = fresh(case), fresh(case), fresh(case)
    p0 = clean.parameters_flat(dev())
    n = p0.numel()
    mask = stat_mask(case)
    slots = mask.nonzero().squeeze(1)
    buf = torch.empty(n + 1, device=dev())
    for k in range(2):                                               # clip active, then inactive
        gk = step_gradient(case, n, k)
        garbage = gk.clone()
        garbage[mask] = torch.randn(slots.numel(), device=dev(), generator=torch.Generator(dev()).manual_seed(90 + k)) * 1e6
        garbage[slots[0]] = float("inf")                             # first element of a range
        garbage[slots[-1]] = float("nan")                            # last element of the last one
        garbage[slots[slots.numel() // 2]] = -float("inf")
        assert torch.equal(garbage[~mask], gk[~mask])
        view = buf[1:]
        view.copy_(garbage)
        n_clean, n_dirty, n_u = clean.adam_step_(gk, S.LR), dirty.adam_step_(garbage, S.LR), dirty_u.adam_step_(view, S.LR)
        assert math.isfinite(float(n_clean)) and torch.equal(n_clean, n_dirty) and torch.equal(n_clean, n_u)
        st = state(clean)
        assert same_state(state(dirty), st) and same_state(state(dirty_u), st), k
        assert torch.equal(st[0][mask], p0[mask])                    # the running statistics did not move
        assert not st[1][mask].any() and not st[2][mask].any()       # their moments are exactly zero
        assert st[1][~mask].any() and st[2][~mask].any()


def test_the_step_reaches_every_packing():
    from tfpnp_amd import ops
    ob, gp, gd = inputs(CASE0, SHAPE0)
    actor = fresh(CASE0)
    ctx = actor.context(dev())
    n = ops.policy_flat_size(ctx)
    runs = (lambda a: ops.policy_forward(a.context(dev()), ob), lambda a: a.forward_train_raw(ob), lambda a: (a.param_grad(ob, gp, gd),))
    before = [run(actor) for run in runs]                            # every packing exists and is current
    actor.adam_step_(step_gradient(CASE0, n, 0), S.LR)
    flat = actor.parameters_flat(dev())
    for name, run, old in zip(("eval forward", "train forward", "parameter gradient"), runs, before):
        new, ref = run(actor), run(fresh(CASE0, flat))
        assert all(torch.equal(a, b) for a, b in zip(new, ref)), name
        assert not all(torch.equal(a, b) for a, b in zip(new, old)), name
    assert actor.context(dev()) is ctx


def test_non_finite_gradient_changes_nothing():
    from tfpnp_amd import ops
    case, shape = T.CASES[1]
    ob = g(T.observation(case, shape))
    net = fresh(case)
    n = net.parameters_flat(dev()).numel()
    grads = [step_gradient(case, n, k) for k in range(2)]
    net.adam_step_(grads[0], S.LR)
    before, out = state(net), ops.policy_forward(net.context(dev()), ob) + net.forward_train_raw(ob)
    assert before[3] == 1
    bad = grads[1].clone()
    live = (~stat_mask(case)).nonzero().squeeze(1)
    bad[live[12345]] = float("nan")
    with pytest.raises(PnpxError, match="not finite"):
        net.adam_step_(bad, S.LR)
    assert same_state(state(net), before)
    bad[live[12345]] = float("inf")
    with pytest.raises(PnpxError, match="not finite"):
        net.adam_step_(bad, S.LR, max_norm=float("inf"))
    assert same_state(state(net), before)
    again = ops.policy_forward(net.context(dev()), ob) + net.forward_train_raw(ob)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    net.adam_step_(grads[1], S.LR)
    after = state(net)
    assert after[3] == 2 and not torch.equal(after[0], before[0])
    twin = fresh(case)                                               # the same two finite steps without the refused ones in between
    twin.adam_step_(grads[0], S.LR)
    twin.adam_step_(grads[1], S.LR)
    assert same_state(state(twin), after)


def test_state_lifetime():
    from tfpnp_amd import _lib, ops
    case = T.CASES[1][0]
    net = fresh(case)
    flat = net.parameters_flat(dev())
    n = flat.numel()
    grads = [step_gradient(case, n, k) for k in range(2)]
    zero = net.optim_state(dev())
    assert zero[2] == 0 and not zero[0].any() and not zero[1].any()               # before the first step
    net.adam_step_(grads[0], S.LR)
    net.adam_step_(grads[1], S.LR)
    _, m, v, t = state(net)
    assert t == 2 and m.any() and v.any()
    net.load_flat_(flat)                                                          # a refresh of the same actor keeps the state
    assert same_state(state(net), (flat, m, v, 2))
    net.reset_optim_()
    m3, v3, t3 = net.optim_state(dev())
    assert t3 == 0 and not m3.any() and not v3.any()
    net.adam_step_(grads[0], S.LR)
    assert net.optim_state(dev())[2] == 1
    net.load_state_dict(T.params(case))                                           # a checkpoint load drops it
    m4, v4, t4 = net.optim_state(dev())
    assert t4 == 0 and not m4.any() and not v4.any()
    ctx = net.context(dev())
    net.adam_step_(grads[0], S.LR)
    ctx.load_policy(T.params(case), *case)                                        # pnpx_policy_load on the same context as well
    assert ctx.policy_optim_state()[2] == 0
    # a step before any load; the library's own argument checks, past the Python guards: PNPX_ERR_ARG, nothing changed
    empty = ops.Context(dev())
    with pytest.raises(PnpxError, match="no actor loaded"):
        empty.policy_adam_step(grads[0], S.LR)
    lib = _lib.lib()
    call = lambda c, nn, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, mx=50.0: lib.pnpx_policy_adam_step(
        c.handle, ops._p(grads[0]), nn, lr, b1, b2, eps, mx, None, ops._stream(grads[0]))
    assert call(empty, n) == 3                                                    # PNPX_ERR_NO_WEIGHTS
    net.adam_step_(grads[0], S.LR)
    before = state(net)
    for bad in (dict(nn=n - 1), dict(lr=-1.0), dict(lr=math.inf), dict(b1=1.0), dict(b2=-0.5), dict(eps=0.0), dict(mx=0.0), dict(mx=math.nan)):
        assert call(ctx, **{"nn": n, **bad}) == 1, bad
    assert same_state(state(net), before)
    assert call(ctx, n, mx=math.inf) == 0 and net.optim_state(dev())[2] == 2      # grad_norm_dev may be NULL


# ------------------------------------------------------------------------------------------------- actor_update
def test_actor_update_teacher_forced():
    """Two steps of actor_update against the composed path run by hand on a twin built from the same vector: forward_train with the
    running update, the torch head, param_grad, and the fp64 restatement of clip + Adam."""
    from tfpnp_amd import ops
    from tfpnp_amd.trainer.mddpg.actor_step import actor_update
    composed, native = example("train_actor"), example("train_actor_native")
    lr = 1e-3
    ob = g(T.observation(CASE0, SHAPE0))
    idx_stop = g(np.array([0, 1, 1, 0], np.int64))
    actor = fresh(CASE0)
    mask = stat_mask(CASE0)
    seen = {}
    kept = actor.param_grad_kept

    def spy(gp, gd):
        seen["gp"], seen["gd"], seen["grad"] = gp, gd, kept(gp, gd)
        return seen["grad"]

    actor.param_grad_kept = spy
    cg_max = torch.zeros(actor.parameters_flat(dev()).numel(), device=dev(), dtype=torch.float64)
    for it in range(2):
        _, m, v, t = state(actor)
        assert t == it
        twin = fresh(CASE0, actor.parameters_flat(dev()))
        tctx = twin.context(dev())
        probs, det = (x.requires_grad_() for x in ops.policy_forward_train(tctx, ob))   # the running statistics move
        loss = composed.toy_loss(twin, probs, det, idx_stop)
        loss.backward()
        grad = twin.param_grad(ob, probs.grad, det.grad)
        p = tctx.policy_params()
        out = actor_update(actor, ob, native.toy_loss_fn(actor), lr, idx_stop=idx_stop)
        assert set(out) == {"policy_loss", "actor_norm", "action", "action_log_prob", "dist_entropy"}
        assert all(isinstance(x, torch.Tensor) and x.is_cuda and not x.requires_grad
                   for x in [*out["action"].values()] + [x for k, x in out.items() if k != "action"])
        action, logp, entropy = twin.head(probs.detach(), det.detach(), idx_stop, True)
        assert list(out["action"]) == list(action) and all(torch.equal(out["action"][k], action[k]) for k in action)   # = det, mapped
        assert torch.equal(out["action_log_prob"], logp) and torch.equal(out["dist_entropy"], entropy)                 # = probs
        assert torch.equal(out["policy_loss"], loss.detach())
        assert torch.equal(seen["gp"], probs.grad) and torch.equal(seen["gd"], det.grad) and torch.equal(seen["grad"], grad)
        p64, m64, v64, norm, c = S.adam_ref(p, m, v, t + 1, grad, lr, max_norm=50.0)
        cg_max = torch.maximum(cg_max, (grad.double() * c).abs())
        p_new, m_new, v_new, t_new = state(actor)
        assert t_new == it + 1
        r = S.bound_ratios(p_new.double() - p64, m_new.double() - m64, v_new.double() - v64, p64, cg_max, 1, lr)
        print(f"actor_update {it}: loss {float(out['policy_loss']):.6f}, norm {float(out['actor_norm']):.5g} (fp64 {norm:.8g}); |err| / bound",
              {q: f"{x:.4f}" for q, x in r.items()})
        assert all(x <= 1.0 for x in r.values()), (it, r)
        assert abs(float(out["actor_norm"]) - norm) <= 1e-5 * norm
        assert torch.equal(p_new[mask], p[mask]) and not torch.equal(p_new[~mask], p[~mask])    # both actors' running statistics
    history, trained = native.run(log=lambda *a: None)
    print("examples/train_actor_native.py:", history)
    assert len(history) == 5 and np.all(np.isfinite(history)) and history[-1] < history[0]
    assert trained.optim_state(dev())[2] == 5


def test_both_examples_run():
    quiet = lambda *a: None
    native, actor = example("train_actor_native").run(steps=2, log=quiet)
    composed, _ = example("train_actor").run(steps=2, log=quiet)
    print("examples: native", native, "composed", composed)
    assert len(native) == len(composed) == 2 and np.all(np.isfinite(native)) and np.all(np.isfinite(composed))
    assert native[0] == composed[0]                                 # the same first forward and the same toy loss
    assert actor.optim_state(dev())[2] == 2
