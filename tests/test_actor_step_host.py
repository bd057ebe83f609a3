"""Host-side checks of the native actor update (no GPU): the C ABI / binding surface of the new entries (kept forward, its gradient,
the optimiser step), the frozen-range table the optimiser is given against tests/actor_train_cases.stat_slices, the O(B) head shared
by ResNetActorBase.forward and actor_update, and the argument checks that need no device."""
import os
import re

import numpy as np
import pytest
import torch

from tests import actor_cases as A
from tests import actor_train_cases as T
from tfpnp_amd import _lib
from tfpnp_amd._lib import PnpxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pnpx_policy_forward_train_keep", "pnpx_policy_param_grad_kept", "pnpx_policy_adam_step", "pnpx_policy_optim_state",
               "pnpx_policy_optim_reset", "pnpx_policy_frozen_ranges")
CASES = [pytest.param(c, id=i) for (c, _), i in zip(T.CASES, T.IDS)]


def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    from tfpnp_amd import ops, policy, torch_ops
    from tfpnp_amd.trainer.mddpg.actor_step import actor_update
    assert callable(actor_update)
    for name in ("policy_forward_train_keep", "policy_param_grad_kept"):
        assert callable(getattr(ops, name)), name
        assert name in torch_ops.ALL_OPS and hasattr(torch.ops.pnpx, name), name
    assert "Tensor grad_probs, Tensor grad_det, SymInt ctx" in str(torch.ops.pnpx.policy_param_grad_kept.default._schema)
    for name in ("policy_adam_step", "policy_optim_state", "policy_optim_reset"):
        assert callable(getattr(ops.Context, name)), name
    for cls in (policy.ResNetActor_ADMM, policy.ResNetActor_SPI):
        for name in ("adam_step_", "optim_state", "reset_optim_", "forward_train_keep", "param_grad_kept", "head"):
            assert callable(getattr(cls, name)), (cls.__name__, name)


def merged(slices):
    out = []
    for first, count in slices:
        if out and out[-1][0] + out[-1][1] == first:
            out[-1] = (out[-1][0], out[-1][1] + count)
        else:
            out.append((first, count))
    return out


@pytest.mark.parametrize("case", CASES)
def test_frozen_ranges_are_the_running_statistics(case):
    from tfpnp_amd import ops
    ranges = ops.policy_frozen_ranges(*case)
    want = merged(T.stat_slices(case))
    assert ranges == want
    assert len(ranges) == 21 and sum(c for _, c in ranges) == 2 * T.N_BN         # running_mean | running_var of a layer: one range
    assert all(a + b < c for (a, b), (c, _) in zip(ranges, ranges[1:]))          # sorted, disjoint, nothing left to merge
    mask = torch.zeros(int(_lib.lib().pnpx_policy_num_params(case[0], case[1], int(case[2]))), dtype=torch.bool)
    for first, count in ranges:
        mask[first:first + count] = True
    assert torch.equal(mask, T.stat_mask(case))
    # the count alone, and a shape the library refuses
    lib = _lib.lib()
    assert lib.pnpx_policy_frozen_ranges(case[0], case[1], int(case[2]), None, None, 0) == 21
    assert lib.pnpx_policy_frozen_ranges(0, case[1], 0, None, None, 0) == -1
    with pytest.raises(PnpxError, match="no actor"):
        ops.policy_frozen_ranges(65, 10)


def test_head_is_what_forward_computed():
    """ResNetActorBase.head against the lines it was factored out of, restated: same values, and differentiable."""
    actor = A.native_actor((9, 10, False))
    rs = np.random.RandomState(5)
    logits = torch.from_numpy(rs.standard_normal((6, 2)).astype(np.float32))
    p = torch.softmax(logits, 1)
    p[0] = torch.tensor([1.0, 0.0])                                               # a saturated row: clamp and xlogy(0, 0) = 0
    det = torch.from_numpy(rs.uniform(0, 1, (6, 10)).astype(np.float32))
    idx = torch.tensor([1, 0, 1, 1, 0, 0])
    action, logp, entropy = actor.head(p, det, idx, True)
    want_logp = torch.log(p.clamp_min(torch.finfo(torch.float32).eps)).gather(1, idx.view(-1, 1))
    assert torch.equal(logp, want_logp) and logp.shape == (6, 1)
    assert torch.equal(entropy, -torch.special.xlogy(p, p).sum(dim=1, keepdim=True)) and float(entropy[0]) == 0.0
    assert list(action) == ["sigma_d", "mu", "idx_stop"] and action["idx_stop"] is idx
    assert torch.equal(action["sigma_d"], det[:, :5] * (70 / 255)) and torch.equal(action["mu"], det[:, 5:])
    greedy, _, _ = actor.head(p, det, None, False)
    assert torch.equal(greedy["idx_stop"], p.argmax(dim=1))
    torch.manual_seed(3)
    sampled, _, _ = actor.head(p, det, None, True)
    torch.manual_seed(3)
    assert torch.equal(sampled["idx_stop"], torch.multinomial(p, 1).squeeze(1))
    pl, dl = p.clone().requires_grad_(), det.clone().requires_grad_()
    action, logp, entropy = actor.head(pl, dl, idx, True)
    (logp.sum() + entropy.sum() + action["mu"].sum()).backward()
    assert pl.grad is not None and dl.grad is not None and bool((dl.grad[:, 5:] == 1).all()) and not dl.grad[:, :5].any()


def _bare_context(policy=(9, 10, False)):
    """an ops.Context that was never created natively: enough for the checks that run before the first native call"""
    from tfpnp_amd import ops
    ctx = ops.Context.__new__(ops.Context)
    ctx.device = torch.device("cuda", 0)
    ctx._policy = policy
    ctx._critic = None
    ctx._h = None
    return ctx


def test_argument_checks_raise_without_a_device():
    from tfpnp_amd import ops
    from tfpnp_amd.trainer.mddpg.actor_step import actor_update
    ctx = _bare_context()
    n = int(_lib.lib().pnpx_policy_num_params(9, 10, 0))
    g = torch.zeros(n)
    with pytest.raises(PnpxError, match="cpu"):
        ctx.policy_adam_step(g, 1e-3)                                             # CPU gradient
    with pytest.raises(PnpxError, match="parameters"):
        ctx.policy_adam_step(torch.zeros(n - 1), 1e-3)                            # wrong length
    with pytest.raises(PnpxError, match="torch.Tensor"):
        ctx.policy_adam_step(np.zeros(4, np.float32), 1e-3)
    for kw, pat in ((dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr=1e-3, betas=(1.0, 0.999)), "betas"),
                    (dict(lr=1e-3, betas=(0.9,)), "betas"), (dict(lr=1e-3, eps=0.0), "eps"), (dict(lr=1e-3, max_norm=0.0), "max_norm")):
        with pytest.raises(PnpxError, match=pat):
            ctx.policy_adam_step(g, **kw)
    none = _bare_context(None)
    with pytest.raises(PnpxError, match="no actor loaded"):
        none.policy_adam_step(g, 1e-3)
    with pytest.raises(PnpxError, match="no actor loaded"):
        none.policy_optim_state()
    ob, gp, gd = torch.zeros(2, 9, 32, 32), torch.zeros(2, 2), torch.zeros(2, 10)
    with pytest.raises(PnpxError, match="cpu"):
        ops.policy_forward_train_keep(ctx, ob)
    with pytest.raises(PnpxError, match="cpu"):
        ops.policy_param_grad_kept(ctx, gp, gd)
    with pytest.raises(PnpxError, match="no policy loaded"):
        ops.policy_param_grad_kept(none, gp, gd)
    with pytest.raises(PnpxError, match="torch.Tensor"):
        ops.policy_param_grad_kept(ctx, [0.0], gd)
    actor = A.native_actor((9, 10, False))
    with pytest.raises(PnpxError, match="cpu"):
        actor.adam_step_(g, 1e-3)
    with pytest.raises(PnpxError, match="torch.Tensor"):
        actor.adam_step_(None, 1e-3)
    with pytest.raises(PnpxError, match="cpu"):
        actor.forward_train_keep(ob)
    with pytest.raises(PnpxError, match="torch.Tensor"):
        actor.forward_train_keep([0.0])
    with pytest.raises(PnpxError, match="cpu"):
        actor.param_grad_kept(gp, gd)
    with pytest.raises(PnpxError, match="torch.Tensor"):
        actor.param_grad_kept(gp, None)
    with pytest.raises(PnpxError, match="cpu"):
        actor_update(actor, ob, lambda *a: None, 1e-3)
    assert actor.state_dict() == {} and actor.device is None
