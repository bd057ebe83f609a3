"""Host-side checks of the native critic update (no GPU): the C ABI / binding surface of the four new entries, the soundness of
the optimiser bounds of tests/critic_step_cases.py at the full parameter count, the fp64 restatement against torch's own
Adam + clip_grad_norm_ in float64, and the argument checks that need no device."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import critic_step_cases as S
from tfpnp_amd import _lib
from tfpnp_amd._lib import PnpxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pnpx_critic_value_loss_grad", "pnpx_critic_adam_step", "pnpx_critic_optim_state", "pnpx_critic_optim_reset")
N9 = 11177042


def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    from tfpnp_amd import ops, torch_ops
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    from tfpnp_amd.trainer.mddpg.critic_step import critic_update
    assert callable(ops.critic_value_loss_grad) and callable(critic_update)
    for name in ("critic_adam_step", "critic_optim_state", "critic_optim_reset"):
        assert callable(getattr(ops.Context, name)), name
    for name in ("value_loss_grad", "adam_step_", "optim_state", "reset_optim_"):
        assert callable(getattr(ResNet_wobn, name)), name
    assert "critic_value_loss_grad" in torch_ops.ALL_OPS
    assert lib.pnpx_critic_num_params(9) == N9
    assert all(lib.pnpx_critic_num_params(c) % 4 == 2 for c in range(1, 65))      # the 4-byte tail is always live


def test_fp32_restatement_stays_within_half_of_every_bound():
    """The k = 6 synthetic steps at the parameter count of num_inputs = 9, from critic_cases.critic_params: a float32 Adam in
    another operation order ends within half of each bound (measured: p 0.353, m 0.016, v 0.0004 of the bound), so a kernel
    that exceeds one is wrong, not unlucky.  The ratios after the earlier steps are printed: the parameter ratio peaks at 0.66
    after step 2, where a weight_g entry steps from 2.0013 down across 2.0 -- its step-1 rounding of half an ulp above 2.0 is a
    whole ulp32(|p64|) below it, for any fp32 parameter vector -- and stays below 1 throughout."""
    p0 = S.flat_params(9)
    n = p0.size
    assert n == N9
    ref = S.Yardstick(p0)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for k in range(S.STEPS):
        g = S.synthetic_gradient(n, k)
        ref.step(g)
        assert (ref.norm > 50.0) == (k % 2 == 0), (k, ref.norm)                   # the clip is active on even steps only
        p, m, v, norm, _ = S.adam_f32(p, m, v, k + 1, g, S.LR)
        assert abs(float(norm) - ref.norm) <= 1e-6 * ref.norm
        r = ref.ratios(p, m, v)
        print(f"fp32 restatement after step {k + 1}: |err| / bound", {q: f"{x:.4f}" for q, x in r.items()})
        assert all(x <= 1.0 for x in r.values()), (k, r)
    assert all(x <= 0.5 for x in r.values()), r
    assert np.all(p[::97] == p0[::97]) and not m[::97].any() and not v[::97].any()  # a zero gradient entry moves nothing


def test_adam_ref_is_torch_adam_in_float64():
    n = 20003
    rs = np.random.RandomState(11)
    p0 = rs.standard_normal(n) * 0.05
    w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([w], lr=S.LR, betas=S.BETAS, eps=S.EPS, foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for k in range(S.STEPS):
        g = S.synthetic_gradient(n, k, seed=3).astype(np.float64) * 30.0         # norms on both sides of 50
        w.grad = torch.from_numpy(g.copy())
        norm_t = float(torch.nn.utils.clip_grad_norm_([w], S.MAX_NORM))
        opt.step()
        p, m, v, norm, c = S.adam_ref(p, m, v, k + 1, g, S.LR)
        assert (c < 1.0) == (k % 2 == 0)
        assert abs(norm - norm_t) <= 1e-12 * norm
        st = opt.state[w]
        for got, want in ((p, w.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
        assert int(st["step"]) == k + 1


def _bare_context(num_inputs=9):
    """an ops.Context that was never created natively: enough for the checks that run before the first native call"""
    from tfpnp_amd import ops
    ctx = ops.Context.__new__(ops.Context)
    ctx.device = torch.device("cuda", 0)
    ctx._critic = num_inputs
    ctx._h = None
    return ctx


def test_argument_checks_raise_without_a_device():
    from tfpnp_amd import ops
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    ctx = _bare_context()
    g = torch.zeros(N9)
    with pytest.raises(PnpxError, match="cpu"):
        ctx.critic_adam_step(g, 1e-3)                                             # CPU gradient
    with pytest.raises(PnpxError, match="parameters"):
        ctx.critic_adam_step(torch.zeros(N9 - 1), 1e-3)                           # wrong length
    with pytest.raises(PnpxError, match="torch.Tensor"):
        ctx.critic_adam_step(np.zeros(4, np.float32), 1e-3)
    for kw, pat in ((dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr=float("inf")), "lr"),
                    (dict(lr=1e-3, betas=(1.0, 0.999)), "betas"), (dict(lr=1e-3, betas=(0.9, -0.1)), "betas"),
                    (dict(lr=1e-3, betas=(0.9,)), "betas"), (dict(lr=1e-3, eps=0.0), "eps"),
                    (dict(lr=1e-3, max_norm=0.0), "max_norm"), (dict(lr=1e-3, max_norm=float("nan")), "max_norm")):
        with pytest.raises(PnpxError, match=pat):
            ctx.critic_adam_step(g, **kw)
    none = _bare_context(None)
    with pytest.raises(PnpxError, match="no critic loaded"):
        none.critic_adam_step(g, 1e-3)
    with pytest.raises(PnpxError, match="no critic loaded"):
        none.critic_optim_state()
    fake = types.SimpleNamespace(_critic=9)
    ob = torch.zeros(2, 9, 32, 32)
    with pytest.raises(PnpxError, match="cpu"):
        ops.critic_value_loss_grad(fake, ob, torch.zeros(2))                      # CPU tensors
    with pytest.raises(PnpxError, match="2 entries"):
        ops.critic_value_loss_grad(fake, ob, torch.zeros(3))                      # wrong length
    net = ResNet_wobn(9, 18, 1)
    with pytest.raises(PnpxError, match="cpu"):
        net.value_loss_grad(ob, torch.zeros(2))
    with pytest.raises(PnpxError, match="cpu"):
        net.adam_step_(g, 1e-3)
    with pytest.raises(PnpxError, match="torch.Tensor"):
        net.adam_step_(None, 1e-3)
