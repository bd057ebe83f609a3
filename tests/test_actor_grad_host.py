"""Host-side tests of the actor's parameter gradients (no GPU): the BatchNorm-backward formulas of csrc/policy_grad.hip restated in
numpy (pieces, border, the two-summand block tail) against autograd in float64, the torch stand-in's autograd pinned to the executed
reference actor's (tests/golden/policy_actor_grad.npz, tools/make_actor_grad_golden.py), and the C ABI / Python surface."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from tests import actor_grad_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "policy_actor_grad.npz")
EPS = 1e-5
PIECE = 5          # pixels per partial sum here (BN_BWD_PIECE = 2048 in the kernel): 2 * 3 * 4 = 24 pixels -> 5 pieces, the last short


def bn_bwd_numpy(g_a, a, zs, weights, piece=PIECE):
    """The three passes of csrc/policy_grad.hip on padded tensors [B][C][h+2][w+2] (zero border, interior pixels only): dy = g_a * [a > 0]
    feeds every z of `zs` (one, or the two summands of a block tail).  -> (d bias, [d weight], [dz padded], dy padded)"""
    B, C, Hp, Wp = g_a.shape
    h, w = Hp - 2, Wp - 2
    n = B * h * w
    inner = lambda t: t[:, :, 1:-1, 1:-1].transpose(1, 0, 2, 3).reshape(C, n)      # pixel index = (b * h + y) * w + x
    dy = inner(g_a) * (inner(a) > 0)
    stats = [(inner(z).mean(axis=1), inner(z).var(axis=1)) for z in zs]
    # partial pass: per piece S1 and, per z, S2 = sum dy (z - mean); finish pass: the pieces in order
    s1 = np.zeros(C)
    s2 = [np.zeros(C) for _ in zs]
    for p0 in range(0, n, piece):
        sl = slice(p0, min(p0 + piece, n))
        s1 += dy[:, sl].sum(axis=1)
        for k, z in enumerate(zs):
            s2[k] += (dy[:, sl] * (inner(z)[:, sl] - stats[k][0][:, None])).sum(axis=1)
    d_weight, dzs = [], []
    for k, z in enumerate(zs):
        mean, var = stats[k]
        rstd = 1.0 / np.sqrt(var + EPS)
        d_weight.append(s2[k] * rstd)
        A = weights[k] * rstd
        c1, c2 = A * s1 / n, A * rstd ** 2 * s2[k] / n
        dz = A[:, None] * dy - c1[:, None] - c2[:, None] * (inner(z) - mean[:, None])      # apply pass
        out = np.zeros_like(g_a)
        out[:, :, 1:-1, 1:-1] = dz.reshape(C, B, h, w).transpose(1, 0, 2, 3)
        dzs.append(out)
    dy_out = np.zeros_like(g_a)
    dy_out[:, :, 1:-1, 1:-1] = dy.reshape(C, B, h, w).transpose(1, 0, 2, 3)
    return s1, d_weight, dzs, dy_out


def pad(t):
    return np.pad(t, ((0, 0), (0, 0), (1, 1), (1, 1)))


def test_bn_backward_formulas_against_autograd():
    r = np.random.RandomState(0)
    B, C, h, w = 2, 3, 3, 4
    z1, z2, res, g_a = (r.standard_normal((B, C, h, w)) for _ in range(4))
    w1, b1, w2, b2 = (r.standard_normal(C) for _ in range(4))
    rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    for tail in ("one", "shortcut", "identity"):
        tz1, tz2, tres = (torch.tensor(t, requires_grad=True) for t in (z1, z2, res))
        tw1, tb1, tw2, tb2 = (torch.tensor(t, requires_grad=True) for t in (w1, b1, w2, b2))
        pre = F.batch_norm(tz1, None, None, tw1, tb1, True, 0.1, EPS)
        if tail == "shortcut":
            pre = pre + F.batch_norm(tz2, None, None, tw2, tb2, True, 0.1, EPS)
        if tail == "identity":
            pre = pre + tres
        act = F.relu(pre)
        (act * torch.tensor(g_a)).sum().backward()
        zs, ws = ([z1, z2], [w1, w2]) if tail == "shortcut" else ([z1], [w1])
        d_bias, d_weight, dzs, dy = bn_bwd_numpy(pad(g_a), pad(act.detach().numpy()), [pad(z) for z in zs], ws)
        assert rel(d_bias, tb1.grad.numpy()) < 1e-12 and rel(d_weight[0], tw1.grad.numpy()) < 1e-12
        assert rel(dzs[0][:, :, 1:-1, 1:-1], tz1.grad.numpy()) < 1e-12
        assert not dzs[0][:, :, 0].any() and not dzs[0][:, :, :, -1].any()           # the border stays zero
        if tail == "shortcut":      # the same dy feeds both layers: one S1, two S2
            assert rel(d_bias, tb2.grad.numpy()) < 1e-12 and rel(d_weight[1], tw2.grad.numpy()) < 1e-12
            assert rel(dzs[1][:, :, 1:-1, 1:-1], tz2.grad.numpy()) < 1e-12
        if tail == "identity":      # dy itself is the identity branch's gradient
            assert rel(dy[:, :, 1:-1, 1:-1], tres.grad.numpy()) < 1e-12


def test_piece_size_does_not_change_the_formulas():
    r = np.random.RandomState(1)
    g_a, a, z = (pad(r.standard_normal((2, 2, 3, 4))) for _ in range(3))
    one = bn_bwd_numpy(g_a, a, [z], [np.ones(2)], piece=5)
    other = bn_bwd_numpy(g_a, a, [z], [np.ones(2)], piece=24)
    assert np.allclose(one[0], other[0], rtol=1e-13) and np.allclose(one[2][0], other[2][0], rtol=1e-12, atol=1e-15)


def test_stand_in_autograd_matches_the_executed_reference():
    """The fp32 stand-in within 1e-5 relative per tensor of the executed reference actor's float64 autograd (measured: norms 1.2e-6,
    samples 5.0e-6; the float64 stand-in 7e-15), so the GPU tests' reference is the reference project's gradient."""
    gd = np.load(GOLDEN)
    case, shape = G.GOLDEN_CASE, G.GOLDEN_SHAPE
    assert tuple(gd["case"]) == tuple(int(v) for v in case) and tuple(gd["shape"]) == shape
    ref = G.reference(case, shape)
    assert abs(ref["loss"] - float(gd["loss"])) <= 1e-12 * abs(float(gd["loss"]))
    tensors = G.tensors(case)
    assert len(tensors) == 67 == len(gd["norms"]) and gd["samples"].shape == (67, G.GOLDEN_SAMPLES)
    for name, bound in (("fp32", 1e-5), ("grad", 1e-12)):
        flat = ref[name].numpy()
        for i, (key, pos, n) in enumerate(tensors):
            t, p = flat[pos:pos + n], G.sample_positions(n)
            assert abs(np.linalg.norm(t) - gd["norms"][i]) <= bound * gd["norms"][i], (name, key)
            assert np.linalg.norm(t[p] - gd["samples"][i]) <= bound * np.linalg.norm(gd["samples"][i]), (name, key)
    assert float(gd["norms"].min()) >= 0.04          # relative errors are meaningful on every tensor


def test_reference_properties():
    for case, shape in G.CASES:
        assert len(G.tensors(case)) == (69 if case[2] else 67)
    case, shape = G.CASES[3]
    ref = G.reference(case, shape)
    worst, _, vec = G.errors(ref["fp32"], ref["grad"], case)
    assert worst <= 1e-5 and vec <= 1e-5             # the fp32 arithmetic's own error: the GPU bounds leave > 30 x over it
    from tests import actor_train_cases as T
    assert not ref["grad"][T.stat_mask(case)].any()


def test_abi_and_python_surface():
    from tfpnp_amd import _lib, ops, torch_ops
    name = "pnpx_policy_param_grad"
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "policy_param_grad" in torch_ops.ALL_OPS and callable(ops.policy_param_grad)
    from tfpnp_amd.policy.network import ResNetActorBase
    assert callable(ResNetActorBase.param_grad) and callable(ResNetActorBase.forward_train_raw)
