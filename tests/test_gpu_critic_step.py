"""GPU tests of the native critic update: pnpx_critic_value_loss_grad (value_loss and its backward from one forward),
pnpx_critic_adam_step (clip_grad_norm_ + Adam on the live parameter vector, csrc/critic_optim.hip) and
trainer/mddpg/critic_step.py::critic_update -- the critic's half of tfpnp/trainer/mddpg/trainer.py::_update.

The optimiser is measured against the fp64 restatement of tests/critic_step_cases.py (bounds: its module docstring; their
soundness: tests/test_critic_step_host.py), here evaluated in float64 on the device; everything the composed path of
examples/train_critic.py computes with the same fp32 steps is compared bit for bit."""
import math

import numpy as np
import pytest
import torch

from tests import critic_cases as K
from tests import critic_step_cases as S
from tests.conftest import golden

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def fresh(flat):
    from tfpnp_amd import _lib
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    num_inputs = next(c for c in (1, 9) if _lib.lib().pnpx_critic_num_params(c) == flat.numel())
    return ResNet_wobn(num_inputs, 18, 1).load_flat_(flat)


@pytest.fixture(scope="module")
def flat9():
    return g(S.flat_params(9))


@pytest.fixture(scope="module")
def grads9(flat9):
    """the first two synthetic gradients at the parameter count of num_inputs = 9 (clip active / inactive), on the device"""
    return [g(S.synthetic_gradient(flat9.numel(), k)) for k in range(2)]


def case_ob(name):
    return g(K.case_inputs(name, golden("critic_value")[f"{name}_try"])[0])


def state(net):
    m, v, t = net.optim_state(dev())
    return net.parameters_flat(dev()), m, v, t


def same_state(a, b):
    return a[3] == b[3] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["arb", "rect"])       # B = 2 and B = 3 (1 / B is not a power of two)
def test_value_loss_grad_is_the_composed_one_bit_for_bit(flat9, name):
    net = fresh(flat9)
    x = case_ob(name)
    B = x.shape[0]
    Q = torch.randn(B, 1, device=dev(), generator=torch.Generator(dev()).manual_seed(4700 + B))
    loss, V, grad = net.value_loss_grad(x, Q)
    assert V.shape == (B, 1) and loss.shape == () and grad.shape == flat9.shape
    assert torch.equal(V, net(x))
    composed = net.param_grad(x, 2.0 * (V - Q) / B)
    differ = int((grad != composed).sum())
    print(f"{name}: B {B}, loss {float(loss):.6f}, gradient elements that differ from the composed path: {differ}")
    assert torch.equal(grad, composed)
    ref = ((V - Q) ** 2).double().mean()
    err = float((loss.double() - ref).abs())
    print(f"{name}: |loss - fp64 mean| {err:.3e} (bound {B * 2.0 ** -23 * float(loss):.3e})")
    assert err <= B * 2.0 ** -23 * float(loss)
    loss2, V2, grad2 = net.value_loss_grad(x, Q.view(-1))            # [B] as well as [B, 1]; the same bytes
    assert torch.equal(loss2, loss) and torch.equal(V2, V) and torch.equal(grad2, grad)
    assert not grad.requires_grad and not loss.requires_grad


def test_opcheck_value_loss_grad(flat9):
    from tfpnp_amd import torch_ops
    assert "critic_value_loss_grad" in torch_ops.ALL_OPS
    net = fresh(flat9)
    x = case_ob("kf9")
    torch.library.opcheck(torch.ops.pnpx.critic_value_loss_grad, (x, torch.ones(1, device=dev()), net.context(dev()).cid))


# ------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("num_inputs", [1, 9])
def test_adam_steps_follow_the_fp64_restatement(num_inputs):
    p0 = g(S.flat_params(num_inputs))
    n = p0.numel()
    assert n % 4 == 2
    net, unaligned, twin = fresh(p0), fresh(p0), fresh(p0)
    ref = S.Yardstick(p0)
    buf = torch.empty(n + 1, device=dev())
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}
    for k in range(S.STEPS):
        gk = g(S.synthetic_gradient(n, k))
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
        r["norm"] = abs(float(norm) - ref.norm) / ref.norm / 1e-6
        print(f"num_inputs {num_inputs}, step {k + 1}: norm {float(norm):.6g} (fp64 {ref.norm:.9g}); |err| / bound", {q: f"{x:.4f}" for q, x in r.items()})
        worst = {q: max(worst[q], r[q]) for q in r}
        assert all(x <= 1.0 for x in r.values()), (k, r)
        assert (ref.norm > S.MAX_NORM) == (k % 2 == 0)
        assert torch.equal(norm_u, norm) and same_state(state(unaligned), st), f"step {k + 1}: the 4-byte path gives other bytes"
        assert torch.equal(norm_t, norm) and same_state(state(twin), st), f"step {k + 1}: two critics fed the same sequence differ"
    print(f"num_inputs {num_inputs}: worst |err| / bound over {S.STEPS} steps", {q: f"{x:.4f}" for q, x in worst.items()})
    p = net.parameters_flat(dev())
    assert torch.equal(p[::97], p0[::97])                           # zero gradient entries: nothing moves


# ------------------------------------------------------------------------------------------------- 3
def test_the_step_reaches_the_packed_weights(flat9, grads9):
    net = fresh(flat9)
    x = case_ob("arb")
    before = net(x)
    net.adam_step_(grads9[0], S.LR)
    after = net(x)
    assert torch.equal(after, fresh(net.parameters_flat(dev()))(x))
    assert not torch.equal(after, before)
    assert not torch.equal(net.parameters_flat(dev()), flat9)


# ------------------------------------------------------------------------------------------------- 4
def test_clip_boundary(flat9, grads9):
    g0 = grads9[0]
    inf = float("inf")
    for target, same in ((25.0, True), (100.0, False)):
        gs = g0 * (target / float(g0.double().norm()))
        a, b = fresh(flat9), fresh(flat9)
        na, nb = a.adam_step_(gs, S.LR, max_norm=50.0), b.adam_step_(gs, S.LR, max_norm=inf)
        assert torch.equal(na, nb) and abs(float(na) - target) <= 1e-5 * target
        assert same_state(state(a), state(b)) == same, target


# ------------------------------------------------------------------------------------------------- 5
def test_non_finite_gradient_changes_nothing(flat9, grads9):
    from tfpnp_amd._lib import PnpxError
    net = fresh(flat9)
    x = case_ob("arb")
    net.adam_step_(grads9[0], S.LR)
    before, V = state(net), net(x)
    assert before[3] == 1
    bad = grads9[1].clone()
    bad[12345] = float("nan")
    with pytest.raises(PnpxError, match="not finite"):
        net.adam_step_(bad, S.LR)
    assert same_state(state(net), before)
    assert torch.equal(net(x), V)
    bad[12345] = float("inf")
    with pytest.raises(PnpxError, match="not finite"):
        net.adam_step_(bad, S.LR, max_norm=float("inf"))
    assert same_state(state(net), before) and torch.equal(net(x), V)
    net.adam_step_(grads9[1], S.LR)
    after = state(net)
    assert after[3] == 2 and not torch.equal(after[0], before[0])
    # the same two finite steps without the refused ones in between
    twin = fresh(flat9)
    twin.adam_step_(grads9[0], S.LR)
    twin.adam_step_(grads9[1], S.LR)
    assert same_state(state(twin), after)


# ------------------------------------------------------------------------------------------------- 6
def test_state_lifetime(flat9, grads9):
    from tfpnp_amd import _lib, ops
    from tfpnp_amd._lib import PnpxError
    net = fresh(flat9)
    zero = net.optim_state(dev())
    assert zero[2] == 0 and not zero[0].any() and not zero[1].any()               # before the first step
    net.adam_step_(grads9[0], S.LR)
    net.adam_step_(grads9[1], S.LR)
    _, m, v, t = state(net)
    assert t == 2 and m.any() and v.any()
    net.load_flat_(flat9)                                                         # a refresh of the same critic keeps the state
    assert same_state(state(net), (flat9, m, v, 2))
    net.soft_update_(flat9 * 1.5, 0.25)
    m2, v2, t2 = net.optim_state(dev())
    assert t2 == 2 and torch.equal(m2, m) and torch.equal(v2, v)
    net.reset_optim_()
    m3, v3, t3 = net.optim_state(dev())
    assert t3 == 0 and not m3.any() and not v3.any()
    net.adam_step_(grads9[0], S.LR)
    assert net.optim_state(dev())[2] == 1
    # a step before any load
    empty = ops.Context(dev())
    with pytest.raises(PnpxError, match="no critic loaded"):
        empty.critic_adam_step(grads9[0], S.LR)
    lib = _lib.lib()
    call = lambda c, nn, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, mx=50.0: lib.pnpx_critic_adam_step(
        c.handle, ops._p(grads9[0]), nn, lr, b1, b2, eps, mx, None, ops._stream(grads9[0]))
    n = flat9.numel()
    assert call(empty, n) == 3                                                    # PNPX_ERR_NO_WEIGHTS
    # the library's own argument checks, past the Python guards: PNPX_ERR_ARG, nothing changed
    ctx = net.context(dev())
    before = state(net)
    for bad in (dict(nn=n - 1), dict(lr=-1.0), dict(lr=math.inf), dict(b1=1.0), dict(b2=-0.5), dict(eps=0.0), dict(mx=0.0), dict(mx=math.nan)):
        assert call(ctx, **{"nn": n, **bad}) == 1, bad
    assert same_state(state(net), before)
    assert call(ctx, n, mx=math.inf) == 0 and net.optim_state(dev())[2] == 2      # grad_norm_dev may be NULL


# ------------------------------------------------------------------------------------------------- 7
def test_critic_update_teacher_forced(flat9):
    from tfpnp_amd.trainer.mddpg.critic_step import critic_update
    rs = np.random.RandomState(4800)
    B, tau, lr, discount = 2, 0.001, 1e-4, K.DISCOUNT
    ob, ob2 = g(rs.uniform(0, 1, (B, 9, 64, 64)).astype(np.float32)), g(rs.uniform(0, 1, (B, 9, 64, 64)).astype(np.float32))
    reward = g(rs.standard_normal((B, 1)).astype(np.float32))
    idx_stop = g(np.array([0, 1], np.int64))
    critic, target = fresh(flat9), fresh(flat9)
    cg_max = torch.zeros(flat9.numel(), device=dev(), dtype=torch.float64)
    for it in range(3):
        p, m, v, t = state(critic)
        tp = target.parameters_flat(dev())
        assert t == it
        Q = discount * (1 - idx_stop.reshape(-1, 1).float()) * target(ob2) + reward
        V = critic(ob)
        grad = critic.param_grad(ob, 2.0 * (V - Q) / B)
        out = critic_update(critic, target, ob, ob2, reward, idx_stop, discount, tau, lr)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in out.values()) and set(out) == {"value_loss", "critic_norm", "V_cur", "Q_target"}
        assert torch.equal(out["Q_target"], Q) and torch.equal(out["V_cur"], V)
        p64, m64, v64, norm, c = S.adam_ref(p, m, v, t + 1, grad, lr, max_norm=50.0)
        cg_max = torch.maximum(cg_max, (grad.double() * c).abs())
        p_new, m_new, v_new, t_new = state(critic)
        assert t_new == it + 1
        r = S.bound_ratios(p_new.double() - p64, m_new.double() - m64, v_new.double() - v64, p64, cg_max, 1, lr)
        print(f"critic_update {it}: value_loss {float(out['value_loss']):.6f}, norm {float(out['critic_norm']):.5g} (fp64 {norm:.8g}); "
              "|err| / bound", {q: f"{x:.4f}" for q, x in r.items()})
        assert all(x <= 1.0 for x in r.values()), (it, r)
        assert abs(float(out["critic_norm"]) - norm) <= 1e-6 * norm
        assert torch.equal(target.parameters_flat(dev()), tp * (1.0 - tau) + p_new * tau)
    assert math.isfinite(float(out["value_loss"]))


def test_example_runs_in_both_modes():
    """examples/train_critic.py: the native path (critic_update) and the composed path it is timed against start from the same
    loss and stay finite."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_critic.py")
    spec = importlib.util.spec_from_file_location("example_train_critic", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    quiet = lambda *a: None
    native, critic, target = mod.run(steps=2, B=2, H=64, native=True, log=quiet)
    composed, _, _ = mod.run(steps=2, B=2, H=64, native=False, log=quiet)
    print("example: native", native, "composed", composed)
    assert len(native) == len(composed) == 2 and np.all(np.isfinite(native)) and np.all(np.isfinite(composed))
    assert abs(native[0] - composed[0]) <= 1e-6 * abs(composed[0])
    assert critic.optim_state(dev())[2] == 2 and target.optim_state(dev())[2] == 0
