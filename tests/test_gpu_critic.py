"""GPU tests of the native value network (csrc/critic.hip): forward and input gradient against the executed reference
critic (tests/golden/critic_value.npz) and the fp64 restatement of tests/critic_cases.py, the adjoint of the observation
pack, and the DDPG value term CSMRIEnv.forward -> get_eval_ob -> critic differentiated into the policy logits
(tfpnp/trainer/mddpg/trainer.py:171-192).

Measured on an MI355X (half-split instances), next to the bounds asserted below:
  V vs the reference:            kf9 9.5e-7, kf17 2.4e-7, arb 4.3e-6, rect 5.7e-6 -- bound 2e-5 * max(1, |V|); ddpg 4.8e-7 (bound 1e-3)
  input gradient vs reference:   kf9 1.06e-6, kf17 9.7e-7 relative L2 (bound 1e-3);  arb 1.3e-6 (bound 2e-2)
  6 x 9 x 256 x 256 vs fp64:     max |dV| 8.7e-6 at V = 16.0 (bound 2e-5 * max(1, |V|) = 3.2e-4)
  DDPG value term (|g| 0.175):   vs restatement autograd on the GPU tensors 7.8e-7 (bound 2e-2), vs the reference 2.0e-3 (bound 0.25)
"""
import os
import sys

import numpy as np
import pytest
import torch

from tests import critic_cases as K
from tests.conftest import golden
from tests.golden_inputs import GRAD_CASE
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def g(a, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return x.requires_grad_(True) if grad else x


def v_bound(ref):
    return 2e-5 * np.maximum(1.0, np.abs(ref))


@pytest.fixture(scope="module")
def critics():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    made = {}

    def get(num_inputs):
        if num_inputs not in made:
            made[num_inputs] = ResNet_wobn(num_inputs, 18, 1, state_dict=K.critic_params(num_inputs))
        return made[num_inputs]
    return get


@pytest.mark.parametrize("name", ["kf9", "kf17", "arb", "rect"])
def test_value_golden(critics, name):
    gd = golden("critic_value")
    ob, _ = K.case_inputs(name, gd[f"{name}_try"])
    V = critics(K.CASES[name][0])(g(ob)).cpu().numpy()
    ref = gd[f"{name}_V"]
    print(f"{name}: V {ref.ravel()}  max|dV| {np.abs(V - ref).max():.2e}  (reference fp32-vs-fp64 {float(gd[name + '_ref_dV']):.2e})")
    assert V.shape == ref.shape == (K.CASES[name][1], 1)
    assert np.all(np.abs(V - ref) <= v_bound(ref))


@pytest.mark.parametrize("name,bound", [("kf9", 1e-3), ("kf17", 1e-3), ("arb", 2e-2)])
def test_input_gradient_golden(critics, name, bound):
    """Against the reference's autograd.  Kink-free cases: 1e-3, the bound of the kink-free VJP test on the half-split
    instances; arbitrary case: the project's kink-flip bound."""
    gd = golden("critic_value")
    ob, w = K.case_inputs(name, gd[f"{name}_try"])
    x = g(ob, True)
    V = critics(K.CASES[name][0])(x)
    assert V.requires_grad
    (V[:, 0] * g(w)).sum().backward()
    e = K.rel_l2(x.grad.cpu().numpy(), gd[f"{name}_grad"])
    print(f"{name}: input gradient rel-L2 vs reference autograd {e:.2e} (bound {bound:g})")
    assert e < bound


def test_full_size_vs_restatement_and_determinism(critics):
    from tfpnp_amd import ops
    net = critics(9)
    ctx = net.context(dev())
    ob = K.big_inputs()
    V = ops.critic_forward(ctx, g(ob))
    ref = K.restate(K.critic_params(9), ob[:2], torch.float64).numpy()
    err = np.abs(V[:2].cpu().numpy() - ref)
    print(f"6x9x256x256: V {ref.ravel()}  max|dV| vs fp64 restatement {err.max():.2e}")
    assert np.all(err <= v_bound(ref))
    gv = g(np.array([1.0, -2.0, 0.5, 3.0, 1.5, -1.0], np.float32))
    G = ops.critic_backward(ctx, g(ob), gv)
    # batch independence, repeatability, workspace reuse with a smaller batch and another size in between
    assert torch.equal(ops.critic_forward(ctx, g(ob[4:5])), V[4:5])
    assert torch.equal(ops.critic_backward(ctx, g(ob[4:5]), gv[4:5]), G[4:5])
    ops.critic_forward(ctx, g(K.case_inputs("rect", 0)[0]))
    assert torch.equal(ops.critic_forward(ctx, g(ob)), V)
    assert torch.equal(ops.critic_backward(ctx, g(ob), gv), G)
    torch.cuda.synchronize()
    assert not ctx.range_tripped()      # neither pass left the half-split range


def test_gradient_is_linear_in_grad_value(critics):
    from tfpnp_amd import ops
    ctx = critics(9).context(dev())
    ob = g(K.case_inputs("rect", 0)[0])
    gv = g(np.array([0.7, 0.0, -1.3], np.float32))
    G = ops.critic_backward(ctx, ob, gv)
    assert float(G[1].abs().max()) == 0.0 and float(G[0].abs().max()) > 0 and float(G[2].abs().max()) > 0
    assert torch.equal(ops.critic_backward(ctx, ob, 2 * gv), 2 * G)
    one = ops.critic_backward(ctx, ob, torch.ones_like(gv))
    assert K.rel_l2((one * gv.view(-1, 1, 1, 1)).cpu().numpy(), G.cpu().numpy()) < 1e-6


LAYOUTS = {   # (shape tail, kind) per entry: the CS-MRI and PR observations
    "csmri": [((3, 2), 1), ((1, 2), 2), ((1, 2), 1), ((1,), 0), ((1,), 0), ((1, 2), 1)],
    "pr": [((3, 2), 1), ((4,), 0), ((4, 2), 2), ((1,), 0), ((1,), 0)],
}


def _entries(layout, B, H, W, seed, grad):
    rs = np.random.RandomState(seed)
    out = []
    for tail, _ in LAYOUTS[layout]:
        shape = (B, tail[0], H, W) + ((2,) if len(tail) == 2 else ())
        out.append(g(rs.standard_normal(shape).astype(np.float32), grad))
    return out


@pytest.mark.parametrize("layout", ["csmri", "pr"])
def test_pack_unpack_are_adjoint(layout):
    """<pack(x), g> == <x, unpack(g)> to fp32 rounding (both sides summed in fp64: pure data movement)."""
    from tfpnp_amd import ops, torch_ops  # noqa: F401
    B, H, W = 3, 32, 64
    xs = _entries(layout, B, H, W, 5, False)
    kinds = [k for _, k in LAYOUTS[layout]]
    names = {0: "raw", 1: "real", 2: "channel"}
    packed = ops.policy_ob_pack([(x, names[k]) for x, k in zip(xs, kinds)])
    assert packed.shape[1] == (9 if layout == "csmri" else 17)
    gr = g(np.random.RandomState(6).standard_normal(tuple(packed.shape)).astype(np.float32))
    back = ops.policy_ob_unpack(gr, kinds, [x.shape[1] for x in xs])
    lhs = float((packed.double() * gr.double()).sum())
    rhs = sum(float((x.double() * b.double()).sum()) for x, b in zip(xs, back))
    print(f"{layout}: <pack x, g> {lhs:.9e}  <x, unpack g> {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-6 * max(1.0, abs(lhs))
    for b, k in zip(back, kinds):
        if k == 1:
            assert float(b[..., 1].abs().max()) == 0.0
    # the differentiable op returns the same tensor and the same gradients
    leaves = [x.clone().requires_grad_(True) for x in xs]
    out = torch.ops.pnpx.policy_ob_pack_diff(leaves, kinds)
    assert torch.equal(out, packed)
    out.backward(gr)
    assert all(torch.equal(l.grad, b) for l, b in zip(leaves, back))


def test_opcheck_new_ops(critics):
    from tfpnp_amd import torch_ops  # noqa: F401
    cid = critics(9).context(dev()).cid
    ob = g(K.case_inputs("kf9", 0)[0], True)
    # piecewise-linear network on deterministic kernels: eager and AOT runs agree exactly
    torch.library.opcheck(torch.ops.pnpx.critic_value, (ob, cid))
    torch.library.opcheck(torch.ops.pnpx.critic_backward, (ob.detach(), g(np.ones(1, np.float32)), cid))
    xs = _entries("csmri", 2, 32, 32, 7, True)
    kinds = [k for _, k in LAYOUTS["csmri"]]
    torch.library.opcheck(torch.ops.pnpx.policy_ob_pack_diff, (xs, kinds))
    gr = torch.randn(2, 9, 32, 32, device=dev())
    torch.library.opcheck(torch.ops.pnpx.policy_ob_unpack, (gr, kinds, [x.shape[1] for x in xs]))
    mask = torch.ones(2, 1, 32, 32, device=dev(), dtype=torch.bool)   # a bool entry gets no gradient
    out = torch.ops.pnpx.policy_ob_pack_diff([xs[0], mask], [1, 0])
    out.sum().backward()
    assert out.shape[1] == 4 and xs[0].grad is not None


def test_rejections(critics):
    from tfpnp_amd import ops
    from tfpnp_amd._lib import PnpxError
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    ctx = critics(9).context(dev())
    ob = lambda c, h, w: np.zeros((1, c, h, w), np.float32)
    with pytest.raises(PnpxError, match="multiples of 32"):
        ops.critic_forward(ctx, g(ob(9, 48, 64)))
    with pytest.raises(PnpxError, match="multiples of 32"):
        ops.critic_backward(ctx, g(ob(9, 64, 16)), g(np.ones(1, np.float32)))
    with pytest.raises(PnpxError, match="channel count"):
        ops.critic_forward(ctx, g(ob(8, 64, 64)))
    with pytest.raises(PnpxError):
        ops.critic_forward(ctx, torch.from_numpy(ob(9, 64, 64)))          # CPU tensor
    empty = ops.Context(dev())
    with pytest.raises(PnpxError, match="no critic loaded"):
        ops.critic_forward(empty, g(ob(9, 64, 64)))
    empty._critic = 9                                                        # past the Python guard: the library's own check
    with pytest.raises(PnpxError, match="before pnpx_critic_load"):
        ops.critic_forward(empty, g(ob(9, 64, 64)))
    bad = dict(K.critic_params(9))
    del bad["layer3.1.relu_2.alpha"]
    with pytest.raises(PnpxError, match="layer3.1.relu_2.alpha"):
        ResNet_wobn(9, 18, 1, state_dict=bad).context(dev())


def test_load_accepts_the_parametrization_spelling(critics):
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    sd = {k.replace(".weight_g", ".parametrizations.weight.original0").replace(".weight_v", ".parametrizations.weight.original1"):
          torch.from_numpy(v) for k, v in K.critic_params(9).items()}
    ob = g(K.case_inputs("kf9", 0)[0])
    assert torch.equal(ResNet_wobn(9, 18, 1, state_dict=sd)(ob), critics(9)(ob))


def _ddpg_chain(unet_params, value_fn):
    """(V(ob2), reward, d value term / d raw) of the ddpg case with the critic evaluated by value_fn(eval_ob2)."""
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.tasks import csmri
    C = GRAD_CASE
    sol = csmri.ADMMSolver_CSMRI(UNetDenoiser2D(state_dict=unet_params))
    d = synth.make_csmri_batch(C.env_B, C.env_H, C.env_W, seed=C.env_data_seed)
    env = csmri.CSMRIEnv(None, sol, max_episode_step=6)
    ob = env.reset({k: g(v) for k, v in d.items() if isinstance(v, np.ndarray)})
    raw = g(np.random.RandomState(C.env_raw_seed).standard_normal((C.env_B, 10)).astype(np.float32), True)
    ob2, reward = env.forward(ob, {"sigma_d": torch.sigmoid(raw[:, :5]) * 70 / 255, "mu": torch.sigmoid(raw[:, 5:])})
    eval_ob2 = env.get_eval_ob(ob2)
    assert eval_ob2.requires_grad and eval_ob2.shape[1] == 9
    V = value_fn(eval_ob2)
    idx_stop = torch.tensor([0, 1], device=dev())
    term = ((K.DISCOUNT * (1 - idx_stop.float())).unsqueeze(-1) * V).mean()
    grad, = torch.autograd.grad(term, raw)
    return V.detach(), reward.detach(), grad


def test_ddpg_value_term(critics, unet_params):
    """The value term on its own (its gradient is 30 times smaller than the reward term's: a test on the sum would not see it)."""
    gd = golden("critic_value")
    V, reward, grad = _ddpg_chain(unet_params, critics(9))
    params = K.critic_params(9)
    V_r, _, grad_r = _ddpg_chain(unet_params, lambda x: K.restate(params, x, torch.float32))
    ref_V = gd["ddpg_V"]
    dV = np.abs(V.cpu().numpy() - ref_V)
    print(f"ddpg: V {V.flatten().tolist()} (reference {ref_V.ravel()}), max|dV| {dV.max():.2e}; reward {reward.flatten().tolist()}")
    assert np.all(dV <= 1e-3 * np.maximum(1.0, np.abs(ref_V)))                               # (d)
    e_a = K.rel_l2(grad.cpu().numpy(), grad_r.cpu().numpy())
    e_b = K.rel_l2(grad.cpu().numpy(), gd["ddpg_grad_value_raw"])
    print(f"ddpg: value-term gradient |g| {float(grad.norm()):.4f}: vs restatement autograd {e_a:.2e} (2e-2), vs reference {e_b:.2e} (0.25)")
    assert e_a < 2e-2                                                                        # (a)
    assert e_b < 0.25                                                                        # (b)
    assert float(grad[1].abs().max()) == 0.0 and float(grad[0].abs().max()) > 0              # (c)


def test_eval_ob_carries_grad_only_when_asked(unet_params):
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.tasks import csmri
    env = csmri.CSMRIEnv(None, csmri.ADMMSolver_CSMRI(UNetDenoiser2D(state_dict=unet_params)), max_episode_step=6)
    d = synth.make_csmri_batch(2, 32, 32, seed=3)
    ob = env.reset({k: g(v) for k, v in d.items() if isinstance(v, np.ndarray)})
    plain = env.get_eval_ob(ob)
    assert not plain.requires_grad and plain.grad_fn is None
    ob.variables = ob.variables.clone().requires_grad_(True)
    diff = env.get_eval_ob(ob)
    assert diff.requires_grad and torch.equal(diff.detach(), plain)
    with torch.no_grad():
        assert not env.get_eval_ob(ob).requires_grad


def test_train_bridge_with_value_term(critics):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_bridge
    grads = {}

    def grab(key):
        def f(it, actor):
            grads[key] = torch.cat([p.grad.flatten().clone() for p in actor.parameters()])
        return f
    h0 = train_bridge.train(steps=1, B=2, H=64, action_pack=3, log=lambda *_: None, after_backward=grab("reward"))
    h1 = train_bridge.train(steps=1, B=2, H=64, action_pack=3, log=lambda *_: None, critic=critics(9), discount=0.99,
                            after_backward=grab("both"))
    assert h0 == h1 and all(v == v for v in h1)
    diff = float((grads["both"] - grads["reward"]).norm())
    print(f"actor gradient: reward term {float(grads['reward'].norm()):.3e}, value term contributes {diff:.3e}")
    assert torch.isfinite(grads["both"]).all() and diff > 1e-6 * float(grads["reward"].norm()) and diff > 0
