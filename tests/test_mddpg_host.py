"""Host-side tests of the native MDDPG trainer (no GPU): the ABI entry and its bindings, the yardstick of tests/mddpg_cases.py
against the closed-form gradients, the argument checks that need no device, MDDPGTrainer.train()'s control flow on CPU stubs and
critic_update's optional q_target."""
import math
import os
import re
from collections import OrderedDict
from types import SimpleNamespace

import pytest
import torch

from tests import mddpg_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_binding_and_trainer_are_present():
    from tfpnp_amd import _lib, ops, torch_ops
    name = "pnpx_mddpg_policy_loss"
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert "-inf for lambda_e > 0" in header                      # what the kernel writes at p == 0 is documented
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert callable(ops.mddpg_policy_loss)
    assert "mddpg_policy_loss" in torch_ops.ALL_OPS and hasattr(torch.ops.pnpx, "mddpg_policy_loss")
    from tfpnp_amd.trainer.mddpg import MDDPGTrainer
    from tfpnp_amd.trainer.mddpg.trainer import MDDPGTrainer as direct
    assert MDDPGTrainer is direct
    for method in ("train", "_update_policy", "_update", "run_policy", "save_experience", "save_model", "load_model"):
        assert callable(getattr(MDDPGTrainer, method)), method
    src = open(os.path.join(ROOT, "tfpnp_amd", "csrc", "Makefile")).read()
    assert "mddpg_loss.hip" in src


@pytest.mark.parametrize("B,kind", [(1, "random"), (7, "random"), (64, "random"), (9, "clamp"), (5, "stopped")])
def test_restatement_autograd_equals_the_closed_forms(B, kind):
    case = M.inputs(B, 100 + B, kind)
    ref = M.restate(case, torch.float64)
    closed = M.closed_form_grads(case, ref)
    for k, want in closed.items():
        assert torch.allclose(ref[k], want, rtol=1e-13, atol=1e-15), k
    assert torch.equal(ref["grad_v_next"][case["idx_stop"] == 1], torch.zeros(int((case["idx_stop"] == 1).sum()), dtype=torch.float64))
    if kind == "clamp":                                            # the taken probability of the even rows is below eps
        p = case["p_stop"].double()
        assert (p[::2, 0] < M.EPS32).all() and (p[::2, 0] > 0).all()
        assert torch.allclose(ref["grad_p_stop"][::2, 0], M.LAMBDA_E * (torch.log(p[::2, 0]) + 1) / B, rtol=1e-13)
        assert torch.allclose(ref["log_prob"][::2], torch.full((len(p[::2]),), math.log(M.EPS32), dtype=torch.float64))
    # the bar is positive everywhere and finite
    _, bound = M.bars(case)
    assert all(bool((b > 0).all()) and bool(torch.isfinite(b).all()) for b in bound.values())


def test_argument_checks_without_a_device():
    from tfpnp_amd import ops
    from tfpnp_amd._lib import PnpxError
    case = M.inputs(4, 1)
    args = lambda **kw: [({**case, **kw})[k] for k in ("p_stop", "idx_stop", "v_cur", "v_next_target", "v_next", "reward")]
    scal = (0.99, 0.05, 0.2)
    with pytest.raises(PnpxError, match="no CPU path"):
        ops.mddpg_policy_loss(None, *args(), *scal)
    with pytest.raises(PnpxError, match="idx_stop: expected torch.int64"):
        ops.mddpg_policy_loss(None, *args(idx_stop=case["idx_stop"].int()), *scal)
    with pytest.raises(PnpxError, match="v_next: expected torch.float32"):
        ops.mddpg_policy_loss(None, *args(v_next=case["v_next"].double()), *scal)
    with pytest.raises(PnpxError, match="reward has 3 values, p_stop has 4 rows"):
        ops.mddpg_policy_loss(None, *args(reward=case["reward"][:3]), *scal)
    with pytest.raises(PnpxError, match=r"p_stop must be \[B, 2\]"):
        ops.mddpg_policy_loss(None, *args(p_stop=case["p_stop"].reshape(-1)), *scal)
    with pytest.raises(PnpxError, match="expected a torch.Tensor"):
        ops.mddpg_policy_loss(None, *args(v_cur=[0.0] * 4), *scal)
    for bad in ((math.nan, 0.05, 0.2), (0.99, math.inf, 0.2), (0.99, 0.05, -math.inf)):
        with pytest.raises(PnpxError, match="must be finite"):
            ops.mddpg_policy_loss(None, *args(), *bad)
    from tfpnp_amd import torch_ops as T
    with pytest.raises(PnpxError, match="no CPU path"):
        T.call("mddpg_policy_loss", *args(), *scal)
    # fake-tensor registration: shapes without a device
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device="cuda")
        out = torch.ops.pnpx.mddpg_policy_loss(f(5, 2), f(5, dtype=torch.int64), f(5, 1), f(5, 1), f(5, 1), f(5, 1), *scal)
    assert [tuple(o.shape) for o in out] == [(2,), (5,), (5,), (5,), (5, 2), (5,), (5,)]
    with pytest.raises(ImportError, match="tensorboardX"):
        from tfpnp_amd.trainer.mddpg import MDDPGTrainer
        MDDPGTrainer(_opt(), None, SimpleNamespace(in_dim=1), None, torch.device("cpu"), "unused", enable_tensorboard=True)


# ------------------------------------------------------------------------------------------------- train() on CPU stubs
class _StubSolver(torch.nn.Module):
    """CPU stand-in with the PnPSolver contract: x <- x + mu * (gt - x) per call."""

    def reset(self, data):
        return data['x0'].clone()

    def get_output(self, state):
        return state

    def filter_aux_inputs(self, state):
        return (state['gt'],)

    def filter_hyperparameter(self, action):
        return (action['mu'],)

    def forward(self, inputs, parameters):
        x, (gt,) = inputs
        (mu,) = parameters
        return x + mu.view(-1, 1, 1, 1) * (gt - x)


class _StubActor(torch.nn.Module):
    """Scripted stop decisions: stops[k] lists the positions (among the live rows) that stop at the k-th forward."""
    in_dim = 1

    def __init__(self, stops, events):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.stops, self.calls, self.events = stops, 0, events

    def init_state(self, B):
        return torch.zeros(B)

    def forward(self, state, idx_stop, train, hidden):
        assert not self.training and not torch.is_grad_enabled()          # run_policy: eval mode, no_grad (trainer.py:216-222)
        B = state.shape[0]
        idx = torch.zeros(B, dtype=torch.int64)
        idx[self.stops.get(self.calls, [])] = 1
        self.calls += 1
        return OrderedDict(mu=torch.full((B,), 0.5), idx_stop=idx), None, None, hidden


def _opt(**kw):
    base = dict(rmsize=8, max_episode_step=3, train_steps=10, warmup=4, validate_interval=1, save_freq=5, output=None,
                episode_train_times=2, env_batch=2, loop_penalty=0.05, discount=0.99, lambda_e=0.2, tau=0.001)
    return SimpleNamespace(**{**base, **kw})


def test_train_control_flow_on_cpu_stubs(tmp_path):
    """B = 3, max_episode_step 3, warmup 4, train_steps 10, episode_train_times 2, save_freq 5 (trainer.py:59-125 by hand):
      steps 1-3   episode 0; row 1 stops at step 1, so the observations stored hold 3, 2, 2 rows; ends by length at step 3, which is
                  not past the warm-up: no update
      steps 4-5   episode 1; every row stops at step 5: ends early, 5 > 4: _update_policy(2, 2, step=5); then reset; then, 5 % 5 == 0,
                  save_model(output, 5)
      steps 6-8   episode 2, full length: _update_policy at step 8
      steps 9-10  episode 3, cut by train_steps: no update; step 10 saves
    Rows stored: 3 + 2 + 2 + 3 + 3 + 3 * 3 + 3 + 3 = 28 into a memory of rmsize * max_episode_step = 24: full, index 28 % 24."""
    from tfpnp_amd.env import PnPEnv
    from tfpnp_amd.trainer.mddpg import MDDPGTrainer

    class Env(PnPEnv):
        policy_layout = (('variables', 'raw'),)

    events = []
    gt = torch.rand(3, 1, 8, 8)
    x0 = torch.rand(3, 1, 8, 8)
    env = Env([dict(gt=gt, x0=x0, output=x0.clone())], _StubSolver(), max_episode_step=3)
    env.metric_fn = lambda out, g: -10 * torch.log10(((out - g) ** 2).flatten(1).mean(1, keepdim=True))
    actor = _StubActor({0: [1], 4: [0, 1, 2]}, events)
    opt = _opt(output=str(tmp_path))
    lines = []
    trainer = MDDPGTrainer(opt, env, actor, lambda step: {'actor': 1e-4 * step, 'critic': 3e-4}, torch.device("cpu"), str(tmp_path),
                           logger=SimpleNamespace(log=lambda m, color=None: lines.append(m)))
    assert trainer.buffer.capacity == 24 and trainer.writer is None

    reset, step, store, update_policy, save = env.reset, env.step, trainer.save_experience, trainer._update_policy, trainer.save_model
    env.reset = lambda *a: (events.append("reset"), reset(*a))[1]
    env.step = lambda action: (events.append("step"), step(action))[1]
    trainer.save_experience = lambda ob, hidden: (events.append(("store", len(ob), len(hidden))), store(ob, hidden))[1]
    trainer._update_policy = lambda *a, **kw: (events.append(("update_policy", a, kw)), update_policy(*a, **kw))[1]
    trainer.save_model = lambda path, s=None: (events.append(("save", s)), save(path, s))[1]
    updates = []

    def recording_update(samples, lr, idx_stop=None):
        updates.append((len(samples), lr, trainer.buffer.size()))
        k = float(len(updates))
        return tuple(torch.tensor(v * k) for v in (1.0, 2.0, 3.0, 4.0, 5.0))

    trainer._update = recording_update
    trainer.train()

    rollout = lambda rows: ["step", ("store", rows, rows)]
    want = (["reset"] + rollout(3) + rollout(2) + rollout(2) + ["reset"] + rollout(3) + rollout(3)
            + [("update_policy", (2, 2), {"step": 5}), "reset", ("save", 5)] + rollout(3) + rollout(3) + rollout(3)
            + [("update_policy", (2, 2), {"step": 8}), "reset"] + rollout(3) + rollout(3) + [("save", 10)])
    assert events == want
    assert trainer.buffer.size() == 24 and trainer.buffer.index == 28 % 24
    assert set(trainer.buffer.storage) == {"gt", "variables", "T", "hidden"}
    assert [u[0] for u in updates] == [2, 2, 2, 2]                                  # env_batch rows, episode_train_times per call
    assert [u[1]['actor'] for u in updates] == [5e-4, 5e-4, 8e-4, 8e-4]             # lr_scheduler(step)
    assert [u[2] for u in updates] == [13, 13, 22, 22]                              # 3+2+2+3+3 rows, then + 9
    assert actor.training and actor.calls == 10
    assert len(lines) == 3 + 2 and "Saving model at Step_0000005" in lines[2] and "Saving model at Step_0000010" in lines[4]
    assert "RPM[13/24]" in lines[1] and "Q: 1.50" in lines[1] and "closs: 3.00" in lines[1] and "cnorm: 17.50" in lines[3]
    for name in ("actor_0000005", "critic_0000005", "actor_0000010", "critic_0000010"):
        assert os.path.exists(tmp_path / "ckpt" / (name + ".pkl")), name
    saved = torch.load(tmp_path / "ckpt" / "critic_0000010.pkl")
    from tests import critic_cases as K
    K.stand_in_module(1).load_state_dict(saved)                                     # the reference's key names and shapes
    assert list(torch.load(tmp_path / "ckpt" / "actor_0000005.pkl")) == ["w"]


# ------------------------------------------------------------------------------------------------- critic_update(q_target=)
def test_critic_update_q_target_is_optional(monkeypatch):
    from tfpnp_amd.trainer.mddpg import critic_step
    calls = {"target": 0, "soft": 0, "q": []}

    class Critic:
        def value_loss_grad(self, x, q):
            calls["q"].append(q.clone())
            return torch.tensor(0.5), torch.zeros(len(q), 1), torch.zeros(3)

        def adam_step_(self, grad, lr, max_norm):
            return torch.tensor(1.0)

    def target(x):
        calls["target"] += 1
        return torch.tensor([[2.0], [4.0]])

    monkeypatch.setattr(critic_step, "soft_update", lambda t, s, tau: calls.__setitem__("soft", calls["soft"] + 1))
    reward, stop = torch.tensor([1.0, -1.0]), torch.tensor([0, 1])
    out = critic_step.critic_update(Critic(), target, "ob", "ob2", reward, stop, 0.5, 0.001, 1e-3)
    assert calls["target"] == 1 and calls["soft"] == 1                            # today's path: the target critic is evaluated
    assert torch.equal(out["Q_target"], torch.tensor([[2.0], [-1.0]])) and torch.equal(calls["q"][0], out["Q_target"])
    given = torch.tensor([7.0, 8.0], requires_grad=True)
    out = critic_step.critic_update(Critic(), target, "ob", None, None, None, 0.5, 0.001, 1e-3, q_target=given)
    assert calls["target"] == 1 and calls["soft"] == 2                            # ... and is not when the target is handed in
    assert torch.equal(out["Q_target"], torch.tensor([[7.0], [8.0]])) and not out["Q_target"].requires_grad
    assert set(out) == {"value_loss", "critic_norm", "V_cur", "Q_target"}
