"""GPU tests of the native MDDPG trainer: pnpx_mddpg_policy_loss (csrc/mddpg_loss.hip) against the float64 restatement of
tests/mddpg_cases.py (the bar: its module docstring), torch.ops.pnpx.mddpg_policy_loss, and MDDPGTrainer -- `_update` against the
composed path on twins, the checkpoint round trip, ten updates on one batch and examples/train_mddpg.py."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import actor_cases as A
from tests import actor_train_cases as TC
from tests import critic_cases as K
from tests import mddpg_cases as M
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("q_target", "log_prob", "entropy", "scalars", "grad_p_stop", "grad_v_next", "grad_reward")
KEYS = ("p_stop", "idx_stop", "v_cur", "v_next_target", "v_next", "reward")
SCAL = (M.DISCOUNT, M.LOOP_PENALTY, M.LAMBDA_E)


def dev():
    return torch.device("cuda:0")


def run_kernel(case, offset=False):
    """ops.mddpg_policy_loss on `case`; offset: every input lives 4 bytes (idx_stop: 8, its natural alignment) past a 16-byte
    boundary -- the outputs are fresh allocations either way, so they are compared through a second, shifted set of views"""
    from tfpnp_amd import ops
    if not offset:
        args = [case[k].to(dev()) for k in KEYS]
    else:
        args = []
        for k in KEYS:
            t = case[k]
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev())
            view = buf[1:].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == t.element_size()
            args.append(view)
    return dict(zip(NAMES, ops.mddpg_policy_loss(None, *args, *SCAL)))


def as_outputs(got):
    out = {k: got[k] for k in NAMES if k != "scalars"}
    out["policy_loss"], out["mean_entropy"] = got["scalars"][0], got["scalars"][1]
    return out


def check_against_bar(got, case, label):
    ref, bound = M.bars(case)
    ratios = {k: M.worst_ratio(as_outputs(got)[k], ref[k], bound[k]) for k in M.OUTPUTS}
    print(f"{label}: worst |kernel - fp64| / bar", {k: f"{r:.3f}" for k, r in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), (label, ratios)
    return ratios


# ------------------------------------------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 256, 257, 1000])
def test_kernel_meets_the_bar(B):
    case = M.inputs(B, 7000 + B)
    if B > 1:
        assert set(case["idx_stop"].tolist()) == {0, 1}
    got = run_kernel(case)
    check_against_bar(got, case, f"B {B}")
    stopped = (case["idx_stop"] == 1).to(dev())
    assert not got["grad_v_next"][stopped].any()                                   # exactly zero where the episode ended
    again, shifted = run_kernel(case), run_kernel(case, offset=True)
    for k in NAMES:
        assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
        assert torch.equal(got[k], shifted[k]), f"{k}: depends on the alignment of the inputs"


def test_kernel_clamp_branch_and_all_stopped():
    B = 65
    case = M.inputs(B, 7100, "clamp")
    got = run_kernel(case)
    check_against_bar(got, case, "clamp")
    p = case["p_stop"].double()
    want = M.LAMBDA_E * (torch.log(p[::2, 0]) + 1) / B                             # entropy part only: zero a2c gradient
    assert torch.allclose(got["grad_p_stop"][::2, 0].double().cpu(), want, rtol=1e-6, atol=0)
    assert torch.equal(got["log_prob"][::2].cpu(), torch.full((33,), float(np.float32(np.log(np.float64(M.EPS32))))))   # log(eps), rounded once
    case = M.inputs(B, 7200, "stopped")
    got = run_kernel(case)
    check_against_bar(got, case, "stopped")
    assert not got["grad_v_next"].any()
    assert torch.equal(got["q_target"].cpu(), case["reward"] - M.LOOP_PENALTY)


def test_kernel_output_pointers_offset_and_bad_arguments():
    """The library entry itself: outputs 4 bytes past a 16-byte boundary give the same bytes; B <= 0, a null pointer and a scalar
    that is not finite return PNPX_ERR_ARG and write nothing."""
    from tfpnp_amd import _lib, ops
    B = 257
    case = M.inputs(B, 7300)
    want = run_kernel(case)
    ins = [case[k].to(dev()) for k in KEYS]
    sizes = dict(q_target=B, log_prob=B, entropy=B, scalars=2, grad_p_stop=2 * B, grad_v_next=B, grad_reward=B)
    bufs = {k: torch.full((n + 1,), -7.5, device=dev()) for k, n in sizes.items()}
    outs = {k: b[1:] for k, b in bufs.items()}
    assert all(o.data_ptr() % 16 == 4 for o in outs.values())
    ctx = ops.default_context(dev())
    call = lambda B_=B, scal=SCAL, skip=None: _lib.lib().pnpx_mddpg_policy_loss(
        ctx.handle, *(ops._p(t) for t in ins), *scal, B_, *(None if k == skip else ops._p(o) for k, o in outs.items()), ops._stream(ins[0]))
    for bad in (dict(B_=0), dict(B_=-3), dict(scal=(float("nan"), 0.05, 0.2)), dict(scal=(0.99, float("inf"), 0.2)),
                dict(scal=(0.99, 0.05, float("-inf"))), dict(skip="scalars"), dict(skip="grad_p_stop")):
        assert call(**bad) == 1, bad
    torch.cuda.synchronize()
    assert all(bool((b == -7.5).all()) for b in bufs.values())
    assert call() == 0
    for k in NAMES:
        assert torch.equal(outs[k].view(want[k].shape), want[k]), k
        assert float(bufs[k][0]) == -7.5


# ------------------------------------------------------------------------------------------------- 2: the dispatcher op
def test_opcheck_and_autograd():
    from tfpnp_amd import torch_ops
    assert "mddpg_policy_loss" in torch_ops.ALL_OPS                                # (the import registers torch.ops.pnpx.*)
    case = M.inputs(9, 7400)
    x = {k: case[k].to(dev()) for k in KEYS}
    x["v_next"], x["reward"] = x["v_next"].view(-1, 1), x["reward"].view(-1, 1)     # [B, 1], as the critic and the env return them
    leaves = [x[k].requires_grad_() for k in ("p_stop", "v_next", "reward")]
    args = tuple(x[k] for k in KEYS) + SCAL
    torch.library.opcheck(torch.ops.pnpx.mddpg_policy_loss, args)
    out = torch.ops.pnpx.mddpg_policy_loss(*args)
    scalars, rest = out[0], out[1:]
    assert scalars.requires_grad and not any(t.requires_grad for t in rest)
    direct = run_kernel(case)
    for k, t in zip(("scalars", "q_target", "log_prob", "entropy", "grad_p_stop", "grad_v_next", "grad_reward"), out):
        assert torch.equal(t.detach(), direct[k]), k
    grads = torch.autograd.grad(scalars[0], leaves, retain_graph=True)
    assert [g.shape for g in grads] == [x.shape for x in leaves]
    for g, k in zip(grads, ("grad_p_stop", "grad_v_next", "grad_reward")):
        assert torch.equal(g.reshape(direct[k].shape), direct[k]), k                # bit for bit
    twice = torch.autograd.grad(2.0 * scalars[0], leaves, retain_graph=True)
    for g2, g in zip(twice, grads):
        assert torch.equal(g2, 2.0 * g)                                             # exactly homogeneous
    none = torch.autograd.grad(scalars[1], leaves, allow_unused=True)               # mean entropy: a diagnostic, no gradient
    assert all(g is None or not bool(g.any()) for g in none)


# ------------------------------------------------------------------------------------------------- trainer fixtures
CASE = (9, 10, False)          # ResNetActor_ADMM, action bundle 5
B, H = 4, 64


def make_opt(**kw):
    base = dict(rmsize=8, max_episode_step=3, train_steps=9, warmup=3, validate_interval=10, save_freq=10 ** 9, output=None,
                episode_train_times=1, env_batch=B, loop_penalty=M.LOOP_PENALTY, discount=M.DISCOUNT, lambda_e=M.LAMBDA_E, tau=0.01, seed=3)
    return SimpleNamespace(**{**base, **kw})


@pytest.fixture(scope="module")
def world():
    """(env, the observation batch of a reset: B = 4, 9 policy channels, 64 x 64) -- built once, read only"""
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.tasks import csmri
    den = UNetDenoiser2D(state_dict=synth.make_unet_params(0))
    data = synth.make_csmri_batch(B, H, H, ratio=4, sigma_n=15.0, seed=11)
    loader = [{k: torch.from_numpy(v) for k, v in data.items() if hasattr(v, "dtype")}]
    env = csmri.CSMRIEnv(loader, csmri.ADMMSolver_CSMRI(den), max_episode_step=3).to(dev())
    ob = env.reset()
    ob["hidden"] = torch.zeros(B, device=dev())
    return env, ob


def make_trainer(env, tmp, **kw):
    from tfpnp_amd.trainer.mddpg import MDDPGTrainer
    actor = A.native_actor(CASE, synth.make_policy_params(*CASE, seed=5))
    quiet = SimpleNamespace(log=lambda m, color=None: None)
    return MDDPGTrainer(make_opt(output=str(tmp), **kw), env, actor, lambda step: {'actor': 1e-3, 'critic': 1e-3}, dev(), str(tmp), logger=quiet)


def full_state(net):
    m, v, t = net.optim_state(dev())
    return net.parameters_flat(dev()), m, v, t


def same_state(a, b):
    return a[3] == b[3] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------------------------------------- 3: _update, teacher-forced
def test_update_teacher_forced_against_the_composed_path(world, tmp_path, monkeypatch):
    from tfpnp_amd import torch_ops as T
    from tfpnp_amd.trainer.mddpg import trainer as trainer_mod
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    from tfpnp_amd.trainer.mddpg.critic_step import critic_update
    env, ob = world
    tr = make_trainer(env, tmp_path)
    idx_stop = torch.tensor([0, 1, 1, 0], device=dev())
    lr = {'actor': 1e-3, 'critic': 2e-3}
    # twins built from the same vectors
    twin_actor = A.native_actor(CASE).load_flat_(tr.actor.parameters_flat(dev()))
    twin_critic = ResNet_wobn(9, 18, 1).load_flat_(tr.critic.parameters_flat(dev()))
    twin_target = ResNet_wobn(9, 18, 1).load_flat_(tr.critic_target.parameters_flat(dev()))
    assert torch.equal(tr.critic_target.parameters_flat(dev()), tr.critic.parameters_flat(dev()))      # hard_update of the constructor

    seen = {"target_calls": 0}
    real_call = T.call

    def spy_call(name, *args):
        out = real_call(name, *args)
        if name == "mddpg_policy_loss":
            seen["loss_in"], seen["loss_out"] = [a.detach().clone() if isinstance(a, torch.Tensor) else a for a in args], out
        return out

    monkeypatch.setattr(trainer_mod.T, "call", spy_call)
    kept = tr.actor.param_grad_kept

    def spy_kept(gp, gd):
        seen["gp"], seen["gd"], seen["grad"] = gp.clone(), gd.clone(), kept(gp, gd)
        return seen["grad"]

    tr.actor.param_grad_kept = spy_kept
    target_forward = tr.critic_target.forward

    def counting_target(x):
        seen["target_calls"] += 1
        seen["eval_ob2"] = x.detach().clone()
        return target_forward(x)

    tr.critic_target.forward = counting_target
    real_critic_update = trainer_mod.critic_update

    def spy_critic_update(*a, **kw):
        seen["eval_ob"] = a[2]
        return real_critic_update(*a, **kw)

    monkeypatch.setattr(trainer_mod, "critic_update", spy_critic_update)

    Q, value_loss, entropy, actor_norm, critic_norm = tr._update(ob, lr, idx_stop=idx_stop)
    for x in (Q, value_loss, entropy, actor_norm, critic_norm):
        assert isinstance(x, torch.Tensor) and x.is_cuda and x.numel() == 1 and not x.requires_grad and bool(torch.isfinite(x))
    assert seen["target_calls"] == 1                                                # (c)

    # (a) the loss launch against the restatement fed the spied inputs
    p_stop, idx, v_cur, v_nt, v_next, reward = seen["loss_in"][:6]
    assert torch.equal(idx, idx_stop) and tuple(seen["loss_in"][6:]) == SCAL
    case = dict(p_stop=p_stop.cpu(), idx_stop=idx.cpu(), v_cur=v_cur.cpu().view(-1), v_next_target=v_nt.cpu().view(-1),
                v_next=v_next.cpu().view(-1), reward=reward.cpu().view(-1))
    scalars, q, logp, ent, gp, gv, gr = seen["loss_out"]
    got = dict(scalars=scalars.detach(), q_target=q, log_prob=logp, entropy=ent, grad_p_stop=gp, grad_v_next=gv, grad_reward=gr)
    check_against_bar(got, case, "_update")
    assert torch.equal(Q, -scalars[0].detach()) and torch.equal(entropy, scalars[1].detach())
    assert torch.equal(seen["gp"], gp)                                              # p_stop reaches the loss through the launch only
    assert bool(seen["gd"].any()) and bool(torch.isfinite(seen["gd"]).all())        # the deterministic actions got their gradient

    # (b) given the spied gradients, everything else is the composed path on the twins, bit for bit
    policy_ob = env.get_policy_ob(ob)
    twin_actor.forward_train_keep(policy_ob)                                        # the running statistics move
    grad = twin_actor.param_grad_kept(seen["gp"], seen["gd"])
    assert torch.equal(grad, seen["grad"])
    norm_a = twin_actor.adam_step_(grad, lr['actor'], max_norm=50)
    assert torch.equal(norm_a, actor_norm) and same_state(full_state(twin_actor), full_state(tr.actor))
    mask = TC.stat_mask(CASE).to(dev())
    before = A.native_actor(CASE, synth.make_policy_params(*CASE, seed=5)).parameters_flat(dev())
    assert not torch.equal(tr.actor.parameters_flat(dev())[mask], before[mask])     # running statistics moved, identically (above)
    # the critic's half as it was before q_target existed: critic_update evaluates the twin target itself (trainer.py:174, :180-186)
    out = critic_update(twin_critic, twin_target, seen["eval_ob"], seen["eval_ob2"], reward.view(-1) - M.LOOP_PENALTY, idx_stop,
                        M.DISCOUNT, 0.01, lr['critic'])
    assert torch.equal(out["Q_target"].view(-1), q)                                 # the kernel's target has torch's bytes
    assert torch.equal(out["value_loss"], value_loss) and torch.equal(out["critic_norm"], critic_norm)
    assert same_state(full_state(twin_critic), full_state(tr.critic))
    assert torch.equal(twin_target.parameters_flat(dev()), tr.critic_target.parameters_flat(dev()))    # the soft-updated target
    assert not torch.equal(twin_target.parameters_flat(dev()), twin_critic.parameters_flat(dev()))
    assert tr.actor.optim_state(dev())[2] == 1 and tr.critic.optim_state(dev())[2] == 1


# ------------------------------------------------------------------------------------------------- 4: checkpoints
def test_checkpoint_round_trip(world, tmp_path):
    env, ob = world
    tr = make_trainer(env, tmp_path)
    tr._update(ob, {'actor': 1e-3, 'critic': 1e-3}, idx_stop=torch.tensor([0, 1, 0, 1], device=dev()))   # live, stepped weights
    tr.save_model(str(tmp_path))
    tr.save_model(str(tmp_path), 12)
    tr.save_model(str(tmp_path), "best")
    ckpt = tmp_path / "ckpt"
    assert sorted(os.listdir(ckpt)) == sorted(f"{n}{p}.pkl" for n in ("actor", "critic") for p in ("", "_0000012", "_best"))
    fresh = make_trainer(env, tmp_path / "other")
    assert not torch.equal(fresh.actor.parameters_flat(dev()), tr.actor.parameters_flat(dev()))
    target_before = fresh.critic_target.parameters_flat(dev())
    fresh.load_model(str(ckpt), 12)
    assert fresh.start_step == 12
    assert torch.equal(fresh.actor.parameters_flat(dev()), tr.actor.parameters_flat(dev()))
    assert torch.equal(fresh.critic.parameters_flat(dev()), tr.critic.parameters_flat(dev()))
    assert torch.equal(fresh.critic_target.parameters_flat(dev()), target_before)   # as in the reference: load_model leaves the target
    fresh.load_model(str(ckpt))
    assert torch.equal(fresh.critic.parameters_flat(dev()), tr.critic.parameters_flat(dev()))
    # the stand-in torch modules take the files
    sd = torch.load(ckpt / "actor.pkl")
    missing, unexpected = A.stand_in_actor(*CASE).load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    K.stand_in_module(9).load_state_dict(torch.load(ckpt / "critic.pkl"))
    assert all(not v.is_cuda for v in sd.values())


# ------------------------------------------------------------------------------------------------- 5: ten updates
def test_ten_updates_on_one_batch(world, tmp_path):
    """value_loss ends below where it started if, and only if, it does for the torch stand-in critic stepped by torch.optim.Adam on
    the same batch and the same targets (the native run's Q_target of every update, replayed)."""
    from tfpnp_amd.trainer.mddpg import trainer as trainer_mod
    env, ob = world
    tr = make_trainer(env, tmp_path)
    idx_stop = torch.tensor([0, 1, 1, 0], device=dev())
    lr = {'actor': 1e-4, 'critic': 1e-3}
    stand_in = K.stand_in_module(9)
    stand_in.load_state_dict(type(tr.critic.state_dict())((k, v.cpu()) for k, v in tr.critic.state_dict().items()))
    stand_in.to(dev())
    targets, real = [], trainer_mod.critic_update

    def recording(*a, **kw):
        targets.append((a[2].detach().clone(), kw["q_target"].detach().clone()))
        return real(*a, **kw)

    trainer_mod.critic_update = recording
    try:
        rows = [torch.stack([x.reshape(()) for x in tr._update(ob, lr, idx_stop=idx_stop)]) for _ in range(10)]
    finally:
        trainer_mod.critic_update = real
    diag = torch.stack(rows).cpu()
    print("ten updates: (-policy_loss, value_loss, entropy, actor_norm, critic_norm)\n", diag)
    assert bool(torch.isfinite(diag).all())
    assert tr.actor.optim_state(dev())[2] == 10 and tr.critic.optim_state(dev())[2] == 10

    # the stand-in has no forward of its own: it is evaluated through restate_live, on its own parameters
    optim = torch.optim.Adam(stand_in.parameters(), lr=lr['critic'])
    losses = []
    for eval_ob, q in targets:
        sd = {k: v for k, v in stand_in.state_dict(keep_vars=True).items()}
        named = {k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v"): v
                 for k, v in sd.items()}
        V = restate_live(named, eval_ob)
        loss = torch.nn.functional.mse_loss(q.view(-1, 1), V)
        optim.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(stand_in.parameters(), 50)
        optim.step()
        losses.append(float(loss))
    native = diag[:, 1].tolist()
    print("value_loss native  ", [f"{v:.5f}" for v in native])
    print("value_loss stand-in", [f"{v:.5f}" for v in losses])
    assert (native[-1] < native[0]) == (losses[-1] < losses[0])


def restate_live(P, x):
    """tests/critic_cases.py::restate on LIVE tensors (differentiable with respect to the stand-in's parameters), fp32 on x's device."""
    import torch.nn.functional as F

    def w(p):
        v, g = P[p + ".weight_v"], P[p + ".weight_g"]
        return g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1), P[p + ".bias"]

    conv = lambda v, p, stride, pad: F.conv2d(v, *w(p), stride=stride, padding=pad)
    trelu = lambda v, key: torch.maximum(v, P[key])
    x = trelu(conv(x, "conv1", 2, 1), "relu_1.alpha")
    for li in range(1, 5):
        for blk in range(2):
            p = f"layer{li}.{blk}"
            out = trelu(conv(x, p + ".conv1", 2 if blk == 0 else 1, 1), p + ".relu_1.alpha")
            out = conv(out, p + ".conv2", 1, 1)
            out = out + (conv(x, p + ".shortcut.0", 2, 0) if blk == 0 else x)
            x = trelu(out, p + ".relu_2.alpha")
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    return F.linear(x, P["fc.weight"], P["fc.bias"])


# ------------------------------------------------------------------------------------------------- 6: the example
def test_example_trains(tmp_path):
    spec = importlib.util.spec_from_file_location("example_train_mddpg", os.path.join(ROOT, "examples", "train_mddpg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    trainer, history, stored = mod.run(episodes=3, B=4, H=64, max_episode_step=3, episode_train_times=2, output=str(tmp_path),
                                       log=lambda *a: None)
    print("examples/train_mddpg.py:", history, "rows stored per step:", stored)
    assert len(history) >= 2                                                        # two episodes past the warm-up, at least
    assert all(np.isfinite(list(h.values())).all() for h in history)
    assert trainer.buffer.size() == min(sum(stored), trainer.buffer.capacity) and sum(stored) > 0
    updates = 2 * len(history)
    assert trainer.actor.optim_state(dev())[2] == updates and trainer.critic.optim_state(dev())[2] == updates
    a0 = A.native_actor(CASE, synth.make_policy_params(9, 10, False, seed=0)).parameters_flat(dev())
    assert not torch.equal(trainer.actor.parameters_flat(dev()), a0)
    assert not torch.equal(trainer.critic.parameters_flat(dev()), trainer.critic_target.parameters_flat(dev()))
    assert os.path.exists(tmp_path / "ckpt" / f"actor_{trainer.opt.train_steps:07d}.pkl")
