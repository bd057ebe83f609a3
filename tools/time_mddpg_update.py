"""Time one MDDPGTrainer._update two ways on the same GPU, CS-MRI ADMM on synthetic data:

  (a) as built   trainer/mddpg/trainer.py::_update: actor_update around the one-launch policy loss
                 (torch.ops.pnpx.mddpg_policy_loss), then critic_update on the Q_target that launch wrote -- the target critic
                 runs once
  (b) torch loss the same update with trainer.py:174-197 written in torch inside the closure (the head's log-probability and
                 entropy, about 25 elementwise launches and their autograd graph) and critic_update evaluating its own target --
                 what a user had to write around actor_update and critic_update before the trainer existed

    python tools/time_mddpg_update.py [out_file]        (GPU box; default profiles/mddpg_update_times.txt)

Both legs run the same native networks, environment step and VJPs on the same sampled batch with the same teacher-forced stop
decisions; they differ in the loss arithmetic and in one target-critic forward.  One GPU process per size, each under its own time
limit; a size that fails or runs out of time ends the run.  Wall clock with a device synchronisation around each update (the
optimiser steps end with a read-back, so HIP events alone would not see them); the two legs alternate inside one process, after
warm-up updates of both.  Before the timed window the first update of each leg, taken from identical weights, is compared: the two
must agree in -policy_loss and value_loss to fp32 rounding, or the timings would compare different work.
"""
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, WARMUP, REPS, BUNDLE = 3, 3, 20, 5
LR = {'actor': 1e-4, 'critic': 3e-4}
SIZES = [(48, 128), (48, 256)]
STEP_LIMIT = 420   # seconds per size


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def update_with_torch_loss(tr, ob, lr, idx_stop):
    """MDDPGTrainer._update with the loss composed in torch and the critic's half left to critic_update alone."""
    from tfpnp_amd.trainer.mddpg.actor_step import actor_update
    from tfpnp_amd.trainer.mddpg.critic_step import critic_update
    opt, env = tr.opt, tr.env
    policy_ob, eval_ob = env.get_policy_ob(ob), env.get_eval_ob(ob)
    kept = {}

    def loss_fn(action, action_log_prob, dist_entropy):
        ob2, reward = env.forward(ob, action)
        reward = reward - opt.loop_penalty
        eval_ob2 = env.get_eval_ob(ob2)
        gamma = (opt.discount * (1 - action['idx_stop'].float())).unsqueeze(-1)
        with torch.no_grad():
            V_cur = tr.critic(eval_ob)
            Q_target = gamma * tr.critic_target(eval_ob2.detach()) + reward
        advantage = (Q_target - V_cur).clone().detach()
        ddpg = gamma * tr.critic(eval_ob2) + reward
        kept.update(eval_ob2=eval_ob2.detach(), reward=reward.detach(), entropy=dist_entropy.detach().mean())
        return -(action_log_prob * advantage + ddpg + opt.lambda_e * dist_entropy).mean()

    a = actor_update(tr.actor, policy_ob, loss_fn, lr['actor'], max_norm=50, idx_stop=idx_stop)
    c = critic_update(tr.critic, tr.critic_target, eval_ob, kept['eval_ob2'], kept['reward'], idx_stop, opt.discount, opt.tau,
                      lr['critic'], max_norm=50)
    return -a['policy_loss'], c['value_loss'], kept['entropy'], a['actor_norm'], c['critic_norm']


def one_size(B, H):
    from tfpnp_amd import policy, synth
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.tasks import csmri
    from tfpnp_amd.trainer.mddpg import MDDPGTrainer
    dev = torch.device("cuda:0")
    den = UNetDenoiser2D(state_dict=synth.make_unet_params(0))
    data = synth.make_csmri_batch(B, H, H, ratio=4, sigma_n=15.0, seed=SEED + 1)
    loader = [{k: torch.from_numpy(v) for k, v in data.items() if hasattr(v, "dtype")}]
    env = csmri.CSMRIEnv(loader, csmri.ADMMSolver_CSMRI(den), max_episode_step=6).to(dev)
    ob = env.reset()
    idx_stop = torch.from_numpy(np.random.RandomState(5).randint(0, 2, B)).to(dev)
    opt = SimpleNamespace(rmsize=1, max_episode_step=6, loop_penalty=0.05, discount=0.99, lambda_e=0.2, tau=0.001, seed=SEED)
    quiet = SimpleNamespace(log=lambda message, color=None: None)
    params = synth.make_policy_params(9, 2 * BUNDLE, False, seed=SEED)

    def trainer():
        actor = policy.ResNetActor_ADMM(6, BUNDLE, state_dict=params)
        return MDDPGTrainer(opt, env, actor, lambda step: LR, dev, os.devnull, logger=quiet)

    built, composed = trainer(), trainer()
    legs = {"built": lambda: built._update(ob, LR, idx_stop=idx_stop),
            "torch": lambda: update_with_torch_loss(composed, ob, LR, idx_stop)}
    first = {k: [float(x) for x in fn()[:2]] for k, fn in legs.items()}          # from identical weights; also the first warm-up
    rel = max(abs(a - b) / max(abs(b), 1e-30) for a, b in zip(first["built"], first["torch"]))
    if not rel < 1e-4:
        print(f"the two legs disagree on their first update: {first}", flush=True)
        return 1
    for fn in legs.values():
        for _ in range(WARMUP - 1):
            fn()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    tripped = den.context(dev).range_tripped()
    med = {k: float(np.median(v)) for k, v in t.items()}
    col = lambda k: f"{med[k]:9.3f} [{min(t[k]):8.3f} .. {max(t[k]):8.3f}]"
    print(f"RESULT {B:3d}  {H}x{H}  {col('built')}  {col('torch')}  {med['built'] / med['torch']:7.3f}  {rel:9.2e}  "
          f"{'TRIPPED' if tripped else 'ok'}", flush=True)
    return 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        return one_size(int(sys.argv[2]), int(sys.argv[3]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mddpg_update_times.txt")
    lines = [f"# MDDPGTrainer._update, CS-MRI ADMM (action bundle {BUNDLE}), synthetic data; ms per update, median [min .. max] of {REPS} "
             f"interleaved updates",
             f"# (wall clock, device synchronised around each; {WARMUP} warm-up updates per leg)",
             "# (a) as built: actor_update around torch.ops.pnpx.mddpg_policy_loss, critic_update(q_target=) -- one target-critic forward",
             "# (b) torch loss: trainer.py:174-197 in torch inside the closure, critic_update evaluating its own target",
             "# a/b: ratio of the medians; first: largest relative difference of (-policy_loss, value_loss) between the legs' first updates;",
             "# guard: the half-split range guard after the run",
             "# B  HxW      (a) as built                   (b) torch loss                 a/b      first      guard"]
    head = len(lines)
    for B, H in SIZES:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--one", str(B), str(H)],
                           capture_output=True, text=True)
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(p.stdout[-2000:], p.stderr[-2000:], sep="\n")
            lines.append(f"# {B} x {H}x{H}: exit status {p.returncode}; the run ends here")
            break
        lines.append(res[0][len("RESULT "):])
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 0 if len(lines) == head + len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
