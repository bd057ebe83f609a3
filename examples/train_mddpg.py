"""MDDPGTrainer.train() end to end on native parts: CS-MRI ADMM on synthetic data.

  rollout   native ResNetActor_ADMM (stochastic stop decisions) -> PnPEnv.step -> device-resident replay memory
  update    after every episode past the warm-up, `episode_train_times` times: sample -> actor_update with the one-launch policy
            loss (torch.ops.pnpx.mddpg_policy_loss) differentiated through the native critic, get_eval_ob, the ADMM VJP and PSNR
            -> critic_update on the Q_target the loss wrote -> target soft update
  save      ckpt/actor_*.pkl and ckpt/critic_*.pkl under `output`, in the reference's state-dict format

usage (GPU box):  python examples/train_mddpg.py [episodes] [B] [H]
"""
import os
import random
import sys
import tempfile
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tfpnp_amd import policy, synth
from tfpnp_amd.pnp import UNetDenoiser2D
from tfpnp_amd.tasks import csmri
from tfpnp_amd.trainer.mddpg import MDDPGTrainer


def run(episodes=3, B=4, H=64, max_episode_step=3, episode_train_times=2, env_batch=4, bundle=5, seed=0, output=None, log=print):
    """The first episode is warm-up (no update); every later one is followed by `episode_train_times` updates.  Episodes are
    `max_episode_step` steps long unless every row stops earlier, so `train_steps` is an upper bound chosen for full episodes.
    -> (trainer, per episode with updates: the result dict of _update_policy, rows stored per save_experience call)"""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    random.seed(seed)
    output = tempfile.mkdtemp(prefix="train_mddpg_") if output is None else output
    den = UNetDenoiser2D(state_dict=synth.make_unet_params(0))
    data = synth.make_csmri_batch(B, H, H, ratio=4, sigma_n=15.0, seed=seed + 1)
    loader = [{k: torch.from_numpy(v) for k, v in data.items() if hasattr(v, "dtype")}]
    env = csmri.CSMRIEnv(loader, csmri.ADMMSolver_CSMRI(den), max_episode_step=max_episode_step).to(dev)
    actor = policy.ResNetActor_ADMM(6, bundle, state_dict=synth.make_policy_params(9, 2 * bundle, False, seed=seed))
    opt = SimpleNamespace(rmsize=8, max_episode_step=max_episode_step, train_steps=episodes * max_episode_step,
                          warmup=max_episode_step, validate_interval=10, save_freq=10 ** 9, output=output,
                          episode_train_times=episode_train_times, env_batch=env_batch, loop_penalty=0.05, discount=0.99,
                          lambda_e=0.2, tau=0.001, seed=seed)
    quiet = SimpleNamespace(log=lambda message, color=None: log(message))
    trainer = MDDPGTrainer(opt, env, actor, lambda step: {'actor': 1e-4, 'critic': 3e-4}, dev, output, logger=quiet)
    history, stored = [], []
    update_policy, save_experience = trainer._update_policy, trainer.save_experience

    def recording_update_policy(*a, **kw):
        out = update_policy(*a, **kw)
        history.append(out[0])
        return out

    def recording_save_experience(ob, hidden):
        stored.append(len(ob))
        return save_experience(ob, hidden)

    trainer._update_policy, trainer.save_experience = recording_update_policy, recording_save_experience
    trainer.train()
    return trainer, history, stored


if __name__ == "__main__":
    run(*[int(v) for v in sys.argv[1:4]])
