"""The shape of MDDPGTrainer.train() (tfpnp/trainer/mddpg/trainer.py:59-125) on native parts, with a device-resident replay
memory between the rollouts and the updates.

  rollout   native ResNetActor_ADMM (stochastic stop decisions, so the live set shrinks) -> PnPEnv.step; after every step
            memory.store_batch(ob, hidden) puts all live rows of the observation into the ring with ONE launch
            (save_experience, trainer.py:224-234, without the trip to the host)
  update    after each episode a few times: memory.sample(env_batch) -- ONE gather launch, the batch convert2batch would build
            (trainer.py:236-241) -- -> env.get_policy_ob -> torch actor -> env.forward (native one-step model with native VJPs)
            -> Adam step on -reward (the DDPG reward term of trainer.py:189-204; no critic here, see examples/target_critic.py)
  follow    hard_update(native, module): the native actor takes over the updated weights on the device (examples/follow_actor.py)

usage (GPU box):  python examples/replay_loop.py [episodes] [updates_per_episode] [env_batch]
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from follow_actor import seeded_actor
from tfpnp_amd import policy, synth
from tfpnp_amd.pnp import UNetDenoiser2D
from tfpnp_amd.tasks import csmri
from tfpnp_amd.utils.misc import hard_update
from tfpnp_amd.utils.rpm import ReplayMemory


def run(episodes=3, updates=2, env_batch=3, B=2, H=64, bundle=5, lr=1e-4, max_episode_step=3, rmsize=4, seed=0, log=print):
    """-> (memory, per update: mean reward of the sampled batch under the torch actor)"""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    random.seed(seed)
    den = UNetDenoiser2D(state_dict=synth.make_unet_params(0))
    env = csmri.CSMRIEnv(None, csmri.ADMMSolver_CSMRI(den), max_episode_step=max_episode_step)
    data = synth.make_csmri_batch(B, H, H, ratio=4, sigma_n=15.0, seed=seed + 1)
    data = {k: torch.from_numpy(v).to(dev) for k, v in data.items() if hasattr(v, "dtype")}
    native = policy.ResNetActor_ADMM(6, bundle)
    module = seeded_actor(native.in_dim, native.n_det, seed).to(dev)
    opt = torch.optim.Adam(module.parameters(), lr=lr)
    memory = ReplayMemory(rmsize * max_episode_step)              # trainer.py:46
    rewards = []
    for episode in range(episodes):
        hard_update(native, module)
        ob = env.reset(data)
        hidden = hidden_full = native.init_state(B).to(dev)
        stored = 0
        for _ in range(max_episode_step):
            with torch.no_grad():                                 # run_policy, :216-222
                action, _, _, hidden = native(env.get_policy_ob(ob), idx_stop=None, train=True, hidden=hidden)
            _, ob2_masked, _, done, _ = env.step(action)
            memory.store_batch(ob, hidden)                        # save_experience
            stored += len(ob)
            ob, hidden = ob2_masked, hidden_full[env.idx_left, ...]
            if done:
                break
        module.train()
        for _ in range(updates):                                  # _update_policy, :127-156
            batch = memory.sample(env_batch)
            ob2, reward = env.forward(batch, module.act(env.get_policy_ob(batch)))
            opt.zero_grad()
            (-reward.mean()).backward()
            opt.step()
            rewards.append(float(reward.detach().mean()))
        log(f"episode {episode}: stored {stored} rows, RPM[{memory.size()}/{memory.capacity}] index {memory.index} "
            f"({memory.nbytes / 2**20:.1f} MiB on {next(iter(memory.storage.values())).device}); "
            f"sampled-batch rewards {[round(r, 4) for r in rewards[-updates:]]} dB")
    return memory, rewards


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:4]]
    run(*a)
