"""A native actor that follows a PyTorch actor while it trains, and runs the rollouts.

The reference's MDDPG loop changes the actor's weights in every update (tfpnp/trainer/mddpg/trainer.py:201-204) and then
runs that actor in eval mode for the next rollout (run_policy, :216-222).  tfpnp_amd has no actor weight gradients, so the
actor being trained stays a torch module here -- optimised through the native one-step model exactly as in
examples/train_bridge.py -- while the ROLLOUTS run on the native ResNetActor_ADMM: before each one,
hard_update(native, module) (tfpnp_amd.utils.misc) gathers the module's parameters and BatchNorm running statistics by name
with one torch.cat and re-derives the native actor's packed weights with HIP kernels.  No host round trip per refresh.

The torch actor below is a plain restatement of the reference's ResNetActor_ADMM (ResNet-18 encoder with BatchNorm2d, the
two heads) under its attribute names (synth.policy_param_specs), which is all hard_update asks of a source module.

usage (GPU box):  python examples/follow_actor.py [updates] [B] [H]
"""
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

from tfpnp_amd import policy, synth
from tfpnp_amd.pnp import UNetDenoiser2D
from tfpnp_amd.tasks import csmri
from tfpnp_amd.utils.misc import hard_update


class Block(nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.shortcut = nn.Sequential()
        if stride != 1 or cin != planes:
            self.shortcut = nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.relu(out + self.shortcut(x))


class Encoder(nn.Module):
    def __init__(self, num_inputs):
        super().__init__()
        self.conv1 = nn.Conv2d(num_inputs, 64, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for li, planes in enumerate((64, 128, 256, 512), start=1):
            setattr(self, f"layer{li}", nn.Sequential(Block(cin, planes, 2), Block(planes, planes, 1)))
            cin = planes

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return F.adaptive_avg_pool2d(x, 1).flatten(1)


class TorchActor(nn.Module):
    """policy_ob [B, num_inputs, H, W] -> (probs [B, 2], det [B, n_det]): the network of ResNetActor_* up to its head
    activations; `act` maps det to the ADMM action dict (tfpnp/policy/network.py:163-175)."""

    def __init__(self, num_inputs, n_det):
        super().__init__()
        self.actor_encoder = Encoder(num_inputs)
        self.fc_softmax = nn.Sequential(nn.Linear(512, 2), nn.Softmax(dim=1))
        self.fc_deterministic = nn.Sequential(nn.Linear(512, n_det), nn.Sigmoid())

    def forward(self, x):
        x = self.actor_encoder(x)
        return self.fc_softmax(x), self.fc_deterministic(x)

    def act(self, policy_ob):
        _, det = self(policy_ob)
        T = det.shape[1] // 2
        return OrderedDict(sigma_d=det[:, :T] * (70 / 255), mu=det[:, T:],
                           idx_stop=torch.zeros(policy_ob.shape[0], dtype=torch.int64, device=policy_ob.device))


def seeded_actor(num_inputs, n_det, seed):
    """A TorchActor holding synth.make_policy_params(num_inputs, n_det, seed=seed)."""
    module = TorchActor(num_inputs, n_det)
    sd = module.state_dict(keep_vars=True)
    with torch.no_grad():
        for key, value in synth.make_policy_params(num_inputs, n_det, False, seed=seed).items():
            sd[key].copy_(torch.from_numpy(value))
    return module


def run(updates=3, B=2, H=64, bundle=5, lr=1e-4, max_episode_step=3, seed=0, log=print):
    """-> (per update: the native rollout's sigma_d of its first policy step as a list, the torch actor, the native actor)"""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    den = UNetDenoiser2D(state_dict=synth.make_unet_params(0))
    env = csmri.CSMRIEnv(None, csmri.ADMMSolver_CSMRI(den), max_episode_step=max_episode_step)
    data = synth.make_csmri_batch(B, H, H, ratio=4, sigma_n=15.0, seed=seed + 1)
    data = {k: torch.from_numpy(v).to(dev) for k, v in data.items() if hasattr(v, "dtype")}
    native = policy.ResNetActor_ADMM(6, bundle)
    module = seeded_actor(native.in_dim, native.n_det, seed).to(dev)
    opt = torch.optim.Adam(module.parameters(), lr=lr)        # bounded steps whatever the batch statistics do to the gradients
    history = []
    for it in range(updates):
        # one actor update through the native one-step model (train_bridge.py); train mode: the running statistics move too
        ob = env.reset(data)
        module.train()
        ob2, reward = env.forward(ob, module.act(env.get_policy_ob(ob)))
        opt.zero_grad()
        (-reward.mean()).backward()
        opt.step()                                            # trainer.py:201-204
        # the native actor follows on the device and runs the rollout in eval mode (trainer.py:216-222)
        hard_update(native, module)
        ob = env.reset(data)
        hidden = native.init_state(B)
        first, total, steps = None, 0.0, 0
        while len(ob):
            action, _, _, hidden = native(env.get_policy_ob(ob), idx_stop=None, train=False, hidden=hidden)
            if first is None:
                first = action["sigma_d"][0].tolist()
            _, ob, r, all_done, _ = env.step(action)
            total += float(r.sum())
            steps += 1
            if all_done:
                break
        history.append(first)
        log(f"update {it}: training reward {float(reward.detach().mean()):+.4f} dB; native rollout {steps} policy steps, "
            f"sum of rewards {total:+.4f} dB, first sigma_d * 255 {[round(v * 255, 2) for v in first]}")
    return history, module, native


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:4]]
    run(*a)
