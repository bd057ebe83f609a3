"""A native target critic that follows a PyTorch critic while it trains.

The reference's MDDPG update (tfpnp/trainer/mddpg/trainer.py:158-212) evaluates V_next_target = critic_target(eval_ob2)
without a gradient (:182), steps `critic` with Adam on the TD error (:209) and then moves the target by
soft_update(critic_target, critic, tau) (:212).  tfpnp_amd has no critic weight gradients, so the critic being trained stays
a torch module here; the TARGET is the native ResNet_wobn.  Its parameters live on the device: hard_update / soft_update
(tfpnp_amd.utils.misc) take the module's parameters with one torch.cat, apply the reference's arithmetic bit for bit and
re-pack the weights with HIP kernels -- no host round trip per update.

The torch critic below is a plain restatement of ResNet_wobn(num_inputs, 18, 1) with the reference's registration order
(synth.critic_param_specs), which is all soft_update asks of a source module.

usage (GPU box):  python examples/target_critic.py [steps] [B] [H]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

from tfpnp_amd import synth
from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
from tfpnp_amd.utils.misc import hard_update, soft_update

wn = torch.nn.utils.parametrizations.weight_norm


class TReLU(nn.Module):
    def __init__(self):
        super().__init__()
        self.alpha = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return F.relu(x - self.alpha) + self.alpha


class Block(nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1 = wn(nn.Conv2d(cin, planes, 3, stride, 1, bias=True))
        self.conv2 = wn(nn.Conv2d(planes, planes, 3, 1, 1, bias=True))
        self.shortcut = nn.Sequential()
        if stride != 1 or cin != planes:
            self.shortcut = nn.Sequential(wn(nn.Conv2d(cin, planes, 1, stride, bias=True)))
        self.relu_1 = TReLU()
        self.relu_2 = TReLU()

    def forward(self, x):
        out = self.conv2(self.relu_1(self.conv1(x)))
        return self.relu_2(out + self.shortcut(x))


class TorchCritic(nn.Module):
    def __init__(self, num_inputs):
        super().__init__()
        self.conv1 = wn(nn.Conv2d(num_inputs, 64, 3, 2, 1, bias=True))
        cin = 64
        for li, planes in enumerate((64, 128, 256, 512), start=1):
            setattr(self, f"layer{li}", nn.Sequential(Block(cin, planes, 2), Block(planes, planes, 1)))
            cin = planes
        self.fc = nn.Linear(512, 1)
        self.relu_1 = TReLU()

    def forward(self, x):
        x = self.relu_1(self.conv1(x))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(F.adaptive_avg_pool2d(x, 1).flatten(1))


def run(steps=5, B=2, H=64, num_inputs=9, tau=0.001, lr=1e-4, discount=0.99, seed=0, log=print):
    """-> (V_next_target per step as lists, the torch critic, the native target)"""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    critic = TorchCritic(num_inputs)
    params = synth.make_critic_params(num_inputs, seed)
    with torch.no_grad():
        for p, (key, _) in zip(critic.parameters(), synth.critic_param_specs(num_inputs)):
            p.copy_(torch.from_numpy(params[key]))
    critic.to(dev)
    target = ResNet_wobn(num_inputs, 18, 1)
    hard_update(target, critic)                               # trainer.py:54-55
    opt = torch.optim.Adam(critic.parameters(), lr=lr)
    ob, ob2 = torch.rand(B, num_inputs, H, H, device=dev), torch.rand(B, num_inputs, H, H, device=dev)
    reward = torch.randn(B, 1, device=dev)
    history = []
    for it in range(steps):
        with torch.no_grad():
            V_next_target = target(ob2)                       # native forward, trainer.py:182
        loss = F.mse_loss(critic(ob), reward + discount * V_next_target)
        opt.zero_grad()
        loss.backward()
        opt.step()                                            # trainer.py:209
        soft_update(target, critic, tau)                      # trainer.py:212: the native target follows on the device
        history.append(V_next_target.flatten().tolist())
        log(f"step {it}: V_next_target {[f'{v:+.6f}' for v in history[-1]]}  value_loss {float(loss):.4f}")
    return history, critic, target


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:4]]
    run(*a)
