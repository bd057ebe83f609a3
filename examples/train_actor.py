"""The actor's side of the MDDPG update with the native gradient (tfpnp/trainer/mddpg/trainer.py:171-212).

    policy_loss.backward(); clip_grad_norm_; actor_optim.step()

The actor is a native ResNetActor_* module; no torch copy of the network.  The trainable state is ONE flat nn.Parameter on the
device (synth.policy_param_specs order).  Per step:

    probs, det = actor.forward_train_raw(ob)         train-mode forward (batch-statistics BatchNorm), leaf tensors here
    loss(probs, det) in torch                        the reference's log_prob / entropy / action_mapping and a toy loss standing in
                                                     for policy_loss (which needs the environment and the critic)
    loss.backward()                                  -> d loss / d probs, d loss / d det
    flat.grad = actor.param_grad(ob, gp, gd)         the backward pass through the network (pnpx_policy_param_grad)
    clip_grad_norm_, Adam on the flat parameter      torch's
    actor.load_flat_(flat)                           the stepped vector back into the native actor (packed on the device)

The running statistics are not trained (their gradient slots are zero); a trainer that wants them moved runs the module's forward in
`.train()` mode with bn_follows_mode=True.

usage (GPU box):  python examples/train_actor.py [steps] [B] [H]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from tfpnp_amd import synth
from tfpnp_amd.policy import ResNetActor_ADMM


def toy_loss(actor, probs, det, idx_stop):
    """log-probability and entropy of the stop head (network.py:149-161), the action mapping (:163-175), and a scalar of all three"""
    logp = torch.log(probs.clamp_min(torch.finfo(probs.dtype).eps)).gather(1, idx_stop.view(-1, 1))
    entropy = -torch.special.xlogy(probs, probs).sum(dim=1, keepdim=True)
    action = actor.action_mapping(det)
    return -(logp.mean() + 0.01 * entropy.mean()) + sum(((v - 0.5 * rng['scale'] - rng['shift']) ** 2).mean()
                                                        for v, rng in zip(action.values(), actor.action_range.values()))


def run(steps=5, B=4, H=64, lr=1e-3, max_norm=50, seed=0, log=print):
    """-> (toy loss per step, the native actor)"""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    actor = ResNetActor_ADMM(6, 5, state_dict=synth.make_policy_params(9, 10, False, seed=seed))
    flat = nn.Parameter(actor.parameters_flat(dev).clone())
    opt = torch.optim.Adam([flat], lr=lr)
    ob = torch.rand(B, 9, H, H, device=dev)
    idx_stop = torch.randint(0, 2, (B,), device=dev)
    history = []
    for it in range(steps):
        probs, det = (t.detach().requires_grad_(True) for t in actor.forward_train_raw(ob))
        loss = toy_loss(actor, probs, det, idx_stop)
        loss.backward()
        flat.grad = actor.param_grad(ob, probs.grad, det.grad)
        norm = torch.nn.utils.clip_grad_norm_([flat], max_norm)
        opt.step()
        actor.load_flat_(flat.detach())
        history.append(float(loss.detach()))
        log(f"step {it}: loss {history[-1]:.6f}  |grad| {float(norm):.4f}")
    return history, actor


if __name__ == "__main__":
    run(*[int(v) for v in sys.argv[1:4]])
