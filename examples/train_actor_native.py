"""The actor's side of the MDDPG update, native end to end (tfpnp/trainer/mddpg/trainer.py:171, 201-204).

    policy_loss.backward(); clip_grad_norm_; actor_optim.step()

examples/train_actor.py with everything network-sized inside the native context: no flat nn.Parameter, no torch optimiser, and the
train-mode forward runs ONCE per step (train_actor.py runs it twice: forward_train_raw, and again inside param_grad).  Per step,
trainer/mddpg/actor_step.py::actor_update does

    probs, det = actor.forward_train_keep(ob)        train-mode forward that keeps its activations; the running statistics move
    head + loss_fn in torch                          log-probability, entropy, action mapping (ResNetActorBase.head) and the caller's
                                                     loss: here the toy loss of train_actor.py, standing in for policy_loss
    d loss / d probs, d loss / d det                 torch autograd, O(B)
    grad = actor.param_grad_kept(gp, gd)             the backward pass on what the forward kept (pnpx_policy_param_grad_kept)
    actor.adam_step_(grad, lr, max_norm=...)         clip + Adam on the context's own vector, running statistics frozen, refresh

Unlike train_actor.py the running statistics move (momentum 0.1), as they do in the reference's `_update`; they are not trained.

usage (GPU box):  python examples/train_actor_native.py [steps] [B] [H]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tfpnp_amd import synth
from tfpnp_amd.policy import ResNetActor_ADMM
from tfpnp_amd.trainer.mddpg.actor_step import actor_update


def toy_loss_fn(actor):
    """train_actor.py's toy loss as the closure actor_update takes: a scalar of log-probability, entropy and the mapped actions"""
    def loss_fn(action, action_log_prob, dist_entropy):
        return -(action_log_prob.mean() + 0.01 * dist_entropy.mean()) + sum(
            ((action[name] - 0.5 * rng['scale'] - rng['shift']) ** 2).mean() for name, rng in actor.action_range.items())
    return loss_fn


def run(steps=5, B=4, H=64, lr=1e-3, max_norm=50, seed=0, log=print):
    """-> (toy loss per step, the native actor)"""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    actor = ResNetActor_ADMM(6, 5, state_dict=synth.make_policy_params(9, 10, False, seed=seed))
    ob = torch.rand(B, 9, H, H, device=dev)
    idx_stop = torch.randint(0, 2, (B,), device=dev)
    loss_fn = toy_loss_fn(actor)
    history = []
    for it in range(steps):
        out = actor_update(actor, ob, loss_fn, lr, max_norm=max_norm, idx_stop=idx_stop)
        history.append(float(out["policy_loss"]))
        log(f"step {it}: loss {history[-1]:.6f}  |grad| {float(out['actor_norm']):.4f}")
    return history, actor


if __name__ == "__main__":
    run(*[int(v) for v in sys.argv[1:4]])
