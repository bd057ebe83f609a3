"""The critic's half of the MDDPG update on native kernels -- tfpnp/trainer/mddpg/trainer.py::_update, lines 180-186 (the
target), 198 (value_loss), 206-209 (backward, clip, step) and 212 (target soft update).

The critic and its target are native ResNet_wobn modules.  One update evaluates the critic once
(value_loss_grad: value, loss and gradient from the same forward), steps the parameter vector where it lives (adam_step_:
clip + Adam + re-pack inside the native context) and moves the target (utils.misc.soft_update).  No torch optimiser and no
torch copy of the parameters are involved; the only host synchronisations are the small read-backs the two re-packs end with.
"""
import torch

from ...utils.misc import soft_update


def critic_update(critic, critic_target, eval_ob, eval_ob2, reward, idx_stop, discount, tau, lr, max_norm=50.0, q_target=None):
    """One critic update.  eval_ob / eval_ob2 [B, num_inputs, H, W]: the evaluation observations of the sampled states and of
    their successors; reward, idx_stop [B] or [B, 1] (idx_stop: 1 where the episode ended).  q_target [B] or [B, 1]: the target
    of lines 180-186 when the caller already holds it (trainer.py::MDDPGTrainer._update: the policy loss needs the same
    numbers); the target critic is then not evaluated and eval_ob2, reward, idx_stop and discount are not read.
    -> dict(value_loss [], critic_norm [] (gradient norm before clipping), V_cur [B, 1], Q_target [B, 1]), device tensors."""
    if q_target is None:
        with torch.no_grad():
            reward = reward.reshape(-1, 1).to(torch.float32)
            stop = idx_stop.reshape(-1, 1).to(torch.float32)
            Q_target = discount * (1 - stop) * critic_target(eval_ob2) + reward       # trainer.py:180-186
    else:
        Q_target = q_target.detach().reshape(-1, 1)
    value_loss, V_cur, grad = critic.value_loss_grad(eval_ob, Q_target)              # :198, :207
    critic_norm = critic.adam_step_(grad, lr, max_norm=max_norm)                      # :208-209
    soft_update(critic_target, critic, tau)                                           # :212
    return {"value_loss": value_loss, "critic_norm": critic_norm, "V_cur": V_cur, "Q_target": Q_target}
