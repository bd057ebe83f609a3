"""The actor's half of the MDDPG update on native kernels -- tfpnp/trainer/mddpg/trainer.py::_update, line 171 (the train-mode
forward of the actor on the sampled states) and lines 201-204 (backward, clip, step).

The actor is a native ResNetActor_* module.  One update runs the train-mode forward once (forward_train_keep: every activation
stays in the native context), takes policy_loss and its gradient with respect to the two head outputs in torch -- the O(B) head
of ResNetActorBase.forward and the caller's loss closure, which holds the environment step, the critic and the advantage --
runs the network's backward pass on what the forward kept (param_grad_kept) and steps the parameter vector where it lives
(adam_step_: clip + Adam + refresh inside the native context; the running statistics are not parameters and stay out of it).
No torch optimiser and no flat nn.Parameter are involved; the only host synchronisation is the small read-back the refresh
ends with.  The closure of the whole policy_loss and the loop around it are trainer.py::MDDPGTrainer (its loss is one native
launch, torch.ops.pnpx.mddpg_policy_loss, which takes p_stop itself: `pass_probs`); examples/train_bridge.py composes a loss by hand.
"""
import torch


def actor_update(actor, policy_ob, loss_fn, lr, max_norm=50.0, idx_stop=None, betas=(0.9, 0.999), eps=1e-8, pass_probs=False):
    """One actor update.  policy_ob [B, num_inputs, H, W]: the policy observations of the sampled states;
    loss_fn(action, action_log_prob, dist_entropy) -> the scalar policy_loss, differentiable in torch with respect to its
    arguments (action: the dict of ResNetActorBase.forward, 'idx_stop' included); with pass_probs it is called as
    loss_fn(action, action_log_prob, dist_entropy, p_stop), p_stop [B, 2] being the softmax output the other two derive from
    (a leaf of the same graph).  idx_stop None: sampled, as the reference's
    train-time forward does (network.py:149-156).  The running statistics move, as in the reference's train-mode forward.
    All of loss_fn's backward runs before the actor's parameters move.
    -> dict(policy_loss [], actor_norm [] (gradient norm before clipping), action, action_log_prob [B, 1], dist_entropy [B, 1]),
    device tensors, detached."""
    probs, det = actor.forward_train_keep(policy_ob)                                   # trainer.py:171
    probs, det = probs.requires_grad_(), det.requires_grad_()                          # leaves: the network's outputs
    action, action_log_prob, dist_entropy = actor.head(probs, det, idx_stop, True)
    policy_loss = loss_fn(action, action_log_prob, dist_entropy, *((probs,) if pass_probs else ()))
    if not isinstance(policy_loss, torch.Tensor) or policy_loss.numel() != 1:
        raise ValueError("actor_update: loss_fn must return a scalar tensor")
    grad_probs, grad_det = torch.autograd.grad(policy_loss, (probs, det), allow_unused=True)     # :202
    grad_probs = torch.zeros_like(probs) if grad_probs is None else grad_probs
    grad_det = torch.zeros_like(det) if grad_det is None else grad_det
    grad = actor.param_grad_kept(grad_probs.contiguous(), grad_det.contiguous())
    actor_norm = actor.adam_step_(grad, lr, betas=betas, eps=eps, max_norm=max_norm)   # :203-204
    return {"policy_loss": policy_loss.detach(), "actor_norm": actor_norm,
            "action": type(action)((k, v.detach()) for k, v in action.items()),
            "action_log_prob": action_log_prob.detach(), "dist_entropy": dist_entropy.detach()}
