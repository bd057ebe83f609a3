"""Value network on MI355X -- drop-in for the evaluation side of tfpnp/trainer/mddpg/critic.py (same class name, same
constructor arguments, `forward(x) -> [B, 1]`).

ResNet_wobn(num_inputs, 18, 1): weight-normalised ResNet-18 without BatchNorm, TReLU activations, scalar head.  The
forward (pnpx_critic_forward) and its gradients with respect to the INPUT (pnpx_critic_backward) and to the PARAMETERS
(pnpx_critic_param_grad) run natively, so the value term of the reference's actor loss (trainer/mddpg/trainer.py:180-192:
V_next = critic(get_eval_ob(ob2)), differentiated into the actions through ob2.variables) can be evaluated on the native
kernels: `forward` is differentiable with respect to x.

The weights are LIVE: the native context keeps the flat parameter vector on the device, and `load_flat_`,
utils.misc.soft_update / hard_update replace or move it there and re-pack on the device (weight-norm fold included), so a
target critic can follow a critic that a torch optimiser trains (trainer.py:182, :212) and the value term can be taken on
the freshly stepped critic (:190) without a host reload.  `load_state_dict` is the checkpoint path (folds on the host).
`param_grad(x, grad_value)` is value_loss.backward() (trainer.py:198,207): the gradient of sum(grad_value * V) with respect to
the parameters as one flat vector in synth.critic_param_specs order (pnpx_critic_param_grad: weight gradients on the fp32
MFMA, thresholds, fc, weight-norm).  A flat nn.Parameter takes it as .grad, a torch optimiser steps it and `load_flat_`
takes the result (examples/train_critic.py); `forward` stays differentiable with respect to x only.
The critic's whole update is native as well: `value_loss_grad(x, q_target)` takes nn.MSELoss()(q_target, V) and its
backward() from ONE forward (pnpx_critic_value_loss_grad), and `adam_step_(grad, lr, ...)` is clip_grad_norm_ +
torch.optim.Adam.step() on the context's own parameter vector followed by the re-pack (pnpx_critic_adam_step): the
parameters and Adam's moments never leave the native context, no torch optimiser is involved (`optim_state`,
`reset_optim_`; trainer/mddpg/critic_step.py::critic_update is the critic's half of trainer.py::_update).
policy_loss (one launch, csrc/mddpg_loss.hip) and the MDDPG trainer loop that joins the two updates are trainer.py::MDDPGTrainer.
Out of scope: weight decay / amsgrad / other optimisers, checkpointing the moments
(the reference's save_model does not save them either), a graph-capturable step, depths other
than 18.  (The native actor has the same live weights and the same optimiser step: policy/network.py, trainer/mddpg/actor_step.py; the replay memory is utils/rpm.py.)
"""
import torch

from ... import ops, synth
from ... import torch_ops as T
from ...live import LiveWeights


class ResNet_wobn(LiveWeights):
    # live weights (live.py): synth.critic_param_specs order -- the 82 tensors of the reference critic under its key names
    # (`*.weight_g` / `*.weight_v`; a state dict in either weight-norm spelling loads), e.g.
    # torch.cat([p.flatten() for p in critic.parameters()])
    _noun, _holds = "critic", "_critic"
    _load, _load_device, _params = "load_critic", "load_critic_device", "critic_params"
    # adam_step_ / optim_state / reset_optim_ (live.py): trainer.py:208-209 on the context's own vector; the moments also survive
    # soft_update_
    _adam_step, _optim_state, _optim_reset = "critic_adam_step", "critic_optim_state", "critic_optim_reset"
    _specs = staticmethod(synth.critic_param_specs)
    _flat_params = staticmethod(ops.critic_flat_params)

    def __init__(self, num_inputs, depth, num_outputs, state_dict=None):
        super().__init__()
        if depth != 18 or num_outputs != 1:
            raise NotImplementedError(f"ResNet_wobn: only depth 18 with one output is implemented (the critic every task "
                                      f"builds), got depth {depth}, {num_outputs} outputs")
        self.in_dim = num_inputs
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def _shape(self):
        return (self.in_dim,)

    def soft_update_(self, src_flat, tau):
        """parameters = parameters * (1.0 - tau) + src_flat * tau on src_flat's device (utils.misc.soft_update)."""
        if not isinstance(src_flat, torch.Tensor):
            raise ops.PnpxError(f"soft_update_: expected a torch.Tensor, got {type(src_flat).__name__}")
        self._mutate(self._key(src_flat.device), lambda ctx: ctx.critic_soft_update(src_flat, tau))
        return self

    def forward(self, x):
        """x [B, num_inputs, H, W] (H, W multiples of 32) -> V [B, 1]; differentiable with respect to x."""
        if isinstance(x, torch.Tensor) and not x.is_cuda:
            raise ops.PnpxError(f"ResNet_wobn: tensor on {x.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        return T.call("critic_value", x, self.context(x.device).cid)

    def param_grad(self, x, grad_value):
        """d sum(grad_value * V(x)) / d parameters -> flat fp32 [n_params] on x's device (synth.critic_param_specs order).
        x [B, num_inputs, H, W] (H, W multiples of 32), grad_value [B] or [B, 1].  Overwrites nothing of the module: assign
        the result to the .grad of a flat parameter and step it with a torch optimiser, then load_flat_."""
        for t in (x, grad_value):
            if isinstance(t, torch.Tensor) and not t.is_cuda:
                raise ops.PnpxError(f"ResNet_wobn: tensor on {t.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        return T.call("critic_param_grad", x.detach(), grad_value.detach().reshape(-1), self.context(x.device).cid)

    def value_loss_grad(self, x, q_target):
        """-> (value_loss [], V [B, 1], grad [n_params]) on x's device from one forward: value_loss = nn.MSELoss()(q_target, V)
        and value_loss.backward() (trainer.py:198,207).  V has forward(x)'s bytes, grad those of
        param_grad(x, 2.0 * (V - q_target) / B).  q_target [B] or [B, 1] is the detached target; nothing here takes part in
        autograd."""
        for t in (x, q_target):
            if isinstance(t, torch.Tensor) and not t.is_cuda:
                raise ops.PnpxError(f"ResNet_wobn: tensor on {t.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        V, loss, grad = T.call("critic_value_loss_grad", x.detach(), q_target.detach().reshape(-1), self.context(x.device).cid)
        return loss, V, grad
