"""Value network on MI355X -- drop-in for the evaluation side of tfpnp/trainer/mddpg/critic.py (same class name, same
constructor arguments, `forward(x) -> [B, 1]`).

ResNet_wobn(num_inputs, 18, 1): weight-normalised ResNet-18 without BatchNorm, TReLU activations, scalar head.  The
forward (pnpx_critic_forward) and its gradient with respect to the INPUT (pnpx_critic_backward) run natively, so the value
term of the reference's actor loss (trainer/mddpg/trainer.py:180-192: V_next = critic(get_eval_ob(ob2)), differentiated into
the actions through ob2.variables) can be evaluated on the native kernels: `forward` is differentiable with respect to x.

The weights are FROZEN between loads: weight-norm is folded on the host by load_state_dict and no weight gradient exists
(the reference throws the critic's weight gradients from the actor loss away, trainer.py:206).  Out of scope: critic weight
gradients, value_loss, optimiser steps, soft update of the target critic, replay, the MDDPG trainer loop, a trainable
actor, depths other than 18, device-side re-packing of changing weights.
"""
import torch
import torch.nn as nn

from ... import ops
from ... import torch_ops as T


class ResNet_wobn(nn.Module):
    def __init__(self, num_inputs, depth, num_outputs, state_dict=None):
        super().__init__()
        if depth != 18 or num_outputs != 1:
            raise NotImplementedError(f"ResNet_wobn: only depth 18 with one output is implemented (the critic every task "
                                      f"builds), got depth {depth}, {num_outputs} outputs")
        self.in_dim = num_inputs
        self._state = None
        self._ctx = {}
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # weights: the reference's own state_dict (torch.load of critic.pkl, trainer.py:254-261), either weight-norm spelling
    def load_state_dict(self, state_dict, strict=True):
        self._state = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in state_dict.items()}
        self._ctx = {}

    def context(self, device):
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._ctx:
            if self._state is None:
                raise ValueError('critic weights were not loaded (load_state_dict)')
            ctx = ops.Context(device)
            ctx.load_critic(self._state, self.in_dim)
            self._ctx[key] = ctx
        return self._ctx[key]

    def forward(self, x):
        """x [B, num_inputs, H, W] (H, W multiples of 32) -> V [B, 1]; differentiable with respect to x."""
        if isinstance(x, torch.Tensor) and not x.is_cuda:
            raise ops.PnpxError(f"ResNet_wobn: tensor on {x.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        return T.call("critic_value", x, self.context(x.device).cid)
