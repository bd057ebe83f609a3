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
Out of scope: the actor's loss and a trainable actor, weight decay / amsgrad / other optimisers, checkpointing the moments
(the reference's save_model does not save them either), a graph-capturable step, the MDDPG trainer loop, depths other
than 18.  (The native actor has the same live weights: policy/network.py; the replay memory is utils/rpm.py.)
"""
import torch
import torch.nn as nn

from ... import ops
from ... import torch_ops as T


def _key(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise ops.PnpxError(f"ResNet_wobn: device {device}; tfpnp_amd runs on MI355X only, there is no CPU path")
    return (device.type, device.index if device.index is not None else torch.cuda.current_device())


class ResNet_wobn(nn.Module):
    def __init__(self, num_inputs, depth, num_outputs, state_dict=None):
        super().__init__()
        if depth != 18 or num_outputs != 1:
            raise NotImplementedError(f"ResNet_wobn: only depth 18 with one output is implemented (the critic every task "
                                      f"builds), got depth {depth}, {num_outputs} outputs")
        self.in_dim = num_inputs
        self._state = None      # CPU copy of the last load_state_dict; None once the weights were changed on a device
        self._live = None       # key of the context whose device-resident parameters are the weights (then _state is None)
        self._ctx = {}
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # weights: the reference's own state_dict (torch.load of critic.pkl, trainer.py:254-261), either weight-norm spelling
    def load_state_dict(self, state_dict, strict=True):
        self._state = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in state_dict.items()}
        self._live = None
        self._ctx = {}

    @property
    def device(self):
        """The device the weights live on: where they were last changed, else the first device they were used on, else None."""
        key = self._live if self._live is not None else next(iter(self._ctx), None)
        return None if key is None else torch.device(*key)

    def context(self, device):
        key = _key(device)
        if key not in self._ctx:
            ctx = ops.Context(torch.device(*key))
            if self._live is not None:
                # the weights were changed on another device: that device's vector is the truth, not the stale CPU copy
                ctx.load_critic_device(self._ctx[self._live].critic_params().to(ctx.device), self.in_dim)
            elif self._state is not None:
                ctx.load_critic(self._state, self.in_dim)
            else:
                raise ValueError('critic weights were not loaded (load_state_dict / load_flat_)')
            self._ctx[key] = ctx
        return self._ctx[key]

    def _changed_on(self, key):
        """The parameters of context `key` were changed on its device: every other copy is stale from here on."""
        self._ctx = {key: self._ctx[key]}
        self._live = key
        self._state = None

    def parameters_flat(self, device):
        """A copy of the parameters as one fp32 vector on `device`, in synth.critic_param_specs order."""
        return self.context(device).critic_params()

    def load_flat_(self, flat):
        """Load a flat fp32 parameter vector that lives on a ROCm device (synth.critic_param_specs order, e.g.
        torch.cat([p.flatten() for p in critic.parameters()]) of the reference critic): fold and packing run on that
        device; a context that already exists there is refreshed in place.  Returns self."""
        if not isinstance(flat, torch.Tensor):
            raise ops.PnpxError(f"load_flat_: expected a torch.Tensor, got {type(flat).__name__}")
        key = _key(flat.device)
        ctx = self._ctx.get(key)
        fresh = ctx is None
        if fresh:
            ctx = ops.Context(torch.device(*key))
        try:
            ctx.load_critic_device(flat, self.in_dim)
        except ops.PnpxError:
            if not fresh and ctx._critic is None:      # the refresh itself failed: this context holds no critic any more
                del self._ctx[key]
                if self._live == key:
                    self._live = None
            raise
        self._ctx[key] = ctx
        self._changed_on(key)
        return self

    def soft_update_(self, src_flat, tau):
        """parameters = parameters * (1.0 - tau) + src_flat * tau on src_flat's device (utils.misc.soft_update)."""
        if not isinstance(src_flat, torch.Tensor):
            raise ops.PnpxError(f"soft_update_: expected a torch.Tensor, got {type(src_flat).__name__}")
        key = _key(src_flat.device)
        ctx = self.context(src_flat.device)
        try:
            ctx.critic_soft_update(src_flat, tau)
        except ops.PnpxError:
            if ctx._critic is None:
                del self._ctx[key]
                if self._live == key:
                    self._live = None
            raise
        self._changed_on(key)
        return self

    def state_dict(self, *args, destination=None, prefix='', keep_vars=False):
        """The 82 tensors under the reference's key names (`*.weight_g` / `*.weight_v`), read from the live weights --
        torch.save(critic.state_dict(), ...) of trainer.py:254-261.  Loading it into a fresh ResNet_wobn reproduces this
        critic bit for bit."""
        from ...synth import critic_param_specs
        out = destination if destination is not None else {}
        specs = critic_param_specs(self.in_dim)
        if self._live is not None:
            flat = self._ctx[self._live].critic_params()
        elif self._state is not None:
            flat = torch.from_numpy(ops.critic_flat_params(self._state, self.in_dim))
        else:
            return out
        pos = 0
        for key, shape in specs:
            n = 1
            for s in shape:
                n *= s
            out[prefix + key] = flat[pos:pos + n].view(shape).clone()
            pos += n
        return out

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

    def adam_step_(self, grad, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=50.0):
        """clip_grad_norm_(parameters, max_norm) + torch.optim.Adam.step() (trainer.py:208-209) on grad's device, in place on
        the native parameter vector, then the re-pack.  Adam's moments and step counter live in the native context; they
        survive load_flat_ / soft_update_ of the same critic.  -> the gradient norm before clipping (0-dim device tensor), as
        clip_grad_norm_ returns it.  A gradient with a non-finite norm raises PnpxError and changes nothing."""
        if not isinstance(grad, torch.Tensor):
            raise ops.PnpxError(f"adam_step_: expected a torch.Tensor, got {type(grad).__name__}")
        key = _key(grad.device)
        ctx = self.context(grad.device)
        try:
            norm = ctx.critic_adam_step(grad, lr, betas, eps, max_norm)
        except ops.PnpxError:
            if ctx._critic is None:
                del self._ctx[key]
                if self._live == key:
                    self._live = None
            raise
        self._changed_on(key)
        return norm

    def optim_state(self, device):
        """(exp_avg, exp_avg_sq, step) of the context on `device`: copies of Adam's moments as flat fp32 vectors
        (synth.critic_param_specs order) and the step counter; zeros and 0 before the first adam_step_."""
        return self.context(device).critic_optim_state()

    def reset_optim_(self):
        """Forget Adam's moments and step counter on every device this critic lives on.  Returns self."""
        for ctx in self._ctx.values():
            ctx.critic_optim_reset()
        return self
