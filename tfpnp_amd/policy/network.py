"""Policy actors on MI355X -- drop-in for the inference side of tfpnp/policy/network.py (same class names, same
constructor arguments, same `forward(state, idx_stop, train, hidden)` contract and action ranges).

The ResNet-18 encoder and both heads run natively (pnpx_policy_forward: BatchNorm folded, stride-2 convolutions on a
space-to-depth grid with tap masks, fp32 MFMA); what stays here is O(B) scalar work: sampling / arg-max of idx_stop,
log-probability, entropy and the action-range mapping (network.py:149-175).  Eval-mode BatchNorm only -- that is how
the reference runs the actor in rollouts (trainer.py:216-221) and in evaluation (evaluator.py:23).

The weights are LIVE, as the native critic's are: the context keeps the flat parameter vector (synth.policy_param_specs
order: parameters AND BatchNorm running statistics) on the device, and `load_flat_` / utils.misc.hard_update replace it
there and re-derive the packed weights on the device (BatchNorm fold included), so the native actor can follow a torch
actor that an optimiser trains (trainer.py:201-204) and run the next rollout (:216-222) without a host reload.
`load_state_dict` is the checkpoint path (folds and packs on the host).

Train-mode BatchNorm is opt-in: an actor built with `bn_follows_mode=True` follows `self.training` as the reference module
does.  After `.train()` its forward normalises every BatchNorm layer with the statistics of the batch and moves the running
statistics (momentum 0.1) in the live parameter vector (pnpx_policy_forward_train); after `.eval()` it runs the path above,
on the moved statistics -- so the reference's `run_policy` (eval -> forward -> train) and `_update` (trainer.py:128,171)
behave as written, and `state_dict()` / `parameters_flat()` return the moved statistics.  The default `False` keeps the
eval-mode forward whatever the mode: an nn.Module is in training mode from construction, and existing callers never call
`.eval()`.  The train-mode forward carries no autograd graph.  Still out of scope: the actor's parameter and input
gradients, its optimiser step and policy_loss, statistics synchronised across devices (dist.py), num_batches_tracked
(momentum is a number, so torch never reads it), graph capture of the train forward.
"""
from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from .. import torch_ops as T


class ResNetActorBase(nn.Module):
    spi_head = False

    bn_momentum = 0.1           # SynchronizedBatchNorm2d's default (sync_batchnorm/batchnorm.py)

    def __init__(self, num_inputs, action_bundle, num_actions, state_dict=None, bn_follows_mode=False):
        super().__init__()
        self.bn_follows_mode = bool(bn_follows_mode)
        self.in_dim = num_inputs
        self.num_actions = num_actions
        self.action_range = None
        self.action_bundle = action_bundle
        self._state = None      # CPU copy of the last load_state_dict; None once the weights were changed on a device
        self._live = None       # key of the context whose device-resident parameters are the weights (then _state is None)
        self._ctx = {}
        if state_dict is not None:
            self.load_state_dict(state_dict)

    @property
    def n_det(self):
        return self.action_bundle * self.num_actions

    # weights: the reference's own state_dict (torch.load of actor.pkl, trainer.py:254-261)
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
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._ctx:
            if self._live is None and self._state is None:
                raise ValueError('actor weights were not loaded (load_state_dict / load_flat_)')
            ctx = ops.Context(device)
            if self._live is not None:
                # the weights were changed on another device: that device's vector is the truth, not the stale CPU copy
                ctx.load_policy_device(self._ctx[self._live].policy_params().to(ctx.device), self.in_dim, self.n_det, self.spi_head)
            else:
                ctx.load_policy(self._state, self.in_dim, self.n_det, self.spi_head)
            self._ctx[key] = ctx
        return self._ctx[key]

    def parameters_flat(self, device):
        """A copy of the weights as one fp32 vector on `device`, in synth.policy_param_specs order."""
        return self.context(device).policy_params()

    def load_flat_(self, flat):
        """Load a flat fp32 vector that lives on a ROCm device (synth.policy_param_specs order: every fp32 state_dict entry
        of the reference actor, running statistics included): BatchNorm fold and packing run on that device; a context that
        already exists there is refreshed in place.  Returns self."""
        if not isinstance(flat, torch.Tensor):
            raise ops.PnpxError(f"load_flat_: expected a torch.Tensor, got {type(flat).__name__}")
        if flat.device.type != "cuda":
            raise ops.PnpxError(f"load_flat_: device {flat.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        key = (flat.device.type, flat.device.index if flat.device.index is not None else torch.cuda.current_device())
        ctx = self._ctx.get(key)
        fresh = ctx is None
        if fresh:
            ctx = ops.Context(torch.device(*key))
        try:
            ctx.load_policy_device(flat, self.in_dim, self.n_det, self.spi_head)
        except ops.PnpxError:
            if not fresh and ctx._policy is None:      # the refresh itself failed: this context holds no actor any more
                del self._ctx[key]
                if self._live == key:
                    self._live = None
            raise
        # every other copy is stale from here on
        self._ctx = {key: ctx}
        self._live = key
        self._state = None
        return self

    def state_dict(self, *args, destination=None, prefix='', keep_vars=False):
        """The fp32 entries of the reference actor's state_dict (synth.policy_param_specs), read from the live weights.
        Loading it into a fresh native actor reproduces this one bit for bit.  The integer `num_batches_tracked` buffers of
        the reference's BatchNorm layers are not kept: eval-mode BatchNorm does not read them."""
        from ..synth import policy_param_specs
        out = destination if destination is not None else OrderedDict()
        if self._live is not None:
            flat = self._ctx[self._live].policy_params()
        elif self._state is not None:
            flat = torch.from_numpy(ops.policy_flat_params(self._state, self.in_dim, self.n_det, self.spi_head))
        else:
            return out
        pos = 0
        for key, shape in policy_param_specs(self.in_dim, self.n_det, self.spi_head):
            n = 1
            for d in shape:
                n *= d
            out[prefix + key] = flat[pos:pos + n].view(shape).clone()
            pos += n
        return out

    def forward(self, state, idx_stop, train, hidden):
        """-> (action dict incl. 'idx_stop', log-prob of idx_stop [B,1], entropy of the stop head [B,1], hidden)"""
        ctx = self.context(state.device)
        if self.bn_follows_mode and self.training:
            # batch statistics; the running statistics move on this device: its vector is the truth from here on
            p_stop, det = T.call("policy_forward_train", state, self.bn_momentum, True, ctx.cid)
            key = next(k for k, c in self._ctx.items() if c is ctx)
            self._ctx = {key: ctx}
            self._live = key
            self._state = None
        else:
            p_stop, det = T.call("policy_forward", state, ctx.cid)   # [B,2] softmax, [B,n_det] sigmoid
        logp = torch.log(p_stop.clamp_min(torch.finfo(p_stop.dtype).eps))     # Categorical's own clamp
        entropy = -torch.special.xlogy(p_stop, p_stop).sum(dim=1, keepdim=True)
        if idx_stop is None:      # stochastic while training, greedy otherwise (network.py:149-156)
            idx_stop = torch.multinomial(p_stop, 1).squeeze(1) if train else p_stop.argmax(dim=1)
        action = self.action_mapping(det)
        action['idx_stop'] = idx_stop
        return action, logp.gather(1, idx_stop.view(-1, 1)), entropy, hidden

    def action_mapping(self, action_deterministic):
        """Sigmoid outputs [B, num_actions * bundle] -> {name: [B, bundle] in the action's range} (network.py:163-175)."""
        per_action = action_deterministic.shape[1] // self.num_actions
        return OrderedDict(
            (name, action_deterministic[:, i * per_action:(i + 1) * per_action] * rng['scale'] + rng['shift'])
            for i, (name, rng) in enumerate(self.action_range.items()))

    def init_state(self, B):      # no recurrent state (the reference returns a dummy as well)
        return torch.zeros(B)


def _actor(name, extra_inputs, num_actions, default_range, spi=False):
    def __init__(self, num_aux_inputs, action_bundle, action_range: Optional[OrderedDict] = None, state_dict=None,
                 bn_follows_mode=False):
        ResNetActorBase.__init__(self, num_aux_inputs + extra_inputs, action_bundle, num_actions, state_dict, bn_follows_mode)
        self.action_range = OrderedDict(default_range) if action_range is None else action_range
    return type(name, (ResNetActorBase,), {"__init__": __init__, "spi_head": spi, "__doc__":
                                           f"tfpnp/policy/network.py {name}: same inputs / action ranges."})


_R = lambda s, sh=0: {'scale': s, 'shift': sh}  # noqa: E731
ResNetActor_ADMM = _actor("ResNetActor_ADMM", 3, 2, [('sigma_d', _R(70 / 255)), ('mu', _R(1))])
ResNetActor_HQS = _actor("ResNetActor_HQS", 2, 2, [('sigma_d', _R(70 / 255)), ('mu', _R(1))])
ResNetActor_PG = _actor("ResNetActor_PG", 1, 2, [('sigma_d', _R(70 / 255)), ('tau', _R(2))])
ResNetActor_APG = _actor("ResNetActor_APG", 2, 3, [('sigma_d', _R(70 / 255)), ('tau', _R(2)), ('beta', _R(2))])
ResNetActor_RED = _actor("ResNetActor_RED", 3, 3, [('sigma_d', _R(70 / 255)), ('mu', _R(1)), ('lamda', _R(2))])
ResNetActor_IADMM = _actor("ResNetActor_IADMM", 3, 3, [('sigma_d', _R(70 / 255)), ('mu', _R(1)), ('tau', _R(2))])
ResNetActor_AMP = _actor("ResNetActor_AMP", 2, 1, [('sigma_d', _R(2))])
ResNetActor_SPI = _actor("ResNetActor_SPI", 3, 2, [('sigma_d', _R(55 / 255, 15 / 255)), ('mu', _R(70, 50))], spi=True)
