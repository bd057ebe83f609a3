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
`.eval()`.  The train-mode forward carries no autograd graph; `forward_train_raw(state)` returns its raw head outputs
(probs, det) without moving anything, and `param_grad(state, grad_probs, grad_det)` is the backward pass through it
(pnpx_policy_param_grad): the flat gradient of sum(grad_probs * probs + grad_det * det) in `parameters_flat()`'s order, so a
flat nn.Parameter and a torch optimiser can train the native actor (examples/train_actor.py).

The actor's whole update is native as well, as the critic's is: `forward_train_keep(state)` is the train-mode forward run once,
where the backward pass reads (pnpx_policy_forward_train_keep: the same bytes, every activation kept in the context);
`param_grad_kept(grad_probs, grad_det)` is `param_grad` without its re-computation (pnpx_policy_param_grad_kept: the same bytes;
refused with the reason once the weights changed or another train forward / param_grad ran); `adam_step_(grad, lr, ...)` is
clip_grad_norm_ + torch.optim.Adam.step() on the context's own vector followed by the refresh (pnpx_policy_adam_step): the
running statistics are frozen ranges of that vector -- the optimiser neither reads their gradient slots nor moves them -- and
Adam's moments never leave the context (`optim_state`, `reset_optim_`).  `head(p_stop, det, idx_stop, train)` is the O(B) part of
`forward`, shared with trainer/mddpg/actor_step.py::actor_update, the actor's half of trainer.py::_update (:171, :201-204).
policy_loss itself (environment, critic, advantage) is one native launch (torch.ops.pnpx.mddpg_policy_loss) inside the closure of
trainer/mddpg/trainer.py::MDDPGTrainer._update, which is also the trainer loop.  Still out of scope: the
actor's input gradient, weight decay / amsgrad / other optimisers, loading Adam's moments from a checkpoint, statistics
synchronised across devices (dist.py), num_batches_tracked (momentum is a number, so torch never reads it), graph capture.
"""
from collections import OrderedDict
from typing import Optional

import torch

from .. import ops, synth
from .. import torch_ops as T
from ..live import LiveWeights


class ResNetActorBase(LiveWeights):
    spi_head = False

    bn_momentum = 0.1           # SynchronizedBatchNorm2d's default (sync_batchnorm/batchnorm.py)

    # live weights (live.py): synth.policy_param_specs order -- every fp32 state_dict entry of the reference actor, running
    # statistics included; the integer `num_batches_tracked` buffers are not kept (eval-mode BatchNorm does not read them)
    _noun, _holds = "actor", "_policy"
    _load, _load_device, _params = "load_policy", "load_policy_device", "policy_params"
    _adam_step, _optim_state, _optim_reset = "policy_adam_step", "policy_optim_state", "policy_optim_reset"
    _specs = staticmethod(synth.policy_param_specs)
    _flat_params = staticmethod(ops.policy_flat_params)
    _dict = OrderedDict

    def __init__(self, num_inputs, action_bundle, num_actions, state_dict=None, bn_follows_mode=False):
        super().__init__()
        self.bn_follows_mode = bool(bn_follows_mode)
        self.in_dim = num_inputs
        self.num_actions = num_actions
        self.action_range = None
        self.action_bundle = action_bundle
        if state_dict is not None:
            self.load_state_dict(state_dict)

    @property
    def n_det(self):
        return self.action_bundle * self.num_actions

    def _shape(self):
        return self.in_dim, self.n_det, self.spi_head

    def forward(self, state, idx_stop, train, hidden):
        """-> (action dict incl. 'idx_stop', log-prob of idx_stop [B,1], entropy of the stop head [B,1], hidden)"""
        ctx = self.context(state.device)
        if self.bn_follows_mode and self.training:
            # batch statistics; the running statistics move on this device: its vector is the truth from here on
            p_stop, det = self._mutate(self._key(state.device),
                                       lambda c: T.call("policy_forward_train", state, self.bn_momentum, True, c.cid))
        else:
            p_stop, det = T.call("policy_forward", state, ctx.cid)   # [B,2] softmax, [B,n_det] sigmoid
        return self.head(p_stop, det, idx_stop, train) + (hidden,)

    def head(self, p_stop, det, idx_stop, train):
        """The O(B) work behind the network: (p_stop [B,2], det [B,n_det]) -> (action dict incl. 'idx_stop', log-prob of
        idx_stop [B,1], entropy of the stop head [B,1]).  Plain torch: differentiable with respect to p_stop and det."""
        logp = torch.log(p_stop.clamp_min(torch.finfo(p_stop.dtype).eps))     # Categorical's own clamp
        entropy = -torch.special.xlogy(p_stop, p_stop).sum(dim=1, keepdim=True)
        if idx_stop is None:      # stochastic while training, greedy otherwise (network.py:149-156)
            idx_stop = torch.multinomial(p_stop, 1).squeeze(1) if train else p_stop.argmax(dim=1)
        action = self.action_mapping(det)
        action['idx_stop'] = idx_stop
        return action, logp.gather(1, idx_stop.view(-1, 1)), entropy

    def forward_train_raw(self, state):
        """(probs [B,2], det [B,n_det]) of the train-mode forward (batch-statistics BatchNorm) on `state`; moves nothing."""
        return T.call("policy_forward_train", state, self.bn_momentum, False, self.context(state.device).cid)

    def param_grad(self, state, grad_probs, grad_det):
        """d sum(grad_probs * probs + grad_det * det) / d parameters_flat(), (probs, det) = forward_train_raw(state): flat fp32
        [n_params] on state's device, the running-statistics slots zero.  Changes nothing (no LiveWeights._mutate)."""
        return T.call("policy_param_grad", state.detach(), grad_probs.detach(), grad_det.detach(), self.context(state.device).cid)

    def forward_train_keep(self, state, update_running=True):
        """forward_train_raw's (probs, det), bit for bit, from the forward that keeps its activations in the context of state's
        device for param_grad_kept; update_running moves the running statistics there (momentum bn_momentum), as the reference's
        train-mode forward does, and makes that device's vector the truth."""
        if not isinstance(state, torch.Tensor):
            raise ops.PnpxError(f"forward_train_keep: expected a torch.Tensor, got {type(state).__name__}")
        if not state.is_cuda:
            raise ops.PnpxError(f"forward_train_keep: tensor on {state.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        run = lambda c: T.call("policy_forward_train_keep", state.detach(), self.bn_momentum, bool(update_running), c.cid)
        return self._mutate(self._key(state.device), run) if update_running else run(self.context(state.device))

    def param_grad_kept(self, grad_probs, grad_det):
        """param_grad(state, grad_probs, grad_det) for the state of the last forward_train_keep, without re-computing the forward:
        the same bytes.  Raises PnpxError, with the reason, if that forward is no longer kept (the weights changed, a train-mode
        forward or param_grad ran since) or none was run.  May be called more than once per kept forward."""
        for t in (grad_probs, grad_det):
            if not isinstance(t, torch.Tensor):
                raise ops.PnpxError(f"param_grad_kept: expected a torch.Tensor, got {type(t).__name__}")
        for t in (grad_probs, grad_det):
            if not t.is_cuda:
                raise ops.PnpxError(f"param_grad_kept: tensor on {t.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        return T.call("policy_param_grad_kept", grad_probs.detach(), grad_det.detach(), self.context(grad_probs.device).cid)

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
