"""tfpnp/utils/misc.py: soft_update / hard_update with a native critic, and hard_update with a native actor, as the target
(trainer/mddpg/trainer.py:212, :54-55).

`target` is a native ResNet_wobn.  `source` is a native ResNet_wobn on the same device, or any nn.Module on a ROCm device
whose parameters() have the shapes of synth.critic_param_specs in order -- the reference's weight-normalised critic in
either weight-norm spelling, e.g. while a torch optimiser trains it.  A module source costs one torch.cat on the device and
one native call; nothing passes through the host.

hard_update also takes a native actor (policy.ResNetActor_*) as `target`.  Its source is another native actor on the same
device, or any nn.Module on a ROCm device whose state_dict() holds the keys of synth.policy_param_specs with those shapes --
the reference's ResNetActor_*: parameters and BatchNorm running statistics, gathered BY NAME (buffers are not in
parameters(); integer num_batches_tracked entries are ignored).  The reference has no target actor, so soft_update onto an
actor is refused.
"""
import torch

from ..ops import PnpxError
from ..policy.network import ResNetActorBase
from ..synth import critic_param_specs, policy_param_specs
from ..trainer.mddpg.critic import ResNet_wobn


def check_param_order(params, num_inputs):
    """Raises PnpxError unless the tensors `params` have the shapes of synth.critic_param_specs(num_inputs), in order."""
    specs = critic_param_specs(num_inputs)
    shapes = [tuple(p.shape) for p in params]
    if len(shapes) != len(specs):
        raise PnpxError(f"source module has {len(shapes)} parameter tensors; a critic with {num_inputs} inputs "
                        f"(num_inputs of the target) has {len(specs)}")
    for i, ((key, want), got) in enumerate(zip(specs, shapes)):
        if tuple(want) != got:
            raise PnpxError(f"parameter {i} of the source module has shape {got}; '{key}' of a critic with {num_inputs} "
                            f"inputs (num_inputs of the target) has shape {tuple(want)}")


def _native_source_vector(target, source, noun, mismatch):
    """The vector of a native `source` for a native `target` of the same class: the same network shape on both sides
    (`mismatch`: the refusal otherwise), on the device either of them lives on -- the same one if both do."""
    if source._shape() != target._shape():
        raise PnpxError(mismatch)
    device = source.device if source.device is not None else target.device
    if device is None:
        raise PnpxError(f"neither {noun} has been used on a device yet; call source.context(device) first")
    if target.device is not None and target.device != device:
        raise PnpxError(f"source {noun} is on {device}, target on {target.device}: both must be on the same device")
    return source.parameters_flat(device)


def _source_vector(target, source):
    if not isinstance(target, ResNet_wobn):
        raise PnpxError(f"target must be a native ResNet_wobn (or, for hard_update, a native actor), got {type(target).__name__}")
    if isinstance(source, ResNet_wobn):
        return _native_source_vector(target, source, "critic", f"num_inputs mismatch: the source critic has {source.in_dim} "
                                                               f"inputs, the target {target.in_dim}")
    params = [p.detach() for p in source.parameters()]
    check_param_order(params, target.in_dim)
    devices = {p.device for p in params}
    if len(devices) != 1 or next(iter(devices)).type != "cuda":
        raise PnpxError(f"source module is on {', '.join(sorted(str(d) for d in devices))}; it must be on one ROCm ('cuda') device "
                        "-- tfpnp_amd has no CPU path")
    device = next(iter(devices))
    if target.device is not None and target.device != device:
        raise PnpxError(f"source module is on {device}, target on {target.device}: both must be on the same device")
    if any(p.dtype != torch.float32 for p in params):
        raise PnpxError("source module must hold float32 parameters")
    return torch.cat([p.reshape(-1) for p in params])


def gather_actor_state(state, num_inputs, n_det, spi_head):
    """The tensors of synth.policy_param_specs(num_inputs, n_det, spi_head), in order, out of the mapping `state` (a module's
    state_dict(keep_vars=True)).  Raises PnpxError naming the first key that is missing, is no tensor or has another shape."""
    out = []
    for key, want in policy_param_specs(num_inputs, n_det, spi_head):
        v = state.get(key)
        if v is None:
            raise PnpxError(f"the state_dict() of the source module has no '{key}', which an actor with {num_inputs} inputs and "
                            f"{n_det} outputs (those of the target) holds")
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != tuple(want):
            got = tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__
            raise PnpxError(f"'{key}' of the source module has shape {got}; an actor with {num_inputs} inputs and {n_det} outputs "
                            f"(those of the target) has shape {tuple(want)}")
        out.append((key, v.detach()))
    return out


def _actor_source_vector(target, source):
    if isinstance(source, ResNetActorBase):
        return _native_source_vector(target, source, "actor",
                                     f"actor mismatch: the source has {source.in_dim} inputs / {source.n_det} outputs / spi_head "
                                     f"{source.spi_head}, the target {target.in_dim} / {target.n_det} / {target.spi_head}")
    if not isinstance(source, torch.nn.Module):
        raise PnpxError(f"source must be a native actor or an nn.Module, got {type(source).__name__}")
    named = gather_actor_state(source.state_dict(keep_vars=True), target.in_dim, target.n_det, target.spi_head)
    for key, v in named:
        if v.dtype != torch.float32:
            raise PnpxError(f"'{key}' of the source module is {v.dtype}; the module must hold float32 parameters and buffers")
        if v.device.type != "cuda":
            raise PnpxError(f"'{key}' of the source module is on {v.device}; the module must be on one ROCm ('cuda') device "
                            "-- tfpnp_amd has no CPU path")
        if v.device != named[0][1].device:
            raise PnpxError(f"'{key}' of the source module is on {v.device}, '{named[0][0]}' on {named[0][1].device}: "
                            "the module must be on one device")
    device = named[0][1].device
    if target.device is not None and target.device != device:
        raise PnpxError(f"source module is on {device}, target on {target.device}: both must be on the same device")
    return torch.cat([v.reshape(-1) for _, v in named])


def soft_update(target, source, tau):
    """target = target * (1.0 - tau) + source * tau, in the reference's fp32 arithmetic, then re-packed on the device."""
    if isinstance(target, ResNetActorBase):
        raise PnpxError("soft_update onto a native actor is not implemented: the reference keeps no target actor "
                        "(trainer/mddpg/trainer.py soft-updates the critic target only); use hard_update")
    flat = _source_vector(target, source)
    target.soft_update_(flat, tau)


def hard_update(target, source):
    """target = source, bit for bit (a device load of the source's parameters; the critic has no buffers, the actor's
    BatchNorm running statistics travel with its parameters)."""
    flat = _actor_source_vector(target, source) if isinstance(target, ResNetActorBase) else _source_vector(target, source)
    target.load_flat_(flat)
