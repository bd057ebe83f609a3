"""tfpnp/utils/misc.py: soft_update / hard_update with a native critic as the target (trainer/mddpg/trainer.py:212, :54-55).

`target` is a native ResNet_wobn.  `source` is a native ResNet_wobn on the same device, or any nn.Module on a ROCm device
whose parameters() have the shapes of synth.critic_param_specs in order -- the reference's weight-normalised critic in
either weight-norm spelling, e.g. while a torch optimiser trains it.  A module source costs one torch.cat on the device and
one native call; nothing passes through the host.
"""
import torch

from ..ops import PnpxError
from ..synth import critic_param_specs
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


def _source_vector(target, source):
    if not isinstance(target, ResNet_wobn):
        raise PnpxError(f"target must be a native ResNet_wobn, got {type(target).__name__}")
    if isinstance(source, ResNet_wobn):
        if source.in_dim != target.in_dim:
            raise PnpxError(f"num_inputs mismatch: the source critic has {source.in_dim} inputs, the target {target.in_dim}")
        device = source.device if source.device is not None else target.device
        if device is None:
            raise PnpxError("neither critic has been used on a device yet; call source.context(device) first")
        if target.device is not None and target.device != device:
            raise PnpxError(f"source critic is on {device}, target on {target.device}: both must be on the same device")
        return source.parameters_flat(device)
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


def soft_update(target, source, tau):
    """target = target * (1.0 - tau) + source * tau, in the reference's fp32 arithmetic, then re-packed on the device."""
    flat = _source_vector(target, source)
    target.soft_update_(flat, tau)


def hard_update(target, source):
    """target = source, bit for bit (a device load of the source's parameters; the critic has no buffers)."""
    flat = _source_vector(target, source)
    target.load_flat_(flat)
