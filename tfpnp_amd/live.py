"""The live weights of a native network: what the actor (policy/network.py) and the critic (trainer/mddpg/critic.py) share.

A module keeps one ops.Context per device it was used on.  The weights are either the CPU copy of the last load_state_dict
(`_state`) or, once they were changed on a device, the flat fp32 parameter vector that device's context holds (`_live` names
it; `_state` is then None and every other context is dropped, so it cannot serve stale weights).  Every call that changes the
weights on a device goes through `_mutate`.

A subclass supplies the names of the ops.Context entries of its network, its shape arguments, its spec list and the flattening
of a CPU state dict; nothing here knows which network it owns.  The native optimiser step (adam_step_, optim_state,
reset_optim_) is one of those calls, written once for both networks.
"""
import torch
import torch.nn as nn

from . import ops


class LiveWeights(nn.Module):
    _noun = None                # "actor" / "critic": the network's name in messages
    _holds = None               # the ops.Context attribute that is None while the context holds no such network
    _load = None                # ops.Context methods: load from a state dict,
    _load_device = None         # ... from a flat vector on the device,
    _params = None              # ... a copy of the live vector
    _adam_step = None           # ... clip + Adam on the live vector, its moments and step counter, forgetting them
    _optim_state = None
    _optim_reset = None
    _specs = None               # synth.*_param_specs(*shape): [(key, shape)] in the vector's order
    _flat_params = None         # ops.*_flat_params(state_dict, *shape): the vector of a CPU state dict (numpy)
    _dict = dict                # what state_dict() returns

    def __init__(self):
        super().__init__()
        self._state = None      # CPU copy of the last load_state_dict; None once the weights were changed on a device
        self._live = None       # key of the context whose device-resident parameters are the weights (then _state is None)
        self._ctx = {}

    def _shape(self):
        """The shape arguments every entry above takes behind the weights."""
        raise NotImplementedError

    def _key(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ops.PnpxError(f"{type(self).__name__}: device {device}; tfpnp_amd runs on MI355X only, there is no CPU path")
        return (device.type, device.index if device.index is not None else torch.cuda.current_device())

    # weights: the reference's own state_dict (torch.load of actor.pkl / critic.pkl, trainer.py:254-261)
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
        key = self._key(device)
        if key not in self._ctx:
            if self._live is None and self._state is None:
                raise ValueError(f'{self._noun} weights were not loaded (load_state_dict / load_flat_)')
            ctx = ops.Context(torch.device(*key))
            if self._live is not None:
                # the weights were changed on another device: that device's vector is the truth, not the stale CPU copy
                flat = getattr(self._ctx[self._live], self._params)()
                getattr(ctx, self._load_device)(flat.to(ctx.device), *self._shape())
            else:
                getattr(ctx, self._load)(self._state, *self._shape())
            self._ctx[key] = ctx
        return self._ctx[key]

    def _mutate(self, key, fn, empty=False):
        """Run fn(ctx), which changes the weights of the context on device `key`, and make that context the truth: every other
        copy is stale from here on.  A device without a context gets one that holds the current weights (empty: none, fn
        loads them).  If fn raises PnpxError the module stays as it was, unless the failed call left a context of this module
        without a network: that one is forgotten -- the next context() of its device raises or reloads from what is left,
        never from a stale copy."""
        ctx = self._ctx.get(key)
        if ctx is None:
            ctx = ops.Context(torch.device(*key)) if empty else self.context(torch.device(*key))
        try:
            out = fn(ctx)
        except ops.PnpxError:
            if self._ctx.get(key) is ctx and getattr(ctx, self._holds) is None:
                del self._ctx[key]
                if self._live == key:
                    self._live = None
            raise
        self._ctx = {key: ctx}
        self._live = key
        self._state = None
        return out

    def parameters_flat(self, device):
        """A copy of the weights as one fp32 vector on `device`, in the order of the network's synth.*_param_specs."""
        return getattr(self.context(device), self._params)()

    def load_flat_(self, flat):
        """Load a flat fp32 vector that lives on a ROCm device (the order of the network's synth.*_param_specs): fold and
        packing run on that device; a context that already exists there is refreshed in place.  Returns self."""
        if not isinstance(flat, torch.Tensor):
            raise ops.PnpxError(f"load_flat_: expected a torch.Tensor, got {type(flat).__name__}")
        self._mutate(self._key(flat.device), lambda ctx: getattr(ctx, self._load_device)(flat, *self._shape()), empty=True)
        return self

    def adam_step_(self, grad, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=50.0):
        """clip_grad_norm_(parameters, max_norm) + torch.optim.Adam.step() (trainer.py:201-204 / :208-209) on grad's device, in
        place on the native parameter vector, then the re-pack.  Adam's moments and step counter live in the native context;
        they survive every refresh of the same network (load_flat_, the critic's soft_update_).  -> the gradient norm before
        clipping (0-dim device tensor), as clip_grad_norm_ returns it.  A gradient with a non-finite norm raises PnpxError and
        changes nothing."""
        if not isinstance(grad, torch.Tensor):
            raise ops.PnpxError(f"adam_step_: expected a torch.Tensor, got {type(grad).__name__}")
        return self._mutate(self._key(grad.device), lambda ctx: getattr(ctx, self._adam_step)(grad, lr, betas, eps, max_norm))

    def optim_state(self, device):
        """(exp_avg, exp_avg_sq, step) of the context on `device`: copies of Adam's moments as flat fp32 vectors (the order of
        parameters_flat) and the step counter; zeros and 0 before the first adam_step_."""
        return getattr(self.context(device), self._optim_state)()

    def reset_optim_(self):
        """Forget Adam's moments and step counter on every device this network lives on.  Returns self."""
        for ctx in self._ctx.values():
            getattr(ctx, self._optim_reset)()
        return self

    def state_dict(self, *args, destination=None, prefix='', keep_vars=False):
        """The fp32 entries of the reference module's state_dict under its key names, read from the live weights.  Loading it
        into a fresh native module reproduces this one bit for bit."""
        out = destination if destination is not None else self._dict()
        if self._live is not None:
            flat = getattr(self._ctx[self._live], self._params)()
        elif self._state is not None:
            flat = torch.from_numpy(type(self)._flat_params(self._state, *self._shape()))
        else:
            return out
        pos = 0
        for key, shape in type(self)._specs(*self._shape()):
            n = 1
            for d in shape:
                n *= d
            out[prefix + key] = flat[pos:pos + n].view(shape).clone()
            pos += n
        return out
