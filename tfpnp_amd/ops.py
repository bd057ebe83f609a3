"""Tensor-level wrappers over the C ABI (include/pnpx.h): torch tensors in, torch tensors out.

PyTorch is plumbing here (device memory, streams); every op below is one libpnpx.so call on the caller's
current HIP stream.  All ops require contiguous fp32 tensors on a ROCm device; anything else raises.
"""
import ctypes as C
import itertools
import threading
import weakref
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import PnpxError, check


_ctx_ids = itertools.count(1)
_ctx_by_id = weakref.WeakValueDictionary()


def _flatten(state_dict, specs, what, alt=None):
    """The entries of `state_dict` that `specs` ([(key, shape)]) names, in its order, as one contiguous fp32 numpy vector; a
    missing key or a wrong shape raises PnpxError naming it (`what`: whose state_dict).  alt: {leaf: other leaf} -- a second
    spelling of a key's last component, tried when the first is absent."""
    chunks = []
    for key, shape in specs:
        v = state_dict.get(key)
        stem, _, leaf = key.rpartition(".")
        if v is None and alt and leaf in alt:
            v = state_dict.get(f"{stem}.{alt[leaf]}")
        if v is None:
            raise PnpxError(f"{what} state_dict is missing '{key}'")
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if tuple(v.shape) != tuple(shape):
            raise PnpxError(f"'{key}' has shape {tuple(v.shape)}, expected {tuple(shape)}")
        chunks.append(np.ascontiguousarray(v, dtype=np.float32).reshape(-1))
    return np.concatenate(chunks)


def critic_flat_params(state_dict, num_inputs):
    """The flat fp32 parameter vector pnpx_critic_load takes (synth.critic_param_specs order) from a critic state_dict.
    Weight-norm entries are accepted under the reference's names (`*.weight_g` / `*.weight_v`) and under the names current
    PyTorch saves the same module with (`*.parametrizations.weight.original0` / `original1`); a missing key or a wrong shape
    raises PnpxError naming it."""
    from .synth import critic_param_specs
    return _flatten(state_dict, critic_param_specs(num_inputs), "critic",
                    {"weight_g": "parametrizations.weight.original0", "weight_v": "parametrizations.weight.original1"})


def policy_flat_params(state_dict, num_inputs, n_det, spi_head=False):
    """The flat fp32 parameter vector pnpx_policy_load takes (synth.policy_param_specs order) from an actor state_dict; a
    missing key or a wrong shape raises PnpxError naming it.  Integer num_batches_tracked entries are not part of it."""
    from .synth import policy_param_specs
    return _flatten(state_dict, policy_param_specs(num_inputs, n_det, spi_head), "policy")


def context_by_id(cid):
    """The live Context with integer handle `cid` (how contexts travel through torch.ops.pnpx.* schemas)."""
    try:
        return _ctx_by_id[int(cid)]
    except KeyError:
        raise PnpxError(f"no live native context with id {cid}") from None


class Context:
    """One pnpx_ctx: a device, (optionally) packed denoiser weights, and the native workspaces."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise PnpxError(f"tfpnp_amd runs on MI355X (ROCm 'cuda' devices) only, got {device}; there is no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        h = C.c_void_p()
        check(_lib.lib().pnpx_ctx_create(self.device.index, C.byref(h)))
        self._h = h
        self._has_weights = False
        self.is_drunet = False
        self._policy = None
        self._kept_rows = None             # observations of the last policy_forward_train_keep (its gradients have that many rows)
        self._critic = None
        self.cid = next(_ctx_ids)          # integer handle for the dispatcher-registered ops (torch_ops.py)
        _ctx_by_id[self.cid] = self

    @property
    def handle(self):
        if self._h is None:
            raise PnpxError("context already destroyed")
        return self._h

    def load_unet(self, state_dict):
        """state_dict: mapping with the reference's 56 key names -> tensors/ndarrays (any device)."""
        from .synth import unet_param_specs
        flat = _flatten(state_dict, unet_param_specs(), "denoiser")
        check(_lib.lib().pnpx_unet_load(self.handle, flat.ctypes.data_as(C.c_void_p), flat.size))
        self._has_weights = True
        self.is_drunet = False

    def load_drunet(self, state_dict, nb=4):
        """state_dict with KAIR's UNetRes / DRUNet key names (synth.drunet_param_specs) -> the context's denoiser."""
        from .synth import drunet_param_specs
        flat = _flatten(state_dict, drunet_param_specs(nb=nb), "DRUNet")
        check(_lib.lib().pnpx_drunet_load(self.handle, flat.ctypes.data_as(C.c_void_p), flat.size, int(nb)))
        self._has_weights = True
        self.is_drunet = True

    def load_policy(self, state_dict, num_inputs, n_det, spi_head=False):
        """state_dict with the reference's ResNetActor_* key names (tfpnp/policy/network.py) -> native actor."""
        flat = policy_flat_params(state_dict, num_inputs, n_det, spi_head)
        check(_lib.lib().pnpx_policy_load(self.handle, flat.ctypes.data_as(C.c_void_p), flat.size, int(num_inputs),
                                          int(n_det), int(bool(spi_head))))
        self._policy = (int(num_inputs), int(n_det), bool(spi_head))

    def _flat_vector(self, t, who, want, what):
        """A flat parameter vector as the library takes it: fp32, contiguous, on this context's device, `want` floats long
        (None: not checked here); `what` names the network that has `want` parameters."""
        if not isinstance(t, torch.Tensor):
            raise PnpxError(f"{who}: expected a torch.Tensor, got {type(t).__name__}")
        if t.device != self.device:
            raise PnpxError(f"{who}: parameter vector is on {t.device}, the context is on {self.device}")
        if t.dtype != torch.float32:
            raise PnpxError(f"{who}: expected float32, got {t.dtype}")
        if t.dim() != 1 or not t.is_contiguous():
            raise PnpxError(f"{who}: expected a contiguous 1-D vector, got shape {tuple(t.shape)} with strides {t.stride()}")
        if want is not None and t.numel() != want:
            raise PnpxError(f"{who}: {what} has {want} parameters, got {t.numel()}")
        return t.detach()

    def _live_vector(self, entry, n):
        """A copy of the live parameter vector of `n` floats that the library's `entry` writes (n None: no such network is
        loaded, and the entry says so)."""
        out = torch.empty((1 if n is None else n,), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(entry(self.handle, _p(out), out.numel(), _stream(out)))
        return out

    def load_policy_device(self, flat, num_inputs, n_det, spi_head=False):
        """flat: the actor's fp32 state as one vector on this context's device, in synth.policy_param_specs order (each
        convolution followed by its BatchNorm weight, bias, running_mean, running_var; then the heads).  BatchNorm fold and
        packing run on the device on the current stream; an actor with the same head already loaded here is refreshed in
        place.  Ends with one small read-back (synchronises the current stream)."""
        want = int(_lib.lib().pnpx_policy_num_params(int(num_inputs), int(n_det), int(bool(spi_head))))
        flat = self._flat_vector(flat, "load_policy_device", want, f"an actor with {num_inputs} inputs and {n_det} outputs"
                                                                    f"{' (SPI head)' if spi_head else ''}")
        with torch.cuda.device(self.device):
            st = _lib.lib().pnpx_policy_load_device(self.handle, _p(flat), flat.numel(), int(num_inputs), int(n_det),
                                                    int(bool(spi_head)), _stream(flat))
        if st != 0:
            self._policy = None        # a failed load leaves the context without an actor
        check(st)
        self._policy = (int(num_inputs), int(n_det), bool(spi_head))

    def policy_params(self):
        """A copy of the live parameter vector (fp32, on this context's device, load_policy_device's order)."""
        lib = _lib.lib()
        return self._live_vector(lib.pnpx_policy_params,
                                 None if self._policy is None else int(lib.pnpx_policy_num_params(*map(int, self._policy))))

    def load_critic(self, state_dict, num_inputs):
        """state_dict of the reference's ResNet_wobn(num_inputs, 18, 1) (tfpnp/trainer/mddpg/critic.py) -> native critic
        (key spellings: critic_flat_params).  Folds and packs on the host: the path for a checkpoint.  Weights that change
        between evaluations go through load_critic_device / critic_soft_update."""
        flat = critic_flat_params(state_dict, num_inputs)
        check(_lib.lib().pnpx_critic_load(self.handle, flat.ctypes.data_as(C.c_void_p), flat.size, int(num_inputs)))
        self._critic = int(num_inputs)

    def load_critic_device(self, flat, num_inputs=None):
        """flat: the critic's parameters as one fp32 vector on this context's device, in synth.critic_param_specs order (the
        order of module.parameters() of the reference's weight-normalised critic).  Weight-norm fold and packing run on the
        device on the current stream; a critic with the same num_inputs already loaded is refreshed in place.  num_inputs
        None: taken from the vector's length.  Ends with one small read-back (synchronises the current stream)."""
        if num_inputs is None and isinstance(flat, torch.Tensor):
            n = flat.numel()
            num_inputs = next((c for c in range(1, 65) if int(_lib.lib().pnpx_critic_num_params(c)) == n), None)
            if num_inputs is None:
                raise PnpxError(f"load_critic_device: {n} floats is not the parameter count of a critic with 1..64 inputs "
                                f"(9 inputs: {int(_lib.lib().pnpx_critic_num_params(9))})")
        want = None if num_inputs is None else int(_lib.lib().pnpx_critic_num_params(int(num_inputs)))   # None: no tensor
        flat = self._flat_vector(flat, "load_critic_device", want, f"a critic with {num_inputs} inputs")
        with torch.cuda.device(self.device):
            st = _lib.lib().pnpx_critic_load_device(self.handle, _p(flat), flat.numel(), int(num_inputs), _stream(flat))
        if st != 0:
            self._critic = None        # a failed load leaves the context without a critic
        check(st)
        self._critic = int(num_inputs)

    def critic_soft_update(self, src_flat, tau):
        """utils/misc.py:81-85 with the loaded critic as the target: params = params * (1.0 - tau) + src_flat * tau in the
        reference's fp32 arithmetic (bit-equal to torch's), then the device-side re-packing of load_critic_device."""
        want = None if self._critic is None else int(_lib.lib().pnpx_critic_num_params(self._critic))   # None: the library refuses
        src_flat = self._flat_vector(src_flat, "critic_soft_update", want, f"a critic with {self._critic} inputs")
        tau = float(tau)
        with torch.cuda.device(self.device):
            st = _lib.lib().pnpx_critic_soft_update(self.handle, _p(src_flat), src_flat.numel(), 1.0 - tau, tau, _stream(src_flat))
        if st == 1:                    # PNPX_ERR_ARG from the refresh: a threshold went non-finite, the critic is unloaded
            self._critic = None
        check(st)

    def critic_params(self):
        """A copy of the live parameter vector (fp32, on this context's device, load_critic_device's order)."""
        lib = _lib.lib()
        return self._live_vector(lib.pnpx_critic_params,
                                 None if self._critic is None else int(lib.pnpx_critic_num_params(self._critic)))

    def _adam_step(self, who, net, noun, n_params, what, step_entry, params_entry, grad, lr, betas, eps, max_norm):
        """critic_adam_step / policy_adam_step: the checks, the call and what a PNPX_ERR_ARG means.  net, noun: "_critic", "critic" /
        "_policy", "actor"; n_params: the loaded network's parameter count (None: none loaded); what: the network in words."""
        if not isinstance(grad, torch.Tensor):
            raise PnpxError(f"{who}: expected a torch.Tensor, got {type(grad).__name__}")
        try:
            lr, eps, max_norm = float(lr), float(eps), float(max_norm)
            b1, b2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise PnpxError(f"{who}: lr, betas = (beta1, beta2), eps and max_norm must be numbers, got lr {lr!r}, "
                            f"betas {betas!r}, eps {eps!r}, max_norm {max_norm!r}") from None
        if not (0.0 <= lr < float("inf")):
            raise PnpxError(f"{who}: lr must be finite and >= 0, got {lr}")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise PnpxError(f"{who}: betas must lie in [0, 1), got {(b1, b2)}")
        if not (0.0 < eps < float("inf")):
            raise PnpxError(f"{who}: eps must be finite and > 0, got {eps}")
        if not max_norm > 0.0:
            raise PnpxError(f"{who}: max_norm must be > 0 (float('inf'): no clipping), got {max_norm}")
        if n_params is None:
            raise PnpxError(f"{who}: no {noun} loaded")
        if grad.numel() != n_params:
            raise PnpxError(f"{who}: {what} has {n_params} parameters, got a gradient of {grad.numel()}")
        grad = self._flat_vector(grad, who, None, None)     # (its length: above)
        norm = torch.empty((), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            st = step_entry(self.handle, _p(grad), grad.numel(), lr, b1, b2, eps, max_norm, _p(norm), _stream(grad))
            if st == 1:                # PNPX_ERR_ARG: a non-finite gradient norm leaves the network as it was; a refresh that meets a
                err = _lib.lib().pnpx_last_error()      # non-finite value unloads it, as any refresh does
                if params_entry(self.handle, None, 0, None) == 3:     # PNPX_ERR_NO_WEIGHTS
                    setattr(self, net, None)
                raise PnpxError(f"pnpx call failed (status 1): {err.decode('utf-8', 'replace')}")
        check(st)
        return norm

    def _optim_state(self, n, entry):
        m = torch.empty((n,), device=self.device, dtype=torch.float32)
        v = torch.empty((n,), device=self.device, dtype=torch.float32)
        step = C.c_longlong(0)
        with torch.cuda.device(self.device):
            check(entry(self.handle, _p(m), _p(v), n, C.byref(step), _stream(m)))
        return m, v, int(step.value)

    def critic_adam_step(self, grad, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=50.0):
        """clip_grad_norm_(max_norm) + torch.optim.Adam.step() (trainer/mddpg/trainer.py:208-209; no weight decay, no amsgrad)
        on the live parameter vector, then the device-side re-packing of load_critic_device.  grad: flat fp32 [n_params] on
        this context's device (critic_param_grad's layout).  The moments and the step counter live in the native context.
        -> the gradient norm before clipping, a 0-dim tensor on the device.  max_norm = float('inf'): no clipping."""
        lib = _lib.lib()
        n = None if self._critic is None else int(lib.pnpx_critic_num_params(self._critic))
        return self._adam_step("critic_adam_step", "_critic", "critic", n, f"a critic with {self._critic} inputs", lib.pnpx_critic_adam_step,
                               lib.pnpx_critic_params, grad, lr, betas, eps, max_norm)

    def critic_optim_state(self):
        """(exp_avg, exp_avg_sq, step): copies of Adam's moments (fp32 [n_params] on this context's device) and its step counter;
        zeros and 0 before the first critic_adam_step."""
        if self._critic is None:
            raise PnpxError("critic_optim_state: no critic loaded")
        return self._optim_state(int(_lib.lib().pnpx_critic_num_params(self._critic)), _lib.lib().pnpx_critic_optim_state)

    def critic_optim_reset(self):
        """Forget Adam's moments and step counter (the state before the first critic_adam_step)."""
        with torch.cuda.device(self.device):
            check(_lib.lib().pnpx_critic_optim_reset(self.handle))

    def policy_adam_step(self, grad, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=50.0):
        """clip_grad_norm_(max_norm) + torch.optim.Adam.step() (trainer/mddpg/trainer.py:201-204) on the actor's live parameter
        vector, then the refresh of load_policy_device.  grad: flat fp32 [n_params] on this context's device (policy_param_grad's
        layout).  The running statistics are frozen: what grad holds at their slots is ignored, they do not move and their
        moments stay zero.  -> the gradient norm before clipping, a 0-dim tensor on the device."""
        lib = _lib.lib()
        n = None if self._policy is None else int(lib.pnpx_policy_num_params(*map(int, self._policy)))
        what = None if self._policy is None else (f"an actor with {self._policy[0]} inputs and {self._policy[1]} outputs"
                                                        f"{' (SPI head)' if self._policy[2] else ''}")
        return self._adam_step("policy_adam_step", "_policy", "actor", n, what, lib.pnpx_policy_adam_step, lib.pnpx_policy_params, grad, lr,
                               betas, eps, max_norm)

    def policy_optim_state(self):
        """(exp_avg, exp_avg_sq, step) of the actor's optimiser, as critic_optim_state."""
        if self._policy is None:
            raise PnpxError("policy_optim_state: no actor loaded")
        return self._optim_state(policy_flat_size(self), _lib.lib().pnpx_policy_optim_state)

    def policy_optim_reset(self):
        """Forget the actor's moments and step counter (the state before the first policy_adam_step)."""
        with torch.cuda.device(self.device):
            check(_lib.lib().pnpx_policy_optim_reset(self.handle))

    def set_option(self, key, value):
        """e.g. set_option('conv_mode', 1) selects the fast half-split f16 MFMA convolutions (default 0 = fp32 arithmetic)."""
        check(_lib.lib().pnpx_ctx_set_option(self.handle, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int(0)
        check(_lib.lib().pnpx_ctx_get_option(self.handle, key.encode(), C.byref(v)))
        return int(v.value)

    def status(self):
        """Raises PnpxError once the half-split range guard has tripped (an earlier call's output was invalid; the
        context has switched itself to conv_mode 0).  Does not synchronise: call it after the stream has drained,
        e.g. right after reading a result back.  Re-arm with set_option('range_guard', 1)."""
        check(_lib.lib().pnpx_ctx_status(self.handle))

    def range_tripped(self):
        """True once the half-split range guard has tripped (see status()); other failures raise.  Like status() it does
        not synchronise -- ask after a point where the stream has drained (PnPEnv.step does, after its one host read)."""
        st = _lib.lib().pnpx_ctx_status(self.handle)
        if st == _lib.PNPX_ERR_RANGE:
            return True
        check(st)
        return False

    def release_train_cache(self):
        """Give the training path's activation ring (raw device memory outside PyTorch's caching allocator) back to the
        device now; it re-grows on the next denoiser forward under autograd.  Outstanding tickets re-compute."""
        check(_lib.lib().pnpx_ctx_set_option(self.handle, b"train_cache_release", 1))

    def reserve(self, B, H, W):
        check(_lib.lib().pnpx_ctx_reserve(self.handle, B, H, W))

    def bytes(self):
        return int(_lib.lib().pnpx_ctx_bytes(self.handle))

    def close(self):
        if self._h is not None:
            _lib.lib().pnpx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}
_default_lock = threading.Lock()


def default_context(device):
    """Weight-less per-device context for the stateless transforms (fft2, cdp, psnr ...)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise PnpxError(f"tfpnp_amd has no CPU path (tensor on {device})")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _default_lock:
        if idx not in _default_ctx:
            _default_ctx[idx] = Context(torch.device("cuda", idx))
        return _default_ctx[idx]


# ------------------------------------------------------------------------------------------------- helpers
def _f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise PnpxError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise PnpxError(f"{name}: tensor is on {t.device}; tfpnp_amd has no CPU path")
    if t.dtype != torch.float32:
        raise PnpxError(f"{name}: expected float32, got {t.dtype}")
    return t.detach().contiguous()


def _mask_u8(mask, name="mask"):
    if mask.device.type != "cuda":
        raise PnpxError(f"{name}: tensor is on {mask.device}; tfpnp_amd has no CPU path")
    m = mask.detach()
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    return (m != 0).contiguous().view(torch.uint8)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _params(B, *ps):
    """Hyper-parameter tensors [B,T] (or [B]) -> contiguous fp32 [B,T], common T and row stride."""
    out = []
    T = None
    for i, p in enumerate(ps):
        p = _f32(p, f"parameter {i}")
        if p.dim() == 1:
            p = p.view(-1, 1)
        if p.dim() != 2 or p.shape[0] != B:
            raise PnpxError(f"hyper-parameter {i} must be [B, iter_num] with B={B}, got {tuple(p.shape)}")
        T = p.shape[1] if T is None else T
        if p.shape[1] != T:
            raise PnpxError("hyper-parameters disagree on iter_num")
        out.append(p)
    return out, T


# ------------------------------------------------------------------------------------------------- denoiser
def unet_denoise(ctx, x, sigma, return_preclamp=False):
    x = _f32(x, "x")
    sigma = _f32(sigma, "sigma").reshape(-1)
    if x.dim() != 4 or x.shape[1] != 1:
        raise PnpxError(f"denoiser input must be [B,1,H,W], got {tuple(x.shape)}")
    B, _, H, W = x.shape
    if sigma.numel() != B:
        raise PnpxError(f"sigma must have {B} entries, got {sigma.numel()}")
    out = torch.empty_like(x)
    pre = torch.empty_like(x) if return_preclamp else None
    if B == 0:                       # every item already stopped: empty in, empty out (as the reference's modules)
        return (out, pre) if return_preclamp else out
    with torch.cuda.device(x.device):
        check(_lib.lib().pnpx_unet_denoise(ctx.handle, _p(x), _p(sigma), _p(out), _p(pre) if pre is not None else None,
                                           B, H, W, _stream(x)))
    return (out, pre) if return_preclamp else out


def unet_denoise_train(ctx, x, sigma):
    """Denoiser forward for autograd -> (out [B,1,H,W], ticket): the activations are parked in the context's training
    ring under `ticket` (0: not parked) so that unet_denoise_backward(..., ticket=) need not re-compute them."""
    x = _f32(x, "x")
    sigma = _f32(sigma, "sigma").reshape(-1)
    if x.dim() != 4 or x.shape[1] != 1 or sigma.numel() != x.shape[0]:
        raise PnpxError(f"denoiser input must be [B,1,H,W] with sigma [B], got {tuple(x.shape)} / {tuple(sigma.shape)}")
    B, _, H, W = x.shape
    out = torch.empty_like(x)
    ticket = C.c_ulonglong(0)
    if B:
        with torch.cuda.device(x.device):
            check(_lib.lib().pnpx_unet_denoise_train(ctx.handle, _p(x), _p(sigma), _p(out), B, H, W, C.byref(ticket),
                                                     _stream(x)))
    return out, int(ticket.value)


def unet_denoise_backward(ctx, x, sigma, grad_out, ticket=0):
    """(grad_x [B,1,H,W], grad_sigma [B]) = J^T grad_out of unet_denoise; the forward pass is re-computed natively unless
    `ticket` names activations the context's training ring still holds."""
    x = _f32(x, "x")
    sigma = _f32(sigma, "sigma").reshape(-1)
    grad_out = _f32(grad_out, "grad_out")
    B, _, H, W = x.shape
    if grad_out.shape != x.shape or sigma.numel() != B:
        raise PnpxError("unet_denoise_backward: shape mismatch")
    gx = torch.empty_like(x)
    gs = torch.empty((B,), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        check(_lib.lib().pnpx_unet_denoise_backward_ticket(ctx.handle, _p(x), _p(sigma), _p(grad_out), _p(gx), _p(gs), B, H,
                                                           W, int(ticket), _stream(x)))
    return gx, gs


def policy_forward(ctx, ob):
    """ob [B,C,H,W] -> (probs [B,2], det [B,n_det]) of the loaded actor (eval mode)."""
    ob = _f32(ob, "ob")
    if ob.dim() != 4 or getattr(ctx, "_policy", None) is None or ob.shape[1] != ctx._policy[0]:
        raise PnpxError("policy_forward: no policy loaded or observation has the wrong channel count")
    B, _, H, W = ob.shape
    probs = torch.empty((B, 2), device=ob.device, dtype=torch.float32)
    det = torch.empty((B, ctx._policy[1]), device=ob.device, dtype=torch.float32)
    if B == 0:
        return probs, det
    with torch.cuda.device(ob.device):
        check(_lib.lib().pnpx_policy_forward(ctx.handle, _p(ob), _p(probs), _p(det), B, H, W, _stream(ob)))
    return probs, det


def policy_forward_train(ctx, ob, momentum=0.1, update_running=True):
    """ob [B,C,H,W] -> (probs [B,2], det [B,n_det]) of the loaded actor in TRAIN mode: every BatchNorm normalises with the
    statistics of this batch (F.batch_norm(training=True, momentum, eps=1e-5)); update_running moves the running statistics
    in the context's live parameter vector (policy_params), and the next eval-mode policy_forward uses them."""
    ob = _f32(ob, "ob")
    if ob.dim() != 4 or getattr(ctx, "_policy", None) is None or ob.shape[1] != ctx._policy[0]:
        raise PnpxError("policy_forward_train: no policy loaded or observation has the wrong channel count")
    B, _, H, W = ob.shape
    probs = torch.empty((B, 2), device=ob.device, dtype=torch.float32)
    det = torch.empty((B, ctx._policy[1]), device=ob.device, dtype=torch.float32)
    with torch.cuda.device(ob.device):
        check(_lib.lib().pnpx_policy_forward_train(ctx.handle, _p(ob), _p(probs), _p(det), B, H, W, float(momentum),
                                                   int(bool(update_running)), _stream(ob)))
    return probs, det


def policy_bn_stats(ctx):
    """(mean, var) of the last policy_forward_train on `ctx`: batch mean and biased batch variance of the actor's 4864
    BatchNorm channels, concatenated in state_dict order (fp32, on the context's device)."""
    n = int(_lib.lib().pnpx_policy_num_bn_channels())
    mean = torch.empty((n,), device=ctx.device, dtype=torch.float32)
    var = torch.empty((n,), device=ctx.device, dtype=torch.float32)
    with torch.cuda.device(ctx.device):
        check(_lib.lib().pnpx_policy_bn_stats(ctx.handle, _p(mean), _p(var), n, _stream(mean)))
    return mean, var


def policy_flat_size(ctx):
    """Length of the loaded actor's flat parameter vector (policy_params)."""
    if getattr(ctx, "_policy", None) is None:
        raise PnpxError("no policy loaded")
    return int(_lib.lib().pnpx_policy_num_params(*map(int, ctx._policy)))


def policy_param_grad(ctx, ob, grad_probs, grad_det):
    """Flat fp32 vector [n_params] on ob's device, policy_params' order: d sum(grad_probs * probs + grad_det * det) / d params
    of the loaded actor, (probs, det) being policy_forward_train(ctx, ob) -- the actor's half of policy_loss.backward()
    (trainer/mddpg/trainer.py:171-212) with grad_probs / grad_det = d policy_loss / d probs, d det.  The running-statistics
    slots are zero.  Overwrites, does not accumulate; the forward is re-computed natively; nothing in the context changes."""
    ob = _f32(ob, "ob")
    if ob.dim() != 4 or getattr(ctx, "_policy", None) is None or ob.shape[1] != ctx._policy[0]:
        raise PnpxError("policy_param_grad: no policy loaded or observation has the wrong channel count")
    B, _, H, W = ob.shape
    grad_probs = _f32(grad_probs, "grad_probs")
    grad_det = _f32(grad_det, "grad_det")
    if tuple(grad_probs.shape) != (B, 2) or tuple(grad_det.shape) != (B, ctx._policy[1]):
        raise PnpxError(f"policy_param_grad: grad_probs / grad_det must be [{B}, 2] / [{B}, {ctx._policy[1]}], got "
                        f"{tuple(grad_probs.shape)} / {tuple(grad_det.shape)}")
    n = policy_flat_size(ctx)
    out = torch.empty((n,), device=ob.device, dtype=torch.float32)
    with torch.cuda.device(ob.device):
        check(_lib.lib().pnpx_policy_param_grad(ctx.handle, _p(ob), _p(grad_probs), _p(grad_det), _p(out), n, B, H, W,
                                                _stream(ob)))
    return out


def policy_forward_train_keep(ctx, ob, momentum=0.1, update_running=True):
    """policy_forward_train, bit for bit, run where the backward pass reads: the context keeps every activation of this forward
    until the weights change, a plain train forward or policy_param_grad runs, or the next kept forward replaces it.
    policy_param_grad_kept(ctx, grad_probs, grad_det) is then the backward pass alone."""
    ob = _f32(ob, "ob")
    if ob.dim() != 4 or getattr(ctx, "_policy", None) is None or ob.shape[1] != ctx._policy[0]:
        raise PnpxError("policy_forward_train_keep: no policy loaded or observation has the wrong channel count")
    B, _, H, W = ob.shape
    probs = torch.empty((B, 2), device=ob.device, dtype=torch.float32)
    det = torch.empty((B, ctx._policy[1]), device=ob.device, dtype=torch.float32)
    with torch.cuda.device(ob.device):
        check(_lib.lib().pnpx_policy_forward_train_keep(ctx.handle, _p(ob), _p(probs), _p(det), B, H, W, float(momentum),
                                                        int(bool(update_running)), _stream(ob)))
    ctx._kept_rows = B
    return probs, det


def policy_param_grad_kept(ctx, grad_probs, grad_det, out=None):
    """policy_param_grad's bytes for the observation of the last policy_forward_train_keep, without re-computing the forward.
    Raises PnpxError, naming the reason, when no kept forward is valid.  May be called more than once per kept forward.
    out: a flat fp32 [n_params] vector on the device to write into (left untouched by a refused call)."""
    if getattr(ctx, "_policy", None) is None:
        raise PnpxError("policy_param_grad_kept: no policy loaded")
    grad_probs = _f32(grad_probs, "grad_probs")
    grad_det = _f32(grad_det, "grad_det")
    # the library reads one row per observation of the kept forward; without one it refuses before it reads anything
    B = getattr(ctx, "_kept_rows", None)
    if B is None:
        B = grad_probs.shape[0] if grad_probs.dim() == 2 else -1
    if tuple(grad_probs.shape) != (B, 2) or tuple(grad_det.shape) != (B, ctx._policy[1]):
        raise PnpxError(f"policy_param_grad_kept: grad_probs / grad_det must be [{B}, 2] / [{B}, {ctx._policy[1]}] (one row per "
                        f"observation of the kept forward), got {tuple(grad_probs.shape)} / {tuple(grad_det.shape)}")
    n = policy_flat_size(ctx)
    if out is None:
        out = torch.empty((n,), device=grad_probs.device, dtype=torch.float32)
    else:
        ctx._flat_vector(out, "policy_param_grad_kept", n, "the loaded actor")
    with torch.cuda.device(grad_probs.device):
        check(_lib.lib().pnpx_policy_param_grad_kept(ctx.handle, _p(grad_probs), _p(grad_det), _p(out), n, _stream(grad_probs)))
    return out


def policy_frozen_ranges(num_inputs, n_det, spi_head=False):
    """[(first, count)] of the actor's flat vector that policy_adam_step leaves alone: the running statistics, sorted, adjacent
    ranges merged.  Needs no device."""
    cap = 64
    first, count = (C.c_size_t * cap)(), (C.c_size_t * cap)()
    n = int(_lib.lib().pnpx_policy_frozen_ranges(int(num_inputs), int(n_det), int(bool(spi_head)), first, count, cap))
    if n < 0 or n > cap:
        raise PnpxError(f"policy_frozen_ranges: no actor with {num_inputs} inputs and {n_det} outputs")
    return [(int(first[i]), int(count[i])) for i in range(n)]


def _critic_ob(ctx, ob, who):
    ob = _f32(ob, "ob")
    if ob.dim() != 4 or getattr(ctx, "_critic", None) is None or ob.shape[1] != ctx._critic:
        raise PnpxError(f"{who}: no critic loaded or observation has the wrong channel count")
    return ob


def critic_forward(ctx, ob):
    """ob [B,C,H,W] -> V [B,1] of the loaded critic (tfpnp/trainer/mddpg/critic.py:121-131)."""
    ob = _critic_ob(ctx, ob, "critic_forward")
    B, _, H, W = ob.shape
    value = torch.empty((B, 1), device=ob.device, dtype=torch.float32)
    if B:
        with torch.cuda.device(ob.device):
            check(_lib.lib().pnpx_critic_forward(ctx.handle, _p(ob), _p(value), B, H, W, _stream(ob)))
    return value


def critic_backward(ctx, ob, grad_value):
    """grad_ob [B,C,H,W] = grad_value[b] * dV_b / d ob_b (weights frozen; the forward is re-computed natively)."""
    ob = _critic_ob(ctx, ob, "critic_backward")
    grad_value = _f32(grad_value, "grad_value").reshape(-1)
    B, _, H, W = ob.shape
    if grad_value.numel() != B:
        raise PnpxError(f"critic_backward: grad_value must have {B} entries, got {grad_value.numel()}")
    grad_ob = torch.empty_like(ob)
    if B:
        with torch.cuda.device(ob.device):
            check(_lib.lib().pnpx_critic_backward(ctx.handle, _p(ob), _p(grad_value), _p(grad_ob), B, H, W, _stream(ob)))
    return grad_ob


def critic_param_grad(ctx, ob, grad_value):
    """Flat fp32 vector [n_params] on ob's device, load_critic_device's order: d sum(grad_value * V) / d params of the loaded
    critic -- value_loss.backward() of trainer/mddpg/trainer.py:198,207 with grad_value = d value_loss / d V.  Overwrites,
    does not accumulate; the forward is re-computed natively."""
    ob = _critic_ob(ctx, ob, "critic_param_grad")
    grad_value = _f32(grad_value, "grad_value").reshape(-1)
    B, _, H, W = ob.shape
    if grad_value.numel() != B:
        raise PnpxError(f"critic_param_grad: grad_value must have {B} entries, got {grad_value.numel()}")
    n = int(_lib.lib().pnpx_critic_num_params(ctx._critic))
    if B == 0:
        return torch.zeros((n,), device=ob.device, dtype=torch.float32)
    out = torch.empty((n,), device=ob.device, dtype=torch.float32)
    with torch.cuda.device(ob.device):
        check(_lib.lib().pnpx_critic_param_grad(ctx.handle, _p(ob), _p(grad_value), _p(out), n, B, H, W, _stream(ob)))
    return out


def critic_value_loss_grad(ctx, ob, q_target):
    """(V [B,1], value_loss [], grad [n_params]) from one forward of the loaded critic: value_loss = nn.MSELoss()(q_target, V) and
    value_loss.backward() (trainer/mddpg/trainer.py:198,207).  V has critic_forward's bytes, grad those of
    critic_param_grad(ctx, ob, 2.0 * (V - q_target) / B); q_target [B] or [B,1] is the detached target."""
    if not isinstance(ob, torch.Tensor) or not isinstance(q_target, torch.Tensor):
        raise PnpxError("critic_value_loss_grad: ob and q_target must be torch.Tensors")
    if ob.dim() == 4 and q_target.numel() != ob.shape[0]:
        raise PnpxError(f"critic_value_loss_grad: q_target must have {ob.shape[0]} entries, got {q_target.numel()}")
    ob = _critic_ob(ctx, ob, "critic_value_loss_grad")
    q_target = _f32(q_target, "q_target").reshape(-1)
    B, _, H, W = ob.shape
    if B == 0:
        raise PnpxError("critic_value_loss_grad: the mean over an empty batch is undefined")
    n = int(_lib.lib().pnpx_critic_num_params(ctx._critic))
    value = torch.empty((B, 1), device=ob.device, dtype=torch.float32)
    loss = torch.empty((), device=ob.device, dtype=torch.float32)
    grad = torch.empty((n,), device=ob.device, dtype=torch.float32)
    with torch.cuda.device(ob.device):
        check(_lib.lib().pnpx_critic_value_loss_grad(ctx.handle, _p(ob), _p(q_target), _p(value), _p(loss), _p(grad), n, B, H, W,
                                                     _stream(ob)))
    return value, loss, grad


def unet_profile(ctx, x, sigma):
    """[(name, ms, flops)] per kernel launch of one denoiser forward (HIP events on the current stream)."""
    x = _f32(x, "x")
    sigma = _f32(sigma, "sigma").reshape(-1)
    B, _, H, W = x.shape
    out = torch.empty_like(x)
    cap = 1000
    ms = (C.c_float * cap)()
    fl = (C.c_double * cap)()
    names = (C.c_char_p * cap)()
    n = C.c_int(0)
    with torch.cuda.device(x.device):
        check(_lib.lib().pnpx_unet_profile(ctx.handle, _p(x), _p(sigma), _p(out), B, H, W, _stream(x), cap, ms, fl,
                                           names, C.byref(n)))
    return [(names[i].decode(), float(ms[i]), float(fl[i])) for i in range(n.value)]


# ------------------------------------------------------------------------------------------------- transforms
def fft2(x, inverse=False, centered=True, ctx=None):
    x = _f32(x, "data")
    if x.dim() < 3 or x.shape[-1] != 2:
        raise AssertionError("fft2 expects [..., H, W, 2]")  # the reference asserts data.size(-1) == 2
    H, W = x.shape[-3], x.shape[-2]
    n_img = x.numel() // (H * W * 2)
    out = torch.empty_like(x)
    ctx = ctx or default_context(x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pnpx_fft2(ctx.handle, _p(x), _p(out), n_img, H, W, int(inverse), int(centered), _stream(x)))
    return out


def cdp_forward(x, mask, ctx=None):
    mask = _f32(mask, "mask")
    if mask.shape[-1] != 2:
        raise AssertionError("mask must be complex [..., 2]")
    x = _f32(x, "data")
    if x.dim() == 4:
        x = torch.stack([x, torch.zeros_like(x)], -1)
    B, S, H, W, _ = mask.shape
    out = torch.empty_like(mask)
    ctx = ctx or default_context(x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pnpx_cdp_forward(ctx.handle, _p(x), _p(mask), _p(out), B, S, H, W, _stream(x)))
    return out


def cdp_backward(y, mask, ctx=None):
    mask = _f32(mask, "mask")
    y = _f32(y, "data")
    B, S, H, W, _ = mask.shape
    out = torch.empty((B, 1, H, W, 2), device=y.device, dtype=torch.float32)
    ctx = ctx or default_context(y.device)
    with torch.cuda.device(y.device):
        check(_lib.lib().pnpx_cdp_backward(ctx.handle, _p(y), _p(mask), _p(out), B, S, H, W, _stream(y)))
    return out


def spi_inverse(ztilde, K1, K, mu, ctx=None):
    ztilde = _f32(ztilde, "ztilde")
    B, _, H, W = ztilde.shape
    K1 = _f32(K1, "K1").expand_as(ztilde).contiguous()
    K = _f32(K, "K").reshape(B, -1)[:, 0].contiguous()
    mu = _f32(mu, "mu").reshape(B, -1)[:, 0].contiguous()
    out = torch.empty_like(ztilde)
    ctx = ctx or default_context(ztilde.device)
    with torch.cuda.device(ztilde.device):
        check(_lib.lib().pnpx_spi_inverse(ctx.handle, _p(ztilde), _p(K1), _p(K), _p(mu), _p(out), B, H, W,
                                          _stream(ztilde)))
    return out


def spi_pg_step(x, x0, Kmap, tau, ctx=None):
    """pnpx_spi_pg_step: one gradient step of PGSolver_SPI without the denoiser, clamp(x - tau h(x), 0, 1) (include/pnpx.h; the
    reference has no counterpart).  x, x0 [B,1,H,W]; Kmap = K / 10 as the solver state carries it, [B,1,H,W] or one value per
    item; tau one value per item."""
    x = _f32(x, "x")
    if x.dim() != 4 or x.shape[1] != 1:
        raise PnpxError(f"spi_pg_step: x must be [B,1,H,W], got {tuple(x.shape)}")
    B, _, H, W = x.shape
    x0 = _f32(x0, "x0")
    Kmap, tau = _f32(Kmap, "K"), _f32(tau, "tau")
    if tuple(x0.shape) != tuple(x.shape) or Kmap.numel() not in (B, x.numel()) or tau.numel() != B:
        raise PnpxError("spi_pg_step: x0 must be [B,1,H,W] like x, K [B,1,H,W] or one value per item, tau one value per item")
    if Kmap.numel() != x.numel():                       # only [b,0,0,0] is read, at item stride H*W
        Kmap = Kmap.reshape(B, 1).expand(B, H * W).contiguous()
    tau = tau.reshape(B).contiguous()
    out = torch.empty_like(x)
    if B == 0:
        return out
    ctx = ctx or default_context(x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().pnpx_spi_pg_step(ctx.handle, _p(x), _p(x0), _p(Kmap), _p(tau), _p(out), B, H, W, _stream(x)))
    return out


def psnr(output, gt, ctx=None):
    output = _f32(output, "output")
    gt = _f32(gt, "gt")
    B = output.shape[0]
    if gt.numel() != output.numel():
        raise PnpxError("psnr: output and gt differ in size")
    out = torch.empty((B, 1), device=output.device, dtype=torch.float32)
    if B == 0:
        return out
    n = output.numel() // B
    ctx = ctx or default_context(output.device)
    with torch.cuda.device(output.device):
        check(_lib.lib().pnpx_psnr(ctx.handle, _p(output), _p(gt), _p(out), B, n, _stream(output)))
    return out


def mddpg_policy_loss(ctx, p_stop, idx_stop, v_cur, v_next_target, v_next, reward, discount, loop_penalty, lambda_e):
    """trainer/mddpg/trainer.py:174, :179-197 and the backward of policy_loss in ONE launch (pnpx_mddpg_policy_loss).
    p_stop [B, 2] fp32; idx_stop [B] int64: 0 = continue, 1 = stop -- the values are not checked (that would be a device read),
    and any other non-zero value counts as 1, as include/pnpx.h says; v_cur, v_next_target, v_next, reward: B fp32 values each ([B] or [B, 1]),
    reward as PnPEnv.forward returns it (loop_penalty is subtracted inside).  ctx None: the default context of p_stop's device.
    -> (q_target [B], log_prob [B], entropy [B], scalars [2] = (policy_loss, mean entropy), grad_p_stop [B, 2], grad_v_next [B],
    grad_reward [B]): the last three are the gradients of policy_loss.  Wrong lengths, CPU tensors, a wrong dtype and scalars
    that are not finite raise PnpxError."""
    named = (("p_stop", p_stop), ("idx_stop", idx_stop), ("v_cur", v_cur), ("v_next_target", v_next_target), ("v_next", v_next),
             ("reward", reward))
    for name, t in named:                      # shapes and types first (they need no device), then where the tensors live
        if not isinstance(t, torch.Tensor):
            raise PnpxError(f"mddpg_policy_loss: {name}: expected a torch.Tensor, got {type(t).__name__}")
        want = torch.int64 if name == "idx_stop" else torch.float32
        if t.dtype != want:
            raise PnpxError(f"mddpg_policy_loss: {name}: expected {want}, got {t.dtype}")
    if p_stop.dim() != 2 or p_stop.shape[1] != 2 or p_stop.shape[0] == 0:
        raise PnpxError(f"mddpg_policy_loss: p_stop must be [B, 2] with B > 0, got {tuple(p_stop.shape)}")
    B = p_stop.shape[0]
    for name, t in named[1:]:
        if t.numel() != B:
            raise PnpxError(f"mddpg_policy_loss: {name} has {t.numel()} values, p_stop has {B} rows")
    scal = [float(discount), float(loop_penalty), float(lambda_e)]
    if not all(np.isfinite(scal)):
        raise PnpxError(f"mddpg_policy_loss: discount, loop_penalty and lambda_e must be finite, got {scal}")
    for name, t in named:
        if t.device.type != "cuda":
            raise PnpxError(f"mddpg_policy_loss: {name} is on {t.device}; tfpnp_amd has no CPU path")
        if t.device != p_stop.device:
            raise PnpxError(f"mddpg_policy_loss: {name} is on {t.device}, p_stop on {p_stop.device}")
    p_stop, *rows = (t.detach().contiguous() for _, t in named)
    new = lambda *shape: torch.empty(shape, device=p_stop.device, dtype=torch.float32)
    outs = (new(B), new(B), new(B), new(2), new(B, 2), new(B), new(B))
    ctx = ctx or default_context(p_stop.device)
    with torch.cuda.device(p_stop.device):
        check(_lib.lib().pnpx_mddpg_policy_loss(ctx.handle, _p(p_stop), *(_p(t) for t in rows), *scal, B,
                                                *(_p(t) for t in outs), _stream(p_stop)))
    return outs


# ------------------------------------------------------------------------------------------------- solver loops
def _vars(variables, nvar, complex_):
    v = _f32(variables, "variables")
    want = 5 if complex_ else 4
    if v.dim() != want or v.shape[1] != nvar or (complex_ and v.shape[-1] != 2):
        raise PnpxError(f"solver state must be [B,{nvar},H,W{',2' if complex_ else ''}], got {tuple(v.shape)}")
    return v


def _train_T(B, params, iter_num):
    ps, T = _params(B, *params)
    if iter_num is not None:
        if iter_num > T:
            raise PnpxError(f"iter_num {iter_num} exceeds the {T} hyper-parameter columns provided")
        T = iter_num
    return ps, T


class _Loop(NamedTuple):
    """One native solver loop (pnpx_<name>, pnpx_<name>_train, pnpx_<name>_backward) as the two call helpers below see it."""
    name: str                      # entry name without the pnpx_ prefix
    nvar: int                      # state variables ...
    complex_: bool                 # ... complex [B,nvar,H,W,2] or real [B,nvar,H,W]
    aux: Callable                  # (loop, state, aux arguments, backward) -> (leading C arguments, size arguments, pixels, S):
                                   # validates the measurement tensors and the extra integers (S, n_view, opnorm)
    nhyper: int                    # hyper-parameter tensors, sigma_d first
    saved_px: Callable             # S -> floats of `saved` per pixel and iteration
    work_px: int                   # floats of the backward's work buffer per pixel ...
    work_tail: Callable = None     # ... plus this many, from the backward's aux arguments (CT keeps its (cos, sin) table there)
    fwd_checks_iter: bool = True   # the inference wrapper rejects iter_num > T (the train wrapper always does, the backward never)


def _c_args(lead):
    return [_p(a) if isinstance(a, torch.Tensor) else a for a in lead]


def _solver_forward(L, ctx, variables, aux_args, params, iter_num, train):
    """pnpx_<name> -> next state, or pnpx_<name>_train -> (next state, saved [saved_px*T*B*pixels], ticket of the context's
    activation cache (int, 0 = not cached))."""
    v = _vars(variables, L.nvar, L.complex_)
    lead, dims, px, S = L.aux(L, v, aux_args, False)
    B = dims[0]
    if train or L.fwd_checks_iter:
        ps, T = _train_T(B, params, iter_num)
    else:
        ps, T = _params(B, *params)
        T = T if iter_num is None else iter_num
    out = torch.empty_like(v)
    saved = torch.empty(L.saved_px(S) * T * B * px, dtype=torch.float32, device=v.device) if train else None
    if B == 0:
        return (out, saved, 0) if train else out
    ticket = C.c_ulonglong(0)
    fn = getattr(_lib.lib(), f"pnpx_{L.name}_train" if train else f"pnpx_{L.name}")
    with torch.cuda.device(v.device):
        check(fn(ctx.handle, _p(v), _p(out), *_c_args(lead), *[_p(p) for p in ps], ps[0].shape[1], *dims, T,
                 *((_p(saved), C.byref(ticket)) if train else ()), _stream(v)))
    return (out, saved, int(ticket.value)) if train else out


def _solver_backward(L, ctx, aux_args, params, saved, grad_out, iter_num, ticket):
    """pnpx_<name>_backward -> (grad variables, one gradient [B,T] per hyper-parameter)."""
    g = _vars(grad_out, L.nvar, L.complex_)
    lead, dims, px, S = L.aux(L, g, aux_args, True)
    B = dims[0]
    ps, T = _params(B, *params)
    T = T if iter_num is None else iter_num
    if saved.numel() != L.saved_px(S) * T * B * px:
        raise PnpxError("saved does not belong to a forward of this shape / iteration count")
    gin = torch.empty_like(g)
    gs = [torch.zeros(T, B, dtype=torch.float32, device=g.device) for _ in range(L.nhyper)]
    if B and T:
        tail = L.work_tail(*aux_args) if L.work_tail else 0
        work = torch.empty(L.work_px * B * px + tail, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            check(getattr(_lib.lib(), f"pnpx_{L.name}_backward")(
                ctx.handle, *_c_args(lead), *[_p(p) for p in ps], ps[0].shape[1], _p(saved), _p(g), _p(gin),
                *[_p(x) for x in gs], _p(work), *dims, T, int(ticket), _stream(g)))
    elif B:
        gin.copy_(g)
    return (gin, *[x.t().contiguous() for x in gs])


def _aux_csmri(L, v, args, backward):
    B, H, W = v.shape[0], v.shape[2], v.shape[3]
    y0, m = _f32(args[0], "y0"), _mask_u8(args[1])
    if not backward and (y0.numel() != B * H * W * 2 or m.numel() != B * H * W):
        raise PnpxError("y0/mask do not match the state's [B,H,W]")
    return [y0, m], (B, H, W), H * W, 1


def _aux_pr(L, v, args, backward):
    B, H, W = v.shape[0], v.shape[2], v.shape[3]
    y0, mask = _f32(args[0], "y0"), _f32(args[1], "mask")
    # pr_iadmm reads S unguarded (a mask of fewer than two dimensions is an IndexError there), pr_pg does not
    S = mask.shape[1] if L.name == "pr_iadmm" or mask.dim() == 5 else 0
    if tuple(mask.shape) != (B, S, H, W, 2) or tuple(y0.shape) != (B, S, H, W):
        raise PnpxError(f"{L.name}: y0 must be [B,S,H,W] and mask [B,S,H,W,2]")
    return [y0, mask], (B, S, H, W), H * W, S


def _aux_spi(L, v, args, backward):
    B, H, W = v.shape[0], v.shape[2], v.shape[3]
    x0, Kmap = _f32(args[0], "x0"), _f32(args[1], "K")
    if not backward and (x0.numel() != B * H * W or Kmap.numel() != B * H * W):
        raise PnpxError(f"{L.name}: x0 and K must be [B,1,H,W]")
    return [x0, Kmap], (B, H, W), H * W, 1


_CSMRI_ADMM = _Loop("csmri_admm", 3, True, _aux_csmri, 2, lambda S: 3, 3)
_CSMRI_HQS = _Loop("csmri_hqs", 2, True, _aux_csmri, 2, lambda S: 3, 3)
_CSMRI_PG = _Loop("csmri_pg", 1, True, _aux_csmri, 2, lambda S: 2, 3)
_CSMRI_APG = _Loop("csmri_apg", 2, True, _aux_csmri, 3, lambda S: 4, 4)
_CSMRI_RED = _Loop("csmri_redadmm", 3, True, _aux_csmri, 3, lambda S: 7, 4)
_PR_IADMM = _Loop("pr_iadmm", 3, True, _aux_pr, 3, lambda S: 2 * S + 5, 4, fwd_checks_iter=False)
_PR_PG = _Loop("pr_pg", 1, True, _aux_pr, 2, lambda S: 2 * S + 2, 3)
_SPI_ADMM = _Loop("spi_admm", 3, False, _aux_spi, 2, lambda S: 2, 3, fwd_checks_iter=False)
_SPI_PG = _Loop("spi_pg", 1, False, _aux_spi, 2, lambda S: 2, 3)


def csmri_admm(ctx, variables, y0, mask, sigma_d, mu, iter_num=None):
    return _solver_forward(_CSMRI_ADMM, ctx, variables, (y0, mask), (sigma_d, mu), iter_num, False)


def csmri_admm_train(ctx, variables, y0, mask, sigma_d, mu, iter_num=None):
    """pnpx_csmri_admm_train: the ADMM forward that also returns what its VJP needs -> (next state, saved [3*T*B*H*W],
    ticket of the context's activation cache (int, 0 = not cached))."""
    return _solver_forward(_CSMRI_ADMM, ctx, variables, (y0, mask), (sigma_d, mu), iter_num, True)


def csmri_admm_backward(ctx, y0, mask, sigma_d, mu, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_csmri_admm_backward -> (grad variables [B,3,H,W,2], grad sigma_d [B,T], grad mu [B,T])."""
    return _solver_backward(_CSMRI_ADMM, ctx, (y0, mask), (sigma_d, mu), saved, grad_out, iter_num, ticket)


def csmri_hqs(ctx, variables, y0, mask, sigma_d, mu, iter_num=None):
    return _solver_forward(_CSMRI_HQS, ctx, variables, (y0, mask), (sigma_d, mu), iter_num, False)


def csmri_hqs_train(ctx, variables, y0, mask, sigma_d, mu, iter_num=None):
    """pnpx_csmri_hqs_train: HQSSolver_CSMRI.forward for autograd (state [B,2,H,W,2]); same returns as csmri_admm_train."""
    return _solver_forward(_CSMRI_HQS, ctx, variables, (y0, mask), (sigma_d, mu), iter_num, True)


def csmri_hqs_backward(ctx, y0, mask, sigma_d, mu, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_csmri_hqs_backward -> (grad variables [B,2,H,W,2], grad sigma_d [B,T], grad mu [B,T])."""
    return _solver_backward(_CSMRI_HQS, ctx, (y0, mask), (sigma_d, mu), saved, grad_out, iter_num, ticket)


def csmri_pg(ctx, variables, y0, mask, sigma_d, tau, iter_num=None):
    return _solver_forward(_CSMRI_PG, ctx, variables, (y0, mask), (sigma_d, tau), iter_num, False)


def csmri_pg_train(ctx, variables, y0, mask, sigma_d, tau, iter_num=None):
    """pnpx_csmri_pg_train: PGSolver_CSMRI.forward for autograd (state [B,1,H,W,2]); saved = 2*T*B*H*W floats."""
    return _solver_forward(_CSMRI_PG, ctx, variables, (y0, mask), (sigma_d, tau), iter_num, True)


def csmri_pg_backward(ctx, y0, mask, sigma_d, tau, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_csmri_pg_backward -> (grad x [B,1,H,W,2], grad sigma_d [B,T], grad tau [B,T])."""
    return _solver_backward(_CSMRI_PG, ctx, (y0, mask), (sigma_d, tau), saved, grad_out, iter_num, ticket)


def csmri_apg(ctx, variables, y0, mask, sigma_d, tau, beta, iter_num=None):
    return _solver_forward(_CSMRI_APG, ctx, variables, (y0, mask), (sigma_d, tau, beta), iter_num, False)


def csmri_apg_train(ctx, variables, y0, mask, sigma_d, tau, beta, iter_num=None):
    """pnpx_csmri_apg_train: APGSolver_CSMRI.forward for autograd -> (next state [B,2,H,W,2], saved [4*T*B*H*W], ticket)."""
    return _solver_forward(_CSMRI_APG, ctx, variables, (y0, mask), (sigma_d, tau, beta), iter_num, True)


def csmri_apg_backward(ctx, y0, mask, sigma_d, tau, beta, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_csmri_apg_backward -> (grad variables [B,2,H,W,2], grad sigma_d, grad tau, grad beta, each [B,T])."""
    return _solver_backward(_CSMRI_APG, ctx, (y0, mask), (sigma_d, tau, beta), saved, grad_out, iter_num, ticket)


def csmri_redadmm(ctx, variables, y0, mask, sigma_d, mu, lamda, iter_num=None):
    return _solver_forward(_CSMRI_RED, ctx, variables, (y0, mask), (sigma_d, mu, lamda), iter_num, False)


def csmri_redadmm_train(ctx, variables, y0, mask, sigma_d, mu, lamda, iter_num=None):
    """pnpx_csmri_redadmm_train: REDADMMSolver_CSMRI.forward for autograd -> (next state [B,3,H,W,2], saved [7*T*B*H*W],
    ticket)."""
    return _solver_forward(_CSMRI_RED, ctx, variables, (y0, mask), (sigma_d, mu, lamda), iter_num, True)


def csmri_redadmm_backward(ctx, y0, mask, sigma_d, mu, lamda, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_csmri_redadmm_backward -> (grad variables [B,3,H,W,2], grad sigma_d, grad mu, grad lamda, each [B,T])."""
    return _solver_backward(_CSMRI_RED, ctx, (y0, mask), (sigma_d, mu, lamda), saved, grad_out, iter_num, ticket)


def csmri_amp(ctx, variables, y0, mask, sigma_d, probe, iter_num=None):
    """pnpx_csmri_amp: AMPSolver_CSMRI.forward (tasks/csmri/solver.py:211-250, prox_fun = prox_mapping, complex_norm = the
    per-item L2 norm).  variables [B,2,H,W,2]; sigma_d [B,T]; probe [>= iter_num, B, 1, H, W] = the Monte-Carlo probe
    delta of each iteration (the reference's torch.randn_like(r))."""
    v = _vars(variables, 2, True)
    B, _, H, W, _ = v.shape
    ps, T = _train_T(B, (sigma_d,), iter_num)
    d = _f32(probe, "probe")
    if d.dim() != 5 or d.shape[0] < T or tuple(d.shape[1:]) != (B, 1, H, W):
        raise PnpxError(f"probe must be [{T}, {B}, 1, {H}, {W}], got {tuple(d.shape)}")
    y0 = _f32(y0, "y0")
    m = _mask_u8(mask)
    if y0.numel() != B * H * W * 2 or m.numel() != B * H * W:
        raise PnpxError("y0/mask do not match the state's [B,H,W]")
    out = torch.empty_like(v)
    if B == 0:
        return out
    with torch.cuda.device(v.device):
        check(_lib.lib().pnpx_csmri_amp(ctx.handle, _p(v), _p(out), _p(y0), _p(m), _p(ps[0]), _p(d), ps[0].shape[1], B, H,
                                        W, T, _stream(v)))
    return out


def pr_iadmm(ctx, variables, y0, mask, sigma_d, mu, tau, iter_num=None):
    return _solver_forward(_PR_IADMM, ctx, variables, (y0, mask), (sigma_d, mu, tau), iter_num, False)


def pr_iadmm_train(ctx, variables, y0, mask, sigma_d, mu, tau, iter_num=None):
    """pnpx_pr_iadmm_train: IADMMSolver_PR.forward for autograd -> (next state [B,3,H,W,2], saved [(2S+5)*T*B*H*W], ticket)."""
    return _solver_forward(_PR_IADMM, ctx, variables, (y0, mask), (sigma_d, mu, tau), iter_num, True)


def pr_iadmm_backward(ctx, y0, mask, sigma_d, mu, tau, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_pr_iadmm_backward -> (grad variables [B,3,H,W,2], grad sigma_d, grad mu, grad tau, each [B,T])."""
    return _solver_backward(_PR_IADMM, ctx, (y0, mask), (sigma_d, mu, tau), saved, grad_out, iter_num, ticket)


def pr_pg(ctx, variables, y0, mask, sigma_d, tau, iter_num=None):
    """pnpx_pr_pg: PGSolver_PR.forward, x [B,1,H,W,2] -> next x (imaginary part 0)."""
    return _solver_forward(_PR_PG, ctx, variables, (y0, mask), (sigma_d, tau), iter_num, False)


def pr_pg_train(ctx, variables, y0, mask, sigma_d, tau, iter_num=None):
    """pnpx_pr_pg_train: PGSolver_PR.forward for autograd -> (next x [B,1,H,W,2], saved [(2S+2)*T*B*H*W], ticket)."""
    return _solver_forward(_PR_PG, ctx, variables, (y0, mask), (sigma_d, tau), iter_num, True)


def pr_pg_backward(ctx, y0, mask, sigma_d, tau, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_pr_pg_backward -> (grad x [B,1,H,W,2], grad sigma_d, grad tau, each [B,T])."""
    return _solver_backward(_PR_PG, ctx, (y0, mask), (sigma_d, tau), saved, grad_out, iter_num, ticket)


def spi_admm(ctx, variables, x0, Kmap, sigma_d, mu, iter_num=None):
    return _solver_forward(_SPI_ADMM, ctx, variables, (x0, Kmap), (sigma_d, mu), iter_num, False)


def spi_admm_train(ctx, variables, x0, Kmap, sigma_d, mu, iter_num=None):
    """pnpx_spi_admm_train: ADMMSolver_SPI.forward for autograd -> (next state [B,3,H,W], saved [2*T*B*H*W], ticket)."""
    return _solver_forward(_SPI_ADMM, ctx, variables, (x0, Kmap), (sigma_d, mu), iter_num, True)


def spi_admm_backward(ctx, x0, Kmap, sigma_d, mu, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_spi_admm_backward -> (grad variables [B,3,H,W], grad sigma_d, grad mu, each [B,T])."""
    return _solver_backward(_SPI_ADMM, ctx, (x0, Kmap), (sigma_d, mu), saved, grad_out, iter_num, ticket)


def spi_pg(ctx, variables, x0, Kmap, sigma_d, tau, iter_num=None):
    """pnpx_spi_pg: PGSolver_SPI.forward, x [B,1,H,W] -> next x (include/pnpx.h; the reference has no counterpart)."""
    return _solver_forward(_SPI_PG, ctx, variables, (x0, Kmap), (sigma_d, tau), iter_num, False)


def spi_pg_train(ctx, variables, x0, Kmap, sigma_d, tau, iter_num=None):
    """pnpx_spi_pg_train: PGSolver_SPI.forward for autograd -> (next x [B,1,H,W], saved [2*T*B*H*W], ticket)."""
    return _solver_forward(_SPI_PG, ctx, variables, (x0, Kmap), (sigma_d, tau), iter_num, True)


def spi_pg_backward(ctx, x0, Kmap, sigma_d, tau, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_spi_pg_backward -> (grad x [B,1,H,W], grad sigma_d, grad tau, each [B,T])."""
    return _solver_backward(_SPI_PG, ctx, (x0, Kmap), (sigma_d, tau), saved, grad_out, iter_num, ticket)


# ------------------------------------------------------------------------------------------------- CT
def radon_det_count(R):
    return int(_lib.lib().pnpx_radon_det_count(int(R)))


def radon_forward(img, n_view, ctx=None):
    img = _f32(img, "img")
    B, _, R, R2 = img.shape
    if R != R2:
        raise PnpxError("radon_forward: square images only")
    out = torch.empty((B, 1, n_view, radon_det_count(R)), device=img.device, dtype=torch.float32)
    ctx = ctx or default_context(img.device)
    with torch.cuda.device(img.device):
        check(_lib.lib().pnpx_radon_forward(ctx.handle, _p(img), _p(out), B, R, n_view, _stream(img)))
    return out


def radon_backprojection(sino, R, ctx=None):
    sino = _f32(sino, "sino")
    B, _, V, det = sino.shape
    if det != radon_det_count(R):
        raise PnpxError(f"sinogram has {det} detectors, resolution {R} needs {radon_det_count(R)}")
    out = torch.empty((B, 1, R, R), device=sino.device, dtype=torch.float32)
    ctx = ctx or default_context(sino.device)
    with torch.cuda.device(sino.device):
        check(_lib.lib().pnpx_radon_backprojection(ctx.handle, _p(sino), _p(out), B, R, V, _stream(sino)))
    return out


def _ct_sino(y0, B, R, n_view):
    """The native CT loops index the sinogram with a (n_view, det) stride: a mismatching tensor must not get through."""
    y0 = _f32(y0, "y0")
    want = (B, 1, int(n_view), radon_det_count(R))
    if tuple(y0.shape) != want:
        raise PnpxError(f"y0: sinogram of shape {tuple(y0.shape)} does not match (B, 1, n_view, det) = {want}")
    return y0


def _aux_ct(L, v, args, backward):
    B, R = v.shape[0], v.shape[2]
    lead = [] if backward else [_ct_sino(args[0], B, R, args[1])]   # the backward entries take no sinogram
    n_view, opnorm = args[-2:]
    return lead + [int(n_view), float(opnorm)], (B, R), R * R, 1


_CT_IADMM = _Loop("ct_iadmm", 3, False, _aux_ct, 3, lambda S: 3, 6, lambda n_view, opnorm: 2 * int(n_view),
                  fwd_checks_iter=False)
# +1: the float2 table stands at an even float offset
_CT_PG = _Loop("ct_pg", 1, False, _aux_ct, 2, lambda S: 2, 3, lambda n_view, opnorm: 1 + 2 * int(n_view),
               fwd_checks_iter=False)


def ct_iadmm(ctx, variables, y0, n_view, opnorm, sigma_d, mu, tau, iter_num=None):
    return _solver_forward(_CT_IADMM, ctx, variables, (y0, n_view, opnorm), (sigma_d, mu, tau), iter_num, False)


def ct_pg(ctx, variables, y0, n_view, opnorm, sigma_d, tau, iter_num=None):
    return _solver_forward(_CT_PG, ctx, variables, (y0, n_view, opnorm), (sigma_d, tau), iter_num, False)


def ct_iadmm_train(ctx, variables, y0, n_view, opnorm, sigma_d, mu, tau, iter_num=None):
    """pnpx_ct_iadmm_train: IADMMSolver_CT.forward for autograd -> (next state [B,3,R,R], saved [3*T*B*R*R], ticket)."""
    return _solver_forward(_CT_IADMM, ctx, variables, (y0, n_view, opnorm), (sigma_d, mu, tau), iter_num, True)


def ct_iadmm_backward(ctx, n_view, opnorm, sigma_d, mu, tau, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_ct_iadmm_backward -> (grad variables [B,3,R,R], grad sigma_d, grad mu, grad tau, each [B,T])."""
    return _solver_backward(_CT_IADMM, ctx, (n_view, opnorm), (sigma_d, mu, tau), saved, grad_out, iter_num, ticket)


def ct_pg_train(ctx, variables, y0, n_view, opnorm, sigma_d, tau, iter_num=None):
    """pnpx_ct_pg_train: PGSolver_CT.forward for autograd -> (next x [B,1,R,R], saved [2*T*B*R*R], ticket)."""
    return _solver_forward(_CT_PG, ctx, variables, (y0, n_view, opnorm), (sigma_d, tau), iter_num, True)


def ct_pg_backward(ctx, n_view, opnorm, sigma_d, tau, saved, grad_out, iter_num=None, ticket=0):
    """pnpx_ct_pg_backward -> (grad x [B,1,R,R], grad sigma_d, grad tau, each [B,T])."""
    return _solver_backward(_CT_PG, ctx, (n_view, opnorm), (sigma_d, tau), saved, grad_out, iter_num, ticket)


# ------------------------------------------------------------------------------------------------- CT, fan beam
def fan_geom(n_view, det_count, source_distance, det_distance, det_spacing):
    """include/pnpx.h: a pnpx_radon_geom of kind PNPX_GEOM_FAN.  Nothing is checked here: the native entries refuse a bad one."""
    return _lib.RadonGeom(_lib.PNPX_GEOM_FAN, int(n_view), int(det_count), float(source_distance), float(det_distance),
                          float(det_spacing))


def fan_det_count(R, source_distance, det_distance, det_spacing):
    """pnpx_fan_det_count: the bin count of the fan that just covers the sampled circle (host only)."""
    n = int(_lib.lib().pnpx_fan_det_count(int(R), float(source_distance), float(det_distance), float(det_spacing)))
    if n <= 0:
        raise PnpxError(_lib.lib().pnpx_last_error().decode("utf-8", "replace"))
    return n


def fan_tables(R, n_view, det_count, source_distance, det_distance, det_spacing):
    """pnpx_fan_tables (host only) -> (view table [n_view, 2], bin table [det_count, 3], LDS window in bins or 0 = gather kernel)."""
    g = fan_geom(n_view, det_count, source_distance, det_distance, det_spacing)
    cs = np.zeros((max(int(n_view), 0), 2), np.float32)
    bins = np.zeros((max(int(det_count), 0), 3), np.float32)
    win = C.c_int(0)
    check(_lib.lib().pnpx_fan_tables(g, int(R), cs.ctypes.data_as(_lib.c_float_p), bins.ctypes.data_as(_lib.c_float_p), C.byref(win)))
    return cs, bins, int(win.value)


def fan_forward(img, n_view, det_count, source_distance, det_distance, det_spacing, ctx=None):
    """pnpx_fan_forward: [B,1,R,R] -> [B,1,n_view,det_count]."""
    img = _f32(img, "img")
    B, _, R, R2 = img.shape
    if R != R2:
        raise PnpxError("fan_forward: square images only")
    g = fan_geom(n_view, det_count, source_distance, det_distance, det_spacing)
    out = torch.empty((B, 1, max(int(n_view), 0), max(int(det_count), 0)), device=img.device, dtype=torch.float32)
    ctx = ctx or default_context(img.device)
    with torch.cuda.device(img.device):
        check(_lib.lib().pnpx_fan_forward(ctx.handle, _p(img), _p(out), g, B, R, _stream(img)))
    return out


_FAN_WEIGHTS = {"adjoint": _lib.PNPX_FAN_W_ADJOINT, "fbp": _lib.PNPX_FAN_W_FBP}


def fan_backprojection(sino, R, source_distance, det_distance, det_spacing, ctx=None, weight=None):
    """pnpx_fan_backprojection: [B,1,n_view,det_count] -> [B,1,R,R] (weighted: include/pnpx.h).  weight 'adjoint' or 'fbp':
    pnpx_fan_backprojection_w with the pair's ray-density weight (the same bytes) or filtered backprojection's (D_so / U)^2."""
    sino = _f32(sino, "sino")
    B, _, V, det = sino.shape
    g = fan_geom(V, det, source_distance, det_distance, det_spacing)
    if weight is not None and weight not in _FAN_WEIGHTS:
        raise PnpxError(f"fan_backprojection: weight must be one of {sorted(_FAN_WEIGHTS)}, got {weight!r}")
    out = torch.empty((B, 1, int(R), int(R)), device=sino.device, dtype=torch.float32)
    ctx = ctx or default_context(sino.device)
    with torch.cuda.device(sino.device):
        if weight is None:
            check(_lib.lib().pnpx_fan_backprojection(ctx.handle, _p(sino), _p(out), g, B, int(R), _stream(sino)))
        else:
            check(_lib.lib().pnpx_fan_backprojection_w(ctx.handle, _p(sino), _p(out), g, _FAN_WEIGHTS[weight], B, int(R),
                                                       _stream(sino)))
    return out


def radon_filter(sino, source_distance=None, det_distance=None, det_spacing=None, ctx=None):
    """pnpx_radon_filter: the ramp filter of filtered backprojection along the detector axis, [B,1,n_view,det] -> the same shape
    (a new tensor).  No distances: the parallel beam's filter (Radon_norm.filter_sinogram's result); with them the fan beam's, with
    the cos gamma pre-weight and S = pi / (n_view dp) (include/pnpx.h)."""
    sino = _f32(sino, "sino")
    B, _, V, det = sino.shape
    g = None if source_distance is None else fan_geom(V, det, source_distance, det_distance, det_spacing)
    out = torch.empty_like(sino)
    ctx = ctx or default_context(sino.device)
    with torch.cuda.device(sino.device):
        check(_lib.lib().pnpx_radon_filter(ctx.handle, _p(sino), _p(out), g, B, V, det, _stream(sino)))
    return out


def fan_fbp(sino, R, source_distance, det_distance, det_spacing, ctx=None):
    """pnpx_fan_fbp: filtered backprojection of a fan-beam sinogram, [B,1,n_view,det_count] -> [B,1,R,R]."""
    sino = _f32(sino, "sino")
    B, _, V, det = sino.shape
    g = fan_geom(V, det, source_distance, det_distance, det_spacing)
    out = torch.empty((B, 1, int(R), int(R)), device=sino.device, dtype=torch.float32)
    ctx = ctx or default_context(sino.device)
    with torch.cuda.device(sino.device):
        check(_lib.lib().pnpx_fan_fbp(ctx.handle, _p(sino), _p(out), g, B, int(R), _stream(sino)))
    return out


def _aux_ct_hqs(L, v, args, backward):
    """aux = ([y0,] n_view, opnorm, det_count, source_distance, det_distance, det_spacing); det_count 0 = parallel beam."""
    B, R = v.shape[0], v.shape[2]
    n_view, opnorm, det_count, dso, dod, du = args[-6:]
    geom = fan_geom(n_view, det_count, dso, dod, du) if int(det_count) else None
    lead = []
    if not backward:            # the backward entry takes no sinogram
        y0 = _f32(args[0], "y0")
        want = (B, 1, int(n_view), int(det_count) if int(det_count) else radon_det_count(R))
        if tuple(y0.shape) != want:
            raise PnpxError(f"y0: sinogram of shape {tuple(y0.shape)} does not match (B, 1, n_view, det) = {want}")
        lead = [y0]
    return lead + [geom, int(n_view), float(opnorm)], (B, R), R * R, 1


_CT_HQS = _Loop("ct_hqs", 2, False, _aux_ct_hqs, 2, lambda S: 3, 5,
                lambda n_view, opnorm, det_count, *_: 4 + 2 * int(n_view) + 4 * int(det_count))


def ct_hqs(ctx, variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, mu, iter_num=None):
    """pnpx_ct_hqs: HQSSolver_CT.forward, state [B,2,R,R]; det_count 0 = the parallel pair (the distances are not read then)."""
    return _solver_forward(_CT_HQS, ctx, variables, (y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing),
                           (sigma_d, mu), iter_num, False)


def ct_hqs_train(ctx, variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, mu,
                 iter_num=None):
    """pnpx_ct_hqs_train: HQSSolver_CT.forward for autograd -> (next state [B,2,R,R], saved [3*T*B*R*R], ticket)."""
    return _solver_forward(_CT_HQS, ctx, variables, (y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing),
                           (sigma_d, mu), iter_num, True)


def ct_hqs_backward(ctx, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, mu, saved, grad_out,
                    iter_num=None, ticket=0):
    """pnpx_ct_hqs_backward -> (grad variables [B,2,R,R], grad sigma_d, grad mu, each [B,T])."""
    return _solver_backward(_CT_HQS, ctx, (n_view, opnorm, det_count, source_distance, det_distance, det_spacing), (sigma_d, mu),
                            saved, grad_out, iter_num, ticket)


# iADMM and PG on a chosen geometry: the aux tuple of ct_hqs; the work tails of ct_iadmm / ct_pg, plus the aligned fan tables
_CT_IADMM_GEOM = _Loop("ct_iadmm_geom", 3, False, _aux_ct_hqs, 3, lambda S: 3, 6,
                       lambda n_view, opnorm, det_count, *_: 2 * int(n_view) + (4 + 4 * int(det_count) if int(det_count) else 0),
                       fwd_checks_iter=False)
_CT_PG_GEOM = _Loop("ct_pg_geom", 1, False, _aux_ct_hqs, 2, lambda S: 2, 3,
                    lambda n_view, opnorm, det_count, *_: 1 + 2 * int(n_view) + (3 + 4 * int(det_count) if int(det_count) else 0),
                    fwd_checks_iter=False)


def ct_iadmm_geom(ctx, variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, mu, tau,
                  iter_num=None):
    """pnpx_ct_iadmm_geom: IADMMSolver_CT.forward on a chosen geometry; det_count 0 = the parallel pair, the bytes of ct_iadmm."""
    return _solver_forward(_CT_IADMM_GEOM, ctx, variables, (y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing),
                           (sigma_d, mu, tau), iter_num, False)


def ct_iadmm_geom_train(ctx, variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, mu, tau,
                        iter_num=None):
    """pnpx_ct_iadmm_geom_train -> (next state [B,3,R,R], saved [3*T*B*R*R], ticket)."""
    return _solver_forward(_CT_IADMM_GEOM, ctx, variables, (y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing),
                           (sigma_d, mu, tau), iter_num, True)


def ct_iadmm_geom_backward(ctx, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, mu, tau, saved,
                           grad_out, iter_num=None, ticket=0):
    """pnpx_ct_iadmm_geom_backward -> (grad variables [B,3,R,R], grad sigma_d, grad mu, grad tau, each [B,T])."""
    return _solver_backward(_CT_IADMM_GEOM, ctx, (n_view, opnorm, det_count, source_distance, det_distance, det_spacing),
                            (sigma_d, mu, tau), saved, grad_out, iter_num, ticket)


def ct_pg_geom(ctx, variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, tau, iter_num=None):
    """pnpx_ct_pg_geom: PGSolver_CT.forward on a chosen geometry; det_count 0 = the parallel pair, the bytes of ct_pg."""
    return _solver_forward(_CT_PG_GEOM, ctx, variables, (y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing),
                           (sigma_d, tau), iter_num, False)


def ct_pg_geom_train(ctx, variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, tau,
                     iter_num=None):
    """pnpx_ct_pg_geom_train -> (next x [B,1,R,R], saved [2*T*B*R*R], ticket)."""
    return _solver_forward(_CT_PG_GEOM, ctx, variables, (y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing),
                           (sigma_d, tau), iter_num, True)


def ct_pg_geom_backward(ctx, n_view, opnorm, det_count, source_distance, det_distance, det_spacing, sigma_d, tau, saved, grad_out,
                        iter_num=None, ticket=0):
    """pnpx_ct_pg_geom_backward -> (grad x [B,1,R,R], grad sigma_d, grad tau, each [B,T])."""
    return _solver_backward(_CT_PG_GEOM, ctx, (n_view, opnorm, det_count, source_distance, det_distance, det_spacing), (sigma_d, tau),
                            saved, grad_out, iter_num, ticket)


# ------------------------------------------------------------------------------------- episode orchestration (env.hip)
def _dense(t, name):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise PnpxError(f"{name}: expected a tensor on a ROCm device (there is no CPU path)")
    return t if t.is_contiguous() else t.contiguous()


def _idx64(idx, name):
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.device.type != "cuda":
        raise PnpxError(f"{name}: expected an int64 tensor on a ROCm device")
    return idx if idx.is_contiguous() else idx.contiguous()


def _rows_call(fn, srcs, dsts, small, idx, n_rows, dev):
    n = len(srcs)
    S = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    D = (C.c_void_p * n)(*[d.data_ptr() for d in dsts])
    RB = (C.c_size_t * n)(*[(t.numel() // max(t.shape[0], 1)) * t.element_size() for t in small])
    ctx = default_context(dev)
    with torch.cuda.device(dev):
        check(fn(ctx.handle, n, S, D, RB, _p(idx), int(n_rows), _stream(idx)))


def rows_gather(tensors, idx, n_rows):
    """[t[idx[:n_rows]] for t in tensors] in ONE launch (tfpnp/env/base.py:162-166).  idx: device int64 (capacity >=
    n_rows); dtypes are preserved (fp32 state, bool masks)."""
    idx = _idx64(idx, "idx")
    srcs = [_dense(t, "tensor") for t in tensors]
    outs = [torch.empty((n_rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in srcs]
    if n_rows > 0 and srcs:
        _rows_call(_lib.lib().pnpx_rows_gather, srcs, outs, outs, idx, n_rows, idx.device)
    return outs


def rows_scatter(values, targets, idx, n_rows):
    """targets[k][idx[:n_rows]] = values[k] for every k, in ONE launch (tfpnp/env/base.py:171-172).  In place."""
    idx = _idx64(idx, "idx")
    vals = []
    for v, t in zip(values, targets):
        if not t.is_contiguous() or t.device.type != "cuda":
            raise PnpxError("rows_scatter: targets must be contiguous device tensors")
        v = _dense(v, "value")
        if v.dtype != t.dtype or tuple(v.shape[1:]) != tuple(t.shape[1:]) or v.shape[0] < n_rows:
            raise PnpxError(f"rows_scatter: value {tuple(v.shape)}/{v.dtype} does not fit target {tuple(t.shape)}/{t.dtype}")
        vals.append(v)
    if n_rows > 0 and vals:
        _rows_call(_lib.lib().pnpx_rows_scatter, vals, list(targets), vals, idx, n_rows, idx.device)


def ring_store(values, storages, first_slot, n_rows):
    """storages[k][(first_slot + r) % capacity] = values[k][r] for r < n_rows and every k, in ONE launch per 12 tensors: the
    replay-memory store of a whole batch (tfpnp/trainer/mddpg/trainer.py:232-234 over tfpnp/utils/rpm.py:10-19).  In place;
    capacity = the storages' common leading dimension; 0 <= first_slot < capacity, 0 <= n_rows <= capacity.  The slot is
    computed on the device, no index tensor is built.  Issued on the current stream of the storages' device."""
    storages = list(storages)
    values = list(values)
    if len(values) != len(storages):
        raise PnpxError(f"ring_store: {len(values)} values for {len(storages)} storages")
    vals = []
    for v, t in zip(values, storages):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or not t.is_contiguous() or t.dim() < 1:
            raise PnpxError("ring_store: storages must be contiguous device tensors")
        if t.shape[0] != storages[0].shape[0] or t.device != storages[0].device:
            raise PnpxError("ring_store: storages must share their leading dimension (the capacity) and their device")
        v = _dense(v, "value")
        if v.dtype != t.dtype or tuple(v.shape[1:]) != tuple(t.shape[1:]) or v.shape[0] < n_rows or v.device != t.device:
            raise PnpxError(f"ring_store: value {tuple(v.shape)}/{v.dtype} does not fit storage {tuple(t.shape)}/{t.dtype}")
        vals.append(v)
    if not vals:
        return
    capacity = int(storages[0].shape[0])
    first_slot, n_rows = int(first_slot), int(n_rows)
    if not (0 <= first_slot < capacity and 0 <= n_rows <= capacity):
        raise PnpxError(f"ring_store: first_slot {first_slot} / n_rows {n_rows} outside a ring of capacity {capacity}")
    if n_rows == 0:
        return
    n = len(vals)
    S = (C.c_void_p * n)(*[v.data_ptr() for v in vals])
    D = (C.c_void_p * n)(*[t.data_ptr() for t in storages])
    RB = (C.c_size_t * n)(*[(t.numel() // capacity) * t.element_size() for t in storages])
    dev = storages[0].device
    ctx = default_context(dev)
    with torch.cuda.device(dev):
        check(_lib.lib().pnpx_ring_store(ctx.handle, n, S, D, RB, first_slot, capacity, n_rows, _stream(storages[0])))


def live_compact(idx_left, idx_stop, n):
    """(idx_left[:n][idx_stop == 0] in a buffer of capacity n, number of survivors as a Python int).
    Synchronises the current stream: the one host read of an env step (tfpnp/env/base.py:180-182)."""
    idx_left = _idx64(idx_left, "idx_left")
    idx_stop = _idx64(idx_stop, "idx_stop")
    if idx_stop.numel() < n or idx_left.numel() < n:
        raise PnpxError("live_compact: idx_left / idx_stop shorter than n")
    out = torch.empty((max(n, 1),), dtype=torch.int64, device=idx_left.device)
    cnt = C.c_int(0)
    ctx = default_context(idx_left.device)
    with torch.cuda.device(idx_left.device):
        check(_lib.lib().pnpx_live_compact(ctx.handle, _p(idx_left), _p(idx_stop), int(n), _p(out), C.byref(cnt),
                                           _stream(idx_left)))
    return out, int(cnt.value)


_PACK_KINDS = {"raw": 0, "real": 1, "channel": 2, "u8": 3}


def policy_ob_pack(entries, idx=None, n_rows=None):
    """Fused get_policy_ob (tasks/*/env.py): entries = [(tensor, 'raw' | 'real' | 'channel'), ...] in channel order;
    'raw' fp32/bool [B,c,H,W], 'real' / 'channel' complex [B,c,H,W,2].  idx/n_rows: gather rows idx[:n_rows] on the fly."""
    srcs, kinds, chans = [], [], []
    H = W = None
    for t, kind in entries:
        t = _dense(t, "observation entry")
        if kind == "raw":
            if t.dim() != 4:
                raise PnpxError(f"policy_ob_pack: raw entry must be [B,c,H,W], got {tuple(t.shape)}")
            if t.dtype in (torch.bool, torch.uint8):
                k = "u8"
            elif t.dtype == torch.float32:
                k = "raw"
            else:
                raise PnpxError(f"policy_ob_pack: unsupported dtype {t.dtype}")
        elif kind in ("real", "channel"):
            if t.dim() != 5 or t.shape[-1] != 2 or t.dtype != torch.float32:
                raise PnpxError(f"policy_ob_pack: {kind} entry must be fp32 [B,c,H,W,2], got {tuple(t.shape)}")
            k = kind
        else:
            raise PnpxError(f"policy_ob_pack: unknown kind {kind}")
        if H is None:
            H, W = t.shape[2], t.shape[3]
        elif (t.shape[2], t.shape[3]) != (H, W):
            raise PnpxError("policy_ob_pack: entries disagree on H, W")
        srcs.append(t)
        kinds.append(_PACK_KINDS[k])
        chans.append(t.shape[1])
    n = len(srcs)
    if n == 0:
        raise PnpxError("policy_ob_pack: no entries")
    rows = srcs[0].shape[0] if n_rows is None else int(n_rows)
    C_out = sum(c * (2 if k == 2 else 1) for c, k in zip(chans, kinds))
    out = torch.empty((rows, C_out, H, W), dtype=torch.float32, device=srcs[0].device)
    if rows == 0:
        return out
    if idx is not None:
        idx = _idx64(idx, "idx")
    S = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    K = (C.c_int * n)(*kinds)
    CH = (C.c_int * n)(*chans)
    ctx = default_context(out.device)
    with torch.cuda.device(out.device):
        check(_lib.lib().pnpx_policy_ob_pack(ctx.handle, n, S, K, CH, _p(idx) if idx is not None else None, rows, H, W,
                                             _p(out), _stream(out)))
    return out


def policy_ob_unpack(grad_out, kinds, channels):
    """Adjoint of policy_ob_pack for dense rows: grad_out [B, sum(channels), H, W] -> one gradient per entry with the
    entry's shape ([B,c,H,W] for kind 0, [B,c,H,W,2] for kinds 1 / 2: imaginary part zero for 'real'); None for kind 3
    (bool / uint8 entries).  kinds / channels: the pack's integer kinds (0 raw, 1 real, 2 channel, 3 u8) and source channels."""
    g = _f32(grad_out, "grad_out")
    kinds, channels = [int(k) for k in kinds], [int(c) for c in channels]
    n = len(kinds)
    if g.dim() != 4 or n == 0 or n != len(channels) or any(k not in (0, 1, 2, 3) for k in kinds) or \
            g.shape[1] != sum(c * (2 if k == 2 else 1) for c, k in zip(channels, kinds)):
        raise PnpxError("policy_ob_unpack: grad_out does not match the entry layout")
    B, _, H, W = g.shape
    outs = [None if k == 3 else torch.empty((B, c, H, W) + ((2,) if k else ()), dtype=torch.float32, device=g.device)
            for k, c in zip(kinds, channels)]
    if B == 0:
        return outs
    D = (C.c_void_p * n)(*[o.data_ptr() if o is not None else None for o in outs])
    K = (C.c_int * n)(*kinds)
    CH = (C.c_int * n)(*channels)
    ctx = default_context(g.device)
    with torch.cuda.device(g.device):
        check(_lib.lib().pnpx_policy_ob_unpack(ctx.handle, n, D, K, CH, B, H, W, _p(g), _stream(g)))
    return outs
