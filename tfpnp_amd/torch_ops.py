"""`torch.ops.pnpx.*` -- the native hot path registered with the PyTorch dispatcher (torch.library custom ops).

Every operator is a thin shim over one C-ABI entry of libpnpx.so (include/pnpx.h, bound in tfpnp_amd/ops.py): schema
+ a ROCm ("cuda") implementation + a fake-tensor (meta) implementation, so the ops trace under FakeTensorMode /
torch.compile / torch.export, and autograd formulas for the ops the training path differentiates (denoiser VJP, the
unitary FFTs, the Radon pair, PSNR, the critic's value, the MDDPG policy loss).  There is no CPU implementation: dispatching a CPU tensor raises
NotImplementedError from the dispatcher itself.

A native context (packed denoiser weights + workspaces) cannot travel through an operator schema, so ops take an
integer handle `ctx` (tfpnp_amd.ops.Context.cid; 0 = the weight-less default context of the tensors' device).
`iter_num = -1` means "all columns of the hyper-parameter tensors" (the reference's iter_num=None).
"""
from typing import List, Sequence, Tuple

import torch
from torch import Tensor

from . import ops

_lib_def = torch.library.custom_op


def _ctx(cid, t):
    return ops.default_context(t.device) if cid == 0 else ops.context_by_id(cid)


def _pin(node, cid, t):
    """setup_context helper: the autograd node keeps the native context ALIVE until its backward has run (the id -> context
    table holds weak references only; a denoiser collected between forward and backward must not strand the node)."""
    node.cid = cid
    node.native = _ctx(cid, t)


def _it(iter_num):
    return None if iter_num < 0 else iter_num


# ------------------------------------------------------------------------------------------------- denoiser prox
@_lib_def("pnpx::unet_denoise", mutates_args=(), device_types="cuda")
def unet_denoise(x: Tensor, sigma: Tensor, ctx: int) -> Tensor:
    """UNetDenoiser2D.forward (tfpnp/pnp/denoiser/base.py:23-32): x [B,1,H,W], sigma [B] -> [B,1,H,W]."""
    return ops.unet_denoise(_ctx(ctx, x), x, sigma)


@unet_denoise.register_fake
def _(x, sigma, ctx):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@_lib_def("pnpx::unet_denoise_preclamp", mutates_args=(), device_types="cuda")
def unet_denoise_preclamp(x: Tensor, sigma: Tensor, ctx: int) -> Tuple[Tensor, Tensor]:
    """(clamped, pre-clamp) denoiser outputs."""
    return ops.unet_denoise(_ctx(ctx, x), x, sigma, return_preclamp=True)


@unet_denoise_preclamp.register_fake
def _(x, sigma, ctx):
    e = lambda: torch.empty_like(x, memory_format=torch.contiguous_format)
    return e(), e()


@_lib_def("pnpx::unet_denoise_backward", mutates_args=(), device_types="cuda")
def unet_denoise_backward(x: Tensor, sigma: Tensor, grad_out: Tensor, ctx: int) -> Tuple[Tensor, Tensor]:
    """VJP of unet_denoise wrt (x, sigma); the forward pass is re-computed inside (gradient checkpointing)."""
    return ops.unet_denoise_backward(_ctx(ctx, x), x, sigma.reshape(-1), grad_out)


@unet_denoise_backward.register_fake
def _(x, sigma, grad_out, ctx):
    return (torch.empty_like(x, memory_format=torch.contiguous_format),
            torch.empty((x.shape[0],), dtype=x.dtype, device=x.device))


def _denoise_setup(ctx, inputs, output):
    x, sigma, cid = inputs
    ctx.save_for_backward(x, sigma)
    _pin(ctx, cid, x)


def _denoise_bwd(ctx, g):
    x, sigma = ctx.saved_tensors
    gx, gs = torch.ops.pnpx.unet_denoise_backward(x, sigma, g.contiguous(), ctx.cid)
    return gx, gs.view_as(sigma), None


unet_denoise.register_autograd(_denoise_bwd, setup_context=_denoise_setup)


@_lib_def("pnpx::unet_denoise_train", mutates_args=(), device_types="cuda")
def unet_denoise_train(x: Tensor, sigma: Tensor, ctx: int) -> Tuple[Tensor, Tensor]:
    """unet_denoise for autograd graphs: also parks the activations in the context's training ring; the second output is
    the ticket (one-element int64 CPU tensor) its VJP presents to skip the re-computation (pnpx_unet_denoise_train)."""
    out, ticket = ops.unet_denoise_train(_ctx(ctx, x), x, sigma)
    return out, torch.tensor([ticket], dtype=torch.int64)


@unet_denoise_train.register_fake
def _(x, sigma, ctx):
    return torch.empty_like(x, memory_format=torch.contiguous_format), torch.empty((1,), dtype=torch.int64)


@_lib_def("pnpx::unet_denoise_backward_ticket", mutates_args=(), device_types="cuda")
def unet_denoise_backward_ticket(x: Tensor, sigma: Tensor, grad_out: Tensor, ticket: Tensor, ctx: int) -> Tuple[Tensor, Tensor]:
    """VJP of unet_denoise_train: served from the training ring if it still holds `ticket`, else by re-computation."""
    return ops.unet_denoise_backward(_ctx(ctx, x), x, sigma.reshape(-1), grad_out, ticket=int(ticket[0]))


@unet_denoise_backward_ticket.register_fake
def _(x, sigma, grad_out, ticket, ctx):
    return (torch.empty_like(x, memory_format=torch.contiguous_format),
            torch.empty((x.shape[0],), dtype=x.dtype, device=x.device))


def _denoise_train_setup(ctx, inputs, output):
    x, sigma, cid = inputs
    _pin(ctx, cid, x)
    ctx.save_for_backward(x, sigma, output[1])


def _denoise_train_bwd(ctx, g, _g_ticket):
    x, sigma, ticket = ctx.saved_tensors
    gx, gs = torch.ops.pnpx.unet_denoise_backward_ticket(x, sigma, g.contiguous(), ticket, ctx.cid)
    return gx, gs.view_as(sigma), None


unet_denoise_train.register_autograd(_denoise_train_bwd, setup_context=_denoise_train_setup)


@_lib_def("pnpx::policy_forward", mutates_args=(), device_types="cuda")
def policy_forward(ob: Tensor, ctx: int) -> Tuple[Tensor, Tensor]:
    """ResNetActorBase.forward in eval mode (tfpnp/policy/network.py:129-147): ob [B,C,H,W] -> (probs [B,2], det [B,n])."""
    return ops.policy_forward(ops.context_by_id(ctx), ob)


@policy_forward.register_fake
def _(ob, ctx):
    n_det = ops.context_by_id(ctx)._policy[1]
    return (torch.empty((ob.shape[0], 2), dtype=ob.dtype, device=ob.device),
            torch.empty((ob.shape[0], n_det), dtype=ob.dtype, device=ob.device))


@_lib_def("pnpx::policy_forward_train", mutates_args=(), device_types="cuda")
def policy_forward_train(ob: Tensor, momentum: float, update_running: bool, ctx: int) -> Tuple[Tensor, Tensor]:
    """ResNetActorBase.forward in train mode (batch-statistics BatchNorm): ob [B,C,H,W] -> (probs [B,2], det [B,n]).
    With update_running it moves the running statistics inside the native context `ctx` -- it mutates the context, none of
    its tensor arguments.  There is no autograd formula: under requires_grad inputs the outputs carry no graph, as for
    policy_forward (the actor's parameter gradient is a call of its own: policy_param_grad)."""
    return ops.policy_forward_train(ops.context_by_id(ctx), ob, momentum, update_running)


@policy_forward_train.register_fake
def _(ob, momentum, update_running, ctx):
    n_det = ops.context_by_id(ctx)._policy[1]
    return (torch.empty((ob.shape[0], 2), dtype=ob.dtype, device=ob.device),
            torch.empty((ob.shape[0], n_det), dtype=ob.dtype, device=ob.device))


@_lib_def("pnpx::policy_param_grad", mutates_args=(), device_types="cuda")
def policy_param_grad(ob: Tensor, grad_probs: Tensor, grad_det: Tensor, ctx: int) -> Tensor:
    """d sum(grad_probs * probs + grad_det * det) / d params through the train-mode forward (ops.policy_param_grad): the flat
    gradient vector in policy_params' order.  Mutates nothing; no autograd formula (it IS the backward pass)."""
    return ops.policy_param_grad(ops.context_by_id(ctx), ob, grad_probs, grad_det)


@policy_param_grad.register_fake
def _(ob, grad_probs, grad_det, ctx):
    return torch.empty((ops.policy_flat_size(ops.context_by_id(ctx)),), dtype=torch.float32, device=ob.device)


@_lib_def("pnpx::policy_forward_train_keep", mutates_args=(), device_types="cuda")
def policy_forward_train_keep(ob: Tensor, momentum: float, update_running: bool, ctx: int) -> Tuple[Tensor, Tensor]:
    """policy_forward_train's outputs from the forward that keeps its activations inside the native context `ctx` for
    policy_param_grad_kept (ops.policy_forward_train_keep).  It mutates the context, none of its tensor arguments; no autograd
    formula."""
    return ops.policy_forward_train_keep(ops.context_by_id(ctx), ob, momentum, update_running)


@policy_forward_train_keep.register_fake
def _(ob, momentum, update_running, ctx):
    n_det = ops.context_by_id(ctx)._policy[1]
    return (torch.empty((ob.shape[0], 2), dtype=ob.dtype, device=ob.device),
            torch.empty((ob.shape[0], n_det), dtype=ob.dtype, device=ob.device))


@_lib_def("pnpx::policy_param_grad_kept", mutates_args=(), device_types="cuda")
def policy_param_grad_kept(grad_probs: Tensor, grad_det: Tensor, ctx: int) -> Tensor:
    """policy_param_grad on the forward the context `ctx` kept (ops.policy_param_grad_kept): the flat gradient vector in
    policy_params' order.  Mutates nothing; no autograd formula (it IS the backward pass)."""
    return ops.policy_param_grad_kept(ops.context_by_id(ctx), grad_probs, grad_det)


@policy_param_grad_kept.register_fake
def _(grad_probs, grad_det, ctx):
    return torch.empty((ops.policy_flat_size(ops.context_by_id(ctx)),), dtype=torch.float32, device=grad_probs.device)


# ------------------------------------------------------------------------------------------------- transforms
@_lib_def("pnpx::fft2", mutates_args=(), device_types="cuda")
def fft2(x: Tensor, inverse: bool, centered: bool) -> Tensor:
    """fft2 / ifft2 (tfpnp/utils/transforms.py:68-103), orthonormal, over dims (-3,-2) of [...,H,W,2]."""
    return ops.fft2(x, inverse=inverse, centered=centered)


@fft2.register_fake
def _(x, inverse, centered):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


def _fft_setup(ctx, inputs, output):
    _, ctx.inverse, ctx.centered = inputs


def _fft_bwd(ctx, g):      # orthonormal transform (+ index permutations): adjoint == inverse
    return torch.ops.pnpx.fft2(g.contiguous(), not ctx.inverse, ctx.centered), None, None


fft2.register_autograd(_fft_bwd, setup_context=_fft_setup)


@_lib_def("pnpx::cdp_forward", mutates_args=(), device_types="cuda")
def cdp_forward(x: Tensor, mask: Tensor) -> Tensor:
    """cdp_forward (transforms.py:282-301): x [B,1,H,W,2], mask [B,S,H,W,2] -> [B,S,H,W,2]."""
    return ops.cdp_forward(x, mask)


@cdp_forward.register_fake
def _(x, mask):
    return torch.empty_like(mask, memory_format=torch.contiguous_format)


@_lib_def("pnpx::cdp_backward", mutates_args=(), device_types="cuda")
def cdp_backward(y: Tensor, mask: Tensor) -> Tensor:
    """cdp_backward (transforms.py:304-320): y, mask [B,S,H,W,2] -> [B,1,H,W,2]."""
    return ops.cdp_backward(y, mask)


@cdp_backward.register_fake
def _(y, mask):
    B, S, H, W, _ = y.shape
    return torch.empty((B, 1, H, W, 2), dtype=y.dtype, device=y.device)


@_lib_def("pnpx::spi_inverse", mutates_args=(), device_types="cuda")
def spi_inverse(ztilde: Tensor, K1: Tensor, K: Tensor, mu: Tensor) -> Tensor:
    """spi_inverse (transforms.py:404-439)."""
    return ops.spi_inverse(ztilde, K1, K, mu)


@spi_inverse.register_fake
def _(ztilde, K1, K, mu):
    return torch.empty_like(ztilde, memory_format=torch.contiguous_format)


@_lib_def("pnpx::spi_pg_step", mutates_args=(), device_types="cuda")
def spi_pg_step(x: Tensor, x0: Tensor, Kmap: Tensor, tau: Tensor) -> Tensor:
    """One gradient step of PGSolver_SPI without the denoiser (include/pnpx.h; the reference has no counterpart).  Forward only."""
    return ops.spi_pg_step(x, x0, Kmap, tau)


@spi_pg_step.register_fake
def _(x, x0, Kmap, tau):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@_lib_def("pnpx::psnr", mutates_args=(), device_types="cuda")
def psnr(output: Tensor, gt: Tensor) -> Tensor:
    """torch_psnr (tfpnp/env/base.py:237-242): [B,...] x 2 -> [B,1]."""
    return ops.psnr(output, gt)


@psnr.register_fake
def _(output, gt):
    return torch.empty((output.shape[0], 1), dtype=output.dtype, device=output.device)


def _psnr_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _psnr_bwd(ctx, g):
    # d psnr_b / d out = -(20 / ln 10) * (clamp(out) - gt) / sse_b on the closed interval [0, 1] (torch.clamp's VJP)
    output, gt = ctx.saved_tensors
    B = output.shape[0]
    o = output.reshape(B, -1)
    diff = o.clamp(0, 1) - gt.reshape(B, -1)
    sse = (diff * diff).sum(dim=1, keepdim=True)
    inside = (o >= 0) & (o <= 1)
    go = (-20.0 / 2.302585092994046) * g.reshape(B, 1) * diff / sse * inside
    return go.view_as(output), None


psnr.register_autograd(_psnr_bwd, setup_context=_psnr_setup)


@_lib_def("pnpx::radon_forward", mutates_args=(), device_types="cuda")
def radon_forward(img: Tensor, n_view: int) -> Tensor:
    """Parallel-beam Radon transform standing in for torch_radon (transforms.py:465-508): [B,1,R,R] -> [B,1,V,det]."""
    return ops.radon_forward(img, n_view)


@radon_forward.register_fake
def _(img, n_view):
    return torch.empty((img.shape[0], 1, n_view, ops.radon_det_count(img.shape[-1])), dtype=img.dtype, device=img.device)


@_lib_def("pnpx::radon_backprojection", mutates_args=(), device_types="cuda")
def radon_backprojection(sino: Tensor, R: int) -> Tensor:
    return ops.radon_backprojection(sino, R)


@radon_backprojection.register_fake
def _(sino, R):
    return torch.empty((sino.shape[0], 1, R, R), dtype=sino.dtype, device=sino.device)


# each is the other's VJP (the unmatched ray-/pixel-driven pair torch_radon also uses)
radon_forward.register_autograd(
    lambda ctx, g: (torch.ops.pnpx.radon_backprojection(g.contiguous(), ctx.R), None),
    setup_context=lambda ctx, inputs, output: setattr(ctx, "R", inputs[0].shape[-1]))
radon_backprojection.register_autograd(
    lambda ctx, g: (torch.ops.pnpx.radon_forward(g.contiguous(), ctx.V), None),
    setup_context=lambda ctx, inputs, output: setattr(ctx, "V", inputs[0].shape[2]))


@_lib_def("pnpx::fan_forward", mutates_args=(), device_types="cuda")
def fan_forward(img: Tensor, n_view: int, det_count: int, source_distance: float, det_distance: float, det_spacing: float) -> Tensor:
    """Fan-beam projector (flat detector, full circle; include/pnpx.h): [B,1,R,R] -> [B,1,n_view,det_count]."""
    return ops.fan_forward(img, n_view, det_count, source_distance, det_distance, det_spacing)


@fan_forward.register_fake
def _(img, n_view, det_count, source_distance, det_distance, det_spacing):
    return torch.empty((img.shape[0], 1, n_view, det_count), dtype=img.dtype, device=img.device)


@_lib_def("pnpx::fan_backprojection", mutates_args=(), device_types="cuda")
def fan_backprojection(sino: Tensor, R: int, source_distance: float, det_distance: float, det_spacing: float) -> Tensor:
    """The weighted pixel-driven fan backprojection: [B,1,n_view,det_count] -> [B,1,R,R]."""
    return ops.fan_backprojection(sino, R, source_distance, det_distance, det_spacing)


@fan_backprojection.register_fake
def _(sino, R, source_distance, det_distance, det_spacing):
    return torch.empty((sino.shape[0], 1, R, R), dtype=sino.dtype, device=sino.device)


# each is the other's VJP, as for the parallel pair
fan_forward.register_autograd(
    lambda ctx, g: (torch.ops.pnpx.fan_backprojection(g.contiguous(), ctx.R, *ctx.geom), None, None, None, None, None),
    setup_context=lambda ctx, inputs, output: (setattr(ctx, "R", inputs[0].shape[-1]), setattr(ctx, "geom", tuple(inputs[3:]))))
fan_backprojection.register_autograd(
    lambda ctx, g: (torch.ops.pnpx.fan_forward(g.contiguous(), ctx.V, ctx.det, *ctx.geom), None, None, None, None),
    setup_context=lambda ctx, inputs, output: (setattr(ctx, "V", inputs[0].shape[2]), setattr(ctx, "det", inputs[0].shape[3]),
                                               setattr(ctx, "geom", tuple(inputs[2:]))))


# filtered backprojection: the start image of an episode is data, so neither op has an autograd formula
@_lib_def("pnpx::radon_filter", mutates_args=(), device_types="cuda")
def radon_filter(sino: Tensor, source_distance: float, det_distance: float, det_spacing: float) -> Tensor:
    """The ramp filter along the detector axis (include/pnpx.h): source_distance 0 = the parallel beam's, else the fan beam's."""
    return ops.radon_filter(sino, *((source_distance, det_distance, det_spacing) if source_distance else ()))


@radon_filter.register_fake
def _(sino, source_distance, det_distance, det_spacing):
    return torch.empty_like(sino, memory_format=torch.contiguous_format)


@_lib_def("pnpx::fan_fbp", mutates_args=(), device_types="cuda")
def fan_fbp(sino: Tensor, R: int, source_distance: float, det_distance: float, det_spacing: float) -> Tensor:
    """Fan-beam filtered backprojection: [B,1,n_view,det_count] -> [B,1,R,R]."""
    return ops.fan_fbp(sino, R, source_distance, det_distance, det_spacing)


@fan_fbp.register_fake
def _(sino, R, source_distance, det_distance, det_spacing):
    return torch.empty((sino.shape[0], 1, R, R), dtype=sino.dtype, device=sino.device)


# ------------------------------------------------------------------------------------------------- solver loops
# ------------------------------------------------------------------------------------------------- solver training ops
def _solver_train_ops(name, aux, hypers, train_fn, backward_fn, saved_per_pixel, bwd_takes_aux=True):
    """Register `pnpx::<name>_train` (+ `_backward` and the autograd formula) for a solver whose native training entry follows the
    common contract: (variables, *aux, *hyper-parameters, iter_num, ctx) -> (next state, saved, ticket) -- the same result as the
    inference op plus what the native VJP replays (`saved`: per-iteration denoiser inputs and data-step intermediates, include/pnpx.h)
    and the ticket of the context's activation cache (a one-element int64 CPU tensor).  This is what PnPEnv.forward reaches under
    autograd (tfpnp/env/base.py:193-206).  `aux` = [(name, schema type)]; non-tensor aux entries (view count, operator norm)
    travel on the autograd node; `saved_per_pixel` = floats per pixel and iteration (a number, or a function of the aux tuple).
    The backward op returns gradients for the hyper-parameter columns that were iterated; the rest of [B, action_pack] gets zeros."""
    n_aux, n_h = len(aux), len(hypers)
    aux_sig = [f"{t} {n}" for n, t in aux]
    hyp_sig = [f"Tensor {h}" for h in hypers]
    fwd_schema = "(" + ", ".join(["Tensor variables"] + aux_sig + hyp_sig + ["int iter_num", "int ctx"]) + ") -> (Tensor, Tensor, Tensor)"
    bwd_schema = ("(" + ", ".join(aux_sig + hyp_sig + ["Tensor saved", "Tensor ticket", "Tensor grad_out", "int iter_num", "int ctx"]) +
                  ") -> (" + ", ".join(["Tensor"] * (1 + n_h)) + ")")

    def n_iter(h0, iter_num):
        return (h0.shape[1] if h0.dim() == 2 else 1) if iter_num < 0 else iter_num

    def fwd(*a):
        variables, auxv, hv, (iter_num, cid) = a[0], a[1:1 + n_aux], a[1 + n_aux:1 + n_aux + n_h], a[-2:]
        out, saved, ticket = train_fn(_ctx(cid, variables), variables, *auxv, *hv, _it(iter_num))
        return out, saved, torch.tensor([ticket], dtype=torch.int64)

    def fwd_fake(*a):
        variables, hv, iter_num = a[0], a[1 + n_aux:1 + n_aux + n_h], a[-2]
        n_px = variables.numel() // variables.shape[1] // (2 if variables.dim() == 5 else 1)
        per = saved_per_pixel(a[1:1 + n_aux]) if callable(saved_per_pixel) else saved_per_pixel
        return (torch.empty_like(variables, memory_format=torch.contiguous_format),
                torch.empty((per * n_iter(hv[0], iter_num) * n_px,), dtype=variables.dtype, device=variables.device),
                torch.empty((1,), dtype=torch.int64))

    def bwd(*a):
        auxv, hv = a[:n_aux], a[n_aux:n_aux + n_h]
        saved, ticket, grad_out, iter_num, cid = a[n_aux + n_h:]
        lead = auxv if bwd_takes_aux else tuple(v for v, (_, t) in zip(auxv, aux) if t != "Tensor")
        return backward_fn(_ctx(cid, grad_out), *lead, *hv, saved, grad_out, _it(iter_num), ticket=int(ticket[0]))

    def bwd_fake(*a):
        hv, grad_out, iter_num = a[n_aux:n_aux + n_h], a[-3], a[-2]
        e = lambda: torch.empty((grad_out.shape[0], n_iter(hv[0], iter_num)), dtype=grad_out.dtype, device=grad_out.device)
        return (torch.empty_like(grad_out, memory_format=torch.contiguous_format), *[e() for _ in range(n_h)])

    op_f = _lib_def(f"pnpx::{name}_train", fwd, mutates_args=(), device_types="cuda", schema=fwd_schema)
    op_f.register_fake(fwd_fake)
    op_b = _lib_def(f"pnpx::{name}_backward", bwd, mutates_args=(), device_types="cuda", schema=bwd_schema)
    op_b.register_fake(bwd_fake)
    tensor_aux = [k for k, (_, t) in enumerate(aux) if t == "Tensor"]

    def setup(ctx, inputs, output):
        auxv, hv = inputs[1:1 + n_aux], inputs[1 + n_aux:1 + n_aux + n_h]
        ctx.iter_num, cid = inputs[-2:]
        _pin(ctx, cid, inputs[0])
        ctx.plain_aux = {k: v for k, v in enumerate(auxv) if k not in tensor_aux}
        ctx.save_for_backward(*[auxv[k] for k in tensor_aux], *hv, output[1], output[2])

    def backward(ctx, g_out, _g_saved, _g_ticket):
        t = ctx.saved_tensors
        auxv = [None] * n_aux
        for j, k in enumerate(tensor_aux):
            auxv[k] = t[j]
        for k, v in ctx.plain_aux.items():
            auxv[k] = v
        hv = t[len(tensor_aux):len(tensor_aux) + n_h]
        res = getattr(torch.ops.pnpx, f"{name}_backward")(*auxv, *hv, t[-2], t[-1], g_out.contiguous(), ctx.iter_num, ctx.cid)

        def like(g, p):
            full = torch.zeros_like(p)
            if p.numel():
                full.view(p.shape[0], -1)[:, :g.shape[1]] = g
            return full

        return (res[0], *[None] * n_aux, *[like(g, p) for g, p in zip(res[1:], hv)], None, None)

    op_f.register_autograd(backward, setup_context=setup)
    return op_f, op_b


_MRI_AUX = [("y0", "Tensor"), ("mask", "Tensor")]
csmri_admm_train, csmri_admm_backward = _solver_train_ops(
    "csmri_admm", _MRI_AUX, ("sigma_d", "mu"), ops.csmri_admm_train, ops.csmri_admm_backward, 3)
csmri_hqs_train, csmri_hqs_backward = _solver_train_ops(
    "csmri_hqs", _MRI_AUX, ("sigma_d", "mu"), ops.csmri_hqs_train, ops.csmri_hqs_backward, 3)
csmri_pg_train, csmri_pg_backward = _solver_train_ops(
    "csmri_pg", _MRI_AUX, ("sigma_d", "tau"), ops.csmri_pg_train, ops.csmri_pg_backward, 2)
csmri_apg_train, csmri_apg_backward = _solver_train_ops(
    "csmri_apg", _MRI_AUX, ("sigma_d", "tau", "beta"), ops.csmri_apg_train, ops.csmri_apg_backward, 4)
csmri_redadmm_train, csmri_redadmm_backward = _solver_train_ops(
    "csmri_redadmm", _MRI_AUX, ("sigma_d", "mu", "lamda"), ops.csmri_redadmm_train, ops.csmri_redadmm_backward, 7)
pr_iadmm_train, pr_iadmm_backward = _solver_train_ops(
    "pr_iadmm", _MRI_AUX, ("sigma_d", "mu", "tau"), ops.pr_iadmm_train, ops.pr_iadmm_backward,
    lambda aux: 2 * aux[1].shape[1] + 5)        # mask [B,S,H,W,2]: S k-space images per iteration
pr_pg_train, pr_pg_backward = _solver_train_ops(
    "pr_pg", _MRI_AUX, ("sigma_d", "tau"), ops.pr_pg_train, ops.pr_pg_backward,
    lambda aux: 2 * aux[1].shape[1] + 2)        # S k-space images, the denoiser input and Re g per iteration
spi_admm_train, spi_admm_backward = _solver_train_ops(
    "spi_admm", [("x0", "Tensor"), ("Kmap", "Tensor")], ("sigma_d", "mu"), ops.spi_admm_train, ops.spi_admm_backward, 2)
spi_pg_train, spi_pg_backward = _solver_train_ops(
    "spi_pg", [("x0", "Tensor"), ("Kmap", "Tensor")], ("sigma_d", "tau"), ops.spi_pg_train, ops.spi_pg_backward, 2)
ct_iadmm_train, ct_iadmm_backward = _solver_train_ops(
    "ct_iadmm", [("y0", "Tensor"), ("n_view", "int"), ("opnorm", "float")], ("sigma_d", "mu", "tau"), ops.ct_iadmm_train,
    ops.ct_iadmm_backward, 3, bwd_takes_aux=False)
ct_pg_train, ct_pg_backward = _solver_train_ops(
    "ct_pg", [("y0", "Tensor"), ("n_view", "int"), ("opnorm", "float")], ("sigma_d", "tau"), ops.ct_pg_train, ops.ct_pg_backward, 2,
    bwd_takes_aux=False)
_CT_GEOM_AUX = [("y0", "Tensor"), ("n_view", "int"), ("opnorm", "float"), ("det_count", "int"), ("source_distance", "float"),
                ("det_distance", "float"), ("det_spacing", "float")]         # det_count 0 = parallel beam
ct_hqs_train, ct_hqs_backward = _solver_train_ops(
    "ct_hqs", _CT_GEOM_AUX, ("sigma_d", "mu"), ops.ct_hqs_train, ops.ct_hqs_backward, 3, bwd_takes_aux=False)
ct_iadmm_geom_train, ct_iadmm_geom_backward = _solver_train_ops(
    "ct_iadmm_geom", _CT_GEOM_AUX, ("sigma_d", "mu", "tau"), ops.ct_iadmm_geom_train, ops.ct_iadmm_geom_backward, 3,
    bwd_takes_aux=False)
ct_pg_geom_train, ct_pg_geom_backward = _solver_train_ops(
    "ct_pg_geom", _CT_GEOM_AUX, ("sigma_d", "tau"), ops.ct_pg_geom_train, ops.ct_pg_geom_backward, 2, bwd_takes_aux=False)


def _same(variables, *a):
    return torch.empty_like(variables, memory_format=torch.contiguous_format)


@_lib_def("pnpx::csmri_admm", mutates_args=(), device_types="cuda")
def csmri_admm(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, mu: Tensor, iter_num: int, ctx: int) -> Tensor:
    """ADMMSolver_CSMRI.forward (tasks/csmri/solver.py:29-57), all inner iterations in one native call."""
    return ops.csmri_admm(_ctx(ctx, variables), variables, y0, mask, sigma_d, mu, _it(iter_num))


csmri_admm.register_fake(_same)


@_lib_def("pnpx::csmri_hqs", mutates_args=(), device_types="cuda")
def csmri_hqs(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, mu: Tensor, iter_num: int, ctx: int) -> Tensor:
    """HQSSolver_CSMRI.forward (tasks/csmri/solver.py:64-89)."""
    return ops.csmri_hqs(_ctx(ctx, variables), variables, y0, mask, sigma_d, mu, _it(iter_num))


csmri_hqs.register_fake(_same)


@_lib_def("pnpx::csmri_amp", mutates_args=(), device_types="cuda")
def csmri_amp(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, probe: Tensor, iter_num: int, ctx: int) -> Tensor:
    """AMPSolver_CSMRI.forward (tasks/csmri/solver.py:211-250, prox_fun = prox_mapping), probe [T,B,1,H,W] given."""
    return ops.csmri_amp(_ctx(ctx, variables), variables, y0, mask, sigma_d, probe, _it(iter_num))


csmri_amp.register_fake(_same)


@_lib_def("pnpx::csmri_pg", mutates_args=(), device_types="cuda")
def csmri_pg(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, tau: Tensor, iter_num: int, ctx: int) -> Tensor:
    """PGSolver_CSMRI.forward (tasks/csmri/solver.py:96-120)."""
    return ops.csmri_pg(_ctx(ctx, variables), variables, y0, mask, sigma_d, tau, _it(iter_num))


csmri_pg.register_fake(_same)


@_lib_def("pnpx::csmri_apg", mutates_args=(), device_types="cuda")
def csmri_apg(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, tau: Tensor, beta: Tensor, iter_num: int,
              ctx: int) -> Tensor:
    """APGSolver_CSMRI.forward (tasks/csmri/solver.py:127-165)."""
    return ops.csmri_apg(_ctx(ctx, variables), variables, y0, mask, sigma_d, tau, beta, _it(iter_num))


csmri_apg.register_fake(_same)


@_lib_def("pnpx::csmri_redadmm", mutates_args=(), device_types="cuda")
def csmri_redadmm(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, mu: Tensor, lamda: Tensor, iter_num: int,
                  ctx: int) -> Tensor:
    """REDADMMSolver_CSMRI.forward (tasks/csmri/solver.py:172-204)."""
    return ops.csmri_redadmm(_ctx(ctx, variables), variables, y0, mask, sigma_d, mu, lamda, _it(iter_num))


csmri_redadmm.register_fake(_same)


@_lib_def("pnpx::pr_iadmm", mutates_args=(), device_types="cuda")
def pr_iadmm(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, mu: Tensor, tau: Tensor, iter_num: int,
             ctx: int) -> Tensor:
    """IADMMSolver_PR.forward (tasks/pr/solver.py:37-76)."""
    return ops.pr_iadmm(_ctx(ctx, variables), variables, y0, mask, sigma_d, mu, tau, _it(iter_num))


pr_iadmm.register_fake(_same)


@_lib_def("pnpx::pr_pg", mutates_args=(), device_types="cuda")
def pr_pg(variables: Tensor, y0: Tensor, mask: Tensor, sigma_d: Tensor, tau: Tensor, iter_num: int, ctx: int) -> Tensor:
    """PGSolver_PR.forward: the loop of tasks/pr/solver.py:79-112 with the PR gradient step of :61-68 (include/pnpx.h)."""
    return ops.pr_pg(_ctx(ctx, variables), variables, y0, mask, sigma_d, tau, _it(iter_num))


pr_pg.register_fake(_same)


@_lib_def("pnpx::spi_admm", mutates_args=(), device_types="cuda")
def spi_admm(variables: Tensor, x0: Tensor, Kmap: Tensor, sigma_d: Tensor, mu: Tensor, iter_num: int, ctx: int) -> Tensor:
    """ADMMSolver_SPI.forward (tasks/spi/solver.py:17-52)."""
    return ops.spi_admm(_ctx(ctx, variables), variables, x0, Kmap, sigma_d, mu, _it(iter_num))


spi_admm.register_fake(_same)


@_lib_def("pnpx::spi_pg", mutates_args=(), device_types="cuda")
def spi_pg(variables: Tensor, x0: Tensor, Kmap: Tensor, sigma_d: Tensor, tau: Tensor, iter_num: int, ctx: int) -> Tensor:
    """PGSolver_SPI.forward: proximal gradient on the SPI data term (include/pnpx.h; the reference has no counterpart)."""
    return ops.spi_pg(_ctx(ctx, variables), variables, x0, Kmap, sigma_d, tau, _it(iter_num))


spi_pg.register_fake(_same)


@_lib_def("pnpx::ct_iadmm", mutates_args=(), device_types="cuda")
def ct_iadmm(variables: Tensor, y0: Tensor, n_view: int, opnorm: float, sigma_d: Tensor, mu: Tensor, tau: Tensor,
             iter_num: int, ctx: int) -> Tensor:
    """IADMMSolver_CT.forward (tasks/ct/solver.py:17-53)."""
    return ops.ct_iadmm(_ctx(ctx, variables), variables, y0, n_view, opnorm, sigma_d, mu, tau, _it(iter_num))


ct_iadmm.register_fake(_same)


@_lib_def("pnpx::ct_pg", mutates_args=(), device_types="cuda")
def ct_pg(variables: Tensor, y0: Tensor, n_view: int, opnorm: float, sigma_d: Tensor, tau: Tensor, iter_num: int,
          ctx: int) -> Tensor:
    """PGSolver_CT.forward (tasks/ct/solver.py:61-87)."""
    return ops.ct_pg(_ctx(ctx, variables), variables, y0, n_view, opnorm, sigma_d, tau, _it(iter_num))


ct_pg.register_fake(_same)


@_lib_def("pnpx::ct_hqs", mutates_args=(), device_types="cuda")
def ct_hqs(variables: Tensor, y0: Tensor, n_view: int, opnorm: float, det_count: int, source_distance: float, det_distance: float,
           det_spacing: float, sigma_d: Tensor, mu: Tensor, iter_num: int, ctx: int) -> Tensor:
    """HQSSolver_CT.forward: state cat(x, z); det_count 0 = parallel beam, else the fan geometry of include/pnpx.h."""
    return ops.ct_hqs(_ctx(ctx, variables), variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing,
                      sigma_d, mu, _it(iter_num))


ct_hqs.register_fake(_same)


@_lib_def("pnpx::ct_iadmm_geom", mutates_args=(), device_types="cuda")
def ct_iadmm_geom(variables: Tensor, y0: Tensor, n_view: int, opnorm: float, det_count: int, source_distance: float,
                  det_distance: float, det_spacing: float, sigma_d: Tensor, mu: Tensor, tau: Tensor, iter_num: int, ctx: int) -> Tensor:
    """IADMMSolver_CT.forward on a chosen geometry: det_count 0 = parallel beam (ct_iadmm's bytes), else the fan geometry."""
    return ops.ct_iadmm_geom(_ctx(ctx, variables), variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing,
                             sigma_d, mu, tau, _it(iter_num))


ct_iadmm_geom.register_fake(_same)


@_lib_def("pnpx::ct_pg_geom", mutates_args=(), device_types="cuda")
def ct_pg_geom(variables: Tensor, y0: Tensor, n_view: int, opnorm: float, det_count: int, source_distance: float, det_distance: float,
               det_spacing: float, sigma_d: Tensor, tau: Tensor, iter_num: int, ctx: int) -> Tensor:
    """PGSolver_CT.forward on a chosen geometry: det_count 0 = parallel beam (ct_pg's bytes), else the fan geometry."""
    return ops.ct_pg_geom(_ctx(ctx, variables), variables, y0, n_view, opnorm, det_count, source_distance, det_distance, det_spacing,
                          sigma_d, tau, _it(iter_num))


ct_pg_geom.register_fake(_same)

# ------------------------------------------------------------------------------------------------- value network
@_lib_def("pnpx::critic_value", mutates_args=(), device_types="cuda")
def critic_value(ob: Tensor, ctx: int) -> Tensor:
    """ResNet_wobn(num_inputs, 18, 1).forward (tfpnp/trainer/mddpg/critic.py:121-131): ob [B,C,H,W] -> V [B,1]."""
    return ops.critic_forward(ops.context_by_id(ctx), ob)


@critic_value.register_fake
def _(ob, ctx):
    return torch.empty((ob.shape[0], 1), dtype=ob.dtype, device=ob.device)


@_lib_def("pnpx::critic_backward", mutates_args=(), device_types="cuda")
def critic_backward(ob: Tensor, grad_value: Tensor, ctx: int) -> Tensor:
    """VJP of critic_value wrt ob (frozen weights; the forward is re-computed inside)."""
    return ops.critic_backward(ops.context_by_id(ctx), ob, grad_value)


@critic_backward.register_fake
def _(ob, grad_value, ctx):
    return torch.empty_like(ob, memory_format=torch.contiguous_format)


@_lib_def("pnpx::critic_param_grad", mutates_args=(), device_types="cuda")
def critic_param_grad(ob: Tensor, grad_value: Tensor, ctx: int) -> Tensor:
    """d sum(grad_value * critic_value(ob)) / d params as one flat vector (value_loss.backward(), trainer.py:198,207)."""
    return ops.critic_param_grad(ops.context_by_id(ctx), ob, grad_value)


@critic_param_grad.register_fake
def _(ob, grad_value, ctx):
    n = int(ops._lib.lib().pnpx_critic_num_params(ops.context_by_id(ctx)._critic))
    return torch.empty((n,), dtype=torch.float32, device=ob.device)


@_lib_def("pnpx::critic_value_loss_grad", mutates_args=(), device_types="cuda")
def critic_value_loss_grad(ob: Tensor, q_target: Tensor, ctx: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(V [B,1], value_loss [], d value_loss / d params [n]) from one forward: nn.MSELoss()(q_target, V) and its backward()
    (trainer.py:198,207); q_target is not differentiated."""
    return ops.critic_value_loss_grad(ops.context_by_id(ctx), ob, q_target)


@critic_value_loss_grad.register_fake
def _(ob, q_target, ctx):
    n = int(ops._lib.lib().pnpx_critic_num_params(ops.context_by_id(ctx)._critic))
    return (torch.empty((ob.shape[0], 1), dtype=torch.float32, device=ob.device), torch.empty((), dtype=torch.float32, device=ob.device),
            torch.empty((n,), dtype=torch.float32, device=ob.device))


def _critic_setup(ctx, inputs, output):
    ob, cid = inputs
    ctx.save_for_backward(ob)
    _pin(ctx, cid, ob)


def _critic_bwd(ctx, g):
    (ob,) = ctx.saved_tensors
    return torch.ops.pnpx.critic_backward(ob, g.contiguous(), ctx.cid), None


critic_value.register_autograd(_critic_bwd, setup_context=_critic_setup)


# ------------------------------------------------------------------------------------------------- observation pack
def _pack_kind(t, kind):
    """integer kind of a pack entry (ops._PACK_KINDS): bool / uint8 'raw' entries are kind 3"""
    return 3 if kind == 0 and t.dtype in (torch.bool, torch.uint8) else kind


@_lib_def("pnpx::policy_ob_pack_diff", mutates_args=(), device_types="cuda")
def policy_ob_pack_diff(entries: Sequence[Tensor], kinds: Sequence[int]) -> Tensor:
    """get_policy_ob / get_eval_ob (tasks/*/env.py) with an autograd formula: entries in channel order, kinds[i] = 0 raw
    [B,c,H,W] (fp32, or bool / uint8 without gradient), 1 complex2real, 2 complex2channel of [B,c,H,W,2] -> [B,C,H,W]."""
    names = {0: "raw", 1: "real", 2: "channel"}
    return ops.policy_ob_pack([(t, names[k]) for t, k in zip(entries, kinds)])


@policy_ob_pack_diff.register_fake
def _(entries, kinds):
    t0 = entries[0]
    C_out = sum(t.shape[1] * (2 if k == 2 else 1) for t, k in zip(entries, kinds))
    return torch.empty((t0.shape[0], C_out, t0.shape[2], t0.shape[3]), dtype=torch.float32, device=t0.device)


@_lib_def("pnpx::policy_ob_unpack", mutates_args=(), device_types="cuda")
def policy_ob_unpack(grad_out: Tensor, kinds: Sequence[int], channels: Sequence[int]) -> List[Tensor]:
    """Adjoint of policy_ob_pack_diff (pnpx_policy_ob_unpack): one gradient per entry; kind-3 entries (bool / uint8) get an
    empty placeholder."""
    outs = ops.policy_ob_unpack(grad_out, kinds, channels)
    return [o if o is not None else grad_out.new_empty((0,)) for o in outs]


@policy_ob_unpack.register_fake
def _(grad_out, kinds, channels):
    B, _, H, W = grad_out.shape
    return [grad_out.new_empty((0,)) if k == 3 else grad_out.new_empty((B, c, H, W) + ((2,) if k else ()))
            for k, c in zip(kinds, channels)]


def _pack_setup(ctx, inputs, output):
    entries, kinds = inputs
    ctx.kinds = [_pack_kind(t, k) for t, k in zip(entries, kinds)]
    ctx.channels = [t.shape[1] for t in entries]


def _pack_bwd(ctx, g):
    grads = torch.ops.pnpx.policy_ob_unpack(g.contiguous(), ctx.kinds, ctx.channels)
    return [None if k == 3 else gi for k, gi in zip(ctx.kinds, grads)], None


policy_ob_pack_diff.register_autograd(_pack_bwd, setup_context=_pack_setup)


# ------------------------------------------------------------------------------------------------- MDDPG policy loss
@_lib_def("pnpx::mddpg_policy_loss", mutates_args=(), device_types="cuda")
def mddpg_policy_loss(p_stop: Tensor, idx_stop: Tensor, v_cur: Tensor, v_next_target: Tensor, v_next: Tensor, reward: Tensor,
                      discount: float, loop_penalty: float, lambda_e: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """trainer/mddpg/trainer.py:174, :179-197 in one launch -> (scalars [2] = (policy_loss, mean entropy), q_target [B],
    log_prob [B], entropy [B], grad_p_stop [B,2], grad_v_next [B], grad_reward [B]).  Differentiable through scalars[0] only, with
    respect to p_stop, v_next and reward (the advantage is detached, :186): its backward scales the three gradient outputs, which
    the same launch wrote.  The mean-entropy slot is a diagnostic (:214) and carries no gradient."""
    q, logp, ent, scalars, gp, gv, gr = ops.mddpg_policy_loss(None, p_stop, idx_stop, v_cur, v_next_target, v_next, reward,
                                                              discount, loop_penalty, lambda_e)
    return scalars, q, logp, ent, gp, gv, gr


@mddpg_policy_loss.register_fake
def _(p_stop, idx_stop, v_cur, v_next_target, v_next, reward, discount, loop_penalty, lambda_e):
    B = p_stop.shape[0]
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=p_stop.device)
    return e(2), e(B), e(B), e(B), e(B, 2), e(B), e(B)


def _mddpg_loss_setup(ctx, inputs, output):
    ctx.save_for_backward(*output[4:])
    ctx.shapes = (inputs[4].shape, inputs[5].shape)
    ctx.mark_non_differentiable(*output[1:])


def _mddpg_loss_bwd(ctx, g, *_unused):
    gp, gv, gr = ctx.saved_tensors
    s = g[0]                                   # d / d policy_loss; the mean-entropy slot g[1] is not differentiated
    return (s * gp, None, None, None, (s * gv).view(ctx.shapes[0]), (s * gr).view(ctx.shapes[1]), None, None, None)


mddpg_policy_loss.register_autograd(_mddpg_loss_bwd, setup_context=_mddpg_loss_setup)


def call(name, *args):
    """torch.ops.pnpx.<name>(*args) with the package's error contract: tensors that are not on a ROCm device raise
    PnpxError (there is no CPU kernel to dispatch to) instead of the dispatcher's NotImplementedError."""
    for a in args:
        if isinstance(a, Tensor) and not a.is_cuda:
            raise ops.PnpxError(f"pnpx::{name}: tensor on {a.device}; tfpnp_amd runs on MI355X only, there is no CPU path")
    return getattr(torch.ops.pnpx, name)(*args)


ALL_OPS = ("unet_denoise", "unet_denoise_preclamp", "unet_denoise_backward", "unet_denoise_train",
           "unet_denoise_backward_ticket", "policy_forward", "policy_forward_train", "policy_param_grad", "policy_forward_train_keep",
           "policy_param_grad_kept", "fft2", "cdp_forward",
           "cdp_backward", "spi_inverse", "psnr", "radon_forward", "radon_backprojection", "csmri_admm", "csmri_admm_train",
           "csmri_admm_backward", "csmri_hqs", "csmri_amp",
           "csmri_pg", "csmri_apg", "csmri_redadmm", "pr_iadmm", "spi_admm", "ct_iadmm", "ct_pg", "pr_pg",
           "fan_forward", "fan_backprojection", "ct_hqs", "ct_hqs_train", "ct_hqs_backward",
           "radon_filter", "fan_fbp", "ct_iadmm_geom", "ct_iadmm_geom_train", "ct_iadmm_geom_backward", "ct_pg_geom",
           "ct_pg_geom_train", "ct_pg_geom_backward",
           "spi_pg_step", "spi_pg", "spi_pg_train", "spi_pg_backward",
           "critic_value", "critic_backward", "critic_param_grad", "critic_value_loss_grad", "policy_ob_pack_diff", "policy_ob_unpack",
           "mddpg_policy_loss")
