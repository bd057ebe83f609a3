"""Helpers of the critic parameter-gradient tests: the restatement of tests/critic_cases.py with the 82 parameters as autograd
leaves (weight_g and weight_v separately: weight-norm is part of the graph), the fixed sample of a tensor that
tests/golden/critic_param_grad.npz stores (tools/make_critic_grad_golden.py), and the per-tensor error measure.
No GPU, no reference import."""
import numpy as np
import torch
import torch.nn.functional as F

from tfpnp_amd import synth

SAMPLE_MAX = 1024
GOLDEN_CASES = ("kf9", "kf17", "arb", "rect")


def leaf_forward(P, x):
    """V [B,1] of ResNet_wobn(num_inputs, 18, 1) (tfpnp/trainer/mddpg/critic.py:95-131) from the raw parameter tensors P
    ({state_dict key: tensor}) -- differentiable with respect to every one of them."""

    def conv(v, p, stride, pad):
        wv, wg = P[p + ".weight_v"], P[p + ".weight_g"]
        w = wg * wv / wv.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
        return F.conv2d(v, w, P[p + ".bias"], stride=stride, padding=pad)

    def trelu(v, key):
        return torch.maximum(v, P[key])

    x = trelu(conv(x, "conv1", 2, 1), "relu_1.alpha")
    for li in range(1, 5):
        for blk in range(2):
            p = f"layer{li}.{blk}"
            out = trelu(conv(x, p + ".conv1", 2 if blk == 0 else 1, 1), p + ".relu_1.alpha")
            out = conv(out, p + ".conv2", 1, 1)
            out = out + (conv(x, p + ".shortcut.0", 2, 0) if blk == 0 else x)
            x = trelu(out, p + ".relu_2.alpha")
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    return F.linear(x, P["fc.weight"], P["fc.bias"])


def leaves(params, dtype, requires_grad=True):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(requires_grad) for k, v in params.items()}


def leaf_grads(params, ob, w, dtype=torch.float64):
    """(V [B,1], {key: d sum(V * w) / d params[key]}) of the leaf restatement in `dtype`, as float64 numpy arrays."""
    P = leaves(params, dtype)
    V = leaf_forward(P, torch.from_numpy(np.ascontiguousarray(ob)).to(dtype))
    (V[:, 0] * torch.from_numpy(np.ascontiguousarray(w)).to(dtype)).sum().backward()
    return V.detach().double().numpy(), {k: P[k].grad.double().numpy() for k in P}


def split_flat(flat, num_inputs):
    """flat vector (synth.critic_param_specs order) -> {key: array of the tensor's shape}"""
    flat = np.asarray(flat)
    out, pos = {}, 0
    for key, shape in synth.critic_param_specs(num_inputs):
        n = int(np.prod(shape))
        out[key] = flat[pos:pos + n].reshape(shape)
        pos += n
    assert pos == flat.size, (pos, flat.size)
    return out


def join_flat(grads, num_inputs, dtype=np.float64):
    return np.concatenate([np.asarray(grads[k], dtype).reshape(-1) for k, _ in synth.critic_param_specs(num_inputs)])


def sample_index(n):
    """the fixed strided sample of a tensor with n entries: at most SAMPLE_MAX of them, first entry included"""
    return np.arange(0, n, max(1, -(-n // SAMPLE_MAX)))


def per_tensor_rel(got, ref):
    """{key: ||got - ref|| / max(||ref||, 1e-6 * max_t ||ref_t||)} over the tensors of ref (dicts of arrays)"""
    norms = {k: float(np.linalg.norm(np.asarray(v, np.float64))) for k, v in ref.items()}
    floor = 1e-6 * max(norms.values())
    return {k: float(np.linalg.norm(np.asarray(got[k], np.float64).reshape(-1) - np.asarray(ref[k], np.float64).reshape(-1)))
            / max(norms[k], floor) for k in ref}


def whole_rel(got, ref, num_inputs):
    a, b = join_flat(got, num_inputs), join_flat(ref, num_inputs)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def worst(rel):
    k = max(rel, key=rel.get)
    return k, rel[k]
