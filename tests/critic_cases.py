"""Cases of the critic tests (tests/golden/critic_value.npz, written by tools/make_critic_golden.py) and a plain
restatement of ResNet_wobn(num_inputs, 18, 1) (tfpnp/trainer/mddpg/critic.py:95-131) used for full-size comparisons:
F.conv2d on weight-norm-folded weights, TReLU as max(x, alpha), in the dtype asked for.  No GPU, no reference import."""
import numpy as np
import torch
import torch.nn.functional as F

from tfpnp_amd import synth

CRITIC_WEIGHT_SEED = 7
DISCOUNT = 0.99
# name -> (num_inputs, B, H, W, base seed); inputs of try k are drawn with seed base + 100 * k
CASES = {"kf9": (9, 1, 32, 32, 4100), "kf17": (17, 1, 32, 32, 4200), "arb": (9, 2, 64, 64, 4300), "rect": (9, 3, 64, 96, 4400)}
KINKFREE_TRIES = 16
# The try index of every case is frozen IN the golden (`<name>_try`) by tools/make_critic_golden.py -- kink-free cases: the
# qualifying try with the largest margin; arb: the first try whose reference fp32-vs-fp64 gradient difference stays below
# ARB_MAX_REF_DIFF, a tenth of the project's kink-flip bound.
ARB_MAX_REF_DIFF = 2e-3


def critic_params(num_inputs):
    return synth.make_critic_params(num_inputs, CRITIC_WEIGHT_SEED)


def case_inputs(name, k):
    """(ob [B,C,H,W] uniform in [0,1], w [B] weights of the scalar sum(V * w)) of case `name`, try k."""
    C, B, H, W, base = CASES[name]
    rs = np.random.RandomState(base + 100 * int(k))
    ob = rs.uniform(0, 1, (B, C, H, W)).astype(np.float32)
    w = rs.standard_normal(B).astype(np.float32)
    return ob, w


def big_inputs(B=6, C=9, H=256, W=256, seed=4500):
    return np.random.RandomState(seed).uniform(0, 1, (B, C, H, W)).astype(np.float32)


def folded(params, dtype):
    """{conv prefix: (weight, bias)} with weight = g * v / ||v|| (norm per output channel), plus alphas and fc, as tensors."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in params.items()}
    out = {}
    for k in t:
        if k.endswith(".weight_v"):
            p = k[:-len(".weight_v")]
            v, g = t[k], t[p + ".weight_g"]
            out[p] = (g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1), t[p + ".bias"])
        elif k.endswith(".alpha") or k.startswith("fc."):
            out[k] = t[k]
    return out


class Probe:
    """Records the smallest distance of any TReLU input from its threshold, relative to the layer's mean |input|, and (optionally)
    every TReLU output."""

    def __init__(self, keep=False):
        self.margin = float("inf")
        self.acts = [] if keep else None

    def see(self, x, alpha, y):
        self.margin = min(self.margin, float(((x - alpha).abs().min() / x.abs().mean()).detach()))
        if self.acts is not None:
            self.acts.append(y.detach())


def restate(params, x, dtype=torch.float64, probe=None):
    """V [B,1] of the critic on x (tensor or array) in `dtype`; differentiable with respect to a tensor x."""
    P = folded(params, dtype)
    x = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(dtype)
    P = {k: (tuple(u.to(x.device) for u in v) if isinstance(v, tuple) else v.to(x.device)) for k, v in P.items()}

    def trelu(v, key):
        y = torch.maximum(v, P[key])
        if probe is not None:
            probe.see(v, P[key], y)
        return y

    def conv(v, key, stride, pad):
        return F.conv2d(v, P[key][0], P[key][1], stride=stride, padding=pad)

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


def restate_value_and_grad(params, ob, w, dtype):
    """(V [B,1], d sum(V * w) / d ob, kink margin) of the restatement in `dtype`, as float64 numpy arrays."""
    x = torch.from_numpy(np.ascontiguousarray(ob)).to(dtype).requires_grad_(True)
    probe = Probe()
    V = restate(params, x, dtype, probe)
    (V[:, 0] * torch.from_numpy(w).to(dtype)).sum().backward()
    return V.detach().double().numpy(), x.grad.double().numpy(), probe.margin


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def stand_in_module(num_inputs):
    """A torch.nn.utils.weight_norm module with the reference critic's registration order, built without the reference."""
    import torch.nn as nn
    wn = torch.nn.utils.weight_norm

    class TReLU(nn.Module):
        def __init__(self):
            super().__init__()
            self.alpha = nn.Parameter(torch.zeros(1))

    class Block(nn.Module):
        def __init__(self, cin, p, stride):
            super().__init__()
            self.conv1 = wn(nn.Conv2d(cin, p, 3, stride, 1, bias=True))
            self.conv2 = wn(nn.Conv2d(p, p, 3, 1, 1, bias=True))
            self.shortcut = nn.Sequential()
            if stride != 1 or cin != p:
                self.shortcut = nn.Sequential(wn(nn.Conv2d(cin, p, 1, stride, bias=True)))
            self.relu_1 = TReLU()
            self.relu_2 = TReLU()

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = wn(nn.Conv2d(num_inputs, 64, 3, 2, 1, bias=True))
            cin = 64
            for li, p in enumerate((64, 128, 256, 512), start=1):
                setattr(self, f"layer{li}", nn.Sequential(Block(cin, p, 2), Block(p, p, 1)))
                cin = p
            self.fc = nn.Linear(512, 1)
            self.relu_1 = TReLU()

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Net()

