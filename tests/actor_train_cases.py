"""Cases and the CPU reference of the actor's train-mode forward tests: the torch stand-in of tests/actor_cases.py in `.train()`
mode (F.batch_norm(training=True, momentum=0.1, eps=1e-5)), run once per case and shared.  No GPU needed to import."""
import functools

import numpy as np
import torch

from tests import actor_cases as A
from tfpnp_amd import synth

# ((num_inputs, n_det, spi), (B, H, W)): last-stage values per channel 16, 9, 8, 10
CASES = [((9, 10, False), (4, 64, 64)), ((7, 10, False), (3, 32, 96)), ((17, 15, False), (2, 64, 64)), ((6, 10, True), (5, 64, 32))]
IDS = ["c9_4x64x64", "c7_3x32x96", "c17_2x64x64", "spi6_5x64x32"]
WEIGHT_SEED, OB_SEED = 3, 11
N_BN = 4864


@functools.lru_cache(maxsize=None)
def params(case):
    return synth.make_policy_params(*case, seed=WEIGHT_SEED)


def observation(case, shape, kind="unit"):
    """RandomState(11).uniform(0, 1); kind 'offset': 0.9 + 0.2 u (a large mean against the spread)."""
    u = np.random.RandomState(OB_SEED).uniform(0, 1, (shape[0], case[0], shape[1], shape[2]))
    return (0.9 + 0.2 * u if kind == "offset" else u).astype(np.float32)


def stat_slices(case):
    """[(first float, count)] of every running_mean / running_var in the flat vector, in order."""
    return [A.offset_of(k, case) for k, _ in synth.policy_param_specs(*case)
            if k.endswith("running_mean") or k.endswith("running_var")]


def stat_mask(case):
    """bool [n_params]: True at the running statistics."""
    n = sum(int(np.prod(s)) for _, s in synth.policy_param_specs(*case))
    m = torch.zeros(n, dtype=torch.bool)
    for pos, cnt in stat_slices(case):
        m[pos:pos + cnt] = True
    return m


def running_of(module):
    sd = module.state_dict()
    return torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith("running_mean") or k.endswith("running_var")])


def train_forward(module, ob):
    """One train-mode forward of the stand-in: (probs, det, batch mean [4864], biased batch variance [4864]) in state_dict order."""
    means, variances, hooks = [], [], []

    def hook(m, inp):
        x = inp[0].detach()
        means.append(x.mean(dim=(0, 2, 3)))
        variances.append(x.var(dim=(0, 2, 3), unbiased=False))

    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            hooks.append(m.register_forward_pre_hook(hook))
    module.train()
    with torch.no_grad():
        probs, det = module(ob)
    for h in hooks:
        h.remove()
    return probs, det, torch.cat(means), torch.cat(variances)


@functools.lru_cache(maxsize=None)
def reference(case, shape, kind="unit", forwards=2):
    """The float64 stand-in: `forwards` train forwards on the observation, then an eval forward.  Also the fp32 stand-in's first
    train forward, for its own error against float64.  Everything as float64 / fp32 CPU tensors; do not modify."""
    ob = torch.from_numpy(observation(case, shape, kind))
    m64 = A.load_params(A.stand_in_actor(*case), params(case)).double()
    out = {}
    for it in range(1, forwards + 1):
        p, d, mean, var = train_forward(m64, ob.double())
        out[f"probs{it}"], out[f"det{it}"], out[f"running{it}"] = p, d, running_of(m64)
        if it == 1:
            out["mean"], out["var"] = mean, var
    m64.eval()
    with torch.no_grad():
        out["probs_eval"], out["det_eval"] = m64(ob.double())
    m32 = A.load_params(A.stand_in_actor(*case), params(case))
    p32, d32, _, _ = train_forward(m32, ob)
    out["fp32_err"] = max(float((p32.double() - out["probs1"]).abs().max()), float((d32.double() - out["det1"]).abs().max()))
    return out
