"""Cases and the CPU reference of the actor's parameter-gradient tests: the torch stand-in of tests/actor_cases.py in `.train()` mode,
in float64, differentiated by autograd.  The loss is sum(gp * probs) + sum(gd * det) with gp, gd from RandomState(5).standard_normal, on
the shapes and observations of tests/actor_train_cases.py.  Run once per case and shared.  No GPU needed to import."""
import functools

import numpy as np
import torch

from tests import actor_cases as A
from tests import actor_train_cases as T
from tfpnp_amd import synth

CASES, IDS = T.CASES, T.IDS
UPSTREAM_SEED = 5
# the project's critic-gradient contract on kink-free input: relative L2 per tensor / on the whole vector
TENSOR_BOUND, VECTOR_BOUND = 1e-3, 1e-4


def upstream(case, shape):
    """(gp [B,2], gd [B,n_det]) fp32: d loss / d probs, d loss / d det."""
    r = np.random.RandomState(UPSTREAM_SEED)
    gp = r.standard_normal((shape[0], 2)).astype(np.float32)
    gd = r.standard_normal((shape[0], case[1])).astype(np.float32)
    return gp, gd


def is_stat(key):
    return key.endswith("running_mean") or key.endswith("running_var")


def autograd_flat(module, ob, gp, gd):
    """Flat gradient (policy_param_specs order, zeros at the running statistics) of sum(gp * probs) + sum(gd * det) through the
    train-mode forward of `module`, in the module's dtype; the running statistics of the module are restored afterwards."""
    case = (module.actor_encoder.conv1.in_channels, gd.shape[1], len(module.fc_deterministic) == 4)
    saved = {k: v.clone() for k, v in module.state_dict().items()}
    module.train()
    module.zero_grad()
    probs, det = module(ob)
    loss = (gp * probs).sum() + (gd * det).sum()
    loss.backward()
    named = dict(module.named_parameters())
    chunks = []
    for key, shp in synth.policy_param_specs(*case):
        chunks.append(torch.zeros(int(np.prod(shp)), dtype=ob.dtype) if is_stat(key) else named[key].grad.detach().reshape(-1).clone())
    module.load_state_dict(saved)
    module.zero_grad()
    return torch.cat(chunks), float(loss.detach())


def stand_in(case, params=None, dtype=torch.float64):
    return A.load_params(A.stand_in_actor(*case), T.params(case) if params is None else params).to(dtype)


@functools.lru_cache(maxsize=None)
def reference(case, shape):
    """{'grad': float64 flat gradient, 'fp32': the fp32 stand-in's, 'loss': float}; do not modify."""
    ob = torch.from_numpy(T.observation(case, shape))
    gp, gd = (torch.from_numpy(a) for a in upstream(case, shape))
    g64, loss = autograd_flat(stand_in(case), ob.double(), gp.double(), gd.double())
    g32, _ = autograd_flat(stand_in(case, dtype=torch.float32), ob, gp, gd)
    return {"grad": g64, "fp32": g32.double(), "loss": loss}


def tensors(case):
    """[(key, first float, count)] of the gradient tensors (everything but the running statistics): 67, or 69 with the SPI head."""
    out, pos = [], 0
    for key, shp in synth.policy_param_specs(*case):
        n = int(np.prod(shp))
        if not is_stat(key):
            out.append((key, pos, n))
        pos += n
    return out


def rel_l2(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def errors(flat, ref, case):
    """(worst per-tensor relative L2, its key, whole-vector relative L2) of a flat gradient against the float64 reference."""
    flat = flat.detach().double().cpu()
    worst, key = 0.0, None
    for k, pos, n in tensors(case):
        e = rel_l2(flat[pos:pos + n], ref[pos:pos + n])
        if e > worst:
            worst, key = e, k
    return worst, key, rel_l2(flat, ref)


# tests/golden/policy_actor_grad.npz (tools/make_actor_grad_golden.py): the executed reference actor's autograd on this case
GOLDEN_CASE, GOLDEN_SHAPE = CASES[1]
GOLDEN_SAMPLES, GOLDEN_SEED = 256, 7


def sample_positions(n):
    """The 256 seeded positions of a tensor of n elements the golden file keeps (with repetition)."""
    return np.random.RandomState(GOLDEN_SEED).randint(0, n, GOLDEN_SAMPLES).astype(np.int64)
