"""Cases and helpers of the actor live-weight tests: a torch stand-in for the reference's ResNetActor_* written from
synth.policy_param_specs (same attribute names, so the same state_dict keys), flat-vector helpers and the output comparison.
No GPU needed to import, no reference import."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tfpnp_amd import synth

# (num_inputs, n_det, spi_head): cin_pad 16; one padded input channel; cin_pad 24; the SPI head
CASES = [(9, 10, False), (7, 10, False), (17, 15, False), (6, 10, True)]
_ACTORS = {(9, 10, False): ("ResNetActor_ADMM", 6), (7, 10, False): ("ResNetActor_HQS", 5),
           (17, 15, False): ("ResNetActor_IADMM", 14), (6, 10, True): ("ResNetActor_SPI", 3)}


def native_actor(case, state_dict=None):
    """A native actor (action bundle 5) with the head of `case`."""
    from tfpnp_amd import policy
    name, num_aux = _ACTORS[tuple(case)]
    actor = getattr(policy, name)(num_aux, 5, state_dict=state_dict)
    assert (actor.in_dim, actor.n_det, bool(actor.spi_head)) == tuple(case)
    return actor


def stand_in_actor(num_inputs, n_det, spi):
    """ResNet-18 encoder with BatchNorm2d + the two heads under the reference actor's attribute names
    (tfpnp/policy/network.py: actor_encoder.{conv1,bn1,layer1..4}, fc_softmax, fc_deterministic)."""

    class Block(nn.Module):
        def __init__(self, cin, p, stride):
            super().__init__()
            self.conv1 = nn.Conv2d(cin, p, 3, stride, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(p)
            self.conv2 = nn.Conv2d(p, p, 3, 1, 1, bias=False)
            self.bn2 = nn.BatchNorm2d(p)
            self.shortcut = nn.Sequential()
            if stride != 1 or cin != p:
                self.shortcut = nn.Sequential(nn.Conv2d(cin, p, 1, stride, bias=False), nn.BatchNorm2d(p))

        def forward(self, x):
            out = F.relu(self.bn1(self.conv1(x)))
            out = self.bn2(self.conv2(out))
            return F.relu(out + self.shortcut(x))

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(num_inputs, 64, 3, 2, 1, bias=False)
            self.bn1 = nn.BatchNorm2d(64)
            cin = 64
            for li, p in enumerate((64, 128, 256, 512), start=1):
                setattr(self, f"layer{li}", nn.Sequential(Block(cin, p, 2), Block(p, p, 1)))
                cin = p

        def forward(self, x):
            x = F.relu(self.bn1(self.conv1(x)))
            for li in range(1, 5):
                x = getattr(self, f"layer{li}")(x)
            return F.adaptive_avg_pool2d(x, 1).flatten(1)

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.actor_encoder = Encoder()
            self.fc_softmax = nn.Sequential(nn.Linear(512, 2), nn.Softmax(dim=1))
            if spi:
                self.fc_deterministic = nn.Sequential(nn.Linear(512, 64), nn.ReLU(), nn.Linear(64, n_det), nn.Sigmoid())
            else:
                self.fc_deterministic = nn.Sequential(nn.Linear(512, n_det), nn.Sigmoid())

        def forward(self, x):
            x = self.actor_encoder(x)
            return self.fc_softmax(x), self.fc_deterministic(x)

    return Actor()


def fp32_entries(state_dict):
    """[(key, shape)] of the floating-point entries of a state_dict, in order (num_batches_tracked is int64)."""
    return [(k, tuple(v.shape)) for k, v in state_dict.items() if v.dtype == torch.float32]


def load_params(module, params):
    """synth.make_policy_params arrays -> the stand-in module (in place); returns the module."""
    with torch.no_grad():
        sd = module.state_dict(keep_vars=True)
        for k, v in params.items():
            sd[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    return module


def flat_vector(state, case):
    """The flat fp32 vector of `state` (arrays or tensors under the reference's keys) in policy_param_specs order, CPU."""
    chunks = []
    for key, shape in synth.policy_param_specs(*case):
        v = state[key]
        v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
        assert tuple(v.shape) == tuple(shape), key
        chunks.append(v.reshape(-1).float())
    return torch.cat(chunks)


def offset_of(key, case):
    """(first float, count) of entry `key` in the flat vector."""
    pos = 0
    for k, shape in synth.policy_param_specs(*case):
        n = int(np.prod(shape))
        if k == key:
            return pos, n
        pos += n
    raise KeyError(key)


def same_outputs(a, b, ob):
    """probs and det of ops.policy_forward agree bit for bit between actors a and b on ob's device, are finite, and probs
    is not constant across rows (a network that ignores its input would pass otherwise)."""
    from tfpnp_amd import ops
    pa, da = ops.policy_forward(a.context(ob.device), ob)
    pb, db = ops.policy_forward(b.context(ob.device), ob)
    finite = bool(torch.isfinite(pa).all() and torch.isfinite(da).all())
    varies = bool((pa[0] != pa[1]).any())
    return torch.equal(pa, pb) and torch.equal(da, db) and finite and varies

