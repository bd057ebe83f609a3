"""Cases and helpers of the actor live-weight tests: a torch stand-in for the reference's ResNetActor_* written from
synth.policy_param_specs (same attribute names, so the same state_dict keys), flat-vector helpers, the output comparison,
and a numpy restatement of the host's dense effective weights (csrc/resnet18_hs.hip: Eff, put_conv_s2, put_shortcut behind csrc/policy.hip: bn_folded; csrc/policy.hip: pack_eff)
that checks the structural-presence rule of the device packing.  No GPU needed to import, no reference import."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tfpnp_amd import synth

# (num_inputs, n_det, spi_head): cin_pad 16; one padded input channel; cin_pad 24; the SPI head
CASES = [(9, 10, False), (7, 10, False), (17, 15, False), (6, 10, True)]
_ACTORS = {(9, 10, False): ("ResNetActor_ADMM", 6), (7, 10, False): ("ResNetActor_HQS", 5),
           (17, 15, False): ("ResNetActor_IADMM", 14), (6, 10, True): ("ResNetActor_SPI", 3)}
BN_EPS = np.float32(1e-5)


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


# ------------------------------------------------------------------------------- structural presence of the fp32 tap slices
def _bn_scale(P, pre):
    return (P[pre + ".weight"] / np.sqrt(P[pre + ".running_var"] + BN_EPS)).astype(np.float32)


def _put_conv_s2(E, w, sc, Cp):
    """csrc/resnet18_hs.hip::put_conv_s2: 3x3 stride-2 convolution over a space-to-depth input with Cp channels per phase."""
    cout, cin = w.shape[:2]
    for dy in range(3):
        for dx in range(3):
            py, ty = (0 if dy == 1 else 1), (0 if dy == 0 else 1)
            px, tx = (0 if dx == 1 else 1), (0 if dx == 0 else 1)
            k0 = (py * 2 + px) * Cp
            E[:cout, k0:k0 + cin, ty * 3 + tx] = w[:, :, dy, dx] * sc[:, None]


def entry_launches(P, num_inputs):
    """The five fp32 launches of policy_load as dense effective weights E[cout][K][9] (BatchNorm folded): the stem, then
    per stage conv1 (rows [0, p)) merged with the 1x1 shortcut (rows [p, 2p), centre tap of phase (0,0)).
    Yields (name, E, rows of conv1, real input channels, channels per phase)."""
    cin_pad = (num_inputs + 7) // 8 * 8
    E = np.zeros((64, 4 * cin_pad, 9), np.float32)
    _put_conv_s2(E, P["actor_encoder.conv1.weight"], _bn_scale(P, "actor_encoder.bn1"), cin_pad)
    yield "stem", E, 64, num_inputs, cin_pad
    cin = 64
    for li, p in enumerate((64, 128, 256, 512), start=1):
        pre = f"actor_encoder.layer{li}.0"
        E = np.zeros((2 * p, 4 * cin, 9), np.float32)
        _put_conv_s2(E, P[pre + ".conv1.weight"], _bn_scale(P, pre + ".bn1"), cin)
        E[p:, :cin, 4] = P[pre + ".shortcut.0.weight"][:, :, 0, 0] * _bn_scale(P, pre + ".shortcut.1")[:, None]
        yield f"layer{li}", E, p, cin, cin
        cin = p


def present_by_value(E):
    """pack_eff's rule: slice (cout tile, 8-channel chunk, tap) exists iff it holds a non-zero value -> bool [nct][nch][9]"""
    cout, K, _ = E.shape
    return (E.reshape(cout // 64, 64, K // 8, 8, 9) != 0).any(axis=(1, 3))


def present_by_structure(cout, K, split, cin, Cp):
    """The device packing's rule: a conv1 tile has tap 4 in phase (0,0), taps 3, 4 in (0,1), 1, 4 in (1,0) and 0, 1, 3, 4 in
    (1,1), in every chunk of the phase that holds a real input channel; a shortcut tile has tap 4 in the phase-(0,0) chunks."""
    taps = {0: (4,), 1: (3, 4), 2: (1, 4), 3: (0, 1, 3, 4)}
    out = np.zeros((cout // 64, K // 8, 9), bool)
    for ct in range(cout // 64):
        for ch in range(K // 8):
            ph, first = divmod(ch * 8, Cp)
            if first >= cin:
                continue
            if ct * 64 < split:
                out[ct, ch, list(taps[ph])] = True
            elif ph == 0:
                out[ct, ch, 4] = True
    return out
