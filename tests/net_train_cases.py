"""Cases, inputs, float64 references, fp32 emulations and bars of the probe of the actor's and the critic's training kernels
(pnpx_net_train_probe, csrc/net_train_probe.hip; launchers: csrc/policy_grad.h, csrc/critic_grad.h; kernels: csrc/policy_bn.hip,
csrc/policy_grad.hip, csrc/critic_grad.hip).  No GPU and no library at import.

Inputs are seeded by the case's name and HS8-representable (drawn, then rounded through hs8_encode / hs8_decode of tests/conv_hs_cases.py):
the decoded values are exact in float64.  References are float64 torch on the decoded inputs, autograd where there is a function to
differentiate (BN_BWD: F.batch_norm(training=True) behind the ReLU mask; WGRAD_*: conv2d with respect to its weight, through weight-norm;
HEAD_GRAD: the heads).  The measure is per element: |y - ref| over the sum of the magnitudes of the terms the output was added up from.

  exact ops (CLIP_MASK, dy_out, the space-to-depth copy against out, the zeros in the running-statistics slots of a gradient, the slot
    and gv of GRAD_SEED): bit-identical to a torch restatement.
  fp32 chains (the wgrad GEMM and what is finished from it, the BN_APPLY and BN_BWD apply passes, HEAD_GRAD, GRAD_SEED's tensor): bar =
    BAR_FACTOR x the largest measure of an fp32 CPU emulation in the kernel's own operation order over the class's cases (DERIVED_KEYS).
  double accumulation, rounded to fp32 once (FIXED_BARS): k x 2^-24, k = the roundings counted on the longest path.
profiles/net_train_probe.md records the emulation maxima and the bars; tests/test_net_train_host.py re-derives them."""
import collections
import functools
import math
import os
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_hs_cases import ASCALE, BAR_FACTOR, hs8_decode, hs8_encode, quantize  # noqa: F401  (re-exported to the tests)
from tests.vjp_glue_cases import bits_equal, measure  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE_NOTE = os.path.join(ROOT, "profiles", "net_train_probe.md")
U = 2.0 ** -24
BN_EPS = 1e-5
BN_PIECE = 2048            # csrc/policy_grad.h: BN_FWD_PIECE, BN_BWD_PIECE
WG_KC = 32                 # csrc/critic_grad.hip: pixels per chunk
RANGE_LIMIT = 4095.0

# include/pnpx.h: enum pnpx_net_train_op
BN_STATS, BN_APPLY, BN_BWD, WGRAD_PLAIN, WGRAD_WN, CLIP_MASK, ALPHA_DOT, FC_GRAD, ALPHA_FINISH, HEAD_GRAD, GRAD_SEED = range(11)
OP_NAMES = ("BN_STATS", "BN_APPLY", "BN_BWD", "WGRAD_PLAIN", "WGRAD_WN", "CLIP_MASK", "ALPHA_DOT", "FC_GRAD", "ALPHA_FINISH", "HEAD_GRAD",
            "GRAD_SEED")

# Fixed bars (units of 2^-24 = the unit roundoff of fp32) and the roundings behind them.  Sums and the arithmetic after them run in
# double (2^-53 per step, far below 2^-24 of the denominators used: the count keeps one unit for all of it).
FIXED_BARS = collections.OrderedDict((
    ("bn_stats", (2, "mean, variance (against the two-pass float64 variance, relative to var + eps), scale, shift: the store to fp32 (1) + the double arithmetic (1)")),
    ("bn_running", (2, "running statistics, the variance times n / (n - 1): the store (1) + the double arithmetic (1)")),
    ("bn_bwd_sums", (4, "d weight, d bias, coef: the fp32 variance the op is given (rstd^3 in c2: 1.5), its fp32 mean (1), the store (1); "
                       "the products with 1 / s and 1 / boost are exact")),
    ("fc_grad", (2, "fc.weight's gradient: the store (1) + the double arithmetic (1)")),
    ("alpha_finish", (2, "thresholds and fc.bias: the store (1) + the double arithmetic (1)")),
))
DOUBLE_BAR = 2.0 ** -40     # outputs left in double (ALPHA_DOT, FC_GRAD's a20): sums of at most 2^12 exact products, 2^-53 each step
DERIVED_KEYS = ("bn_apply", "bn_bwd_dz", "wgrad", "wgrad_bias", "wgrad_wn_v", "wgrad_wn_g", "head_gf", "head_param", "grad_seed")


def fixed_bar(key):
    return FIXED_BARS[key][0] * U


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def q(x):
    """x rounded to what an HS8 record holds, as fp32 (exact: hi + lo has at most 22 significant bits)."""
    return quantize(x, torch.float32)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _signed(g, *shape):
    """Magnitudes in [0.1, 1], random signs."""
    return (0.1 + 0.9 * torch.rand(*shape, generator=g)) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def records(x, garbage=None):
    """hs8_encode(x); garbage (a name): every border record holds finite non-zero values instead of zeros."""
    r = hs8_encode(x)
    if garbage is not None:
        B, C, H, W = x.shape
        junk = hs8_encode(q(3.0 * _signed(_gen("border " + garbage), B, C, H + 2, W + 2)))[:, :, 1:-1, 1:-1]
        junk[:, :, 1:-1, 1:-1] = r[:, :, 1:-1, 1:-1]
        r = junk.contiguous()
    return r


def interior_records(x):
    return hs8_encode(x)[:, :, 1:-1, 1:-1].contiguous()


def decode_interior(rec):
    """[B][G][H][W][16] f16 records (no border) -> float64 values [B][8 G][H][W]."""
    v = (rec[..., :8].double() + rec[..., 8:].double()) / ASCALE
    B, G, H, W, _ = v.shape
    return v.permute(0, 1, 4, 2, 3).reshape(B, G * 8, H, W)


def s2d(x):
    """[B][C][H][W] -> [B][4 C][H/2][W/2], channel (2 (y & 1) + (x & 1)) C + c (whole groups of 8 move together when C % 8 == 0)."""
    return torch.cat([x[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], 1).contiguous()


# =================================================================================================================================
# plans, restated

def bn_pieces(B, h, w):
    return (B * h * w + BN_PIECE - 1) // BN_PIECE


def wgrad_pieces(cout, K, B, h, w):
    """(pieces, chunks per piece): csrc/critic_grad.hip, critic_wgrad_pieces."""
    tiles = (cout // 32) * (K // 32)
    nchunks = (B * h * w + WG_KC - 1) // WG_KC
    want = max(1, min((512 + tiles - 1) // tiles, 64, nchunks // 2))
    cpp = (nchunks + want - 1) // want
    pieces = (nchunks + cpp - 1) // cpp               # no empty piece
    return pieces, (nchunks + pieces - 1) // pieces   # launch_critic_wgrad: chunks per piece from the piece count


KIND_WINDOW = {0: 0x1FF, 1: 0x01B, 2: 0x010}


def window_taps(kind):
    return [t for t in range(9) if (KIND_WINDOW[kind] >> t) & 1]


def plan_py(op, **kw):
    """pnpx_net_train_probe_plan in plain Python; 0 = refused.  Sizes only (no operands)."""
    k = collections.defaultdict(int, kw)
    B, G, h, w = k["B"], k["G"], k["h"], k["w"]
    wg = op in (WGRAD_PLAIN, WGRAD_WN)
    has_G = op in (BN_STATS, BN_APPLY, BN_BWD, CLIP_MASK, ALPHA_DOT)
    has_hw = op != ALPHA_FINISH
    if op < 0 or op > GRAD_SEED:
        return 0
    if not wg and any(k[n] for n in ("cout", "K", "cin", "Cp", "kind", "Gg", "Xg")):
        return 0
    if (not has_G and G) or (not has_hw and (h or w)) or (op != ALPHA_DOT and (k["resG"] or k["mG"])) or (op != HEAD_GRAD and (k["n_det"] or k["spi"])):
        return 0
    if (op != BN_STATS and (k["update"] or k["momentum"])) or (op not in (CLIP_MASK, FC_GRAD) and k["thr"]) or (op not in (BN_BWD, GRAD_SEED) and k["boost"]):
        return 0
    if (not wg and op != ALPHA_FINISH and k["inv_w"]) or (op != WGRAD_WN and k["inv_b"]):
        return 0
    if B <= 0 or (has_hw and (h <= 0 or w <= 0)) or (has_G and G <= 0):
        return 0
    npix = B * h * w if has_hw else B
    if npix > 1 << 24:
        return 0
    groups = G if has_G else max(k["Gg"], k["Xg"]) if wg else 64
    if has_hw and B * groups * (h + 2) * (w + 2) > 1 << 28:
        return 0
    pow2 = lambda v: v > 0 and math.isfinite(v) and math.frexp(v)[0] == 0.5
    if op == BN_STATS:
        if not 0 <= k["momentum"] <= 1 or k["update"] not in (0, 1) or (k["update"] and npix < 2):
            return 0
        return bn_pieces(B, h, w)
    if op == BN_APPLY:
        return (npix * G + 255) // 256
    if op == BN_BWD:
        return bn_pieces(B, h, w) if (k["boost"] == 0 or pow2(k["boost"])) else 0
    if wg:
        cout, K, cin, Cp, kind = k["cout"], k["K"], k["cin"], k["Cp"], k["kind"]
        if cout <= 0 or K <= 0 or cin <= 0 or cout % 32 or K % 32 or kind not in (0, 1, 2):
            return 0
        if (Cp <= 0 or K != 4 * Cp or cin > Cp) if kind == 1 else (Cp != 0 or cin > K):
            return 0
        if k["Gg"] < cout // 8 or k["Xg"] < K // 8 or not k["inv_w"] or (op == WGRAD_WN and not k["inv_b"]):
            return 0
        p, cpp = wgrad_pieces(cout, K, B, h, w)
        return p + 256 * cpp
    if op == ALPHA_DOT:
        rG, mG = k["resG"], k["mG"]
        return 0 if (rG < 0 or mG < rG or (rG == 0) != (mG == 0)) else 1
    if op == HEAD_GRAD:
        if not 1 <= k["n_det"] <= 64 or k["spi"] not in (0, 1):
            return 0
        return 2 + (64 + k["n_det"] if k["spi"] else k["n_det"])
    if op == GRAD_SEED:
        return 1 if pow2(k["boost"]) else 0
    return 1


def plan(op, **kw):
    """pnpx_net_train_probe_plan (the library; host only)."""
    import ctypes
    from tfpnp_amd import _lib
    d = _lib.NetTrainProbeDesc(op=op, **kw)
    return _lib.lib().pnpx_net_train_probe_plan(ctypes.byref(d))


# =================================================================================================================================
# BatchNorm

BnCase = collections.namedtuple("BnCase", "name B G h w two res out s2d update momentum dy_out slot boost trip")


def _bn(name, B, G, h, w, two=False, res=False, out=True, s2d=False, update=0, momentum=0.0, dy_out=False, slot=None, boost=0.0, trip=False):
    return BnCase(name, B, G, h, w, two, res, out, s2d, update, momentum, dy_out, slot, boost, trip)


BN_SHAPES = ((2, 8, 2, 3), (2, 1, 32, 32), (1, 2, 33, 63), (3, 1, 40, 37), (2, 64, 2, 2), (2, 3, 4, 6))     # pieces 1, 1, 2, 3, 1, 1
STATS_CASES = tuple(_bn("stats_%dx%dx%dx%d" % s, *s, update=i % 2, momentum=(0.1, 0.25, 0.5)[i % 3]) for i, s in enumerate(BN_SHAPES)) + (
    _bn("stats_m1_2x1x3x5", 2, 1, 3, 5, update=1, momentum=1.0),)
_FORMS = (("a", False, False), ("ab", True, False), ("ares", False, True))
APPLY_CASES = tuple(_bn("apply_%s_%s_2x2x4x6" % (f, o), 2, 2, 4, 6, two=t, res=r, out=o != "s2d", s2d=o != "out")
                    for f, t, r in _FORMS for o in ("out", "s2d", "both")) + \
    tuple(_bn("apply_%s_%dx%dx%dx%d" % ((_FORMS[i % 3][0],) + s), *s, two=_FORMS[i % 3][1], res=_FORMS[i % 3][2],
              s2d=(s[2] % 2 == 0 and s[3] % 2 == 0 and i % 2 == 0)) for i, s in enumerate(BN_SHAPES))
BWD_CASES = tuple(_bn("bwd_%dx%dx%dx%d" % s, *s, two=i % 2 == 1, dy_out=i % 3 == 0) for i, s in enumerate(BN_SHAPES)) + (
    _bn("bwd_two_dy_2x2x5x7", 2, 2, 5, 7, two=True, dy_out=True),
    _bn("bwd_slot_boost_2x1x6x5", 2, 1, 6, 5, slot=(2.0 ** 7, 2.0 ** -7), boost=8.0),
    _bn("bwd_trip_2x1x4x5", 2, 1, 4, 5, two=True, trip=True),
)
BN_CASE_BY_NAME = {c.name: c for c in STATS_CASES + APPLY_CASES + BWD_CASES}


def _bn_z(g, c):
    """A raw convolution output: per-channel mean and spread; channel 0 has its mean at 100 x the spread, channel 1 zero variance."""
    C = 8 * c.G
    mu = 2 * torch.rand(C, generator=g) - 1
    sd = 0.5 + torch.rand(C, generator=g)
    mu[0], sd[0] = 50.0, 0.5
    z = mu.view(1, C, 1, 1) + sd.view(1, C, 1, 1) * _randn(g, c.B, C, c.h, c.w)
    z[:, 1] = 0.75
    return q(z)


def _bn_params(g, C):
    """weight, bias, running_mean, running_var [4][C], fp32."""
    wt = _signed(g, C)
    return torch.stack([wt + 0.5 * torch.sign(wt), _signed(g, C), _signed(g, C), 0.5 + torch.rand(C, generator=g)]).float()      # 0.6 <= |weight| <= 1.5


@functools.lru_cache(maxsize=None)
def stats_inputs(name):
    c, g = BN_CASE_BY_NAME[name], _gen(name)
    return {"z0": _bn_z(g, c), "params": _bn_params(g, 8 * c.G)}


def stats_reference(c, d, border_cell=None, n_for_n1=False, drop_pixel=None, double_pixel=None):
    """{output: (ref, den)} in float64.  Mutants: border_cell = a (padded) value counted in channel 0's sums; n in place of n - 1; a pixel
    (index (b h + y) w + x) of every channel dropped from / doubled in the sums."""
    z = d["z0"].double()
    B, C, h, w = z.shape
    n = B * h * w
    P = d["params"].double()
    zf = z.permute(1, 0, 2, 3).reshape(C, n)
    wts = torch.ones(n, dtype=torch.float64)
    if drop_pixel is not None:
        wts[drop_pixel] = 0
    if double_pixel is not None:
        wts[double_pixel] = 2
    s = (zf * wts).sum(1)
    if border_cell is not None:
        s[0] += border_cell
    mean = s / n
    dev = zf - mean.view(C, 1)
    var = (dev * dev * wts).sum(1) / n
    if border_cell is not None:
        var[0] += (border_cell - mean[0]) ** 2 / n
    scale = P[0] / torch.sqrt(var + BN_EPS)
    shift = P[1] - mean * scale
    m = float(np.float32(c.momentum))
    out = {"mean": (mean, zf.abs().sum(1) / n), "var": (var, var + BN_EPS), "scale": (scale, scale.abs()),
           "shift": (shift, P[1].abs() + (mean * scale).abs())}
    if c.update:
        unb = var * (n / (n if n_for_n1 else n - 1.0))
        out["running_mean"] = ((1 - m) * P[2] + m * mean, ((1 - m) * P[2]).abs() + (m * mean).abs())
        out["running_var"] = ((1 - m) * P[3] + m * unb, ((1 - m) * P[3]).abs() + (m * unb).abs())
    return out


@functools.lru_cache(maxsize=None)
def apply_inputs(name):
    """z0 / st0 (mean, scale, beta) [, z1 / st1] [, res].  Channel 2 has scale = beta = 0 (and no second summand's share, no residual): an
    exact zero before the ReLU.  Everywhere else the float64 pre-activation is at least 1e-3 from zero (z0 is moved where it is not)."""
    c, g = BN_CASE_BY_NAME[name], _gen(name)
    C = 8 * c.G

    def stat(z):
        zz = z.double()
        st = torch.stack([zz.mean((0, 2, 3)), (0.5 + torch.rand(C, generator=g)).double() * torch.sign(_signed(g, C)).double(), _signed(g, C).double()]).float()
        st[1, 2] = st[2, 2] = 0.0
        return st
    d = {"z0": _bn_z(g, c)}
    d["st0"] = stat(d["z0"])
    if c.two:
        d["z1"] = _bn_z(g, c)
        d["st1"] = stat(d["z1"])
    if c.res:
        d["res"] = q(torch.relu(_randn(g, c.B, C, c.h, c.w)))
        d["res"][:, 2] = 0.0
    for _ in range(8):
        pre = apply_reference(c, d)["pre"]
        near = pre.abs() < 1e-3
        near[:, 2] = False
        if not bool(near.any()):
            break
        st = d["st0"].double()
        d["z0"] = q(torch.where(near, d["z0"].double() + 0.25 / st[1].view(1, C, 1, 1), d["z0"].double()))
    else:
        raise AssertionError(name + ": a pre-activation stays near the kink")
    return d


def apply_reference(c, d, emulate=False):
    """{"pre": float64 pre-activation, "out": (ref, den)}; emulate: fp32 in the kernel's order, the output through the records."""
    dt = torch.float32 if emulate else torch.float64
    C = 8 * c.G
    v = den = None
    for zk, sk in (("z0", "st0"), ("z1", "st1")):
        if zk in d:
            st = d[sk].to(dt).view(3, 1, C, 1, 1)
            t = (d[zk].to(dt) - st[0]) * st[1] + st[2]
            dn = (d[zk].double() - d[sk][0].double().view(1, C, 1, 1)).abs() * d[sk][1].double().abs().view(1, C, 1, 1) + d[sk][2].double().abs().view(1, C, 1, 1)
            v, den = (t, dn) if v is None else (v + t, den + dn)
    if "res" in d:
        v, den = v + d["res"].to(dt), den + d["res"].double().abs()
    y = torch.relu(v)
    if emulate:
        return q(y).double()
    return {"pre": v, "out": (y, den)}


@functools.lru_cache(maxsize=None)
def bwd_inputs(name):
    """g, act, z0, st0 = fp32 (batch mean, biased variance) of z0, params [nl][4][C] [, z1, st1].  act holds +0.0, -0.0 and negatives."""
    c, g = BN_CASE_BY_NAME[name], _gen(name)
    C = 8 * c.G
    shape = (c.B, C, c.h, c.w)
    act = q(torch.relu(_randn(g, *shape)) + 0.01 * (torch.rand(*shape, generator=g) < 0.1))
    flat = act.view(-1)
    flat[0], flat[1], flat[2] = 0.0, -0.0, -0.5
    flat[-1] = -0.0
    d = {"g": q((3000.0 if c.trip else 1.0) * _signed(g, *shape)), "act": act}
    nl = 2 if c.two else 1
    P = torch.stack([_bn_params(g, C) for _ in range(nl)])
    if c.trip:
        P[:, 0] = torch.sign(P[:, 0]) * 8.0
    d["params"] = P
    for i in range(nl):
        z = _bn_z(g, c)
        if i == 0:
            z[:, 1] = q(z[:, 1] + 0.01 * _randn(g, c.B, c.h, c.w))     # layer 0: a narrow channel; layer 1 keeps the constant one (var = 0, rstd = 1 / sqrt(eps))
        zz = z.double()
        d["z%d" % i] = z
        d["st%d" % i] = torch.stack([zz.mean((0, 2, 3)), zz.var((0, 2, 3), unbiased=False)]).float()
    return d


def bwd_mask(d):
    return (d["act"] > 0).double()


def bwd_reference(c, d, flip=None, mean_from=None):
    """{output: (ref, den)} by autograd through F.batch_norm(training=True) in float64, dy = g [act > 0].  Mutants: flip = a flat index
    whose mask bit is inverted; mean_from = 1: layer 0's sums use layer 1's mean."""
    C, n = 8 * c.G, c.B * c.h * c.w
    mask = bwd_mask(d)
    if flip is not None:
        mask = mask.clone()
        mask.view(-1)[flip] = 1 - mask.view(-1)[flip]
    dy = d["g"].double() * mask
    s, inv_boost = (c.slot or (1.0, 1.0))[1], (1.0 / c.boost if c.boost else 1.0)
    out = {"dy_out": (dy, dy.abs())}
    S1 = dy.sum((0, 2, 3))
    A1 = dy.abs().sum((0, 2, 3))
    for i in range(2 if c.two else 1):
        z = d["z%d" % i].double().requires_grad_(True)
        wt = d["params"][i, 0].double().requires_grad_(True)
        bs = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        y = F.batch_norm(z, None, None, wt, bs, True, 0.0, BN_EPS)
        dz, dw, db = torch.autograd.grad((y * dy).sum(), (z, wt, bs))
        zd = z.detach()
        mean, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
        if mean_from is not None and i == 0:
            m2 = d["z%d" % mean_from].double().mean((0, 2, 3))
            dw = (dy * (zd - m2.view(1, C, 1, 1))).sum((0, 2, 3)) / torch.sqrt(var + BN_EPS)
        rstd = 1 / torch.sqrt(var + BN_EPS)
        A = wt.detach() * rstd
        S2 = (dy * (zd - mean.view(1, C, 1, 1))).sum((0, 2, 3))
        A2 = (dy.abs() * (zd.abs() + mean.abs().view(1, C, 1, 1))).sum((0, 2, 3))
        coef = torch.stack([A, A * S1 / n, A * rstd * rstd * S2 / n])
        cden = torch.stack([A.abs(), A.abs() * A1 / n, A.abs() * rstd * rstd * A2 / n])
        v = lambda t: t.view(1, C, 1, 1)
        dzden = v(cden[0]) * dy.abs() + v(cden[1]) + v(coef[2].abs()) * (zd.abs() + v(mean.abs()))
        out["dz%d" % i] = (dz, dzden)
        out["dweight%d" % i] = (dw * s * inv_boost, A2 * rstd * s * inv_boost)
        out["dbias%d" % i] = (db * s * inv_boost, A1 * s * inv_boost)
        out["coef%d" % i] = (coef, cden)
    return out


def bwd_emulate(c, d):
    """dz of every layer as the kernels compute it: sums and coefficients in double from the fp32 statistics the op is given, rounded to
    fp32; the apply pass in fp32, A dy - c1 - c2 (z - mean); the output through the records."""
    C, n = 8 * c.G, c.B * c.h * c.w
    dy64 = d["g"].double() * bwd_mask(d)
    dy = dy64.float()
    out = {}
    for i in range(2 if c.two else 1):
        z, st = d["z%d" % i], d["st%d" % i]
        mean, var = st[0].double(), st[1].double()
        rstd = 1 / torch.sqrt(var + BN_EPS)
        S1 = dy64.sum((0, 2, 3))
        S2 = (dy64 * (z.double() - mean.view(1, C, 1, 1))).sum((0, 2, 3))
        A = d["params"][i, 0].double() * rstd
        cf = torch.stack([A, A * S1 / n, A * rstd * rstd * S2 / n]).float().view(3, 1, C, 1, 1)
        v = cf[0] * dy - cf[1] - cf[2] * (z - st[0].view(1, C, 1, 1))
        out["dz%d" % i] = q(v).double()
    return out


# =================================================================================================================================
# weight gradients

WgCase = collections.namedtuple("WgCase", "name wn kind cout K cin Cp B h w Gg Xg")
WG_SHAPES = ((32, 32, 2, 5, 7), (32, 32, 1, 12, 13), (32, 32, 1, 14, 16), (64, 64, 3, 6, 10), (128, 256, 2, 8, 8), (32, 32, 4, 32, 32),
             (64, 64, 2, 33, 31), (512, 512, 3, 2, 3))
WG_PIECES = (1, 2, 3, 3, 2, 64, 32, 1)


def _wg(wn, kind, shape, i):
    cout, K, B, h, w = shape
    Cp = K // 4 if kind == 1 else 0
    cin = (9 if K == 64 else Cp) if kind == 1 else K       # K = 64: the stem, 9 inputs in 16 padded channels
    Gg = cout // 8 + (1 if (kind == 0 and i == 0 and not wn) else 0)
    Xg = 4 * K // 8 if kind == 2 else K // 8
    return WgCase("%s_k%d_%dx%d_%dx%dx%d" % (("wn" if wn else "plain", kind) + shape), wn, kind, cout, K, cin, Cp, B, h, w, Gg, Xg)


WGRAD_CASES = tuple(_wg(False, 0, s, i) for i, s in enumerate(WG_SHAPES)) + \
    tuple(_wg(False, k, s, i) for k in (1, 2) for i, s in enumerate(WG_SHAPES[:4])) + \
    tuple(_wg(True, 0, s, i) for i, s in enumerate(WG_SHAPES[:4])) + (_wg(True, 1, WG_SHAPES[3], 3), _wg(True, 2, WG_SHAPES[1], 1))
WG_CASE_BY_NAME = {c.name: c for c in WGRAD_CASES}
WG_INV_W, WG_INV_B = 1.0 / 256, 1.0 / 16


def wg_fan(c):
    return c.cin if c.kind == 2 else 9 * c.cin


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    """G [B][8 Gg][h][w] (fp32 values of the records), X [B][8 Xg][h][w] (kind 1 / 2: the space-to-depth tensor of `full`, padding
    channels zero), full [B][cin][2h][2w], gv [B] (distinct, one zero where B >= 3, one negative where B >= 2), v / wg / bias for WN."""
    c, g = WG_CASE_BY_NAME[name], _gen(name)
    d = {"G": q(_signed(g, c.B, 8 * c.Gg, c.h, c.w))}
    if c.kind == 0:
        d["X"] = q(_signed(g, c.B, 8 * c.Xg, c.h, c.w))
    else:
        Cfull = c.Cp if c.kind == 1 else c.K
        full = q(_signed(g, c.B, Cfull, 2 * c.h, 2 * c.w))
        full[:, c.cin:] = 0.0 if c.kind == 1 else full[:, c.cin:]
        d["full"] = full
        d["X"] = s2d(full)
        assert d["X"].shape[1] == 8 * c.Xg or c.kind == 1
    gv = 0.5 + torch.arange(c.B).float() * 0.375
    if c.B >= 2:
        gv[1] = -0.75
    if c.B >= 3:
        gv[2] = 0.0
    if c.B >= 4:
        gv[3] = 1.625
    d["gv"] = gv
    if c.wn:
        d["v"] = _signed(g, c.cout, wg_fan(c)).float()
        d["wg"] = (_signed(g, c.cout) * 2).float()
        d["bias"] = _signed(g, c.cout).float()
    return d


def wgrad_operands(c, d):
    """(Gop [B][cout][h][w] float64 = the gradient operand BEFORE gv, taps' X [nt][B][K][h][w] float64) in stored units (x 16 each)."""
    Gs = d["G"][:, :c.cout].double() * ASCALE
    Xp = F.pad(d["X"][:, :c.K].double() * ASCALE, (1, 1, 1, 1))
    Xt = torch.stack([Xp[:, :, t // 3:t // 3 + c.h, t % 3:t % 3 + c.w] for t in window_taps(c.kind)])
    return Gs, Xt


def eff_pos(c, i):
    """csrc/pack_desc.h, eff_pos_of_src: raw element i of a fan -> (k, index of its tap in the window)."""
    taps = window_taps(c.kind)
    if c.kind == 0:
        return i // 9, taps.index(i % 9)
    if c.kind == 1:
        ci, t = i // 9, i % 9
        dy, dx = t // 3, t % 3
        py, ty, px, tx = (0 if dy == 1 else 1), (0 if dy == 0 else 1), (0 if dx == 1 else 1), (0 if dx == 0 else 1)
        return (py * 2 + px) * c.Cp + ci, taps.index(ty * 3 + tx)
    return i, 0


def _gather(c, E):
    """Effective-weight gradient [cout][nt][K] -> raw [cout][fan]."""
    pos = [eff_pos(c, i) for i in range(wg_fan(c))]
    return E[:, [p[1] for p in pos], [p[0] for p in pos]]


def wgrad_emulate_slab(c, d):
    """(sum of the pieces in double of slab[co][tap][k], of the bias column [co]): per piece fp32 fma chains in pixel order (operands as
    the kernel rebuilds them: the gradient times gv[b] rounded to fp32), the pieces added in double."""
    Gs, Xt = wgrad_operands(c, d)
    B, hw = c.B, c.h * c.w
    gop = (Gs.float() * d["gv"].view(B, 1, 1, 1)).double().permute(1, 0, 2, 3).reshape(c.cout, B * hw)        # one fp32 rounding
    xop = Xt.permute(0, 2, 1, 3, 4).reshape(Xt.shape[0], c.K, B * hw)
    pieces, cpp = wgrad_pieces(c.cout, c.K, c.B, c.h, c.w)
    tot = torch.zeros(c.cout, Xt.shape[0], c.K, dtype=torch.float64)
    btot = torch.zeros(c.cout, dtype=torch.float64)
    for p in range(pieces):
        acc = torch.zeros(c.cout, Xt.shape[0], c.K, dtype=torch.float64)
        bacc = torch.zeros(c.cout, dtype=torch.float64)
        for i in range(p * cpp * WG_KC, min((p + 1) * cpp * WG_KC, B * hw)):
            acc = (acc + gop[:, i].view(-1, 1, 1) * xop[:, :, i].unsqueeze(0)).float().double()        # fma: one rounding of the exact sum
            bacc = (bacc + gop[:, i]).float().double()
        tot += acc
        btot += bacc
    return tot, btot


def _weight_norm(v, g):
    return v * (g / v.norm(dim=1)).view(-1, 1)


def wgrad_forward(c, d, W, swap=False, tap_shift=None):
    """The convolution of the case in float64 with raw weights W [cout][fan]: [B][cout][h][w].  Mutants: swap = the kernel transposed in
    space; tap_shift = a raw tap index whose input is read one pixel to the right."""
    if c.kind == 2:
        return F.conv2d(d["full"][:, :c.cin].double(), W.view(c.cout, c.cin, 1, 1), stride=2)
    Wk = W.view(c.cout, c.cin, 3, 3)
    if swap:
        Wk = Wk.transpose(2, 3)
    x = (d["X"][:, :c.cin] if c.kind == 0 else d["full"][:, :c.cin]).double()
    st = 1 if c.kind == 0 else 2
    if tap_shift is None:
        return F.conv2d(x, Wk, stride=st, padding=1)
    keep = torch.ones(9, dtype=torch.float64)
    keep[tap_shift] = 0
    only = (1 - keep).view(1, 1, 3, 3)
    xs = F.pad(x, (0, 1))[..., 1:]       # x shifted left: the tap reads one pixel to the right
    return F.conv2d(x, Wk * keep.view(1, 1, 3, 3), stride=st, padding=1) + F.conv2d(xs, Wk * only, stride=st, padding=1)


def wgrad_reference(c, d, gv_swap=None, pixel_scale=None, swap=False, tap_shift=None, wrong_g_row=None):
    """{output: (ref, den)} in float64 by autograd: out = conv(x, W), L = sum_b gv[b] <G[b], out[b]>; the outputs times 16 * 16 * inv_w
    (bias: 16 * inv_b), the scales the records carry and the finishing kernels undo.
    Mutants: gv_swap = (lo, hi, b): pixels [lo, hi) of the flat pixel axis weighted with gv[b]; pixel_scale = (pixel, factor);
    swap / tap_shift: wgrad_forward; wrong_g_row = a row of the weight-norm that takes its neighbour's g."""
    B, hw = c.B, c.h * c.w
    wpix = d["gv"].double().view(B, 1).repeat(1, hw).reshape(-1)
    if gv_swap:
        wpix[gv_swap[0]:gv_swap[1]] = float(d["gv"][gv_swap[2]])
    if pixel_scale:
        wpix[pixel_scale[0]] *= pixel_scale[1]
    up = d["G"][:, :c.cout].double() * wpix.view(B, 1, c.h, c.w)
    fan = wg_fan(c)
    sw, sb = ASCALE * ASCALE * WG_INV_W, ASCALE * WG_INV_B
    if not c.wn:
        W = torch.zeros(c.cout, fan, dtype=torch.float64, requires_grad=True)
        (dW,) = torch.autograd.grad((wgrad_forward(c, d, W, swap, tap_shift) * up).sum(), (W,))
        return {"dw": (dW * sw, wgrad_den(c, d) * sw)}
    v = d["v"].double().requires_grad_(True)
    g = d["wg"].double().requires_grad_(True)
    gg = g
    if wrong_g_row is not None:
        idx = torch.arange(c.cout)
        idx[wrong_g_row] = wrong_g_row + 1
        gg = g[idx]
    b = d["bias"].double().requires_grad_(True)
    out = wgrad_forward(c, d, _weight_norm(v, gg), swap, tap_shift) + b.view(1, -1, 1, 1)
    dv, dg, db = torch.autograd.grad((out * up).sum(), (v, g, b))
    dWden = wgrad_den(c, d)
    vd, gd_ = v.detach(), gg.detach()
    n = vd.norm(dim=1)
    dotden = (dWden * vd.abs()).sum(1)
    return {"dv": (dv * sw, (gd_.abs() / n).view(-1, 1) * (dWden + (dotden / (n * n)).view(-1, 1) * vd.abs()) * sw),
            "dg": (dg * sw, dotden / n * sw),
            "db": (db * sb, (d["G"][:, :c.cout].double() * d["gv"].double().view(B, 1, 1, 1)).abs().sum((0, 2, 3)) * sb)}


def wgrad_den(c, d):
    """sum |gv G X| of every raw element [cout][fan], in values (no record scale)."""
    Gs, Xt = wgrad_operands(c, d)
    Ga = (Gs * d["gv"].double().view(c.B, 1, 1, 1)).abs().permute(1, 0, 2, 3).reshape(c.cout, -1)
    Xa = Xt.abs().permute(0, 2, 1, 3, 4).reshape(Xt.shape[0], c.K, -1)
    return _gather(c, torch.einsum("cp,tkp->ctk", Ga, Xa)) / (ASCALE * ASCALE)


def wgrad_emulate(c, d):
    """The outputs as the two kernels compute them (wgrad_emulate_slab, then the finishing kernel in double, stored as fp32)."""
    tot, btot = wgrad_emulate_slab(c, d)
    dW = (_gather(c, tot) * float(np.float32(WG_INV_W))).float().double()
    if not c.wn:
        return {"dw": dW}
    v, g = d["v"].double(), d["wg"].double()
    dot, nn = (dW * v).sum(1), (v * v).sum(1)
    n = torch.sqrt(nn)
    return {"dv": ((g / n).view(-1, 1) * (dW - (dot / nn).view(-1, 1) * v)).float().double(), "dg": (dot / n).float().double(),
            "db": (btot * float(np.float32(WG_INV_B))).float().double()}


WG_KEYS = {"dw": "wgrad", "dv": "wgrad_wn_v", "dg": "wgrad_wn_g", "db": "wgrad_bias"}


# =================================================================================================================================
# critic threshold ops (record units: a stored value is 16 x the activation)

ThrCase = collections.namedtuple("ThrCase", "name B G h w resG mG")
CLIP_CASES = (ThrCase("clip_2x1x3x5", 2, 1, 3, 5, 0, 0), ThrCase("clip_3x4x8x9", 3, 4, 8, 9, 0, 0))
DOT_CASES = (ThrCase("dot_2x2x3x5", 2, 2, 3, 5, 0, 0), ThrCase("dot_res_3x4x7x9", 3, 4, 7, 9, 4, 4), ThrCase("dot_resG_2x4x17x16", 2, 4, 17, 16, 2, 3))
FC_CASES = (ThrCase("fc_2x1x2", 2, 64, 1, 2, 0, 0), ThrCase("fc_3x3x2", 3, 64, 3, 2, 0, 0))
FIN_CASES = (ThrCase("fin_B1", 1, 0, 0, 0, 0, 0), ThrCase("fin_B5", 5, 0, 0, 0, 0, 0))
THR = 0.3125 * ASCALE       # record units, representable


@functools.lru_cache(maxsize=None)
def clip_inputs(name):
    c, g = {x.name: x for x in CLIP_CASES + FC_CASES}[name], _gen(name)
    act = q(torch.relu(_randn(g, c.B, 8 * c.G, c.h, c.w)) * 0.5)
    act.view(-1)[::7] = THR / ASCALE                       # exactly at the threshold: clipped
    act.view(-1)[3::11] = float(np.nextafter(np.float32(THR / ASCALE), np.float32(1)))     # its fp32 neighbour above: the lo half holds the difference, not clipped
    act.view(-1)[5::13] = THR / ASCALE + 2.0 ** -12        # the record's next value above: not clipped
    d = {"act": q(act)}
    if name.startswith("fc"):
        d["gv"] = torch.tensor([0.5, -0.75, 0.0][:c.B])
        d["fc_w"] = _signed(g, 512).float()
    return d


def clip_restate(d):
    """The mask's interior records: hi = 16 where the stored value does not exceed THR."""
    st = interior_records(d["act"])
    stored = st[..., :8].float() + st[..., 8:].float()
    out = torch.zeros_like(st)
    out[..., :8] = torch.where(stored > THR, 0.0, ASCALE).half()
    return out


def fc_reference(c, d):
    stored = d["act"].double() * ASCALE
    gv = d["gv"].double().view(-1, 1)
    hw = c.h * c.w
    pooled = (gv * stored.sum((2, 3))).sum(0) / hw / ASCALE
    pden = (gv.abs() * stored.abs().sum((2, 3))).sum(0) / hw / ASCALE
    cnt = (stored <= THR).double().sum((2, 3))
    a20 = (gv * cnt).sum(0) / hw * d["fc_w"].double()
    aden = (gv.abs() * cnt).sum(0) / hw * d["fc_w"].double().abs()
    return {"grad_fcw": (pooled, pden), "a20": (a20, aden)}


@functools.lru_cache(maxsize=None)
def dot_inputs(name):
    c, g = {x.name: x for x in DOT_CASES}[name], _gen(name)
    d = {"g": q(_signed(g, c.B, 8 * c.G, c.h, c.w)), "wm": q(_signed(g, c.B, 8 * c.G, c.h, c.w))}
    if c.resG:
        d["res"] = q(_signed(g, c.B, 8 * c.resG, c.h, c.w))
        d["m"] = q((torch.rand(c.B, 8 * c.mG, c.h, c.w, generator=g) < 0.4).float())
    return d


def dot_reference(c, d):
    t = (d["g"].double() * d["wm"].double()).flatten(1) * ASCALE * ASCALE
    ref, den = t.sum(1), t.abs().sum(1)
    if c.resG:
        r = (d["res"].double() * d["m"][:, :8 * c.resG].double()).flatten(1) * ASCALE * ASCALE
        ref, den = ref + r.sum(1), den + r.abs().sum(1)
    return ref, den


FIN_INV = 1.0 / 512


@functools.lru_cache(maxsize=None)
def fin_inputs(name):
    c, g = {x.name: x for x in FIN_CASES}[name], _gen(name)
    src = list(range(21))
    perm = torch.randperm(21, generator=g).tolist()
    src = [(-1 if i in (3, 11, 20) else perm[i]) for i in range(21)]
    return {"alpha_src": src, "dots": _signed(g, 21, c.B).double() * 100, "a20": _signed(g, 512).double(),
            "gv": torch.tensor([0.5, -0.75, 0.0, 1.25, 2.0][:c.B])}


def fin_reference(c, d):
    """{grad index: (ref, den)}; indices no alpha_src names stay untouched."""
    out = {}
    gv = d["gv"].double()
    for t, sidx in enumerate(d["alpha_src"]):
        if sidx >= 0:
            out[sidx] = (float((d["dots"][t] * gv).sum() * FIN_INV), float((d["dots"][t] * gv).abs().sum() * FIN_INV))
    out[21] = (float(d["a20"].sum()), float(d["a20"].abs().sum()))
    out[22] = (float(gv.sum()), float(gv.abs().sum()))
    return out


# =================================================================================================================================
# actor heads

HeadCase = collections.namedtuple("HeadCase", "name B h w n_det spi")
HEAD_CASES = (HeadCase("head_B2_10", 2, 1, 2, 10, 0), HeadCase("head_B5_15", 5, 2, 2, 15, 0), HeadCase("head_B2_15_spi", 2, 2, 1, 15, 1),
              HeadCase("head_B5_10_spi", 5, 1, 2, 10, 1))
HEAD_BY_NAME = {c.name: c for c in HEAD_CASES}


def head_sizes(c):
    n1 = 64 if c.spi else c.n_det
    sizes = [("sm_w", (2, 512)), ("sm_b", (2,)), ("d_w", (n1, 512)), ("d_b", (n1,))]
    if c.spi:
        sizes += [("d2_w", (c.n_det, 64)), ("d2_b", (c.n_det,))]
    return sizes


@functools.lru_cache(maxsize=None)
def head_inputs(name):
    """feat [B][512][h][w]; the head tensors (fp32); gp [B][2], gd [B][n_det].  SPI: no hidden unit within 0.05 of the ReLU's zero, units
    0..3 clearly negative."""
    c, g = HEAD_BY_NAME[name], _gen(name)
    d = {"feat": q(torch.relu(_randn(g, c.B, 512, c.h, c.w)))}
    for k, shp in head_sizes(c):
        d[k] = (_signed(g, *shp) * (1.0 if len(shp) == 1 else 2.0 / math.sqrt(shp[1]))).float()
    d["gp"] = torch.stack([_signed(g, c.B), _signed(g, c.B) + 2.5], 1).float()
    d["gd"] = _signed(g, c.B, c.n_det).float()
    if c.spi:
        f = d["feat"].double().mean((2, 3))
        d["d_b"][:4] = -20.0
        for _ in range(40):
            pre = f @ d["d_w"].double().t() + d["d_b"].double()
            near = (pre.abs() < 0.05).any(0)
            if not bool(near.any()):
                break
            d["d_b"][near] += 0.13
        else:
            raise AssertionError(name + ": a hidden unit stays near the kink")
    return d


def head_params(c, d):
    return torch.cat([d[k].reshape(-1) for k, _ in head_sizes(c)])


def _head_forward(c, d, t, f):
    logits = f @ t["sm_w"].t() + t["sm_b"]
    p = torch.softmax(logits, 1)
    if c.spi:
        hid = torch.relu(f @ t["d_w"].t() + t["d_b"])
        det = torch.sigmoid(hid @ t["d2_w"].t() + t["d2_b"])
    else:
        hid = None
        det = torch.sigmoid(f @ t["d_w"].t() + t["d_b"])
    return p, det, hid


def head_reference(c, d):
    """{"gf": (ref, den), "grad": (ref, den)} by autograd in float64; grad in the layout of head_params."""
    t = {k: d[k].double().requires_grad_(True) for k, _ in head_sizes(c)}
    f = d["feat"].double().mean((2, 3)).requires_grad_(True)
    p, det, hid = _head_forward(c, d, t, f)
    gp, gd = d["gp"].double(), d["gd"].double()
    grads = torch.autograd.grad((p * gp).sum() + (det * gd).sum(), [f] + [t[k] for k, _ in head_sizes(c)])
    # denominators: the magnitudes of the terms each gradient is added up from
    with torch.no_grad():
        fa = d["feat"].double().abs().mean((2, 3))
        gl_den = p * (gp.abs() + (gp.abs() * p).sum(1, keepdim=True))
        gdet = gd * det * (1 - det)
        W = {k: t[k].detach() for k in t}
        if c.spi:
            g1_den = (hid > 0).double() * (gdet.abs() @ W["d2_w"].abs())
            hid_den = (hid > 0).double() * (fa @ W["d_w"].abs().t() + W["d_b"].abs())
        else:
            g1_den = gdet.abs()
        gf_den = gl_den @ W["sm_w"].abs() + g1_den @ W["d_w"].abs()
        dens = [gl_den.t() @ fa, gl_den.sum(0), g1_den.t() @ fa, g1_den.sum(0)]
        if c.spi:
            dens += [gdet.abs().t() @ hid_den, gdet.abs().sum(0)]
    return {"gf": (grads[0], gf_den), "grad": (torch.cat([x.reshape(-1) for x in grads[1:]]), torch.cat([x.reshape(-1) for x in dens]))}


def _fma_dot(w, x):
    """fp32 fma chain s = fma(w[..., k], x[..., k], s) over the last axis, k ascending (double holds each product + sum exactly enough:
    one rounding to fp32 per step)."""
    s = torch.zeros(torch.broadcast_shapes(w.shape[:-1], x.shape[:-1]), dtype=torch.float64)
    wd, xd = w.double(), x.double()
    for k in range(w.shape[-1]):
        s = (s + wd[..., k] * xd[..., k]).float().double()
    return s.float()


def head_emulate(c, d):
    """pol_head_grad_kernel and pol_head_param_grad_kernel in fp32, in their order."""
    B, n_det = c.B, c.n_det
    stored = (d["feat"] * ASCALE).float().flatten(2)            # [B][512][h w], exact
    s = torch.zeros(B, 512)
    for i in range(stored.shape[2]):
        s = s + stored[:, :, i]
    f = s * (np.float32(1.0) / (np.float32(c.h * c.w) * np.float32(ASCALE)))
    dot = lambda Wm: _fma_dot(Wm.unsqueeze(0), f.unsqueeze(1))                  # [B][rows]
    logit = dot(d["sm_w"]) + d["sm_b"]
    m = logit.max(1, keepdim=True).values
    e = torch.exp(logit - m)
    p = e / e.sum(1, keepdim=True)
    gp = d["gp"]
    dotp = gp[:, 0] * p[:, 0] + gp[:, 1] * p[:, 1]
    gl = p * (gp - dotp.unsqueeze(1))
    if c.spi:
        hid = torch.relu(dot(d["d_w"]) + d["d_b"])
        pre = torch.zeros(B, n_det)
        acc = d["d2_b"].double().unsqueeze(0).repeat(B, 1)
        for k in range(64):
            acc = (acc + d["d2_w"][:, k].double().unsqueeze(0) * hid[:, k].double().unsqueeze(1)).float().double()
        pre = acc.float()
    else:
        hid = torch.zeros(B, 64)
        pre = dot(d["d_w"]) + d["d_b"]
    dd = 1.0 / (1.0 + torch.exp(-pre))
    gdet = d["gd"] * (dd * (1.0 - dd))
    if c.spi:
        g1 = torch.where(hid > 0, _fma_dot(gdet.unsqueeze(1), d["d2_w"].t().unsqueeze(0)), torch.zeros(()))
    else:
        g1 = gdet
    acc = (gl[:, 1:2].double() * d["sm_w"][1].double() + (gl[:, 0:1] * d["sm_w"][0]).double()).float().double()
    for r in range(g1.shape[1]):
        acc = (acc + g1[:, r:r + 1].double() * d["d_w"][r].double()).float().double()
    gf = acc
    outs = [gl.double().t() @ f.double(), gl.double().sum(0), g1.double().t() @ f.double(), g1.double().sum(0)]
    if c.spi:
        outs += [gdet.double().t() @ hid.double(), gdet.double().sum(0)]
    return {"gf": gf, "grad": torch.cat([x.reshape(-1) for x in outs]).float().double()}


SeedCase = collections.namedtuple("SeedCase", "name B h w boost kind")
SEED_CASES = (SeedCase("seed_pow2", 2, 1, 2, 1.0, "pow2"), SeedCase("seed_below_one", 3, 3, 2, 1.0, "below_one"),
              SeedCase("seed_zero", 2, 1, 2, 1.0, "zero"), SeedCase("seed_boost", 2, 3, 2, 16.0, "random"),
              SeedCase("seed_f16_ties", 2, 3, 2, 1.0, "ties"))
SEED_TIES = 128
SEED_BY_NAME = {c.name: c for c in SEED_CASES}


@functools.lru_cache(maxsize=None)
def seed_inputs(name):
    c, g = SEED_BY_NAME[name], _gen(name)
    gf = (_signed(g, c.B, 512) * 0.2).float()
    if c.kind == "pow2":
        gf[1, 77] = -0.25
    elif c.kind == "below_one":
        gf[2, 5] = float(np.nextafter(np.float32(1), np.float32(0)))
    elif c.kind == "zero":
        gf.zero_()
    elif c.kind == "ties":
        # h w = 6: the factor 16 / 6 is no power of two, so (g_f s) k16 is a ROUNDED product.  Elements 0 .. SEED_TIES - 1 of image 0 are chosen
        # so that this fp32 product is exactly an f16 tie T = (2 m + 1) 2^-11 while the unrounded product lies beside it: a kernel that
        # took hi from the one and lo from the other would store a record one hi-ulp (2^-11 relative) off where the two round apart.
        gf[1, 500] = 0.75                                        # the maximum: s = 1
        k16 = np.float32(ASCALE) / np.float32(c.h * c.w)
        m = torch.randint(1024, 2048, (8 * SEED_TIES,), generator=g).numpy()
        T = ((2 * m + 1) * 2.0 ** -11).astype(np.float32)
        v = (T / k16).astype(np.float32)
        ok = ((v * k16).astype(np.float32) == T) & (v.astype(np.float64) * np.float64(k16) != T.astype(np.float64))
        v = v[ok][:SEED_TIES]
        assert v.size == SEED_TIES, name
        gf[0, :SEED_TIES] = torch.from_numpy(v * np.where(np.arange(SEED_TIES) % 2, -1, 1).astype(np.float32))
    return {"gf": gf}


def seed_restate(c, d):
    """(slot [2] fp32, gv [B] fp32, ga values fp32 [B][512][h][w] BEFORE the records) exactly as the kernels compute them."""
    m = float(d["gf"].abs().max())
    if m > 0:
        e = max(math.frexp(m)[1], -126)
        s, inv = math.ldexp(1.0, -e), math.ldexp(1.0, e)
    else:
        s = inv = 0.0
    k16 = np.float32(c.boost) * np.float32(ASCALE) / np.float32(c.h * c.w)
    ga16 = (d["gf"] * np.float32(s)) * k16
    return (torch.tensor([s, inv], dtype=torch.float32), torch.full((c.B,), np.float32(inv) * np.float32(1.0 / c.boost), dtype=torch.float32),
            (ga16 / ASCALE).view(c.B, 512, 1, 1).expand(c.B, 512, c.h, c.w).contiguous())


def half_of_double(p):
    """float64 -> f16 in ONE rounding (through fp32 the value would be rounded twice): the nearest of the fp32 route's result and its two
    f16 neighbours."""
    h = p.float().half().contiguous()
    bits = h.view(torch.int16)
    cands = torch.stack([(bits + k).view(torch.float16) for k in (-1, 0, 1)])
    best = (cands.double() - p.unsqueeze(0)).abs().argmin(0, keepdim=True)
    return cands.gather(0, best).squeeze(0)


def seed_fused_pack(c, d):
    """The mutant of seed_restate's tensor: hi = f16 of the fp32 product, lo = f16(p - f16(p)) of the UNROUNDED product p (a multiply
    fused into both conversions of the pack separately).  float64 values [B][512][h][w]."""
    s = float(seed_restate(c, d)[0][0])
    k16 = np.float32(c.boost) * np.float32(ASCALE) / np.float32(c.h * c.w)
    p = (d["gf"] * np.float32(s)).double() * float(k16)
    hi = p.float().half()
    lo = (p - half_of_double(p).double()).half()
    return ((hi.double() + lo.double()) / ASCALE).view(c.B, 512, 1, 1).expand(c.B, 512, c.h, c.w)


def seed_reference(c, d):
    s = float(seed_restate(c, d)[0][0])
    ref = (d["gf"].double() * s * c.boost / (c.h * c.w)).view(c.B, 512, 1, 1).expand(c.B, 512, c.h, c.w)
    return ref, ref.abs()


# =================================================================================================================================
# the derived bars and the profile note

def _worse(a, b):
    return a if a[0] >= b[0] else b


@functools.lru_cache(maxsize=None)
def emulation_maxima():
    """{key: (largest measure of the fp32 emulation over the class's cases, case)}; keys: DERIVED_KEYS."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = {k: (-1.0, "") for k in DERIVED_KEYS}
        for c in APPLY_CASES:
            d = apply_inputs(c.name)
            ref, den = apply_reference(c, d)["out"]
            out["bn_apply"] = _worse(out["bn_apply"], (measure(apply_reference(c, d, emulate=True), ref, den), c.name))
        for c in BWD_CASES:
            d = bwd_inputs(c.name)
            ref, emu = bwd_reference(c, d), bwd_emulate(c, d)
            for k, y in emu.items():
                ok = ref[k][0].abs() < 0.99 * RANGE_LIMIT
                out["bn_bwd_dz"] = _worse(out["bn_bwd_dz"], (measure(y[ok], ref[k][0][ok], ref[k][1][ok]), c.name))
        for c in WGRAD_CASES:
            d = wgrad_inputs(c.name)
            ref, emu = wgrad_reference(c, d), wgrad_emulate(c, d)
            for k, y in emu.items():
                out[WG_KEYS[k]] = _worse(out[WG_KEYS[k]], (measure(y, *ref[k]), c.name))
        for c in HEAD_CASES:
            d = head_inputs(c.name)
            ref, emu = head_reference(c, d), head_emulate(c, d)
            out["head_gf"] = _worse(out["head_gf"], (measure(emu["gf"], *ref["gf"]), c.name))
            out["head_param"] = _worse(out["head_param"], (measure(emu["grad"], *ref["grad"]), c.name))
        for c in SEED_CASES:
            d = seed_inputs(c.name)
            out["grad_seed"] = _worse(out["grad_seed"], (measure(q(seed_restate(c, d)[2]), *seed_reference(c, d)), c.name))
        return out
    finally:
        torch.set_num_threads(threads)


def recorded_bars():
    """{key: (emulation maximum, bar)} as profiles/net_train_probe.md records them (table rows `| key | max | bar | ...`)."""
    out = {}
    for line in open(PROFILE_NOTE):
        m = re.match(r"\|\s*(%s)\s*\|\s*([0-9.eE+-]+)\s*\|\s*([0-9.eE+-]+)\s*\|" % "|".join(DERIVED_KEYS), line)
        if m:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    assert set(out) == set(DERIVED_KEYS), f"{PROFILE_NOTE}: bars of {sorted(set(DERIVED_KEYS) - set(out))} missing"
    return out


def bar(key):
    if key in FIXED_BARS:
        return fixed_bar(key)
    return recorded_bars()[key][1]
