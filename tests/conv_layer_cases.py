"""Cases, inputs, float64 references and fp32 emulations of the per-layer convolution probe (pnpx_conv3x3_probe, csrc/conv_probe.hip).

One CASE is one layer geometry with its operands; every probe kind whose launcher accepts the geometry runs it (tests/
test_gpu_conv_layers.py).  References are float64 torch on the CPU, computed from the very fp32 inputs.  The error measure is per element:

    max |y - ref| / (conv2d(|in|, |w|) + |bias| + |res|)        (adjoint kinds: conv_transpose2d(|g|, |w|))

i.e. the error of one output against the sum of the magnitudes of the terms it was added up from, so one wrong pixel is not averaged
away.  The bar of an algorithm class (direct, F(2x2), F(4x4)) is BAR_FACTOR x the largest value the class's fp32 CPU emulation reaches in
the same measure on the same cases (profiles/conv_layer_probe.md records them; tests/test_conv_layer_host.py re-derives them).  No GPU."""
import collections
import functools
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE_NOTE = os.path.join(ROOT, "profiles", "conv_layer_probe.md")
PADL = 4                  # csrc/common.h
BAR_FACTOR = 8.0          # an fp32 sum of 9 cin terms moves with the summation order, and the MFMA's order is not the emulation's
SLOPE = 0.2

# include/pnpx.h: enum pnpx_probe_kind
DIRECT, WINO4, WINO8, WINO8_KSPLIT, WINOF4, WINO8_UPS, DIRECT_GRAD, WINO8_GRAD = range(8)
KIND_NAMES = ("DIRECT", "WINO4", "WINO8", "WINO8_KSPLIT", "WINOF4", "WINO8_UPS", "DIRECT_GRAD", "WINO8_GRAD")
KIND_CLASS = ("direct", "f2", "f2", "f2", "f4", "f2", "direct", "f2")
CLASSES = ("direct", "f2", "f4")
FORWARD_KINDS = (DIRECT, WINO4, WINO8, WINO8_KSPLIT, WINOF4)
GRAD_KINDS = (DIRECT_GRAD, WINO8_GRAD)

# op "fwd": out = leaky(conv(cat(in0 [C0], in1 [C1]), w [cout][C0 + C1]) + bias) (+ res); "ups": in1 is low-resolution and up-sampled x2;
# "adj": out [cout] = conv_transpose(in0 [C0], w [C0][cout]) (x LeakyReLU'(mask) in the masked variant of the same case)
Case = collections.namedtuple("Case", "name op C0 C1 cout H W res pool")


def _c(op, C0, C1, cout, H, W, res=False, pool=False):
    name = f"{op}_{C0}" + (f"+{C1}" if C1 else "") + f"to{cout}_{H}x{W}" + ("_res" if res else "") + ("_pool" if pool else "")
    return Case(name, op, C0, C1, cout, H, W, res, pool)


# The smallest geometries at which each kernel can still go wrong: one region and several, W of one and of two 32-pixel regions plus a
# 16-pixel rest (48), channel counts of the two networks' layers; the wide layers at the small sizes (the reference is float64 on the CPU).
CASES = (
    # plain layers; 32-cout tile (W % 32)
    _c("fwd", 32, 0, 32, 16, 32), _c("fwd", 32, 0, 32, 32, 64), _c("fwd", 64, 0, 96, 16, 32),
    # 64-cout tile
    _c("fwd", 32, 0, 64, 16, 16), _c("fwd", 32, 0, 64, 32, 48), _c("fwd", 64, 0, 64, 16, 32), _c("fwd", 64, 0, 64, 32, 16),
    _c("fwd", 64, 0, 64, 32, 48, res=True), _c("fwd", 128, 0, 256, 16, 16), _c("fwd", 128, 0, 256, 32, 16), _c("fwd", 512, 0, 512, 16, 16),
    _c("fwd", 512, 0, 512, 16, 32), _c("fwd", 64, 0, 64, 32, 64),
    # F(4x4) extras: two chunks, an odd chunk count (no network has it), the fused pool
    _c("fwd", 16, 0, 64, 16, 32), _c("fwd", 24, 0, 64, 32, 64), _c("fwd", 64, 0, 64, 16, 32, pool=True), _c("fwd", 64, 0, 128, 32, 32, pool=True),
    # decoder entries (two sources)
    _c("fwd", 32, 64, 32, 16, 32), _c("fwd", 32, 64, 32, 32, 64), _c("fwd", 64, 128, 64, 16, 16), _c("fwd", 64, 128, 64, 32, 48),
    _c("fwd", 256, 512, 256, 16, 16), _c("fwd", 256, 512, 256, 32, 16),
    # K-split geometries (pieces: KSPLIT_PIECES)
    _c("fwd", 256, 0, 256, 16, 16), _c("fwd", 64, 0, 64, 16, 16), _c("fwd", 256, 0, 256, 32, 32), _c("fwd", 128, 256, 256, 16, 16),
    # fused up-sampling: the smallest accepted geometry of each tile and one size larger
    _c("ups", 48, 16, 64, 32, 16), _c("ups", 64, 128, 64, 32, 16), _c("ups", 64, 128, 64, 32, 32), _c("ups", 32, 64, 32, 32, 32),
    _c("ups", 32, 64, 32, 32, 64), _c("ups", 256, 512, 256, 32, 16),
    # adjoints: C0 = channels of the incoming gradient
    _c("adj", 64, 0, 32, 16, 32), _c("adj", 64, 0, 32, 32, 64), _c("adj", 32, 0, 96, 16, 32), _c("adj", 32, 0, 96, 32, 64),
    _c("adj", 512, 0, 256, 16, 16), _c("adj", 512, 0, 256, 32, 48), _c("adj", 256, 0, 768, 16, 32), _c("adj", 256, 0, 768, 32, 16),
)
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
B_MAX = 3
# K-split pieces of the cases that are in the table for the WINO8_KSPLIT kind's sake (every case: ksplit_pieces); the last one has a piece
# that straddles the boundary of its two sources (pieces of 6 chunks, the first source holds 8)
KSPLIT_PIECES = {"fwd_128to256_16x16": 2, "fwd_256to256_16x16": 4, "fwd_64to64_16x16": 1, "fwd_256to256_32x32": 2, "fwd_128+256to256_16x16": 4}
# geometries every Winograd kind must refuse: W = 48 on a 32-cout tile, H = 24, 12 input channels; F(4x4) with a second source
REFUSED = ((WINO4, 32, 0, 32, 16, 48), (WINO8, 32, 0, 32, 16, 48), (WINO8_GRAD, 64, 0, 32, 16, 48), (WINO8_UPS, 32, 64, 32, 32, 48),
           (WINO4, 64, 0, 64, 24, 32), (WINO8, 64, 0, 64, 24, 32), (WINO8_KSPLIT, 64, 0, 64, 24, 32), (WINOF4, 64, 0, 64, 24, 32),
           (WINO8_GRAD, 64, 0, 64, 24, 32), (WINO8_UPS, 64, 128, 64, 24, 32),
           (WINO4, 12, 0, 64, 16, 32), (WINO8, 12, 0, 64, 16, 32), (WINOF4, 12, 0, 64, 16, 32), (WINO8_GRAD, 12, 0, 64, 16, 32),
           (WINOF4, 32, 32, 64, 16, 32))


def kinds_of(case):
    """Probe kinds the case is meant for (whether a kind ACCEPTS it is the plan's word: pnpx_conv3x3_probe_plan)."""
    if case.op == "ups":
        return (WINO8_UPS,)
    if case.op == "adj":
        return GRAD_KINDS
    if case.res:
        return (DIRECT, WINO4, WINO8)
    if case.pool:
        return (WINO4, WINO8, WINOF4)
    return FORWARD_KINDS


def _wino_tile(C0, C1, cout, H, W, eight):
    if C0 <= 0 or H < 16 or H % 16:
        return 0
    if cout % 64 == 0:
        return 64 if C0 % 16 == 0 and C1 % 16 == 0 and W % 16 == 0 else 0
    if cout % 32 == 0:
        return 32 if C0 % 8 == 0 and C1 % 8 == 0 and W % 32 == 0 and (not eight or C0 + C1 >= 16) else 0
    return 0


def accepts(kind, c):
    """The cout tile the kind runs the geometry with, 0 = it refuses: a plain restatement of the launchers' predicates, so that the
    test table needs no library at collection time (tests/test_conv_layer_host.py holds it against pnpx_conv3x3_probe_plan)."""
    C0, C1, cout, H, W = c.C0, c.C1, c.cout, c.H, c.W
    if kind == DIRECT:
        mt, cc = (64 if cout >= 64 else 32), (8 if (C0 + C1) % 8 == 0 else 2)
        return mt if C0 % cc == 0 and C1 % cc == 0 and cout % mt == 0 and not (mt == 64 and cc != 8) else 0
    if kind == DIRECT_GRAD:
        return (64 if cout % 64 == 0 else 32) if C1 == 0 and C0 % 8 == 0 and cout % 32 == 0 else 0
    if kind == WINOF4:
        return 64 if C1 == 0 and C0 >= 16 and C0 % 8 == 0 and cout % 64 == 0 and H >= 16 and H % 16 == 0 and W >= 32 and W % 32 == 0 else 0
    if kind == WINO8_GRAD:
        return _wino_tile(C0, 0, cout, H, W, True) if C1 == 0 else 0
    ct = _wino_tile(C0, C1, cout, H, W, kind != WINO4)
    if kind == WINO8_UPS and ct:
        nr, nqp, chunks = (11, 12, C0 // 16 >= 3) if ct == 64 else (11, 20, C0 // 8 >= 4)
        ok = C1 > 0 and H % 2 == 0 and W % 2 == 0 and chunks and H // 2 + 1 >= nr and W // 2 + PADL >= nqp
        return ct if ok else 0
    return ct


def ksplit_pieces(c, rule=1):
    """conv3x3_wino8_ksplit restated: 4 pieces up to 8 tiles per image, 2 up to 16; <= 32 (tile, piece) slots; every piece >= 4 chunks."""
    if _wino_tile(c.C0, c.C1, c.cout, c.H, c.W, True) != 64:
        return 1
    t, nch = (c.H // 16) * (c.W // 16) * (c.cout // 64), (c.C0 + c.C1) // 16
    g = 4 if t <= 8 else (2 if t <= 16 else 1)
    while g > 1 and g * t > 32:
        g //= 2
    while g > 1 and (nch % g or nch // g < 4):
        g //= 2
    return g


def runs():
    """[(kind, case)] of the GPU suite: every kind on every case meant for it that it accepts."""
    return [(k, c) for c in CASES for k in kinds_of(c) if accepts(k, c)]


def plan(kind, case_or_geom, ks_rule=1):
    """(cout tile, K-split pieces) from the library's host-only plan; (0, 0) = refused."""
    from tfpnp_amd import _lib
    g = case_or_geom
    C0, C1, cout, H, W = (g.C0, g.C1, g.cout, g.H, g.W) if isinstance(g, Case) else g
    v = _lib.lib().pnpx_conv3x3_probe_plan(kind, C0, C1, cout, H, W, ks_rule)
    return (v & 255, v >> 8) if kind == WINO8_KSPLIT else (v, 1 if v else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

def _seed(case):
    return 9000 + 17 * CASES.index(case)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp32 operands of a case at B_MAX images (a B = 1 launch takes image 0): dict of torch tensors, never modified by the callers."""
    c = CASE_BY_NAME[name]
    rs = np.random.RandomState(_seed(c))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    cin = c.C0 + c.C1
    d = {}
    if c.op == "adj":
        d["w"] = t(rs.standard_normal((c.C0, c.cout, 3, 3)) / np.sqrt(9.0 * c.C0))
        d["in0"] = t(rs.standard_normal((B_MAX, c.C0, c.H, c.W)))
        # mask: magnitudes in [0.1, 1] (nothing near the kink), random signs, and a handful of exact +0.0 / -0.0 cells (factor = slope)
        m = rs.uniform(0.1, 1.0, (B_MAX, c.cout, c.H, c.W)) * rs.choice([-1.0, 1.0], (B_MAX, c.cout, c.H, c.W))
        m = m.astype(np.float32)
        flat = m.reshape(-1)
        idx = rs.choice(flat.size, 12, replace=False)
        flat[idx[:6]] = 0.0
        flat[idx[6:]] = -0.0
        flat[0] = 0.0               # image 0 holds both zeros whatever the draw
        flat[1] = -0.0
        d["mask"] = torch.from_numpy(m)
        d["zero_cells"] = torch.from_numpy(np.sort(np.concatenate([idx, [0, 1]])))
        return d
    d["w"] = t(rs.standard_normal((c.cout, cin, 3, 3)) / np.sqrt(9.0 * cin))
    d["bias"] = t(0.1 * rs.standard_normal(c.cout))
    d["in0"] = t(rs.standard_normal((B_MAX, c.C0, c.H, c.W)))
    if c.C1:
        hw = (c.H // 2, c.W // 2) if c.op == "ups" else (c.H, c.W)
        d["in1"] = t(rs.standard_normal((B_MAX, c.C1) + hw))
    if c.res:
        d["res"] = t(rs.standard_normal((B_MAX, c.cout, c.H, c.W)))
    return d


def pad(x):
    """[B][C][H][W] -> the denoiser's padded planar layout [B][C][H + 2][W + 2 PADL], zero border."""
    return F.pad(x, (PADL, PADL, 1, 1))


def interior(xp):
    return xp[..., 1:-1, PADL:-PADL]


def border_cells(xp):
    """Every cell of a padded tensor outside the interior, as one flat tensor."""
    return torch.cat([xp[..., 0, :].reshape(-1), xp[..., -1, :].reshape(-1), xp[..., :PADL].reshape(-1), xp[..., -PADL:].reshape(-1)])


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references and the error measure

def upsample64(low):
    return F.interpolate(low.double(), scale_factor=2, mode="bilinear", align_corners=True)


def source64(c, d):
    x = d["in0"].double()
    if c.C1:
        x = torch.cat([x, upsample64(d["in1"]) if c.op == "ups" else d["in1"].double()], 1)
    return x


def reference(c, d, masked=False, slope=SLOPE):
    """(ref, denom) in float64 of a case on the operands d (the measure's numerator reference and its denominator)."""
    w = d["w"].double()
    if c.op == "adj":
        ref = F.conv_transpose2d(d["in0"].double(), w, padding=1)
        den = F.conv_transpose2d(d["in0"].double().abs(), w.abs(), padding=1)
        if masked:
            ref = ref * torch.where(d["mask"] > 0, 1.0, slope).double()
        return ref, den
    x = source64(c, d)
    b = d["bias"].double().view(1, -1, 1, 1)
    ref = F.leaky_relu(F.conv2d(x, w, padding=1) + b, slope)
    den = F.conv2d(x.abs(), w.abs(), padding=1) + b.abs()
    if c.res:
        ref = ref + d["res"].double()
        den = den + d["res"].double().abs()
    return ref, den


@functools.lru_cache(maxsize=None)
def case_reference(name, masked=False):
    c = CASE_BY_NAME[name]
    return reference(c, inputs(name), masked)


def measure(y, ref, den):
    """The per-element error measure; NaN anywhere = inf."""
    e = (y.double() - ref).abs() / den
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the three algorithm classes

def upsample32(low, H, W):
    """The kernels' own bilinear x2 (align_corners) in fp32: f = s * index, i0 = (int) f, l = f - i0, h = 1 - l,
    v = hy (hx v00 + lx v01) + ly (hx v10 + lx v11)."""
    h, w = low.shape[-2:]
    def table(n_out, n_in):
        s = np.float32(n_in - 1) / np.float32(n_out - 1)
        f = (s * np.arange(n_out, dtype=np.float32)).astype(np.float32)
        i0 = f.astype(np.int64)
        l = (f - i0.astype(np.float32)).astype(np.float32)
        return torch.from_numpy(i0), torch.from_numpy(l), torch.from_numpy((np.float32(1) - l).astype(np.float32))
    y0, ly, hy = table(H, h)
    x0, lx, hx = table(W, w)
    lp = F.pad(low, (0, 1, 0, 1))                         # i0 + 1 beyond the image carries weight ~0 and reads the zero border
    r0, r1 = lp[..., y0, :], lp[..., y0 + 1, :]
    top = hx * r0[..., x0] + lx * r0[..., x0 + 1]
    bot = hx * r1[..., x0] + lx * r1[..., x0 + 1]
    return hy.view(-1, 1) * top + ly.view(-1, 1) * bot


def _wino_mats(cls):
    if cls == "f2":
        G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
        BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
        AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
        return G, BT, AT
    from tfpnp_amd import _lib
    g, bt, at = np.zeros((6, 3)), np.zeros((6, 6)), np.zeros((4, 6))
    _lib.lib().pnpx_winof4_matrices(g.ctypes.data, bt.ctypes.data, at.ctypes.data)
    return g, bt, at


def winograd32(x, w, cls):
    """conv2d(x, w, padding 1) by the transform-domain algorithm in fp32: U = G g G^T rounded once from fp64, V = B^T d B, one fp32
    matrix product over the channels per transform position, Y = A^T M A.  x fp32 [B][C][H][W] (H, W multiples of the output tile)."""
    G, BT, AT = _wino_mats(cls)
    m, a = AT.shape                                       # output tile, transform size
    G64, BT32, AT32 = torch.from_numpy(G), torch.from_numpy(BT).float(), torch.from_numpy(AT).float()
    U = (G64 @ w.double() @ G64.T).float()                # [K][C][a][a]
    B_, C, H, W = x.shape
    K = w.shape[0]
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, a, m).unfold(3, a, m)          # [B][C][ty][tx][a][a]
    V = BT32 @ d @ BT32.T
    ty, tx = V.shape[2], V.shape[3]
    Vp = V.permute(4, 5, 1, 0, 2, 3).reshape(a * a, C, B_ * ty * tx)
    Up = U.permute(2, 3, 0, 1).reshape(a * a, K, C)
    M = torch.bmm(Up, Vp).reshape(a, a, K, B_, ty, tx).permute(3, 2, 4, 5, 0, 1)      # [B][K][ty][tx][a][a]
    Y = AT32 @ M @ AT32.T                                 # [B][K][ty][tx][m][m]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B_, K, ty * m, tx * m)


def adjoint_weights(w):
    """w [C0][cout][3][3] of a forward layer -> the adjoint convolution's own conv2d weights [cout][C0][3][3] (transposed, taps flipped)."""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def emulate32(c, d, cls, masked=False, slope=SLOPE):
    """The case computed in fp32 on the CPU by the class's algorithm (direct: torch's own fp32 convolutions)."""
    if c.op == "adj":
        if cls == "direct":
            y = F.conv_transpose2d(d["in0"], d["w"], padding=1)
        else:
            y = winograd32(d["in0"], adjoint_weights(d["w"]), cls)
        return y * torch.where(d["mask"] > 0, 1.0, slope).float() if masked else y
    x = d["in0"]
    if c.C1:
        x = torch.cat([x, upsample32(d["in1"], c.H, c.W) if c.op == "ups" else d["in1"]], 1)
    lin = F.conv2d(x, d["w"], padding=1) if cls == "direct" else winograd32(x, d["w"], cls)
    y = F.leaky_relu(lin + d["bias"].view(1, -1, 1, 1), slope)
    return y + d["res"] if c.res else y


def class_runs(cls, c):
    """Does the class's emulation (and bar) cover the case: the direct kernels run everything but the fused up-sampling; F(2x2) everything;
    F(4x4) the plain single-source 64-cout layers with W % 32 == 0."""
    if cls == "direct":
        return c.op != "ups"
    if cls == "f4":
        return c.op == "fwd" and not c.C1 and not c.res and c.cout % 64 == 0 and c.W % 32 == 0 and c.H % 16 == 0
    return True


@functools.lru_cache(maxsize=None)
def emulation_maxima():
    """{class: (largest measure of its fp32 emulation over the case table, the case it was found at)}."""
    out = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)       # an fp32 sum must not move with the number of threads the host happens to have
    try:
        for cls in CLASSES:
            worst, where = 0.0, None
            for c in CASES:
                if not class_runs(cls, c):
                    continue
                for masked in ((False, True) if c.op == "adj" else (False,)):
                    ref, den = case_reference(c.name, masked)
                    e = measure(emulate32(c, inputs(c.name), cls, masked), ref, den)
                    if e > worst:
                        worst, where = e, c.name + ("_mask" if masked else "")
            out[cls] = (worst, where)
    finally:
        torch.set_num_threads(threads)
    return out


def recorded_bars():
    """{class: (emulation maximum, bar)} as profiles/conv_layer_probe.md records them (table rows `| class | max | bar | ...`)."""
    out = {}
    for line in open(PROFILE_NOTE):
        m = re.match(r"\|\s*(direct|f2|f4)\s*\|\s*([0-9.eE+-]+)\s*\|\s*([0-9.eE+-]+)\s*\|", line)
        if m:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    assert set(out) == set(CLASSES), f"{PROFILE_NOTE}: bars of {sorted(set(CLASSES) - set(out))} missing"
    return out


def bar(kind_or_class):
    cls = kind_or_class if isinstance(kind_or_class, str) else KIND_CLASS[kind_or_class]
    return recorded_bars()[cls][1]


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants of the reference: subtle errors the bar must catch (tests/test_conv_layer_host.py)

def mutants(c, d, masked):
    """[(name, mutated reference)]: one weight zeroed, one input element zeroed, one mask sign flipped (masked adjoints), the result
    shifted by one pixel in x inside one 16-wide tile."""
    rs = np.random.RandomState(_seed(c) + 1)
    out = []
    w2 = d["w"].clone()
    w2[rs.randint(w2.shape[0]), rs.randint(w2.shape[1]), rs.randint(3), rs.randint(3)] = 0.0
    out.append(("weight_zeroed", reference(c, dict(d, w=w2), masked)[0]))
    src = "in1" if c.C1 and rs.randint(2) else "in0"
    x2 = d[src].clone()
    x2[rs.randint(x2.shape[0]), rs.randint(x2.shape[1]), rs.randint(x2.shape[2]), rs.randint(x2.shape[3])] = 0.0
    out.append(("input_zeroed", reference(c, dict(d, **{src: x2}), masked)[0]))
    if masked:
        m2 = d["mask"].clone()
        flat = m2.view(-1)
        i = int(rs.randint(flat.numel()))
        while float(flat[i]) == 0.0:                      # a zero cell has no sign to flip in this sense
            i = (i + 1) % flat.numel()
        flat[i] = -flat[i]
        out.append(("mask_flipped", reference(c, dict(d, mask=m2), masked)[0]))
    ref = reference(c, d, masked)[0]
    sh = ref.clone()
    x0 = 16 * rs.randint(c.W // 16)
    b, y0 = rs.randint(ref.shape[0]), 16 * rs.randint(c.H // 16)
    sh[b, :, y0:y0 + 16, x0 + 1:x0 + 16] = ref[b, :, y0:y0 + 16, x0:x0 + 15]
    out.append(("tile_shifted", sh))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# impulse cases: exact up to the rounding of U

IMPULSE_SLOPE = 0.5        # a power of two: LeakyReLU of a dyadic number stays exact
IMPULSE_GEOMS = (          # (op, C0, C1, cout, H, W): every tile shape, one and several regions, all three chunk positions
    ("fwd", 32, 0, 32, 16, 32), ("fwd", 64, 0, 64, 16, 16), ("fwd", 64, 0, 64, 32, 48), ("fwd", 64, 0, 64, 32, 64), ("fwd", 256, 0, 256, 16, 16),
    ("fwd", 512, 0, 512, 16, 32), ("fwd", 32, 64, 32, 32, 64), ("fwd", 64, 128, 64, 32, 48), ("fwd", 128, 256, 256, 16, 16),
    ("ups", 64, 128, 64, 32, 32), ("ups", 32, 64, 32, 32, 64),
    ("adj", 64, 0, 32, 32, 64), ("adj", 32, 0, 96, 16, 32), ("adj", 512, 0, 256, 16, 16), ("adj", 256, 0, 768, 32, 16), ("adj", 64, 0, 64, 32, 48),
)
IMPULSE_CASES = tuple(_c(*g) for g in IMPULSE_GEOMS)


def impulse_weights(c):
    """Every w[k][c][t] a different dyadic number: +-(index + 1) 2^-22 (index < 2^24: exact in fp32), signs alternating."""
    shape = (c.C0, c.cout, 3, 3) if c.op == "adj" else (c.cout, c.C0 + c.C1, 3, 3)
    n = int(np.prod(shape))
    assert n < 1 << 24
    idx = np.arange(n, dtype=np.float64)
    w = (idx + 1) * 2.0 ** -22 * np.where(idx.astype(np.int64) % 2 == 0, 1.0, -1.0)
    return torch.from_numpy(w.astype(np.float32).reshape(shape))


def impulse_sites(c, chunk):
    """[(source, channel, y, x)], one per image.  Positions: x, y in {0, 1, 15, 16, 17, 31, 32, last} as far as the shape has them (the
    four corners, both sides of every tile and region boundary), each with one of the channels in turn; plus every channel at the four
    corners.  Channels: first and last of the first, a middle and the last chunk of `chunk` channels of each source; so also the last of
    in0 and the first of in1."""
    pos = lambda n: sorted({p for p in (0, 1, 15, 16, 17, 31, 32, n - 1) if p < n})
    chans = []
    for src, C in (("in0", c.C0), ("in1", c.C1)):
        if not C:
            continue
        if c.op == "ups" and src == "in1":
            continue                                      # the low-resolution source: impulse_planes
        nch = C // chunk
        for ch in sorted({0, nch // 2, nch - 1}):
            chans += [(src, ch * chunk), (src, ch * chunk + chunk - 1)]
    sites = []
    for i, (y, x) in enumerate((y, x) for y in pos(c.H) for x in pos(c.W)):
        sites.append(chans[i % len(chans)] + (y, x))
    for src, ch in chans:
        sites += [(src, ch, y, x) for y in (0, c.H - 1) for x in (0, c.W - 1)]
    return sites


def impulse_inputs(c, sites, planes=()):
    """Operands with one 1.0 per image at its site; `planes` (fused up-sampling): further images whose low-resolution in1 holds one
    channel of constant 1.0, which up-samples to exactly 1.0 everywhere, so the output is a sum of the channel's taps."""
    n = len(sites) + len(planes)
    d = {"w": impulse_weights(c), "in0": torch.zeros(n, c.C0, c.H, c.W)}
    if c.op != "adj":
        d["bias"] = torch.zeros(c.cout)
    if c.C1:
        hw = (c.H // 2, c.W // 2) if c.op == "ups" else (c.H, c.W)
        d["in1"] = torch.zeros((n, c.C1) + hw)
    for i, (src, ch, y, x) in enumerate(sites):
        d[src][i, ch, y, x] = 1.0
    for j, ch in enumerate(planes):
        d["in1"][len(sites) + j, ch] = 1.0
    return d


def impulse_planes(c):
    return (0, c.C1 // 2, c.C1 - 1) if c.op == "ups" else ()
