"""Cases, inputs, float64 references, fp32 restatements and emulations of the probe of the launches between the convolutions of the two
denoisers' forward passes and of the DRUNet VJP's own glue (pnpx_fwd_glue_probe, csrc/fwd_glue_probe.hip; launchers: csrc/fwd_glue.h;
kernels: csrc/unet.hip, csrc/conv_first.h, csrc/drunet_f32.hip, csrc/drunet.hip, csrc/hs_relayout.h).

References are float64 torch on the CPU, computed from the very fp32 inputs (half-split: from the decoded records).  Bars:

  exact ops (PREP_INPUT, MAXPOOL2, S2D, D2S, ADD, TAIL_OUT, TAIL_MASK, the image half of DRU_INPUT_GRAD): fp32 results are BIT-IDENTICAL
    to a torch restatement; half-split record copies (S2D, D2S) bit-identical records; half-split PREP_INPUT and ADD equal to hs8_encode
    of the fp32 restatement; half-split MAXPOOL2 equal DECODED values (re-encoding a decoded tie need not give the same pair of halves).
  CONV_FIRST, OUTC_RESIDUAL: per element |y - ref| / (sum |w f| + |b| (+ |x|)); bar = BAR_FACTOR x the largest value the fp32 CPU emulation
    of the kernel (its fma chain in its order; half-split: the HS8 rounding of the output, and of the inputs where the kernel reads
    records) reaches on the same cases.  The clamp is continuous (|clamp(a) - clamp(b)| <= |a - b|), so `out` takes the bar of `out_pre`.
  UPSAMPLE2X: per element |y - ref| / sum |w_y w_x v|.  Tier (a): ref = a float64 sum with the kernel's own fp32 weights (weight_table of
    tests/vjp_glue_cases.py: the clamp i1 = i0 + (i0 < n - 1) and l as the form computes it, ups_contracted), bar UPS_TIER_A =
    6 * 2^-24: hx v00, + lx v01, hy (.), + ly (.) are at most 5 roundings on the longest path (4 where the compiler fuses), each of a
    partial sum no larger than the denominator, plus one for second-order terms; half-split UPS_TIER_A_HS = 11 * 2^-24: the same plus
    the record's hi + lo split (22 significant bits: 4 * 2^-24) and lo's subnormal step.  Tier (b): ref = F.interpolate(align_corners=True)
    in float64; bar = BAR_FACTOR x the emulation's maximum.
  sigma sums: against the float64 sum, relative to sum |terms|, k * 2^-24 with k the summation depth (sigma_depth).
profiles/fwd_glue_probe.md records the emulation maxima and the bars; tests/test_fwd_glue_host.py re-derives them.  No GPU."""
import collections
import functools
import os
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_hs_cases import ASCALE, hs8_border, hs8_decode, hs8_encode, quantize, split  # noqa: F401  (re-exported to the tests)
from tests.conv_layer_cases import BAR_FACTOR, PADL, border_cells, interior, pad, upsample32  # noqa: F401
from tests.vjp_glue_cases import SIG_CHUNKS, bits_equal, measure, sigma_depth, weight_table  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE_NOTE = os.path.join(ROOT, "profiles", "fwd_glue_probe.md")
U = 2.0 ** -24
UPS_TIER_A = 6 * U
UPS_TIER_A_HS = 11 * U
B_MAX = 3
GRID_Z_MAX = 65535         # csrc/fwd_glue.h: FG_GRID_Z_MAX

# include/pnpx.h: enum pnpx_fwd_glue_op; the form ids of pnpx_fwd_glue_probe_desc
PREP_INPUT, CONV_FIRST, MAXPOOL2, UPSAMPLE2X, OUTC_RESIDUAL, S2D, D2S, ADD, TAIL_OUT, TAIL_MASK, DRU_INPUT_GRAD = range(11)
OP_NAMES = ("PREP_INPUT", "CONV_FIRST", "MAXPOOL2", "UPSAMPLE2X", "OUTC_RESIDUAL", "S2D", "D2S", "ADD", "TAIL_OUT", "TAIL_MASK", "DRU_INPUT_GRAD")
F32_ONLY = (TAIL_OUT, DRU_INPUT_GRAD)
UPS_SCALAR, UPS_V4 = 1, 2          # family 0
UPS_HS32, UPS_HS64 = 1, 2          # family 1
UPS_FORM_NAMES = ({0: "auto", 1: "scalar", 2: "v4"}, {0: "auto", 1: "hs32", 2: "hs64"})


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _signed(g, *shape):
    """Magnitudes in [0.1, 1], random signs: no window is all-positive."""
    return (0.1 + 0.9 * torch.rand(*shape, generator=g)) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def decoded(x):
    """What a half-split kernel reads back from hs8_encode(x), as fp32 (exact: hi + lo has at most 22 significant bits)."""
    return quantize(x, torch.float32)


def _next(v, towards):
    return float(np.nextafter(np.float32(v), np.float32(towards)))


# cells at the ends of a clamp / an inclusive mask: inside ... and their outward neighbours
EDGES_IN = (0.0, -0.0, 1.0)
EDGES_OUT = (_next(0, -1), _next(1, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# the launchers' host-only form decisions, restated (tests/test_fwd_glue_host.py holds them against pnpx_fwd_glue_probe_plan)

def ups_form(family, planes, w):
    if family:
        return UPS_HS64 if 2 * w > 32 else UPS_HS32
    return UPS_V4 if (2 * w) % 4 == 0 and planes <= GRID_Z_MAX else UPS_SCALAR


def ups_forms_admitted(family, planes, w):
    if family:
        return (UPS_HS32, UPS_HS64)
    return (UPS_SCALAR, UPS_V4) if (2 * w) % 4 == 0 and planes <= GRID_Z_MAX else (UPS_SCALAR,)


def ups_hs_launches(B, G):
    per = GRID_Z_MAX // G
    return 0 if per == 0 else (B + per - 1) // per


def plan_restated(op, family, form=0, B=1, C=0, H=1, W=1, Ht=0, Wt=0, sigma_stride=0, k=0, slope=0.0):
    """(form, launches) of pnpx_fwd_glue_probe_plan in plain Python; (0, 0) = refused."""
    no = (0, 0)
    if family not in (0, 1) or not 0 <= op <= DRU_INPUT_GRAD or (family == 1 and op in F32_ONLY):
        return no
    image_op = op in (PREP_INPUT, TAIL_MASK)
    if op != UPSAMPLE2X and (Ht or Wt):
        return no
    if op not in (PREP_INPUT, CONV_FIRST) and sigma_stride:
        return no
    if not (op == CONV_FIRST and family == 1) and k:
        return no
    if op != CONV_FIRST and slope:
        return no
    if image_op and C:
        return no
    if B <= 0 or H <= 0 or W <= 0 or form < 0 or sigma_stride < 0 or (not image_op and C <= 0) or H * W > 0x7fffffff:
        return no
    if family == 1 and not image_op and C % 8:
        return no
    grid_yz = family == 0 and (B > GRID_Z_MAX or H > GRID_Z_MAX)
    if op == PREP_INPUT and grid_yz:
        return no
    if op == CONV_FIRST and (C not in (32, 64) or B > GRID_Z_MAX or (family == 0 and W % 4) or not 0 <= k <= 24):
        return no
    if op == MAXPOOL2 and (H < 2 or W < 2):
        return no
    if op in (OUTC_RESIDUAL, TAIL_OUT) and (C != 32 or grid_yz):
        return no
    if op == S2D and (H % 2 or W % 2):
        return no
    if op == DRU_INPUT_GRAD and (C < 2 or B > GRID_Z_MAX):
        return no
    if op != UPSAMPLE2X:
        return (1, 1) if form in (0, 1) else no
    if not (2 * H <= Ht <= 2 * H + 1 and 2 * W <= Wt <= 2 * W + 1):
        return no
    planes = B * (C // 8 if family else C)
    f = form or ups_form(family, planes, W)
    if f not in ups_forms_admitted(family, planes, W):
        return no
    n = ups_hs_launches(B, C // 8) if family else 1
    return (f, n) if n else no


def plan(op, family, form=0, **kw):
    """pnpx_fwd_glue_probe_plan: (form, launches), (0, 0) = refused."""
    from tfpnp_amd import _lib
    import ctypes
    d = _lib.FwdGlueProbeDesc(op=op, family=family, form=form, **kw)
    v = _lib.lib().pnpx_fwd_glue_probe_plan(ctypes.byref(d))
    return (v & 255, (v >> 8) + 1) if v else (0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# images: PREP_INPUT, CONV_FIRST, OUTC_RESIDUAL, TAIL_OUT, TAIL_MASK

# 1 x 1; odd sizes; 70 columns cross the 64-wide block in x of the row-per-block kernels; 50 x 39 = 1950 pixels: several 256-thread blocks
# and a partial one; 33 x 36: 297 quads (more than one block) of the fp32 first convolution, which needs W % 4 == 0
IMAGE_SHAPES = ((1, 1, 1), (2, 5, 7), (3, 16, 70), (2, 50, 39), (3, 33, 36))
QUAD_SHAPES = ((1, 1, 4), (2, 5, 8), (3, 33, 36), (3, 16, 72))       # fp32 first convolution: one quad, two per row, 297 and 288 quads

PrepCase = collections.namedtuple("PrepCase", "name B H W sigma_stride")
PREP_CASES = tuple(PrepCase(f"prep_{B}x{H}x{W}_s{ss}", B, H, W, ss) for B, H, W in IMAGE_SHAPES for ss in (1, 3)) + (PrepCase("prep_2x5x7_s0", 2, 5, 7, 0),)
PREP_BY_NAME = {c.name: c for c in PREP_CASES}


def sigma_vector(g, B, stride):
    """[1 + (B - 1) stride] fp32: signed levels at the read positions, a marker value elsewhere (stride 0: one zero, what the DRUNet seed
    passes)."""
    if stride == 0:
        return torch.zeros(1)
    s = torch.full((1 + (B - 1) * stride,), 777.0)
    s[::stride] = _signed(g, B) * 0.5
    return s


@functools.lru_cache(maxsize=None)
def prep_inputs(name):
    c = PREP_BY_NAME[name]
    g = _gen(name)
    x = _signed(g, c.B, c.H, c.W)
    x.view(-1)[0] = -0.0
    return {"x": x, "sigma": sigma_vector(g, c.B, c.sigma_stride)}


def sigma_of(d, B, stride):
    return d["sigma"][torch.arange(B) * stride]


def prep_restate(c, d, sigma_in_border=False):
    """[B][2][H + 2][W + 8] fp32, the whole padded tensor: channel 0 = x, channel 1 = sigma inside the image, a zero border.
    sigma_in_border: the mutant that fills the noise map's whole plane."""
    s = sigma_of(d, c.B, c.sigma_stride).view(c.B, 1, 1, 1).expand(c.B, 1, c.H, c.W)
    out = pad(torch.cat([d["x"].unsqueeze(1), s], 1))
    if sigma_in_border:
        out[:, 1] = sigma_of(d, c.B, c.sigma_stride).view(c.B, 1, 1)
    return out.contiguous()


def prep_restate_hs(c, d, prefill, sigma_in_border=False):
    """The records [B][2][H + 2][W + 2][16] after the launch on `prefill`: the interior of group 0 = hs8_encode of (x, sigma, 0 x 6);
    its border and group 1 keep what the test put there.  sigma_in_border: the mutant that writes the noise map's border too."""
    v = torch.zeros(c.B, 8, c.H, c.W)
    v[:, 0] = d["x"]
    v[:, 1] = sigma_of(d, c.B, c.sigma_stride).view(c.B, 1, 1)
    out = prefill.clone()
    out[:, 0, 1:-1, 1:-1] = hs8_encode(v)[:, 0, 1:-1, 1:-1]
    if sigma_in_border:
        hi, lo = split(sigma_of(d, c.B, c.sigma_stride) * ASCALE)
        m = ~_interior_mask(c.H, c.W)
        out[:, 0, :, :, 1] = torch.where(m, hi.view(c.B, 1, 1), out[:, 0, :, :, 1])
        out[:, 0, :, :, 9] = torch.where(m, lo.view(c.B, 1, 1), out[:, 0, :, :, 9])
    return out


def _interior_mask(H, W):
    m = torch.zeros(H + 2, W + 2, dtype=torch.bool)
    m[1:-1, 1:-1] = True
    return m


FirstCase = collections.namedtuple("FirstCase", "name family B H W cout slope k sigma_stride")


def _first_cases():
    out = []
    for fam, shapes in ((0, QUAD_SHAPES), (1, IMAGE_SHAPES)):
        for B, H, W in shapes:
            out.append(FirstCase(f"first_{'hs' if fam else 'f32'}_{B}x{H}x{W}_c32", fam, B, H, W, 32, 0.2, 0, 1))
        B, H, W = shapes[2]
        out.append(FirstCase(f"first_{'hs' if fam else 'f32'}_{B}x{H}x{W}_c64_lin_s3" + ("_k2" if fam else ""), fam, B, H, W, 64, 1.0, 2 * fam, 3))
        B, H, W = shapes[1]      # the DRUNet VJP's seed: 64 channels, linear, sigma_stride 0 on a zero buffer
        out.append(FirstCase(f"first_{'hs' if fam else 'f32'}_{B}x{H}x{W}_c64_seed", fam, B, H, W, 64, 1.0, 0, 0))
    return tuple(out)


FIRST_CASES = _first_cases()
FIRST_BY_NAME = {c.name: c for c in FIRST_CASES}
FIRST_REFUSED_F32 = tuple(s for s in IMAGE_SHAPES if s[2] % 4)       # the fp32 kernel refuses these widths


@functools.lru_cache(maxsize=None)
def first_inputs(name):
    c = FIRST_BY_NAME[name]
    g = _gen(name)
    return {"x": _signed(g, c.B, c.H, c.W), "sigma": sigma_vector(g, c.B, c.sigma_stride), "w": torch.randn(c.cout, 2, 9, generator=g) / 3,
            "bias": torch.randn(c.cout, generator=g) / 4}


def _first_taps(c, d, dtype, unmasked=False):
    """(taps of the image [B][9][H][W], taps of the noise map [B][9][H][W]) in the kernel's tap order t = 3 (dy + 1) + (dx + 1)."""
    x = F.pad(d["x"].to(dtype), (1, 1, 1, 1))
    s = sigma_of(d, c.B, c.sigma_stride).to(dtype).view(c.B, 1, 1).expand(c.B, c.H, c.W)
    s = F.pad(s, (1, 1, 1, 1), mode="replicate") if unmasked else F.pad(s, (1, 1, 1, 1))
    win = lambda t: torch.stack([t[:, i:i + c.H, j:j + c.W] for i in range(3) for j in range(3)], 1)
    return win(x), win(s)


def first_reference(c, d):
    """(ref, den) float64 [B][cout][H][W]: LeakyReLU(bias + sum w x + sum w sigma 1[inside]); den = sum |w f| + |b| of the pre-activation."""
    tx, ts = _first_taps(c, d, torch.float64)
    w, b = d["w"].double(), d["bias"].double().view(1, -1, 1, 1)
    pre = torch.einsum("ct,bthw->bchw", w[:, 0], tx) + torch.einsum("ct,bthw->bchw", w[:, 1], ts) + b
    den = torch.einsum("ct,bthw->bchw", w[:, 0].abs(), tx.abs()) + torch.einsum("ct,bthw->bchw", w[:, 1].abs(), ts.abs()) + b.abs()
    return F.leaky_relu(pre, c.slope), den


def _fma32(a, b, acc):
    """fp32 fma of fp32 operands: the product is exact in float64, the sum is rounded to fp32 (a double rounding: at worst an ulp's tie)."""
    return (a.double() * b.double() + acc.double()).float()


def first_emulate32(c, d, unmasked=False):
    """The kernels' order in fp32: acc = bias, the image's nine taps, the noise map's nine taps as fma; max(acc, acc slope); family 1:
    times HS_ASCALE 2^-k, split into hi + lo.  Returns values (family 1: float64 of the decoded record, scale undone).
    unmasked: the mutant whose noise-map taps are not masked outside the image."""
    tx, ts = _first_taps(c, d, torch.float32, unmasked)
    acc = d["bias"].view(1, -1, 1, 1).expand(c.B, c.cout, c.H, c.W).contiguous()
    for taps, ch in ((tx, 0), (ts, 1)):
        for t in range(9):
            acc = _fma32(d["w"][:, ch, t].view(1, -1, 1, 1), taps[:, t].unsqueeze(1), acc)
    v = torch.maximum(acc, acc * np.float32(c.slope))
    if c.family == 1:
        sc = ASCALE * 2.0 ** -c.k
        hi, lo = split(v * np.float32(sc))
        return (hi.double() + lo.double()) / sc
    return v


OutcCase = collections.namedtuple("OutcCase", "name B H W")
OUTC_CASES = tuple(OutcCase(f"outc_{B}x{H}x{W}", B, H, W) for B, H, W in IMAGE_SHAPES)
OUTC_BY_NAME = {c.name: c for c in OUTC_CASES}


@functools.lru_cache(maxsize=None)
def outc_inputs(name, family=0):
    """feat [B][32][H][W] (family 1: decoded), x [B][H][W] in [-0.6, 1.6], w [32], bias [1]: the pre-clamp values straddle 0 and 1."""
    c = OUTC_BY_NAME[name]
    g = _gen(name)
    feat = _signed(g, c.B, 32, c.H, c.W)
    d = {"feat": decoded(feat) if family else feat, "x": -0.6 + 2.2 * torch.rand(c.B, c.H, c.W, generator=g), "w": torch.randn(32, generator=g) / 4,
         "bias": torch.randn(1, generator=g) / 4}
    return d


def outc_reference(c, d):
    """(pre, den) float64 [B][H][W]: x + (sum_c w_c feat_c + bias); den = sum |w f| + |b| + |x|."""
    w = d["w"].double().view(1, 32, 1, 1)
    f = d["feat"].double()
    return d["x"].double() + ((w * f).sum(1) + d["bias"].double()), (w * f).abs().sum(1) + d["bias"].double().abs() + d["x"].double().abs()


def outc_emulate32(c, d, family=0, zeroed=None):
    """The kernels' order in fp32: acc = 0, fma over the 32 channels in order, v = x + (acc + bias) (family 1: the records hold 16 x the
    values, acc * (1 / 16): the same numbers, powers of two apart) -> (pre, clamp(pre)).  zeroed: the mutant with w[zeroed] = 0."""
    w = d["w"].clone()
    if zeroed is not None:
        w[zeroed] = 0.0
    acc = torch.zeros(c.B, c.H, c.W)
    for ch in range(32):
        acc = _fma32(w[ch].view(1, 1, 1), d["feat"][:, ch], acc)
    pre = d["x"] + (acc + d["bias"])
    return pre, pre.clamp(0.0, 1.0)


def straddles(pre):
    return bool((pre < 0).any()) and bool((pre > 1).any()) and bool(((pre > 0) & (pre < 1)).any())


TAIL_SHAPES = IMAGE_SHAPES


def _edge_image(g, B, H, W, with_nan):
    """[B][H][W] in [-0.5, 1.5] holding exact 0.0, -0.0, 1.0 and their outward neighbours (and a NaN) from the first cell on, image 0
    whatever the size allows, every image where it has room."""
    p = -0.5 + 2.0 * torch.rand(B, H, W, generator=g)
    e = torch.tensor(EDGES_IN + EDGES_OUT + ((float("nan"),) if with_nan else ()))
    flat = p.view(B, -1)
    n = min(flat.shape[1], e.numel())
    flat[:, :n] = e[:n]
    return p


@functools.lru_cache(maxsize=None)
def tail_out_inputs(B, H, W):
    g = _gen(f"tail_out_{B}x{H}x{W}")
    t = _signed(g, B, 32, H, W)
    t[:, 0] = _edge_image(g, B, H, W, False)
    return {"t32": t}


def unsigned_zeros(t):
    """t with every zero as +0.0: the sign of a zero that comes out of the clamp is the instruction's business (the compiler folds
    fminf(fmaxf(v, 0), 1) into a clamp modifier; torch.clamp keeps -0.0) and no part of the contract -- every other bit is."""
    return torch.where(t == 0, torch.zeros((), dtype=t.dtype), t)


def tail_out_restate(d):
    """(out_pre, out) = channel 0 and its clamp; compare `out` through unsigned_zeros."""
    v = d["t32"][:, 0].contiguous()
    return v, v.clamp(0.0, 1.0)


@functools.lru_cache(maxsize=None)
def tail_mask_inputs(B, H, W):
    g = _gen(f"tail_mask_{B}x{H}x{W}")
    return {"g": _signed(g, B, H, W), "pre": _edge_image(g, B, H, W, True)}


HS_SC = (2.0 ** -3, 2.0 ** 3)      # the {1 / m, m} pair the half-split cases hand the kernels


def tail_mask_restate(d, scale=None, exclusive_one=False):
    """g 1[0 <= pre <= 1] (family 1: g times sc[0]); a NaN compares false.  exclusive_one: the mutant with `< 1`."""
    p = d["pre"]
    inside = (p >= 0) & ((p < 1) if exclusive_one else (p <= 1))
    gs = d["g"] if scale is None else d["g"] * torch.tensor(scale, dtype=torch.float32)
    return torch.where(inside, gs, torch.zeros(()))


# ---------------------------------------------------------------------------------------------------------------------------------
# pooling

PoolCase = collections.namedtuple("PoolCase", "name B C H W")
# one window; odd sizes (the last row and column are dropped), C no multiple of 8: fp32 only.  Then both families: one block, odd sizes,
# 3 * 2 * 4 * 17 = 408 outputs = two blocks
POOL_CASES = tuple(PoolCase(f"pool_{B}x{C}x{H}x{W}", B, C, H, W) for B, C, H, W in ((1, 1, 2, 2), (2, 3, 5, 7), (2, 8, 16, 16), (1, 8, 25, 19), (3, 16, 9, 34)))
POOL_BY_NAME = {c.name: c for c in POOL_CASES}
# tie-rich windows [v00, v01, v10, v11]: all four equal, each pair equal, +-0 cells in one window
TIE_WINDOWS = ((1., 1., 1., 1.), (-.5, -.5, -.5, -.5), (1., 1., 0., 0.), (0., 0., 1., 1.), (1., 0., 1., 0.), (0., 1., 0., 1.), (0., -0., -0., 0.),
               (-0., 0., -1., -1.), (-0., -0., -0., -0.), (-1., -0., 0., -1.), (-1., .5, .5, -1.), (-.25, -.5, -1., -.75))


def pool_families(c):
    return (0, 1) if c.C % 8 == 0 else (0,)


@functools.lru_cache(maxsize=None)
def pool_inputs(name, family=0):
    """[B][C][H][W]: signed draws, every third window one of TIE_WINDOWS in turn (a lone window: the +-0 one)."""
    c = POOL_BY_NAME[name]
    g = _gen(name)
    a = _signed(g, c.B, c.C, c.H, c.W)
    Ho, Wo = c.H // 2, c.W // 2
    win = a[..., :2 * Ho, :2 * Wo].reshape(c.B, c.C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4).clone()
    k = torch.arange(0, win.shape[0], 3)
    win[k] = torch.tensor(TIE_WINDOWS)[(k // 3 + 6) % len(TIE_WINDOWS)]
    a[..., :2 * Ho, :2 * Wo] = win.reshape(c.B, c.C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(c.B, c.C, 2 * Ho, 2 * Wo)
    return {"x": decoded(a) if family else a}


def pool_restate(x, ceil_index=False):
    """MaxPool2d(2), floor semantics, in the kernel's order max(max(v00, v01), max(v10, v11)) with the GPU's maximum: v_max_f32 orders the
    zeros (-0 < +0), which torch.maximum leaves to the operand order -- so a zero maximum is +0 unless every zero of the window is -0.
    ceil_index: the mutant that numbers the output columns by ceil(W / 2) (the flat index decoded with the wrong width)."""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    if ceil_index:
        y = F.max_pool2d(x, 2, ceil_mode=True)
        return y.reshape(B, C, -1)[..., :Ho * Wo].reshape(B, C, Ho, Wo).contiguous()
    v = x[..., :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)
    m = v.max(-1).values
    plus_zero = ((v == 0) & ~torch.signbit(v)).any(-1)
    return torch.where(m == 0, torch.where(plus_zero, 0.0, -0.0).float(), m).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# up-sampling

UpsCase = collections.namedtuple("UpsCase", "name h w Ht Wt C B")


def _u(h, w, odd=0, C=8, B=B_MAX):
    Ht, Wt = 2 * h + odd, 2 * w + odd
    return UpsCase(f"ups_{h}x{w}_to{Ht}x{Wt}" + (f"_c{C}_B{B}" if (C, B) != (8, B_MAX) else ""), h, w, Ht, Wt, C, B)


# 1 x 1 (sy = sx = 0), 1 x 2, 2 x 3 (odd w: scalar only in fp32); 3 x 2: v4 with 2h = 6 no multiple of its 4 rows; 8 x 8, 8 x 16, 9 x 17: the
# half-split TX boundary 2w = 16 / 32 / 34; 16 x 66: a 33-wide v4 block; 5 x 130: two blocks in x (65 quads, 260 columns = 5 half-split
# tiles); 20 x 40: several half-split tiles both ways; 25 x 19.  Odd targets (the padded level): the extra row and column stay untouched.
UPS_CASES = (_u(1, 1), _u(1, 2), _u(2, 3), _u(2, 3, 1), _u(3, 2), _u(8, 8), _u(8, 16), _u(8, 16, 1), _u(9, 17), _u(9, 17, 1), _u(16, 66), _u(5, 130),
             _u(20, 40), _u(25, 19), _u(25, 19, 1))
# the plane boundary: fp32 65535 planes (v4 still runs) and 65536 (scalar only) at 1 x 2; half-split 65544 (image, group) planes at 1 x 1
UPS_F32_OVER_LIMIT = _u(1, 2, C=8, B=8192)
UPS_HS_SLICED = _u(1, 1, C=64, B=8193)
UPS_F32_65535 = UpsCase("ups_1x2_to2x4_c65535_B1", 1, 2, 2, 4, 65535, 1)
UPS_BY_NAME = {c.name: c for c in UPS_CASES + (UPS_F32_OVER_LIMIT, UPS_HS_SLICED, UPS_F32_65535)}


@functools.lru_cache(maxsize=None)
def ups_inputs(name, family=0):
    c = UPS_BY_NAME[name]
    x = _signed(_gen(name), c.B, c.C, c.h, c.w)
    return {"x": decoded(x) if family else x}


def ups_contracted(family, form):
    """Which weight arithmetic a form runs, read from the library's code as compiled (tests/vjp_glue_cases.py: weight_table): the scalar
    fp32 kernel and both half-split instances take l = fma(s, d, -i0) -- the compiler fuses `s * d - i0` --, the four-outputs-per-thread
    fp32 kernel (the form the forward dispatches) keeps the product and the subtraction apart, l = fp32(s * d) - i0, in x and in y.  The
    two tables differ by up to an absolute 2^-24 per unit of the index, so tier (a) and the impulses tell them apart at once; the GPU
    test reports the measure against the other table beside a failure."""
    return not (family == 0 and form == UPS_V4)


def ups_reference_a(x, contracted=True):
    """(ref, den) float64: the sum with the kernel's own fp32 weights (weight_table: [n][2n]), and sum |w_y w_x v|."""
    h, w = x.shape[-2:]
    Wy = torch.from_numpy(weight_table(h, contracted)).double()
    Wx = torch.from_numpy(weight_table(w, contracted)).double()
    return Wy.T @ x.double() @ Wx, Wy.T @ x.double().abs() @ Wx


def ups_reference_b(x):
    return F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)


def ups_tables(n, clamp=True, contracted=True):
    """(i0, i1, l, 1 - l) of the 2n destinations as the kernels compute them: f = s * d, i0 = (int) f, i1 = i0 + (i0 < n - 1), l = fma(s, d,
    -i0) (contracted) or fp32(f) - i0.  clamp=False: the mutant with i1 = i0 + 1 read from beyond the image."""
    s = np.float32(n - 1) / np.float32(2 * n - 1) if 2 * n > 1 else np.float32(0)
    dst = np.arange(2 * n)
    f = (s * dst.astype(np.float32)).astype(np.float32)
    i0 = f.astype(np.int64)
    i1 = i0 + ((i0 < n - 1) if clamp else 1)
    l = (np.float64(s) * dst - i0).astype(np.float32) if contracted else (f - i0.astype(np.float32)).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l), torch.from_numpy((np.float32(1) - l).astype(np.float32))


def ups_emulate32(x, family=0, clamp=True, contracted=True):
    """The kernels' arithmetic in fp32 on the CPU: hy (hx v00 + lx v01) + ly (hx v10 + lx v11); family 1 works on 16 x the values and
    splits the result into hi + lo like hs_pack (-> float64 of the decoded record).  clamp=False: the mutant without the `x0 < w - 1`
    clamp, whose second tap reads one cell to the right of / below the image.  Its weight there is 0 or a few 2^-25, so on a zero border
    the mutant hides below every bar; the GPU test therefore hands the kernels sources whose BORDER is NaN (a correct kernel never reads
    it), and so does this emulation: the mutant's last row and column come out NaN."""
    h, w = x.shape[-2:]
    y0, y1, ly, hy = ups_tables(h, clamp, contracted)
    x0, x1, lx, hx = ups_tables(w, clamp, contracted)
    v = x * np.float32(ASCALE) if family else x
    v = F.pad(v, (0, 1, 0, 1), value=float("nan"))
    r0, r1 = v[..., y0, :], v[..., y1, :]
    top = hx * r0[..., x0] + lx * r0[..., x1]
    bot = hx * r1[..., x0] + lx * r1[..., x1]
    y = hy.view(-1, 1) * top + ly.view(-1, 1) * bot
    if family:
        hi, lo = split(y)
        return (hi.double() + lo.double()) / ASCALE
    return y


def nan_border(padded, family):
    """A padded source tensor (pad(x) or hs8_encode(x)) with every border cell NaN instead of zero."""
    out = torch.full_like(padded, float("nan"))
    if family:
        out[:, :, 1:-1, 1:-1] = padded[:, :, 1:-1, 1:-1]
    else:
        interior(out)[...] = interior(padded)
    return out


def ups_impulse_sites(c, family):
    """Source pixels (sy, sx) for the impulse launches, one per plane: the four corners, and both sides of every boundary the output
    crosses -- x: the 64- and 32-column half-split tiles and the fp32 blocks (256 columns) map back to source columns around
    (int)(s * X0); y: the 16-row tiles and the v4 kernel's 4-row groups."""
    ys, xs = {0, c.h - 1}, {0, c.w - 1}
    for n, sites, steps in ((c.w, xs, (32, 64, 256)), (c.h, ys, (4, 16))):
        s = (n - 1) / (2 * n - 1) if n > 1 else 0.0
        for step in steps:
            for X0 in range(step, 2 * n, step):
                k = int(s * X0)
                sites.update(v for v in (k - 1, k, k + 1) if 0 <= v < n)
    ys, xs = sorted(ys), sorted(xs)
    # every boundary row at both ends in x, every boundary column at both ends in y, and the two lists paired off
    pts = {(y, x) for y in ys for x in (0, c.w - 1)} | {(y, x) for y in (0, c.h - 1) for x in xs}
    pts |= {(ys[i % len(ys)], xs[i % len(xs)]) for i in range(max(len(ys), len(xs)))}
    return sorted(pts)


def ups_impulse_input(c, sites):
    """[1][8 * ceil(len / 8)][h][w]: plane i holds one 1.0 at sites[i]."""
    n = (len(sites) + 7) // 8 * 8
    x = torch.zeros(1, n, c.h, c.w)
    for i, (sy, sx) in enumerate(sites):
        x[0, i, sy, sx] = 1.0
    return x


def ups_impulse_expected(c, sites, n_planes, contracted=True):
    """[1][n][2h][2w] float64: the outer product of the two 1-D weight tables' rows of each site -- where a table holds a zero, the output
    holds an exact zero."""
    Wy, Wx = torch.from_numpy(weight_table(c.h, contracted)).double(), torch.from_numpy(weight_table(c.w, contracted)).double()
    out = torch.zeros(1, n_planes, 2 * c.h, 2 * c.w, dtype=torch.float64)
    for i, (sy, sx) in enumerate(sites):
        out[0, i] = Wy[sy].view(-1, 1) * Wx[sx].view(1, -1)
    return out


# relative to w_y w_x, per element: the product is rounded once (a clamped end adds hx + lx).  Half-split: + the record's hi + lo split
# (4 * 2^-24), beyond an absolute 2^-29: lo's (for tiny weights also hi's) f16 subnormal half-step 2^-25 in record units, / 16
IMPULSE_BAR = 3 * U
IMPULSE_BAR_HS = 7 * U
IMPULSE_FLOOR_HS = 2.0 ** -29


def impulse_measure(v, want, family):
    """(exact zeros wherever the table holds a zero [fp32: and nowhere else], max (|v - want| - floor) / |want|)."""
    v = v.double()
    zeros_ok = bool((v[want == 0] == 0).all()) and (family == 1 or bool((v[want != 0] != 0).all()))
    err = ((v - want).abs() - (IMPULSE_FLOOR_HS if family else 0.0)).clamp_min(0.0) / want.abs().clamp_min(1e-300)
    return zeros_ok, float(err.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# re-layouts and the skip sum

RelayoutCase = collections.namedtuple("RelayoutCase", "name B C h w")      # C channels at h x w <-> 4C at h/2 x w/2
# one output pixel per plane; 2 x 3 outputs; two groups, 5 columns; 64 channels: 8 groups, 32 out
RELAYOUT_CASES = tuple(RelayoutCase(f"relayout_{B}x{C}x{h}x{w}", B, C, h, w) for B, C, h, w in ((1, 8, 2, 2), (2, 8, 4, 6), (3, 16, 8, 10), (2, 64, 8, 8)))
RELAYOUT_BY_NAME = {c.name: c for c in RELAYOUT_CASES}


@functools.lru_cache(maxsize=None)
def relayout_inputs(name, family=0):
    c = RELAYOUT_BY_NAME[name]
    g = _gen(name)
    x, y = _signed(g, c.B, c.C, c.h, c.w), _signed(g, c.B, c.C, c.h, c.w)
    x.view(-1)[:2] = torch.tensor([0.0, -0.0])
    y.view(-1)[:2] = torch.tensor([-0.0, -0.0])
    return {"x": decoded(x) if family else x, "y": decoded(y) if family else y}


def s2d_restate(x, swapped=False):
    """[B][C][h][w] -> [B][4C][h/2][w/2], PHASE-MAJOR: out[(2 dy + dx) C + c][y][x] = in[c][2y + dy][2x + dx] -- not pixel_unshuffle's
    order, which is c * 4 + (2 dy + dx).  swapped: the mutant with dy and dx exchanged in the phase."""
    B, C, h, w = x.shape
    out = torch.empty(B, 4 * C, h // 2, w // 2, dtype=x.dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            ph = (2 * dx + dy) if swapped else (2 * dy + dx)
            out[:, ph * C:(ph + 1) * C] = x[:, :, dy::2, dx::2]
    return out


def d2s_restate(x, swapped=False):
    """[B][4C][h][w] -> [B][C][2h][2w]: out[c][2y + dy][2x + dx] = in[(2 dy + dx) C + c][y][x]."""
    B, C4, h, w = x.shape
    C = C4 // 4
    out = torch.empty(B, C, 2 * h, 2 * w, dtype=x.dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            ph = (2 * dx + dy) if swapped else (2 * dy + dx)
            out[:, :, dy::2, dx::2] = x[:, ph * C:(ph + 1) * C]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the DRUNet's fp32 input gradient

InCase = collections.namedtuple("InCase", "name B C H W")
# H W = 5 (59 empty chunks), 64 (one pixel per chunk), 65 (per = 2: 32 full chunks, one of one pixel), 1950 (per = 31)
INGRAD_CASES = tuple(InCase(f"ingrad_{B}x{C}x{H}x{W}", B, C, H, W) for B, C, H, W in ((3, 32, 1, 5), (3, 32, 8, 8), (3, 2, 5, 13), (2, 32, 50, 39)))
INGRAD_BY_NAME = {c.name: c for c in INGRAD_CASES}


@functools.lru_cache(maxsize=None)
def ingrad_inputs(name):
    c = INGRAD_BY_NAME[name]
    g = torch.randn(c.B, c.C, c.H, c.W, generator=_gen(name))
    g[:, 0].reshape(c.B, -1)[:, 0] = -0.0
    return {"g": g}


def ingrad_reference(c, d):
    """gx = g[:, 0] (exact); float64: the sigma terms g[:, 1] chunked like the kernel -> part [B][64], sum |terms| per chunk, gsigma [B],
    sum |terms|."""
    n = c.H * c.W
    per = (n + SIG_CHUNKS - 1) // SIG_CHUNKS
    t = F.pad(d["g"][:, 1].double().reshape(c.B, n), (0, per * SIG_CHUNKS - n)).reshape(c.B, SIG_CHUNKS, per)
    return d["g"][:, 0].contiguous(), t.sum(2), t.abs().sum(2), t.sum((1, 2)), t.abs().sum((1, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage: every (op, family, form) the probe can run, and the cases that reach it

def reached_forms():
    """{(op, family, form)} the case tables run (tests/test_gpu_fwd_glue.py launches exactly these)."""
    got = set()
    for fam in (0, 1):
        for op in (PREP_INPUT, OUTC_RESIDUAL, S2D, D2S, ADD, TAIL_MASK) + (() if fam else F32_ONLY):
            got.add((op, fam, 1))
        if any(fam in pool_families(c) for c in POOL_CASES):
            got.add((MAXPOOL2, fam, 1))
        if any(c.family == fam for c in FIRST_CASES):
            got.add((CONV_FIRST, fam, 1))
        for c in UPS_CASES:
            for f in ups_forms_admitted(fam, c.B * (c.C // 8 if fam else c.C), c.w):
                got.add((UPSAMPLE2X, fam, f))
    return got


def all_forms():
    out = set()
    for fam in (0, 1):
        for op in range(DRU_INPUT_GRAD + 1):
            if fam and op in F32_ONLY:
                continue
            for f in ((1, 2) if op == UPSAMPLE2X else (1,)):
                out.add((op, fam, f))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the derived bars and the profile note

def _one_thread(fn):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(threads)


@functools.lru_cache(maxsize=None)
def emulation_maxima():
    """{key: (largest measure of the fp32 emulation over the class's cases, case)}; keys: BAR_KEYS."""
    def run():
        out = {}
        for fam, key in ((0, "first_f32"), (1, "first_hs")):
            worst = (-1.0, "")
            for c in FIRST_CASES:
                if c.family == fam:
                    d = first_inputs(c.name)
                    ref, den = first_reference(c, d)
                    worst = max(worst, (measure(first_emulate32(c, d), ref, den), c.name))
            out[key] = worst
        for fam, key in ((0, "outc_f32"), (1, "outc_hs")):
            worst = (-1.0, "")
            for c in OUTC_CASES:
                d = outc_inputs(c.name, fam)
                ref, den = outc_reference(c, d)
                worst = max(worst, (measure(outc_emulate32(c, d, fam)[0], ref, den), c.name))
            out[key] = worst
        for fam, key in ((0, "ups_f32"), (1, "ups_hs")):
            worst = (-1.0, "")
            for c in UPS_CASES:
                x = ups_inputs(c.name, fam)["x"]
                for form in ups_forms_admitted(fam, c.B * (c.C // 8 if fam else c.C), c.w):      # each form's own weight arithmetic
                    y = ups_emulate32(x, fam, contracted=ups_contracted(fam, form))
                    worst = max(worst, (measure(y, ups_reference_b(x), ups_reference_a(x)[1]), c.name))
            out[key] = worst
        return out
    return _one_thread(run)


BAR_KEYS = ("first_f32", "first_hs", "outc_f32", "outc_hs", "ups_f32", "ups_hs")


def recorded_bars():
    """{key: (emulation maximum, bar)} as profiles/fwd_glue_probe.md records them (table rows `| key | max | bar | ...`)."""
    out = {}
    for line in open(PROFILE_NOTE):
        m = re.match(r"\|\s*(%s)\s*\|\s*([0-9.eE+-]+)\s*\|\s*([0-9.eE+-]+)\s*\|" % "|".join(BAR_KEYS), line)
        if m:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    assert set(out) == set(BAR_KEYS), f"{PROFILE_NOTE}: bars of {sorted(set(BAR_KEYS) - set(out))} missing"
    return out


def bar(key):
    return recorded_bars()[key][1]
