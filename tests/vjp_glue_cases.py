"""Cases, inputs, float64 references, fp32 restatements and emulations of the probe of the launches between the UNet VJP's adjoint
convolutions (pnpx_vjp_glue_probe, csrc/vjp_glue_probe.hip; kernels: csrc/unet_bwd.hip, csrc/grad_common.h).

References are float64 torch autograd of the forward op on the CPU, computed from the very fp32 inputs (half-split: from the decoded
records); the saved activation stands in for the pre-activation, whose sign is all that matters.  Bars:

  single-product ops (out-conv tail, skip / pool merge, the image half of the input gradient): the GPU result is BIT-IDENTICAL to an fp32
    torch restatement in the kernel's operation order (half-split: to hs8_encode of it); the host test holds the restatement within
    SINGLE_BAR = 3 * 2^-24 relative, per element, of the autograd reference (two roundings plus slack).
  up-sampling adjoint: per element |y - ref| / sum |w_y w_x g| over the contributing destination pixels.  Tier (a): ref = a float64 sum with
    the kernel's own fp32 weights, bar UPS_TIER_A = 12 * 2^-24 (at most 9 terms of two products, 8 additions, the final factor).  Tier (b):
    ref = autograd, bar = BAR_FACTOR x the largest value the fp32 emulation of the kernel reaches on the same cases
    (profiles/vjp_glue_probe.md records it; tests/test_vjp_glue_host.py re-derives it).
  sigma sums: against the float64 sum, relative to sum |terms|, k * 2^-24 with k the summation depth (sigma_depth).
No GPU."""
import collections
import functools
import os
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_hs_cases import ASCALE, hs8_decode, hs8_encode, quantize, split
from tests.conv_layer_cases import BAR_FACTOR, PADL, border_cells, interior, pad, upsample32  # noqa: F401  (re-exported to the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE_NOTE = os.path.join(ROOT, "profiles", "vjp_glue_probe.md")
U = 2.0 ** -24
SLOPE = 0.2
SINGLE_BAR = 3 * U
UPS_TIER_A = 12 * U
B_MAX = 3
SIG_CHUNKS = 64            # csrc/grad_common.h
GRID_Z_MAX = 65535         # csrc/grad_common.h: VG_GRID_Z_MAX

# include/pnpx.h: enum pnpx_vjp_glue_op; the form ids of pnpx_vjp_glue_probe_desc
OUTC_BWD, UPSAMPLE_BWD, SKIP_POOL_MERGE, INPUT_GRAD, GRAD_SCALE = range(5)
UPS_PLAIN, UPS_LDS16, UPS_LDS64 = 1, 2, 3
SPM_PIXEL, SPM_BLOCK = 1, 2
UPS_FORM_NAMES = {UPS_PLAIN: "plain", UPS_LDS16: "lds16", UPS_LDS64: "lds64"}
SPM_FORM_NAMES = {SPM_PIXEL: "pixel", SPM_BLOCK: "block"}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def dlrelu(a):
    """LeakyReLU' as the kernels take it from a saved activation: 1 where a > 0, else 0.2 (so 0.2 at +0 and -0)."""
    return torch.where(a > 0, torch.ones((), dtype=a.dtype), torch.tensor(SLOPE, dtype=torch.float32).to(a.dtype))     # the kernels' 0.2f


def _signed(g, *shape):
    """Activations away from the kink: magnitudes in [0.1, 1], random signs."""
    return (0.1 + 0.9 * torch.rand(*shape, generator=g)) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def _zero_cells(g, x, n=6):
    """n cells of +0.0 and n of -0.0 at seeded places of x (in place); image 0 holds both whatever the draw."""
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:2 * n]
    flat[idx[:n]] = 0.0
    flat[idx[n:]] = -0.0
    if flat.numel() >= 2:
        flat[0], flat[1] = 0.0, -0.0
    return x


def decoded(x):
    """What a half-split kernel reads back from hs8_encode(x), as fp32 (exact: hi + lo has at most 22 significant bits)."""
    return quantize(x, torch.float32)


def rel_err(y, ref):
    """max per element |y - ref| / |ref| (ref = 0: y must be 0); NaN anywhere = inf."""
    y, ref = y.double(), ref.double()
    e = (y - ref).abs() / ref.abs()
    e = torch.where(ref == 0, torch.where(y == 0, 0.0, float("inf")).double(), e)
    return float("inf") if bool(torch.isnan(e).any()) else float(e.max())


def measure(y, ref, den):
    e = (y.double() - ref).abs() / den
    e = torch.where(den == 0, torch.where(y.double() == ref, 0.0, float("inf")).double(), e)
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


def bits_equal(a, b):
    v = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(v), b.contiguous().view(v)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the launchers' host-only form decisions, restated (tests/test_vjp_glue_host.py holds them against pnpx_vjp_glue_probe_plan)

def ups_form(B, C, w):
    if B * C > GRID_Z_MAX:
        return UPS_PLAIN
    return UPS_LDS64 if w >= 64 else UPS_LDS16


def ups_forms_admitted(B, C):
    return (UPS_PLAIN, UPS_LDS16, UPS_LDS64) if B * C <= GRID_Z_MAX else (UPS_PLAIN,)


def spm_form(H, W):
    return SPM_BLOCK if H % 2 == 0 and W % 2 == 0 else SPM_PIXEL


def spm_forms_admitted(H, W):
    return (SPM_PIXEL, SPM_BLOCK) if H % 2 == 0 and W % 2 == 0 else (SPM_PIXEL,)


def ups_hs_launches(B, Gs):
    per = GRID_Z_MAX // Gs
    return 0 if per == 0 else (B + per - 1) // per


def fp32_chain_batches(B, fp32_chains=2):
    """The batch sizes unet_denoise_backward hands the fp32 launchers: with option fp32_chains >= 2 (the default is 2) and B >= 2 the
    adjoint chain forks exactly two launch chains over images [B c / 2, B (c + 1) / 2) (csrc/common.h: fan_out_chains), and every form
    decision is taken per chain; otherwise the whole batch runs as one."""
    return [B * (c + 1) // 2 - B * c // 2 for c in (0, 1)] if fp32_chains >= 2 and B >= 2 else [B]


def vjp_levels(H, W):
    """The four up-sampling adjoints of an H x W VJP, level 0 first: (source channels C, source h, w, Ccat, c_off, Ht, Wt); the skip /
    pool merge of the level has C / 2 channels at Ht x Wt."""
    return [(2 * (32 << l), H >> (l + 1), W >> (l + 1), 3 * (32 << l), 32 << l, H >> l, W >> l) for l in range(4)]


def plan(op, family, form=0, B=1, C=8, H=16, W=16, Ccat=0, c_off=0, Ht=0, Wt=0):
    """pnpx_vjp_glue_probe_plan: (form, launches), (0, 0) = refused."""
    from tfpnp_amd import _lib
    import ctypes
    d = _lib.VjpGlueProbeDesc(op=op, family=family, form=form, B=B, C=C, H=H, W=W, Ccat=Ccat, c_off=c_off, Ht=Ht, Wt=Wt)
    v = _lib.lib().pnpx_vjp_glue_probe_plan(ctypes.byref(d))
    return (v & 255, (v >> 8) + 1) if v else (0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# up-sampling adjoint

UpsCase = collections.namedtuple("UpsCase", "name h w Ht Wt C c_off Ccat B")


def _u(h, w, odd, C=8, c_off=8, extra=0, B=B_MAX, tag=""):
    Ht, Wt = 2 * h + odd, 2 * w + odd
    name = f"ups_{h}x{w}_to{Ht}x{Wt}_c{C}at{c_off}of{c_off + C + extra}" + (f"_B{B}" if B != B_MAX else "") + tag
    return UpsCase(name, h, w, Ht, Wt, C, c_off, c_off + C + extra, B)


# source sizes: a 1 x 1 source (sy = sx = 0), tiny, below a tile, one tile, partial tiles both ways, one 64-wide tile, a 1-column and an
# 8-column rest of the 64-wide form, several tiles.  Each at Ht x Wt = 2h x 2w (concat ends with the channels) and at 2h + 1 x 2w + 1
# (the padded odd level; channels follow in the concat); c_off > 0 everywhere.
UPS_SIZES = ((1, 1), (2, 2), (8, 8), (16, 16), (17, 19), (16, 64), (16, 65), (18, 72), (33, 130))
UPS_CASES = tuple(_u(h, w, odd, extra=8 * odd) for h, w in UPS_SIZES for odd in (0, 1))
# B * C = 65536 planes: the fp32 auto dispatch must take the plain form; half-split: B * groups = 65536 runs as two launches
UPS_MANY_PLANES = _u(2, 2, 0, C=8, c_off=0, B=8192)
UPS_HS_SLICED = _u(1, 1, 0, C=8, c_off=0, B=65536)
# the adjoint identity against the library's forward up-sampling (c_off = 0, concat = the channels, Ht x Wt = 2h x 2w)
UPS_ADJOINT_CASES = (_u(17, 19, 0, c_off=0), _u(18, 72, 0, c_off=0), _u(16, 65, 0, c_off=0))
UPS_BY_NAME = {c.name: c for c in UPS_CASES + (UPS_MANY_PLANES, UPS_HS_SLICED) + UPS_ADJOINT_CASES}


@functools.lru_cache(maxsize=None)
def ups_inputs(name, family=0, positive_mask=False):
    """{"g": [B][Ccat][Ht][Wt], "act": [B][C][h][w]} fp32; family 1: the values the kernel decodes from hs8_encode of the seeded draw."""
    c = UPS_BY_NAME[name]
    g = _gen(name)
    d = {"g": torch.randn(c.B, c.Ccat, c.Ht, c.Wt, generator=g)}
    a = _signed(g, c.B, c.C, c.h, c.w)
    d["act"] = a.abs() if positive_mask else _zero_cells(g, a, min(6, a.numel() // 2))
    if family == 1:
        d = {k: decoded(v) for k, v in d.items()}
    return d


def weight_table(n, contracted=True):
    """[n][2n] fp32: the weight of destination row / column d towards source s in the kernels' own float arithmetic
    (f = s * d, i0 = (int) f, i1 = i0 + (i0 < n - 1), l = f - i0; w[i0] += 1 - l, w[i1] += l) AS COMPILED: the library is built with the
    compiler's default floating-point contraction (csrc/Makefile sets no -ffp-contract; tests/test_vjp_glue_host.py holds that), which
    fuses `sy * yd - y0` into one fma in all four kernels, so l = fma(s, d, -i0) is rounded once, from the exact product (i0 still comes
    from the rounded f).  contracted=False: l = fp32(f) - i0, what a build without contraction computes; the two tables differ by up to
    an absolute 2^-24 per unit of the index, 14 x the tier-(a) bar at 130 columns, so a compiler that stops contracting fails tier (a)
    everywhere at once -- tests/test_gpu_vjp_glue.py then reports the measure against this second table beside the failure."""
    s = np.float32(n - 1) / np.float32(2 * n - 1) if 2 * n > 1 else np.float32(0)
    dst = np.arange(2 * n)
    f = (s * dst.astype(np.float32)).astype(np.float32)
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < n - 1)
    if contracted:
        l = (np.float64(s) * dst - i0).astype(np.float32)     # exact in float64 (24 + 9 bits), rounded once: the fma
    else:
        l = (f - i0.astype(np.float32)).astype(np.float32)
    T = np.zeros((n, 2 * n), np.float32)
    T[i0, dst] = (T[i0, dst] + (np.float32(1) - l)).astype(np.float32)
    T[i1, dst] = (T[i1, dst] + l).astype(np.float32)
    return T


def _ups_g(c, d):
    return d["g"][:, c.c_off:c.c_off + c.C, :2 * c.h, :2 * c.w]


def ups_reference_a(c, d, wy=None, wx=None):
    """(ref, den) float64: the sum with the kernel's own fp32 weights, and sum |w_y w_x g|."""
    Wy = torch.from_numpy(weight_table(c.h) if wy is None else wy).double()
    Wx = torch.from_numpy(weight_table(c.w) if wx is None else wx).double()
    g = _ups_g(c, d).double()
    ref = Wy @ g @ Wx.T * dlrelu(d["act"].double())
    return ref, Wy @ g.abs() @ Wx.T


def ups_reference_b(c, d):
    """float64 autograd of pad(interpolate(leaky_relu(z), x2, bilinear, align_corners)) placed at channels [c_off, c_off + C) of the concat."""
    z = d["act"].double().clone().requires_grad_(True)
    up = F.interpolate(F.leaky_relu(z, SLOPE), scale_factor=2, mode="bilinear", align_corners=True)
    up = F.pad(up, (0, c.Wt - 2 * c.w, 0, c.Ht - 2 * c.h))
    zeros = lambda n: torch.zeros(c.B, n, c.Ht, c.Wt, dtype=torch.float64)
    cat = torch.cat([zeros(c.c_off), up, zeros(c.Ccat - c.c_off - c.C)], 1)
    (cat * d["g"].double()).sum().backward()
    return z.grad


def ups_emulate32(c, d, family=0, mutant=None):
    """The kernels' arithmetic in fp32 on the CPU: the 7 x 7 candidate loop in its order, acc += (wy wx) g, the final factor; family 1
    works on 16 x the values and splits the result into hi + lo like hs_pack.  Returns the values (fp32; family 1: float64 of the decoded
    record).  mutant: "shifted_table" (the column weights of the next destination pixel), "dropped_column" (the last column of the first
    tile is not written: it keeps a zero), "c_off_ignored"."""
    Wy, Wx = weight_table(c.h), weight_table(c.w)
    if mutant == "shifted_table":
        Wx = np.roll(Wx, 1, axis=1)
    g = (d["g"][:, :c.C] if mutant == "c_off_ignored" else d["g"][:, c.c_off:c.c_off + c.C])[..., :2 * c.h, :2 * c.w]
    if family == 1:
        g = g * ASCALE
    ys, xs = np.arange(c.h), np.arange(c.w)
    acc = torch.zeros(c.B, c.C, c.h, c.w)
    for i in range(7):
        yd = 2 * ys - 3 + i
        ok = (yd >= 0) & (yd < 2 * c.h)
        ydc = np.clip(yd, 0, 2 * c.h - 1)
        wy = torch.from_numpy(np.where(ok, Wy[ys, ydc], np.float32(0)).astype(np.float32))
        for j in range(7):
            xd = 2 * xs - 3 + j
            okx = (xd >= 0) & (xd < 2 * c.w)
            xdc = np.clip(xd, 0, 2 * c.w - 1)
            wx = torch.from_numpy(np.where(okx, Wx[xs, xdc], np.float32(0)).astype(np.float32))
            acc = acc + (wy.view(-1, 1) * wx.view(1, -1)) * g[..., torch.from_numpy(ydc).view(-1, 1), torch.from_numpy(xdc).view(1, -1)]
    y = acc * dlrelu(d["act"])
    if mutant == "dropped_column":
        y[..., min(c.w, 64 if c.w >= 64 else 16) - 1] = 0.0
    if family == 1:
        hi, lo = split(y)
        return (hi.double() + lo.double()) / ASCALE
    return y


UPS_MUTANTS = ("shifted_table", "dropped_column", "c_off_ignored")


def ups_forward_emulate32(x):
    """The library's forward x2 up-sampling in fp32 (tests/conv_layer_cases.py: upsample32)."""
    return upsample32(x, 2 * x.shape[-2], 2 * x.shape[-1])


def adjoint_gap(up_x, g, x, bwd_g):
    """|<up(x), g> - <x, up_bwd(g)>| / <|up(x)|, |g|>, both inner products accumulated in float64."""
    lhs = (up_x.double() * g.double()).sum()
    rhs = (x.double() * bwd_g.double()).sum()
    return float((lhs - rhs).abs() / (up_x.double().abs() * g.double().abs()).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# skip / pool merge

SpmCase = collections.namedtuple("SpmCase", "name H W C Ccat pool ties B")
SPM_SIZES = ((2, 2), (16, 16), (16, 18), (17, 23), (3, 5))     # the last two: the last row and column get no pooled gradient
SPM_CASES = tuple(SpmCase(f"spm_{H}x{W}" + ("" if pool else "_nopool") + ("_ties" if ties else ""), H, W, 8, 16, pool, ties, B_MAX)
                  for H, W in SPM_SIZES for pool, ties in ((True, False), (False, False), (True, True)))
SPM_BY_NAME = {c.name: c for c in SPM_CASES}
# tie-rich windows [v00, v01, v10, v11]: all four equal, each pair equal, +-0 cells
TIE_WINDOWS = ((1., 1., 1., 1.), (-.5, -.5, -.5, -.5), (1., 1., 0., 0.), (0., 0., 1., 1.), (1., 0., 1., 0.), (0., 1., 0., 1.), (1., 0., 0., 1.),
               (0., 1., 1., 0.), (0., -0., -0., 0.), (-0., 0., -1., -1.), (-0., -0., -0., -0.), (-1., .5, .5, -1.))
TIE_VALUES = (-1.0, -0.5, -0.0, 0.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def spm_inputs(name, family=0):
    """{"g": [B][Ccat][H][W], "act": [B][C][H][W], "g_pool": [B][C][H/2][W/2] (pool cases)} fp32 (family 1: decoded)."""
    c = SPM_BY_NAME[name]
    g = _gen(name)
    d = {"g": torch.randn(c.B, c.Ccat, c.H, c.W, generator=g)}
    if c.ties:       # a few exactly representable values; every third window one of TIE_WINDOWS in turn
        a = torch.tensor(TIE_VALUES)[torch.randint(0, len(TIE_VALUES), (c.B, c.C, c.H, c.W), generator=g)]
        Ho, Wo = c.H // 2, c.W // 2
        win = a[..., :2 * Ho, :2 * Wo].reshape(c.B, c.C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4).clone()
        k = torch.arange(0, win.shape[0], 3)
        win[k] = torch.tensor(TIE_WINDOWS)[(k // 3) % len(TIE_WINDOWS)]
        a[..., :2 * Ho, :2 * Wo] = win.reshape(c.B, c.C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(c.B, c.C, 2 * Ho, 2 * Wo)
        d["act"] = a
    else:
        d["act"] = _zero_cells(g, _signed(g, c.B, c.C, c.H, c.W), 4)
    if c.pool:
        d["g_pool"] = torch.randn(c.B, c.C, c.H // 2, c.W // 2, generator=g)
    if family == 1:
        d = {k: decoded(v) for k, v in d.items()}
    return d


def spm_reference(c, d):
    """float64 autograd: the skip channels of the concat read leaky(z), the level below reads max_pool2d(leaky(z), 2)."""
    z = d["act"].double().clone().requires_grad_(True)
    a = F.leaky_relu(z, SLOPE)
    loss = (a * d["g"][:, :c.C].double()).sum()
    if c.pool:
        loss = loss + (F.max_pool2d(a, 2) * d["g_pool"].double()).sum()
    loss.backward()
    return z.grad


def spm_restate32(c, d, last_max=False):
    """The kernels' order in fp32: g = skip (+ the pooled gradient at the window's first maximum in scan order), then g * LeakyReLU'(act).
    last_max: the mutant that routes to the LAST maximum."""
    a = d["act"]
    gsum = d["g"][:, :c.C].clone()
    if c.pool:
        Ho, Wo = c.H // 2, c.W // 2
        v = a[..., :2 * Ho, :2 * Wo].reshape(c.B, c.C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(c.B, c.C, Ho, Wo, 4)
        m, arg = v[..., 0], torch.zeros(v.shape[:-1], dtype=torch.long)
        for k in (1, 2, 3):
            better = (v[..., k] >= m) if last_max else (v[..., k] > m)
            m, arg = torch.where(better, v[..., k], m), torch.where(better, k, arg)
        route = F.one_hot(arg, 4).bool()
        gp = torch.where(route, d["g_pool"].unsqueeze(-1), torch.zeros(()))
        add = gp.reshape(c.B, c.C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(c.B, c.C, 2 * Ho, 2 * Wo)
        sel = route.reshape(c.B, c.C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(c.B, c.C, 2 * Ho, 2 * Wo)
        # the kernel adds only at the routed cell (g += gp): elsewhere g keeps its own bits, -0.0 included
        gsum[..., :2 * Ho, :2 * Wo] = torch.where(sel, gsum[..., :2 * Ho, :2 * Wo] + add, gsum[..., :2 * Ho, :2 * Wo])
    return gsum * dlrelu(a)


# ---------------------------------------------------------------------------------------------------------------------------------
# out-conv tail

OutcCase = collections.namedtuple("OutcCase", "name H W B")
OUTC_CASES = (OutcCase("outc_16x16", 16, 16, B_MAX), OutcCase("outc_17x23", 17, 23, B_MAX))
OUTC_BY_NAME = {c.name: c for c in OUTC_CASES}
HS_SC = (2.0 ** -3, 2.0 ** 3)      # the {1 / m, m} pair the half-split cases hand the kernels
# cells of `pre` at the ends of the clamp: inside (inclusive) ... and just outside
PRE_EDGES_IN = (0.0, -0.0, 1.0)
PRE_EDGES_OUT = (float(np.nextafter(np.float32(0), np.float32(-1))), float(np.nextafter(np.float32(1), np.float32(2))))


@functools.lru_cache(maxsize=None)
def outc_inputs(name, family=0):
    """{"g": [B][H][W], "pre": [B][H][W], "w": [32], "act": [B][32][H][W]}; every image holds every edge value of `pre` (cells 0 .. 4 of
    its first row) and feat cells at +0 and -0."""
    c = OUTC_BY_NAME[name]
    g = _gen(name)
    d = {"g": torch.randn(c.B, c.H, c.W, generator=g), "pre": -0.3 + 1.6 * torch.rand(c.B, c.H, c.W, generator=g),
         "w": torch.randn(32, generator=g) / 4}
    d["pre"][:, 0, :5] = torch.tensor(PRE_EDGES_IN + PRE_EDGES_OUT)
    a = _zero_cells(g, _signed(g, c.B, 32, c.H, c.W), 12)
    a[:, 0, 0, :5] = 0.0             # +0 and -0 feat cells under every edge value of pre, in two channels
    a[:, 1, 0, :5] = -0.0
    d["act"] = decoded(a) if family == 1 else a
    return d


def outc_reference(c, d, scale=1.0):
    """float64 autograd of clamp(x + sum_c w_c leaky(z_c), 0, 1) at a point where its argument is exactly `pre` -> (g_feat, g_res)."""
    z = d["act"].double().clone().requires_grad_(True)
    p = d["pre"].double().clone().requires_grad_(True)
    a = F.leaky_relu(z, SLOPE)
    s = (d["w"].double().view(1, 32, 1, 1) * (a - a.detach())).sum(1)          # value 0, gradient w_c leaky'(z_c)
    out = torch.clamp(p + s, 0.0, 1.0)
    (out * (d["g"].double() * scale)).sum().backward()
    return z.grad, p.grad


def outc_restate32(c, d, scale=None, exclusive=False, unit_at_plus_zero=False):
    """The kernel's order in fp32 -> (g_feat = (w[c] * g) * LeakyReLU'(feat[c]), g_res = g), g = g_out (times sc[0], family 1) under the
    inclusive mask.  Mutants: an exclusive mask; LeakyReLU' = 1 at +0."""
    p = d["pre"]
    inside = ((p > 0) & (p < 1)) if exclusive else ((p >= 0) & (p <= 1))
    gs = d["g"] if scale is None else d["g"] * torch.tensor(scale, dtype=torch.float32)
    g = torch.where(inside, gs, torch.zeros(()))
    a = d["act"]
    dl = dlrelu(a)
    if unit_at_plus_zero:
        dl = torch.where((a == 0) & ~torch.signbit(a), 1.0, dl).float()
    return d["w"].view(1, 32, 1, 1) * g.unsqueeze(1) * dl, g


# ---------------------------------------------------------------------------------------------------------------------------------
# input gradient and the sigma sums

InCase = collections.namedtuple("InCase", "name H W C B")
INGRAD_CASES = (InCase("ingrad_16x16", 16, 16, 32, B_MAX), InCase("ingrad_17x23", 17, 23, 32, B_MAX),     # 391 pixels: per = 7, chunks 56 .. 63 empty
                InCase("ingrad_16x144", 16, 144, 32, B_MAX))
INGRAD_BY_NAME = {c.name: c for c in INGRAD_CASES}


@functools.lru_cache(maxsize=None)
def ingrad_inputs(name, family=0):
    c = INGRAD_BY_NAME[name]
    g = _gen(name)
    d = {"g": torch.randn(c.B, c.C, c.H, c.W, generator=g), "g_res": torch.randn(c.B, c.H, c.W, generator=g)}
    if family == 1:
        d["g"] = decoded(d["g"])
    return d


def ingrad_reference(c, d, m=1.0):
    """float64: gx = g_in0[:, 0] + g_res, the sigma terms g_in0[:, 1] chunked like the kernel (-> part [B][64], sum |terms| per chunk), gsigma,
    sum |terms|; all times m."""
    g = d["g"].double()
    gx = (g[:, 0] + d["g_res"].double()) * m
    n = c.H * c.W
    per = (n + SIG_CHUNKS - 1) // SIG_CHUNKS
    t = F.pad(g[:, 1].reshape(c.B, n), (0, per * SIG_CHUNKS - n)).reshape(c.B, SIG_CHUNKS, per) * m
    return gx, t.sum(2), t.abs().sum(2), t.sum((1, 2)), t.abs().sum((1, 2))


def ingrad_restate32(c, d, m=None):
    """gx in the kernels' order in fp32: g0 + g_res; family 1: (v0 / 16 + g_res) * m with v0 / 16 the decoded value (exact)."""
    gx = d["g"][:, 0] + d["g_res"]
    return gx if m is None else gx * torch.tensor(m, dtype=torch.float32)


def sigma_depth(H, W):
    """(k of a partial sum, k of the final sum), read from input_grad_kernel / sigma_grad_final_kernel: a thread adds ceil(per / 256) terms
    serially (per = ceil(HW / 64) pixels per chunk), 6 shuffle steps fold a wave, 2 additions fold the four waves; the final kernel adds
    the 64 partial sums serially.  The error of such a sum is at most depth * 2^-24 of sum |terms| (first order)."""
    per = (H * W + SIG_CHUNKS - 1) // SIG_CHUNKS
    serial = (per + 255) // 256
    return serial + 6 + 2, serial + 6 + 2 + 64


# ---------------------------------------------------------------------------------------------------------------------------------
# gradient scale

GSCALE_N = (3, 17, 23)         # B, H, W of the probe call: 1173 values


def _gs_base(name):
    return 0.4 * (2 * torch.rand(GSCALE_N[0] * GSCALE_N[1] * GSCALE_N[2], generator=_gen(name)) - 1)


def gscale_cases():
    """{name: fp32 values}: max |g| an exact power of two (2^-20, 1, 2^7; placed with either sign), all zeros, one inf, one NaN, a denormal max."""
    out = {}
    for k in (-20, 0, 7):
        x = _gs_base(f"gs_pow{k}") * 2.0 ** k
        x[777] = -(2.0 ** k)
        out[f"gs_pow{k}"] = x
    out["gs_generic"] = _gs_base("gs_generic") * 3.0
    out["gs_zeros"] = torch.zeros_like(_gs_base("z"))
    out["gs_zeros"][5] = -0.0
    x = _gs_base("gs_inf")
    x[100] = float("-inf")
    out["gs_inf"] = x
    x = _gs_base("gs_nan")
    x[100] = float("nan")
    out["gs_nan"] = x
    x = torch.zeros_like(_gs_base("z"))
    x[3], x[900] = 2.0 ** -140, -3 * 2.0 ** -141
    out["gs_denormal"] = x
    return out


def gscale_expected(x):
    """(bits of max |g|, 1 / m, m) as absmax_kernel + grad_scale_kernel define them: fmaxf drops a NaN, so the maximum is that of the other
    values; 0 -> {0, 0}; inf -> {1, 1}; else m = 2^e from frexp (max = f 2^e, f in [0.5, 1)), e no lower than -126 so that 1 / m is finite."""
    a = np.abs(x.numpy())
    mx = np.float32(np.fmax.reduce(a, initial=np.float32(0)))
    bits = int(mx.view(np.uint32))
    if mx == 0:
        return bits, np.float32(0), np.float32(0)
    if not np.isfinite(mx):
        return bits, np.float32(1), np.float32(1)
    _, e = np.frexp(mx)
    e = max(int(e), -126)
    return bits, np.ldexp(np.float32(1), -e), np.ldexp(np.float32(1), e)


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
    """{"ups_f32" | "ups_hs": (largest tier-(b) measure of the fp32 emulation over UPS_CASES, case), "adjoint": (largest adjoint gap of the
    fp32 emulations of the two sides over UPS_ADJOINT_CASES, case)}."""
    def run():
        out = {}
        for fam, key in ((0, "ups_f32"), (1, "ups_hs")):
            worst, where = 0.0, None
            for c in UPS_CASES:
                d = ups_inputs(c.name, fam)
                e = measure(ups_emulate32(c, d, fam), ups_reference_b(c, d), ups_reference_a(c, d)[1])
                if e > worst:
                    worst, where = e, c.name
            out[key] = (worst, where)
        worst, where = 0.0, None
        for c in UPS_ADJOINT_CASES:
            d = ups_inputs(c.name, 0, True)
            x = adjoint_x(c)
            e = adjoint_gap(ups_forward_emulate32(x), d["g"], x, ups_emulate32(c, d))
            if e > worst:
                worst, where = e, c.name
        out["adjoint"] = (worst, where)
        return out
    return _one_thread(run)


@functools.lru_cache(maxsize=None)
def adjoint_x(c):
    return torch.randn(c.B, c.C, c.h, c.w, generator=_gen(c.name + "/x"))


BAR_KEYS = ("ups_f32", "ups_hs", "adjoint")


def recorded_bars():
    """{key: (emulation maximum, bar)} as profiles/vjp_glue_probe.md records them (table rows `| key | max | bar | ...`)."""
    out = {}
    for line in open(PROFILE_NOTE):
        m = re.match(r"\|\s*(ups_f32|ups_hs|adjoint)\s*\|\s*([0-9.eE+-]+)\s*\|\s*([0-9.eE+-]+)\s*\|", line)
        if m:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    assert set(out) == set(BAR_KEYS), f"{PROFILE_NOTE}: bars of {sorted(set(BAR_KEYS) - set(out))} missing"
    return out


def bar(key):
    return recorded_bars()[key][1]
