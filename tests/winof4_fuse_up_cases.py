"""Cases of the F(4x4,3x3) kernel's up-sampling instance (probe kind PNPX_PROBE_WINOF4_FUSE_UP, csrc/conv3x3_winof4.hip) and a CPU
restatement of how it interpolates -- per 16 x 32 region a low-resolution window, per-row and per-column tables (first tap, weights, CLAMPED
second tap) and the separate up-sampling kernel's rounding sequence -- next to a restatement of that kernel itself, so that the equality
the GPU test asserts between the two forms can be shown to fail for the ways the window form goes wrong.  tests/winof4_entry_cases.py
and tests/conv_layer_cases.py supply cases, inputs, references, the measure and the bar.  No GPU."""
import functools

import numpy as np
import torch

from tests import conv_layer_cases as CL
from tests import winof4_entry_cases as EC

FUSE_UP = 11                               # include/pnpx.h: PNPX_PROBE_WINOF4_FUSE_UP (9 stays reserved, 10 is no kind)
MIN_C0 = 16                                # conv3x3_winof4_ups_ok: the pipeline gathers two chunks of the first source per tile
SR, SC = 11, 20                            # rows and columns of the staging window (csrc/conv3x3_winof4.hip CfgF4)

# The three entry cases and 1 x (16+16) -> 64 at 48 x 96: 3 x 3 regions, so one region touches no image border, and the window origins
# (7 and 15 source rows / columns apart) are of both parities.  The pipeline's minimum of first-source chunks is 2: C0 = 16 stays.
CASES = EC.ENTRY_CASES + ((1, CL._c("ups", 16, 16, 64, 48, 96)),)


@functools.lru_cache(maxsize=None)
def inputs(i):
    """fp32 operands of case i at EC.B_ALL images; in1 is the low-resolution second source.  Never modified by the callers."""
    if i < len(EC.ENTRY_CASES):
        return EC.inputs(i)
    _, c = CASES[i]
    rs = np.random.RandomState(4300 + 13 * i)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    cin = c.C0 + c.C1
    return {"w": t(rs.standard_normal((c.cout, cin, 3, 3)) / np.sqrt(9.0 * cin)), "bias": t(0.1 * rs.standard_normal(c.cout)),
            "in0": t(rs.standard_normal((EC.B_ALL, c.C0, c.H, c.W))), "in1": t(rs.standard_normal((EC.B_ALL, c.C1, c.H // 2, c.W // 2)))}


@functools.lru_cache(maxsize=None)
def case_reference(i):
    """(ref, denom) in float64 from the low-resolution operands."""
    return EC.case_reference(i) if i < len(EC.ENTRY_CASES) else CL.reference(CASES[i][1], inputs(i))


def ups_ok(C0, C1, cout, H, W):
    """conv3x3_winof4_ups_ok restated: the entry rules and two chunks of the first source."""
    return (cout % 64 == 0 and H >= 16 and H % 16 == 0 and W >= 32 and W % 32 == 0 and C0 >= MIN_C0 and C0 % 8 == 0
            and C1 >= 8 and C1 % 8 == 0)


# ------------------------------------------------------------------------------------------------ the two forms of the up-sampling, in fp32

def _fma(a, b, c):
    """fp32 fma of arrays: the product of two fp32 numbers is exact in float64 (48 bits)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _blend(hy, ly, hx, lx, v00, v01, v10, v11):
    """upsample2x_v4_kernel's rounding sequence: the products with l round on their own, the products with h are fused into them."""
    with np.errstate(invalid="ignore"):      # (0 x inf where a mutant reads a border the test made infinite)
        top = _fma(hx, v00, (lx * v01).astype(np.float32))
        bot = _fma(hx, v10, (lx * v11).astype(np.float32))
        return _fma(hy, top, (ly * bot).astype(np.float32))


def _axis(n_out, n_in, clamp=True):
    """(i0, i1, l, h) of every output index: f = s * index, i0 = (int) f, l = f - i0, h = 1 - l, i1 = i0 + (i0 < n - 1)."""
    s = np.float32(n_in - 1) / np.float32(n_out - 1)
    f = (s * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = f.astype(np.int64)
    l = (f - i0.astype(np.float32)).astype(np.float32)
    i1 = i0 + (i0 < n_in - 1) if clamp else i0 + 1
    return i0, i1, l, (np.float32(1) - l).astype(np.float32)


def upsample_separate(low):
    """What the separate up-sampling kernel writes: [.., h, w] -> [.., 2h, 2w], one pixel at a time from the whole plane."""
    low = np.asarray(low, dtype=np.float32)
    h, w = low.shape[-2:]
    y0, y1, ly, hy = _axis(2 * h, h)
    x0, x1, lx, hx = _axis(2 * w, w)
    g = lambda ys, xs: low[..., ys[:, None], xs[None, :]]
    return _blend(hy[:, None], ly[:, None], hx[None, :], lx[None, :], g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1))


def upsample_windowed(low, mutant=None, border=0.0):
    """What the kernel's up-sampling instance puts into its halo buffers, region by region (16 x 32 output pixels + a halo of one):
    a window of SR x SC source pixels whose origin is the first tap of the first halo row / column inside the image (pulled back to stay
    in the padded plane), tables per halo row and column, zero outside the image.  Returns the up-sampled image assembled from the
    regions' interiors and checks that every region's halo agrees with its neighbours'.
    mutant: "origin" (window one column to the right of where the tables think it is), "unclamped" (second tap i0 + 1 always, as the
    8-wave kernel's tables have it), "swapped" (h and l exchanged).  border: what the padded tensor's border cells hold (the layout's
    contract is zero; the interpolation must not depend on it)."""
    low = np.asarray(low, dtype=np.float32)
    h, w = low.shape[-2:]
    H, W = 2 * h, 2 * w
    assert H % 16 == 0 and W % 32 == 0
    y0, y1, ly, hy = _axis(H, h, clamp=mutant != "unclamped")
    x0, x1, lx, hx = _axis(W, w, clamp=mutant != "unclamped")
    if mutant == "swapped":
        ly, hy, lx, hx = hy, ly, hx, lx
    padded = np.full(low.shape[:-2] + (h + 2, w + 2 * CL.PADL), border, np.float32)   # the padded planar tensor the window is cut from
    padded[..., 1:-1, CL.PADL:-CL.PADL] = low
    out = np.zeros(low.shape[:-2] + (H + 2, W + 2), np.float32)                   # with the convolution's zero padding around it
    for ty in range(H // 16):
        for tx in range(W // 32):
            gy = np.arange(16 * ty - 1, 16 * ty + 17)
            gx = np.arange(32 * tx - 1, 32 * tx + 33)
            vy, vx = (gy >= 0) & (gy < H), (gx >= 0) & (gx < W)
            rs = min(int(y0[max(16 * ty - 1, 0)]) + 1, max(h + 2 - SR, 0))
            cs = min(int(x0[max(32 * tx - 1, 0)]) + CL.PADL, w + 2 * CL.PADL - SC)
            rows = np.minimum(rs + np.arange(SR), h + 1)                          # a plane of fewer than SR rows repeats its last one
            win = padded[..., rows[:, None], (cs + (1 if mutant == "origin" else 0) + np.arange(SC))[None, :] % (w + 2 * CL.PADL)]
            cy, cx = np.clip(gy, 0, H - 1), np.clip(gx, 0, W - 1)
            r0, r1, c0, c1 = y0[cy] + 1 - rs, y1[cy] + 1 - rs, x0[cx] + CL.PADL - cs, x1[cx] + CL.PADL - cs
            assert r0.min() >= 0 and r1.max() < SR and c0.min() >= 0 and c1.max() < SC, "a tap outside the staging window"
            g = lambda r, c: win[..., r[:, None], c[None, :]]
            v = _blend(hy[cy][:, None], ly[cy][:, None], hx[cx][None, :], lx[cx][None, :], g(r0, c0), g(r0, c1), g(r1, c0), g(r1, c1))
            v = np.where(vy[:, None] & vx[None, :], v, np.float32(0))
            dst = out[..., 16 * ty:16 * ty + 18, 32 * tx:32 * tx + 34]
            seen = dst != 0
            assert (dst[seen].view(np.int32) == v[seen].view(np.int32)).all(), "two regions disagree about a shared halo pixel"
            dst[...] = v
    return out[..., 1:-1, 1:-1]


def window_corners(H, W):
    """Low-resolution (y, x) of the first and last source pixel every region's halo taps, the image's last row and column included."""
    h, w = H // 2, W // 2
    y0, y1, _, _ = _axis(H, h)
    x0, x1, _, _ = _axis(W, w)
    ys, xs = set(), set()
    for ty in range(H // 16):
        ys |= {int(y0[max(16 * ty - 1, 0)]), int(y1[min(16 * ty + 16, H - 1)])}
    for tx in range(W // 32):
        xs |= {int(x0[max(32 * tx - 1, 0)]), int(x1[min(32 * tx + 32, W - 1)])}
    return sorted(ys | {h - 1}), sorted(xs | {w - 1})
