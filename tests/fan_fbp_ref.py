"""Fan-beam filtered backprojection and the CT iADMM / PG loops restated in torch / numpy on top of tests/fanbeam_ref.py, independent
of the native side (nothing here imports tfpnp_amd's library bindings).  Kak & Slaney section 3.4.2, equispaced flat detector, full circle:
  * filter, per sinogram row:  r[m] = p[m] c[m],  q[j] = S * sum over m ascending of r[m] h[j - m],
    h[0] = 1/4, h[odd n] = -1 / (pi n)^2, h[even n != 0] = 0 (even lags are skipped, not multiplied by zero);
    fan: c[m] = cos gamma_m (the bin table's first column), S = pi / (V dp), dp = du D_so / D; parallel (geometry None): c = 1, S = pi / V;
  * backprojection: the position of fanbeam_ref.fan_backprojection, the weight w = (D_so / U)^2; views summed in order.
dtype float32 keeps the kernels' operation order, one rounding per operation: the taps are -1 / ((pi n) (pi n)) from the fp32 pi, the
sum runs over m ascending with the centre tap in its place, S is computed in double, rounded once and applied last.  dtype float64
is the same definition with exact taps and the unrounded D."""
import math

import numpy as np
import torch

from tests import fanbeam_ref as F
from tests.golden_inputs import ellipse_phantom

WIDE = (2, 64, 3, 2.0, 2.0, 1500, 0.1)      # a row of 1500 bins: more bins than a workgroup has threads (geometry(64, 3, 128, 128, 1500, 0.1))

# exact-chord reconstructions at 128^2, 360 views: (D_so, D_od) / R, ellipses of the phantom (also its seed), raster sub-sampling
CHORD_CASES = [(2.0, 2.0, 1, 4), (1.5, 0.5, 1, 4), (2.0, 2.0, 5, 2), (1.5, 0.5, 5, 2)]
# rel-L2 of the float64 restatement's FBP from the rastered phantom, measured on the CPU when this was committed (profiles/fan_fbp.md):
# what a ramp-filtered reconstruction loses at the sharp edges of ellipses of 6 .. 25 pixels; scales 0.9944 .. 0.9950
CHORD_REL_L2 = {(2.0, 2.0, 1): 5.503e-2, (1.5, 0.5, 1): 5.728e-2, (2.0, 2.0, 5): 4.946e-2, (1.5, 0.5, 5): 5.092e-2}


def chord_case(a, b, n, ss, R=128, V=360):
    """-> (geometry, rastered phantom [R,R] float64, exact fan sinogram [1,1,V,det] float64)."""
    g = F.geometry(R, V, a * R, b * R)
    ells = ellipse_phantom.make(n, n=n, R=R)
    return g, ellipse_phantom.raster(ells, R, ss=ss).astype(np.float64), F.ellipse_fan_sinogram(ells, g)[None, None]


def all_cases():
    return list(F.CASES) + [WIDE]


def filter_scale(g, V, dtype):
    """S: pi / V for the parallel beam (g None), pi / (V dp) for a fan; float32: from the fp32 D, rounded once."""
    if g is None:
        s = math.pi / V
    else:
        D = float(np.float32(g.source_distance + g.det_distance)) if dtype == torch.float32 else g.source_distance + g.det_distance
        s = math.pi / (V * (g.det_spacing * g.source_distance / D))
    return float(np.float32(s)) if dtype == torch.float32 else s


def taps(det, dtype):
    """h[1], h[3], ...: det // 2 values; float32 as the kernel forms them."""
    n = 2 * np.arange(det // 2) + 1
    if dtype == torch.float32:
        pn = np.float32(math.pi) * n.astype(np.float32)
        return np.float32(-1.0) / (pn * pn)
    return -1.0 / (math.pi * n) ** 2


def fan_filter(sino, g, dtype=torch.float32):
    """sino [B,1,V,det] -> the pre-weighted, ramp-filtered and scaled sinogram, same shape, in `dtype`.  g None: parallel beam."""
    sino = torch.as_tensor(sino).to(dtype)
    B, _, V, det = sino.shape
    r = sino.reshape(B * V, det)
    if g is not None:
        c = torch.from_numpy(F.bin_table(g, np.float32 if dtype == torch.float32 else np.float64)[:, 0].copy())
        r = r * c[None]
    t = torch.from_numpy(np.ascontiguousarray(taps(det, dtype)))
    j = torch.arange(det)
    S = filter_scale(g, V, dtype)
    if dtype != torch.float32:                        # the definition as one matrix
        lag = (j[:, None] - j[None, :]).abs()
        H = torch.where(lag % 2 == 1, t[(lag // 2).clamp(max=max(det // 2 - 1, 0))], torch.zeros((), dtype=dtype))
        H = H + 0.25 * torch.eye(det, dtype=dtype)
        return (S * (r @ H.T)).reshape(B, 1, V, det)
    acc = torch.zeros(B * V, det, dtype=dtype)
    for m in range(det):                              # the kernel's order: m ascending, the centre tap where m == j
        lag = (j - m).abs()
        h = torch.where(lag == 0, torch.tensor(0.25, dtype=dtype), t[(lag // 2).clamp(max=max(det // 2 - 1, 0))])
        acc = torch.where(((lag % 2 == 1) | (lag == 0))[None], acc + r[:, m:m + 1] * h[None], acc)
    return (acc * S).reshape(B, 1, V, det)


def fan_backprojection_fbp(sino, g, dtype=torch.float32):
    """fanbeam_ref.fan_backprojection with the weight of filtered backprojection, w = (D_so / U)^2."""
    sino = torch.as_tensor(sino).to(dtype)
    B, _, V, det = sino.shape
    R = g.R
    cs = F.view_table(V)
    dso, du = g.source_distance, g.det_spacing
    D = float(np.float32(dso + g.det_distance)) if dtype == torch.float32 else dso + g.det_distance
    c0 = torch.arange(R, dtype=dtype) - (R / 2 - 0.5)
    ys, xs = torch.meshgrid(c0, c0, indexing="ij")
    half = det / 2 - 0.5
    out = torch.zeros(B, 1, R, R, dtype=dtype)
    for v in range(V):
        cb, sb = float(cs[v, 0]), float(cs[v, 1])
        s = xs * cb + ys * sb
        t = ys * cb - xs * sb
        U = dso + t
        u = (s * D) / U
        pos = u / du + half
        f0 = torch.floor(pos)
        f = pos - f0
        s0 = f0.long()
        row = sino[:, 0, v]
        r0 = row[:, s0.clamp(0, det - 1)] * ((s0 >= 0) & (s0 < det))[None]
        r1 = row[:, (s0 + 1).clamp(0, det - 1)] * ((s0 + 1 >= 0) & (s0 + 1 < det))[None]
        m = dso / U
        out[:, 0] = out[:, 0] + (m * m)[None] * (r0 * (1 - f)[None] + r1 * f[None])
    return out


def fan_fbp(sino, g, dtype=torch.float32):
    return fan_backprojection_fbp(fan_filter(sino, g, dtype), g, dtype)


def fft_filter64(sino):
    """Radon_norm.filter_sinogram restated in numpy float64: zero-pad to L = max(64, next power of two >= 2 det), multiply the
    spectrum by the ramp's response 2 Re FFT(f) (the float32 table of utils.transforms.ramp_filter, as the product uses it),
    invert, crop, scale by pi / (2 V)."""
    y = np.asarray(sino, np.float64)
    V, det = y.shape[-2:]
    L = max(64, 1 << int(np.ceil(np.log2(2 * det))))
    n = np.concatenate((np.arange(1, L // 2 + 1, 2), np.arange(L // 2 - 1, 0, -2)))
    f = np.zeros(L)
    f[0] = 0.25
    f[1::2] = -1.0 / (np.pi * n) ** 2
    resp = (2 * np.real(np.fft.fft(f))).astype(np.float32).astype(np.float64)
    pad = np.zeros(y.shape[:-1] + (L,))
    pad[..., :det] = y
    return np.real(np.fft.ifft(np.fft.fft(pad, axis=-1) * resp, axis=-1))[..., :det] * (np.pi / (2 * V))


def ct_iadmm(den, A, AT, variables, y0, opnorm, sigma_d, mu, tau, iter_num=None):
    """oracle.pnp_oracle.ct_iadmm (tasks/ct/solver.py:17-53) on a passed-in denoiser den(x, sigma) and projector pair A, AT,
    operation for operation."""
    x, z, u = torch.split(variables, variables.shape[1] // 3, dim=1)
    B = x.shape[0]
    T = sigma_d.shape[-1] if iter_num is None else iter_num
    for i in range(T):
        x = den(z - u, sigma_d[:, i])
        _tau = tau[:, i].view(B, 1, 1, 1)
        _mu = mu[:, i].view(B, 1, 1, 1)
        g = AT(A(z) - y0) / opnorm ** 2
        z = z - _tau * (g + _mu * (z - (x + u)))
        u = u + x - z
    return torch.cat([x, z, u], dim=1)


def ct_pg(den, A, AT, variables, y0, opnorm, sigma_d, tau, iter_num=None):
    """oracle.pnp_oracle.ct_pg (tasks/ct/solver.py:61-87) on a passed-in denoiser and projector pair, operation for operation."""
    x = variables
    B = x.shape[0]
    T = sigma_d.shape[-1] if iter_num is None else iter_num
    for i in range(T):
        _tau = tau[:, i].view(B, 1, 1, 1)
        z = x - _tau * AT(A(x) - y0) / opnorm ** 2
        x = den(z, sigma_d[:, i])
    return x


def lsq_scale(rec, gt):
    rec, gt = np.asarray(rec, np.float64), np.asarray(gt, np.float64)
    return float((rec * gt).sum() / (gt * gt).sum())
