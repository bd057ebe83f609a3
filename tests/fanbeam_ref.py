"""The fan-beam Radon pair and the CT HQS loop restated in torch / numpy, independent of the native side (nothing here imports
tfpnp_amd's library bindings).  Geometry, in centred pixel units (x = column - (R/2 - 0.5), y = row - (R/2 - 0.5)),
e_s(b) = (cos b, sin b), e_t(b) = (-sin b, cos b):
  * view angles beta_v = 2 pi v / V, computed in double and rounded to fp32; cos / sin taken in double of that fp32 angle and rounded;
  * source at -D_so e_t, bin j centred at D_od e_t + u_j e_s, u_j = (j - det/2 + 0.5) du, D = D_so + D_od,
    L_j = sqrt(D^2 + u_j^2), cos gamma_j = D / L_j, sin gamma_j = u_j / L_j;
  * forward: ray (v, j) is the parallel ray of angle theta = beta_v - gamma_j and offset s = D_so sin gamma_j, sampled at
    p_k = s (cos theta, sin theta) + t_k (-sin theta, cos theta), t_k = k - n/2 + 0.5, k < n = ceil(sqrt 2 R); bilinear, zero outside;
  * backprojection: s = x cos b + y sin b, t = -x sin b + y cos b, U = D_so + t, u = s D / U, linear interpolation at bin
    u / du + det/2 - 0.5 (zero outside), times w = sqrt(D^2 + u^2) / (U du); views summed in order.
dtype float32 keeps the kernels' operation order (one rounding per operation; torch on the CPU does not contract); dtype float64 is
the same geometry with the bin table and D left unrounded (only the view table is fp32 by definition).
D_so, D_od and du are the float32 values the native entries receive."""
import math
from collections import namedtuple

import numpy as np
import torch

Geom = namedtuple("Geom", "R n_view det_count source_distance det_distance det_spacing")


def n_steps(R):
    return int(math.ceil(math.sqrt(2.0) * R))


def default_det_count(R, dso, dod, du):
    n = n_steps(R)
    return int(math.ceil(2.0 * (dso + dod) * math.tan(math.asin((n / 2.0) / dso)) / du))


def geometry(R, V, source_distance, det_distance=None, det_count=None, det_spacing=None):
    """Defaults: det_distance = source_distance, det_spacing = D / source_distance, det_count = the fan covering the sampled circle."""
    f32 = lambda v: float(np.float32(v))
    dso = f32(source_distance)
    dod = dso if det_distance is None else f32(det_distance)
    du = f32((dso + dod) / dso) if det_spacing is None else f32(det_spacing)
    det = default_det_count(R, dso, dod, du) if det_count is None else int(det_count)
    return Geom(int(R), int(V), det, dso, dod, du)


def view_table(V):
    """[V, 2] float32 (cos, sin) of the fp32-rounded angles."""
    out = np.zeros((V, 2), np.float32)
    for v in range(V):
        a = float(np.float32((2.0 * math.pi * v) / V))
        out[v] = (np.float32(math.cos(a)), np.float32(math.sin(a)))
    return out


def bin_table(g, dtype=np.float32):
    """[det, 3] (cos gamma, sin gamma, D_so sin gamma), computed in double; float32: D rounded first, as the kernels receive it."""
    D = float(np.float32(g.source_distance + g.det_distance)) if dtype == np.float32 else g.source_distance + g.det_distance
    u = (np.arange(g.det_count, dtype=np.float64) - g.det_count / 2.0 + 0.5) * g.det_spacing
    L = np.sqrt(D * D + u * u)
    return np.stack([D / L, u / L, g.source_distance * (u / L)], 1).astype(dtype)


def ray_table(g):
    """float64 (theta, s) of every ray, [V, det] each: the parallel ray a fan ray is."""
    cs = view_table(g.n_view).astype(np.float64)
    beta = np.arctan2(cs[:, 1], cs[:, 0])
    bt = bin_table(g, np.float64)
    gamma = np.arctan2(bt[:, 1], bt[:, 0])
    return beta[:, None] - gamma[None, :], np.broadcast_to(bt[None, :, 2], (g.n_view, g.det_count))


def fan_forward(img, g, dtype=torch.float32):
    """img [B,1,R,R] -> [B,1,V,det] in `dtype`."""
    img = torch.as_tensor(img).to(dtype)
    B, _, R, _ = img.shape
    n, off = n_steps(R), R / 2 - 0.5
    cs = view_table(g.n_view)
    bt = torch.from_numpy(bin_table(g, np.float32 if dtype == torch.float32 else np.float64))
    cg, sg, so = bt[:, 0], bt[:, 1], bt[:, 2]
    t = (torch.arange(n, dtype=dtype) - n / 2 + 0.5)[None, :]
    flat = img[:, 0].reshape(B, R * R)
    out = torch.zeros(B, 1, g.n_view, g.det_count, dtype=dtype)

    def tap(xi, yi):
        ok = (xi >= 0) & (xi < R) & (yi >= 0) & (yi < R)
        return flat[:, (yi.clamp(0, R - 1) * R + xi.clamp(0, R - 1)).long()] * ok[None]

    for v in range(g.n_view):
        cb, sb = float(cs[v, 0]), float(cs[v, 1])
        c = cb * cg + sb * sg                       # cos(beta - gamma)
        sn = sb * cg - cb * sg                      # sin(beta - gamma)
        sc, ss = so * c, so * sn
        px = (sc[:, None] - t * sn[:, None]) + off
        py = (ss[:, None] + t * c[:, None]) + off
        x0, y0 = torch.floor(px), torch.floor(py)
        fx, fy = px - x0, py - y0
        xi, yi = x0.long(), y0.long()
        v00, v01, v10, v11 = tap(xi, yi), tap(xi + 1, yi), tap(xi, yi + 1), tap(xi + 1, yi + 1)      # v[dy][dx]
        # the kernel interpolates along the copy's columns first: x for a plain ray, y for a ray that reads the transposed copy
        top = v00 + fx * (v01 - v00)
        bot = v10 + fx * (v11 - v10)
        plain = top + fy * (bot - top)
        lft = v00 + fy * (v10 - v00)
        rgt = v01 + fy * (v11 - v01)
        trans = lft + fx * (rgt - lft)
        tr = (sn.abs() > c.abs())[None, :, None]
        out[:, 0, v] = torch.where(tr, trans, plain).sum(-1)
    return out


def fan_backprojection(sino, g, dtype=torch.float32, weight=True):
    """sino [B,1,V,det] -> [B,1,R,R] in `dtype`; weight False: the unweighted pixel-driven sum (for the adjoint test's contrast)."""
    sino = torch.as_tensor(sino).to(dtype)
    B, _, V, det = sino.shape
    R = g.R
    cs = view_table(V)
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
        val = r0 * (1 - f)[None] + r1 * f[None]
        if weight:
            w = torch.sqrt(D * D + u * u) / (U * du)
            val = w[None] * val
        out[:, 0] = out[:, 0] + val
    return out


def view_projection(g, cb, sb, x, y):
    """float64: (bin position, weight w) of the points (x, y), in centred pixel units, under the view (cos beta, sin beta)."""
    D = g.source_distance + g.det_distance
    s = x * cb + y * sb
    U = g.source_distance + (y * cb - x * sb)
    u = s * D / U
    return u / g.det_spacing + g.det_count / 2 - 0.5, np.sqrt(D * D + u * u) / (U * g.det_spacing)


def pixel_projection(g, x, y):
    """float64, per view: (bin position, weight w) of the one point (x, y)."""
    cs = view_table(g.n_view).astype(np.float64)
    return view_projection(g, cs[:, 0], cs[:, 1], x, y)


def ellipse_fan_sinogram(ells, g):
    """Exact fan sinogram [V, det] float64 of an ellipse phantom (tests.golden_inputs.ellipse_phantom): the chord of each ray
    from its (theta, s)."""
    th, s = ray_table(g)
    out = np.zeros(th.shape, np.float64)
    for e in ells:
        r2 = (e["a"] * np.cos(th - e["phi"])) ** 2 + (e["b"] * np.sin(th - e["phi"])) ** 2
        tt = s - (e["cx"] * np.cos(th) + e["cy"] * np.sin(th))
        out += e["rho"] * 2 * e["a"] * e["b"] * np.sqrt(np.maximum(r2 - tt ** 2, 0.0)) / r2
    return out


def ct_hqs(den, A, AT, variables, y0, opnorm, sigma_d, mu, iter_num=None):
    """HQS for CT on a passed-in denoiser den(x, sigma) and projector pair A, AT: state cat(x, z);
    x = D(z, sigma_d_i);  z <- z - (AT(A z - y0) / opnorm^2 + mu_i (z - x)) / (1 + mu_i)."""
    x, z = torch.split(variables, 1, dim=1)
    B = x.shape[0]
    T = sigma_d.shape[-1] if iter_num is None else iter_num
    for i in range(T):
        x = den(z, sigma_d[:, i])
        m = mu[:, i].view(B, 1, 1, 1)
        g = AT(A(z) - y0) / opnorm ** 2
        z = z - (g + m * (z - x)) / (1 + m)
    return torch.cat([x, z], dim=1)


def loud_sinogram(B, V, det, seed):
    """Random sinogram with loud first / last bins and first / last views: an addressing mistake at an edge shows."""
    y = np.random.RandomState(seed).standard_normal((B, 1, V, det)).astype(np.float32)
    y[..., :2], y[..., -2:] = 5.0, -3.0
    y[:, :, 0, 2:-2] = 7.0
    if V > 1:
        y[:, :, -1, 2:-2] = -2.0
    return y


# (B, R, V, D_so / R, D_od / R, det_count, det_spacing): the cases of tests/test_gpu_fanbeam.py, whose fp32-vs-float64 distances
# tests/test_fanbeam_host.py measures on the CPU (profiles/fanbeam.md)
CASES = [(3, 100, 17, 1.0, 1.0, None, None),
         (9, 64, 8, 0.8, 0.4, None, None),        # B > 8 (XCD dealing), close source: wide LDS window
         (1, 97, 5, 4.0, 0.0, None, None),        # odd size, detector through the isocentre
         (2, 33, 1, 2.0, 2.0, None, None),
         (2, 48, 6, 1.5, 0.5, 45, 1.7)]           # explicit det_count (no multiple of 8; corner pixels project outside), du != D / D_so


def case_geometry(case):
    B, R, V, a, b, det, du = case
    return geometry(R, V, a * R, b * R, det, du)


def case_image(case):
    B, R = case[0], case[1]
    rs = np.random.RandomState(7000 + R)
    img = rs.uniform(0, 1, (B, 1, R, R)).astype(np.float32)
    img[:, :, 0, :], img[:, :, -1, :], img[:, :, :, 0], img[:, :, :, -1] = 3.0, -2.0, 4.0, -1.0      # loud border rows / columns
    return img


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())
