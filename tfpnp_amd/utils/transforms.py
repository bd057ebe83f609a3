"""Mirror of the hot-path part of tfpnp/utils/transforms.py (same function names and argument meaning).

Layout helpers (real2complex ...) are plain tensor views/stacks -- pure data movement, exactly as in the
reference.  Everything that computes (fft2, ifft2, cdp_*, spi_inverse, Radon) is a libpnpx.so call.
"""
import collections

import numpy as np
import torch

from .. import ops
from .. import torch_ops as T


def real2complex(x):
    """transforms.py:12-13"""
    return torch.stack([x, torch.zeros_like(x)], dim=4)


def complex2real(x):
    """transforms.py:16-17"""
    return x[..., 0]


def complex2channel(x):
    """transforms.py:20-26"""
    N, C, H, W, _ = x.shape
    return x.permute(0, 1, 4, 2, 3).contiguous().view(N, C * 2, H, W)


def fft2(data):
    """Centered orthonormal 2-D FFT over dims (-3,-2) of [...,H,W,2].  transforms.py:68-84"""
    assert data.size(-1) == 2
    return T.call("fft2", data, False, True)


def ifft2(data):
    """transforms.py:87-103"""
    assert data.size(-1) == 2
    return T.call("fft2", data, True, True)


def complex_abs(data):
    """transforms.py:106-118 (layout glue used outside the solver loops)."""
    assert data.size(-1) == 2
    return (data ** 2).sum(dim=-1).sqrt()


def complex_mul(x1, x2):
    """transforms.py:260-270"""
    assert x1.size(-1) == 2 and x2.size(-1) == 2
    return torch.stack((x1[..., 0] * x2[..., 0] - x1[..., 1] * x2[..., 1],
                        x1[..., 0] * x2[..., 1] + x1[..., 1] * x2[..., 0]), -1)


def conjugate(x):
    """transforms.py:273-274"""
    return torch.stack([x[..., 0], -x[..., 1]], -1)


def cdp_forward(data, mask):
    """transforms.py:282-301"""
    assert mask.size(-1) == 2
    return T.call("cdp_forward", data, mask)


def cdp_backward(data, mask):
    """transforms.py:304-320"""
    assert mask.size(-1) == 2
    return T.call("cdp_backward", data, mask)


def spi_inverse(ztilde, K1, K, mu):
    """transforms.py:404-439"""
    return T.call("spi_inverse", ztilde, K1, K, mu)


def spi_pg_step(x, x0, K, tau):
    """One gradient step of PGSolver_SPI on the likelihood behind spi_inverse, without the denoiser (no counterpart in the
    reference; include/pnpx.h pnpx_spi_pg_step).  x, x0 [B,1,H,W]; K = the K / 10 map of the solver state; tau per item."""
    return T.call("spi_pg_step", x, x0, K, tau)


# ------------------------------------------------------------------------------------------------ CT
class Radon_norm:
    """Stands in for transforms.py:465-484 (a torch_radon.Radon subclass): parallel beam,
    angles = linspace(0, 179/180*pi, view), det_count = ceil(sqrt(2)*resolution) (transforms.py:487-491).
    torch_radon is CUDA-only and absent; the discretisation is this project's own."""

    def __init__(self, resolution, view, opnorm=None, device=None, seed=0):
        self.resolution = resolution
        self.view = view
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if opnorm is None:
            # power_method_opnorm (transforms.py:447-462); seeded start vector instead of an unseeded randn
            x = torch.from_numpy(np.random.RandomState(seed).standard_normal((1, 1, resolution, resolution))
                                 .astype(np.float32)).to(self.device)
            x = x / x.norm()
            v = 1.0
            for _ in range(10):
                nx = self.backprojection(self.forward(x))
                v = float(nx.norm())
                x = nx / v
            opnorm = v ** 0.5
        self.opnorm = opnorm

    def forward(self, x):
        return T.call("radon_forward", x, int(self.view))

    def backprojection(self, sinogram):
        return T.call("radon_backprojection", sinogram, int(self.resolution))

    backward = backprojection

    def backprojection_norm(self, sinogram):
        return self.backprojection(sinogram) / self.opnorm ** 2

    def normal_operator(self, x):
        return self.backprojection_norm(self.forward(x))

    def filter_sinogram(self, sinogram, filter_name='ramp'):
        """Ramp-filter every projection along the detector axis (torch_radon.Radon.filter_sinogram as used by
        transforms.py:479-481): zero-pad to max(64, next power of two >= 2*det), multiply the spectrum by the
        Kak-Slaney ramp (the DFT of the band-limited spatial kernel, not |f|), crop, scale by pi / (2 * n_views).
        The 1-D FFTs are native (H = 1 images)."""
        if filter_name != 'ramp':
            raise NotImplementedError(filter_name)
        B, C, V, D = sinogram.shape
        L = max(64, 1 << int(np.ceil(np.log2(2 * D))))
        x = torch.zeros(B * C * V, 1, L, 2, device=sinogram.device, dtype=torch.float32)
        x[:, 0, :D, 0] = sinogram.reshape(-1, D)
        spec = T.call("fft2", x, False, False)
        filt = torch.from_numpy(ramp_filter(L)).to(sinogram.device)
        out = T.call("fft2", spec * filt.view(1, 1, L, 1), True, False)
        return (out[:, 0, :D, 0] * (np.pi / (2 * V))).reshape(B, C, V, D).contiguous()

    def filter_backprojection(self, sinogram):
        """transforms.py:479-481"""
        return self.backprojection(self.filter_sinogram(sinogram, filter_name='ramp'))

    fbp = filter_backprojection      # one name for both geometries (FanBeam_norm.fbp)


def ramp_filter(size):
    """Frequency response of the discrete ramp filter (Kak & Slaney eq. 61; the construction skimage / torch_radon
    use): spatial kernel f[0] = 1/4, f[odd n] = -1/(pi n)^2, response = 2 Re FFT(f).  float32 [size]."""
    n = np.concatenate((np.arange(1, size // 2 + 1, 2), np.arange(size // 2 - 1, 0, -2)))
    f = np.zeros(size)
    f[0] = 0.25
    f[1::2] = -1.0 / (np.pi * n) ** 2
    return (2 * np.real(np.fft.fft(f))).astype(np.float32)


FanGeometry = collections.namedtuple("FanGeometry", "n_view det_count source_distance det_distance det_spacing")


class FanBeam:
    """A fan-beam geometry (flat detector, full circle; include/pnpx.h and DESIGN.md section 7), in pixel units.  What is left None
    takes its default when the geometry meets a resolution: det_distance = source_distance, det_spacing = D / source_distance
    (unit ray spacing at the isocentre, D = source_distance + det_distance) and det_count = the fan that just covers the sampled
    circle (pnpx_fan_det_count).  The values travel as float32, as the native entries take them."""

    def __init__(self, source_distance, det_distance=None, det_count=None, det_spacing=None):
        self.source_distance, self.det_distance, self.det_count, self.det_spacing = source_distance, det_distance, det_count, det_spacing

    def key(self):
        return (self.source_distance, self.det_distance, self.det_count, self.det_spacing)

    def resolve(self, resolution, view):
        f32 = lambda v: float(np.float32(v))
        dso = f32(self.source_distance)
        dod = dso if self.det_distance is None else f32(self.det_distance)
        du = f32((dso + dod) / dso) if self.det_spacing is None else f32(self.det_spacing)
        det = ops.fan_det_count(resolution, dso, dod, du) if self.det_count is None else int(self.det_count)
        return FanGeometry(int(view), det, dso, dod, du)


class FanBeam_norm(Radon_norm):
    """Radon_norm's surface on a fan-beam pair: forward, the weighted backprojection, their normalised forms and the same seeded
    ten-step power method for opnorm.  Filtered backprojection is `fbp` (pnpx_fan_fbp: the cos gamma pre-weight, the ramp filter in
    the detector domain and the (D_so / U)^2 backprojection; include/pnpx.h) and its filter alone `filter_fan`.  The parallel
    beam's method names, filter_sinogram and filter_backprojection, keep raising here: they promise torch_radon's FFT filter."""

    def __init__(self, resolution, view, geometry, opnorm=None, device=None, seed=0):
        self.geometry = geometry.resolve(resolution, view)
        super().__init__(resolution, view, opnorm=opnorm, device=device, seed=seed)

    def forward(self, x):
        g = self.geometry
        return T.call("fan_forward", x, g.n_view, g.det_count, g.source_distance, g.det_distance, g.det_spacing)

    def backprojection(self, sinogram):
        g = self.geometry
        return T.call("fan_backprojection", sinogram, int(self.resolution), g.source_distance, g.det_distance, g.det_spacing)

    backward = backprojection

    def filter_fan(self, sinogram):
        """The pre-weighted, ramp-filtered and scaled sinogram that `fbp` backprojects."""
        g = self.geometry
        return T.call("radon_filter", sinogram, g.source_distance, g.det_distance, g.det_spacing)

    def fbp(self, sinogram):
        """Fan-beam filtered backprojection (Kak & Slaney section 3.4.2, full circle)."""
        g = self.geometry
        return T.call("fan_fbp", sinogram, int(self.resolution), g.source_distance, g.det_distance, g.det_spacing)

    def filter_sinogram(self, sinogram, filter_name='ramp'):
        """Not the fan beam's filter: use filter_fan."""
        raise NotImplementedError("fan-beam filtered backprojection is not provided")

    def filter_backprojection(self, sinogram):
        """Not the fan beam's reconstruction: use fbp."""
        raise NotImplementedError("fan-beam filtered backprojection is not provided")


class RadonGenerator:
    """transforms.py:494-508: caches the operator norm per (resolution, view), and per geometry when one is given (a FanBeam;
    None = the reference's parallel beam)."""

    def __init__(self):
        self.opnorms = {}

    def __call__(self, resolution, view, device=None, geometry=None):
        if geometry is None:
            key = (resolution, view)
            radon = Radon_norm(resolution, view, opnorm=self.opnorms.get(key), device=device)
        else:
            key = (resolution, view, geometry.key())
            radon = FanBeam_norm(resolution, view, geometry, opnorm=self.opnorms.get(key), device=device)
        self.opnorms[key] = radon.opnorm
        return radon
