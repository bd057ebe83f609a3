"""The fan-beam Radon pair on the GPU (radon_fan_forward_kernel, radon_fan_backproject_lds_kernel and its gather fallback) against
the restatement of tests/fanbeam_ref.py in fp32 and float64, and by its own properties (impulses, exact chords, the adjoint
identity, each projector as the other's autograd formula, refusals)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import fanbeam_ref as F
from tests.golden_inputs import ellipse_phantom
from tfpnp_amd import _lib, ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def geom_args(gm):
    return (gm.source_distance, gm.det_distance, gm.det_spacing)


def forward(img, gm):
    return ops.fan_forward(g(img) if isinstance(img, np.ndarray) else img, gm.n_view, gm.det_count, *geom_args(gm))


def backproject(y, gm):
    return ops.fan_backprojection(g(y) if isinstance(y, np.ndarray) else y, gm.R, *geom_args(gm))


@functools.lru_cache(maxsize=None)
def references():
    """Per case: inputs and the fp32 / float64 restatements of both directions, computed once on the CPU and left unchanged."""
    out = []
    for case in F.CASES:
        gm = F.case_geometry(case)
        img, y = F.case_image(case), F.loud_sinogram(case[0], gm.n_view, gm.det_count, 40 + case[1])
        out.append(dict(case=case, geom=gm, img=img, sino=y,
                        fwd32=F.fan_forward(img, gm, torch.float32), fwd64=F.fan_forward(img, gm, torch.float64),
                        bwd32=F.fan_backprojection(y, gm, torch.float32), bwd64=F.fan_backprojection(y, gm, torch.float64)))
    return out


@functools.lru_cache(maxsize=None)
def bar():
    """The kernels' bar against float64: 4 x the largest rel-L2 of the fp32 restatement from the float64 one over every case and
    both directions (the margin covers the butterfly's summation order and the fused lerps), and no more than 1e-5 -- the parallel
    tests' bar -- unless that measurement itself exceeds 1e-5.  Measured: 3.5e-6 (backprojection of case 0), so the bar is 1e-5."""
    m = max(max(F.rel_l2(r["fwd32"], r["fwd64"]), F.rel_l2(r["bwd32"], r["bwd64"])) for r in references())
    b = 4 * m if m > 1e-5 else min(4 * m, 1e-5)
    print(f"  fp32 restatement vs float64, worst of all cases: {m:.2e} -> bar {b:.2e}")
    return b


@pytest.mark.parametrize("k", range(len(F.CASES)))
def test_forward_vs_restatements(k):
    r = references()[k]
    out = forward(r["img"], r["geom"]).cpu()
    assert tuple(out.shape) == tuple(r["fwd32"].shape)
    e32, e64 = F.rel_l2(out, r["fwd32"]), F.rel_l2(out, r["fwd64"])
    print(f"  forward {r['case']}: vs fp32 restatement {e32:.2e}, vs float64 {e64:.2e} (bar {bar():.2e})")
    assert e32 <= bar() and e64 <= bar()
    for b in range(out.shape[0]):                     # per item: a mis-dealt image must be named
        assert F.rel_l2(out[b], r["fwd64"][b]) <= bar(), (r["case"], b)


@pytest.mark.parametrize("k", range(len(F.CASES)))
def test_backprojection_vs_restatements(k):
    r = references()[k]
    gm = r["geom"]
    out = backproject(r["sino"], gm).cpu()
    assert tuple(out.shape) == tuple(r["bwd32"].shape)
    e32, e64 = F.rel_l2(out, r["bwd32"]), F.rel_l2(out, r["bwd64"])
    win = ops.fan_tables(gm.R, gm.n_view, gm.det_count, *geom_args(gm))[2]
    print(f"  backprojection {r['case']} (LDS window {win}): vs fp32 restatement {e32:.2e} (bit-identical: "
          f"{torch.equal(out, r['bwd32'])}), vs float64 {e64:.2e} (bar {bar():.2e})")
    assert win > 0                                    # these cases run the LDS kernel; case 1 with a window past the parallel kernel's 64
    assert e32 <= bar() and e64 <= bar()
    for b in range(out.shape[0]):
        assert F.rel_l2(out[b], r["bwd64"][b]) <= bar(), (r["case"], b)


def test_lds_and_gather_kernels_give_equal_bytes():
    """Both kernels on the same views: beta_v = 2 pi v / V, so the even views of a 2V-view geometry ARE the V views (same doubles),
    and a silent odd view adds w * 0 = +0.  V = 120 windows of 92 bins fit the LDS budget, 240 do not (pnpx_fan_tables says which
    kernel runs).  Close source, so tiles see wide windows and pixels see out-of-detector taps (det_count cut to 150)."""
    R, V, B = 64, 120, 2
    gm = F.geometry(R, V, 0.8 * R, 0.4 * R, det_count=150)
    gm2 = gm._replace(n_view=2 * V)
    assert ops.fan_tables(R, V, gm.det_count, *geom_args(gm))[2] > 64
    assert ops.fan_tables(R, 2 * V, gm.det_count, *geom_args(gm))[2] == 0
    y = F.loud_sinogram(B, V, gm.det_count, 77)
    y2 = np.zeros((B, 1, 2 * V, gm.det_count), np.float32)
    y2[:, :, 0::2] = y
    lds, gather = backproject(y, gm), backproject(y2, gm2)
    ref = F.fan_backprojection(y, gm, torch.float64)
    assert F.rel_l2(lds.cpu(), ref) <= bar()
    assert float(lds.abs().max()) > 0 and torch.equal(lds, gather)


def test_one_hot_image_lights_the_bins_of_its_projection():
    """A one-hot image under eight views (two per quadrant of beta).  A sample sees the pixel only within 1 px of it in x and in y,
    so a lit ray passes within sqrt 2 px of the pixel centre, i.e. within sqrt 2 * w bins of the exact projection (w = the
    reciprocal ray spacing at the pixel, 0.9 .. 1.13 here): the lit bins lie within one bin of the two bins that bracket the
    projection, those two are lit, and each view's sum is the ray density w times a unit-area footprint (within 25 %: 8 lanes x
    unit steps sample the footprint coarsely)."""
    R, V = 64, 8
    gm = F.geometry(R, V, 2.0 * R)
    for row, col in ((20, 41), (50, 9)):
        img = np.zeros((1, 1, R, R), np.float32)
        img[0, 0, row, col] = 1.0
        s = forward(img, gm)[0, 0].cpu().numpy()
        pos, w = F.pixel_projection(gm, col - (R / 2 - 0.5), row - (R / 2 - 0.5))
        for v in range(V):
            lit = np.nonzero(s[v])[0]
            assert lit.size and lit.min() >= math.floor(pos[v]) - 1 and lit.max() <= math.ceil(pos[v]) + 1, (row, col, v, pos[v], lit)
            assert np.abs(lit - pos[v]).max() <= math.sqrt(2.0) * w[v] + 1e-3, (row, col, v)
            assert s[v, math.floor(pos[v])] > 0 and s[v, math.ceil(pos[v])] > 0
            assert abs(s[v].sum() - w[v]) <= 0.25 * w[v], (row, col, v, s[v].sum(), w[v])


def test_one_hot_sinogram_backprojects_onto_its_ray_with_weight_w():
    """Bin j of view v alone: pixel (x, y) receives w (1 - |pos - j|) where its exact projection pos lies within one bin of j,
    and nothing elsewhere -- the ray, weighted."""
    R, V = 64, 8
    gm = F.geometry(R, V, 1.2 * R, 0.6 * R)
    c0 = np.arange(R) - (R / 2 - 0.5)
    X, Y = np.meshgrid(c0, c0)                        # Y along rows
    cs = F.view_table(V).astype(np.float64)
    for v, j in ((0, gm.det_count // 2 + 7), (3, gm.det_count // 3), (5, gm.det_count - 30), (6, 40)):
        y = np.zeros((1, 1, V, gm.det_count), np.float32)
        y[0, 0, v, j] = 1.0
        out = backproject(y, gm)[0, 0].cpu().numpy().astype(np.float64)
        pos, w = F.view_projection(gm, cs[v, 0], cs[v, 1], X, Y)
        want = w * np.clip(1.0 - np.abs(pos - j), 0.0, None)
        assert want.max() > 0.5
        # fp32 positions of ~100 bins carry ~1e-5 bins of rounding, times the tent's slope w ~ 1
        assert np.abs(out - want).max() <= 1e-4 * want.max(), (v, j, np.abs(out - want).max())
        assert not out[np.abs(pos - j) >= 1.0 + 1e-3].any(), (v, j)


@pytest.mark.parametrize("a,b", [(2.0, 2.0), (1.0, 1.0), (1.5, 0.5)])
def test_kernel_reproduces_exact_fan_chords(a, b):
    """The chord check of tests/test_fanbeam_host.py on the kernel: 256^2, 30 views, rel-L2 < 1e-2."""
    R, V = 256, 30
    gm = F.geometry(R, V, a * R, b * R)
    ells = ellipse_phantom.make(1)
    s = forward(ellipse_phantom.raster(ells, R)[None, None], gm)[0, 0].cpu().numpy()
    ana = F.ellipse_fan_sinogram(ells, gm)
    err = np.linalg.norm(s - ana) / np.linalg.norm(ana)
    print(f"  HIP fan forward ({a}, {b}) R vs exact chords: rel-L2 {err:.3e}")
    assert err < 1e-2


def test_pair_is_adjoint_on_the_smooth_phantom():
    R, V = 256, 30
    gm = F.geometry(R, V, 2.0 * R, 2.0 * R)
    x = g(ellipse_phantom.raster(ellipse_phantom.make(5), R, ss=2)[None, None])
    y = forward(x, gm)
    lhs = float((y.double() * y.double()).sum())
    rhs = float((x.double() * backproject(y, gm).double()).sum())
    print(f"  HIP fan pair, adjoint mismatch on the smooth phantom: {abs(lhs - rhs) / lhs:.3e}")
    assert abs(lhs - rhs) < 1e-4 * lhs


def test_torch_ops_are_each_other_under_autograd():
    from tfpnp_amd import torch_ops  # noqa: F401  (registers torch.ops.pnpx.*)
    r = references()[4]
    gm = r["geom"]
    x = g(r["img"]).requires_grad_(True)
    gy = g(r["sino"])
    y = torch.ops.pnpx.fan_forward(x, gm.n_view, gm.det_count, *geom_args(gm))
    assert torch.equal(y.detach(), forward(r["img"], gm))
    (gx,) = torch.autograd.grad(y, x, gy)
    assert torch.equal(gx, backproject(r["sino"], gm))
    s = gy.clone().requires_grad_(True)
    im = torch.ops.pnpx.fan_backprojection(s, gm.R, *geom_args(gm))
    (gs,) = torch.autograd.grad(im, s, x.detach())
    assert torch.equal(gs, forward(r["img"], gm))
    torch.library.opcheck(torch.ops.pnpx.fan_forward, (x.detach(), gm.n_view, gm.det_count, *geom_args(gm)))
    torch.library.opcheck(torch.ops.pnpx.fan_backprojection, (gy, gm.R, *geom_args(gm)))


def test_refused_geometries_launch_nothing():
    """A refused call returns its status and message and leaves the output buffer as it was."""
    R, V, det = 64, 8, 120
    ctx = ops.default_context(dev())
    img = g(np.ones((1, 1, R, R), np.float32))
    lib = _lib.lib()
    for change, status, text in [(dict(source_distance=20.0), 2, "inside the sampled span"),
                                 (dict(det_spacing=0.0), 1, "det_spacing must be positive"),
                                 (dict(det_distance=-1.0), 1, "det_distance must not be negative"),
                                 (dict(det_count=1), 2, "det_count")]:
        kw = {**dict(n_view=V, det_count=det, source_distance=128.0, det_distance=64.0, det_spacing=1.5), **change}
        gm = ops.fan_geom(**kw)
        sino = torch.full((1, 1, V, max(kw["det_count"], 2)), -7.0, device=dev())
        out = torch.full((1, 1, R, R), -7.0, device=dev())
        with torch.cuda.device(dev()):
            st_f = lib.pnpx_fan_forward(ctx.handle, ops._p(img), ops._p(sino), gm, 1, R, ops._stream(img))
            msg_f = lib.pnpx_last_error().decode()
            st_b = lib.pnpx_fan_backprojection(ctx.handle, ops._p(sino), ops._p(out), gm, 1, R, ops._stream(img))
            msg_b = lib.pnpx_last_error().decode()
        torch.cuda.synchronize()
        assert st_f == st_b == status and text in msg_f and text in msg_b, (change, st_f, st_b, msg_f)
        assert bool((sino == -7.0).all()) and bool((out == -7.0).all()), change
    with pytest.raises(_lib.PnpxError, match="inside the sampled span"):
        ops.fan_forward(img, V, det, 20.0, 64.0, 1.5)
