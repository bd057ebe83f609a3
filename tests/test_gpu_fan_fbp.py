"""Fan-beam filtered backprojection on the GPU (radon_filter_kernel, the FBP weight of both fan backprojection kernels, pnpx_fan_fbp)
against the restatements of tests/fan_fbp_ref.py in fp32 and float64, and by its own properties: impulses, the parallel beam's FFT
filter, equal bytes of the LDS and gather kernels, exact chords, refusals, and ct_measure's start image."""
import functools

import numpy as np
import pytest
import torch

from tests import fan_fbp_ref as P
from tests import fanbeam_ref as F
from tfpnp_amd import _lib, ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def geom_args(gm):
    return (gm.source_distance, gm.det_distance, gm.det_spacing)


def bar_of(m):
    """tests/test_gpu_fanbeam.py::bar per figure: 4 x the fp32 restatement's rel-L2 from the float64 one (the margin covers a
    last-place difference of a division or a square root), and no more than 1e-5 unless that measurement itself exceeds 1e-5."""
    return 4 * m if m > 1e-5 else min(4 * m, 1e-5)


@functools.lru_cache(maxsize=None)
def references():
    """Per case (fanbeam_ref.CASES and the wide one): a loud sinogram and the fp32 / float64 restatements of the filter, the
    FBP-weighted backprojection and FBP, computed once on the CPU and left unchanged."""
    out = []
    for case in P.all_cases():
        gm = F.case_geometry(case)
        y = F.loud_sinogram(case[0], gm.n_view, gm.det_count, 40 + case[1])
        r = dict(case=case, geom=gm, sino=y)
        for name, fn in (("filter", P.fan_filter), ("backprojection", P.fan_backprojection_fbp), ("fbp", P.fan_fbp)):
            r[name] = (fn(y, gm, torch.float32), fn(y, gm, torch.float64))
        out.append(r)
    return out


@pytest.mark.parametrize("k", range(len(P.all_cases())))
def test_kernels_vs_restatements(k):
    """det below a wave (45), odd (199, 141), above the thread count (1500); B > 8; V = 1."""
    r = references()[k]
    gm, y = r["geom"], g(r["sino"])
    got = {"filter": ops.radon_filter(y, *geom_args(gm)),
           "backprojection": ops.fan_backprojection(y, gm.R, *geom_args(gm), weight="fbp"),
           "fbp": ops.fan_fbp(y, gm.R, *geom_args(gm))}
    for name, out in got.items():
        r32, r64 = r[name]
        out = out.cpu()
        assert tuple(out.shape) == tuple(r32.shape), name
        bar = bar_of(F.rel_l2(r32, r64))
        e32, e64 = F.rel_l2(out, r32), F.rel_l2(out, r64)
        print(f"  {name} {r['case']}: vs fp32 restatement {e32:.2e} (bit-identical: {torch.equal(out, r32)}), vs float64 {e64:.2e} "
              f"(bar {bar:.2e})")
        assert e32 <= bar and e64 <= bar, (name, r["case"])
        for b in range(out.shape[0]):
            assert F.rel_l2(out[b], r64[b]) <= bar, (name, r["case"], b)      # per item: a mis-dealt row or image must be named


@pytest.mark.parametrize("k", [0, 4])
def test_filter_impulse_returns_the_scaled_taps(k):
    """A one-hot row at bins 0, det / 2 and det - 1 returns S c[m] h[j - m]: within 1e-6 of the largest value (six fp32 roundings:
    the pre-weight, three in the tap, the product and S), every even-lag output exactly 0.0, every other row exactly 0.0."""
    gm = F.case_geometry(F.CASES[k])
    B, V, det = 2, gm.n_view, gm.det_count
    S, c = P.filter_scale(gm, V, torch.float64), F.bin_table(gm, np.float64)[:, 0]
    j = np.arange(det)
    for m in (0, det // 2, det - 1):
        y = np.zeros((B, 1, V, det), np.float32)
        y[1, 0, V - 1, m] = 1.0
        out = ops.radon_filter(g(y), *geom_args(gm)).cpu().numpy().astype(np.float64)
        lag = np.abs(j - m)
        h = np.where(lag == 0, 0.25, np.where(lag % 2 == 1, -1.0 / (np.pi * np.maximum(lag, 1)) ** 2, 0.0))
        want = S * c[m] * h
        row = out[1, 0, V - 1]
        assert np.abs(row - want).max() <= 1e-6 * np.abs(want).max(), (m, np.abs(row - want).max())
        assert not row[(lag % 2 == 0) & (lag > 0)].any(), m
        out[1, 0, V - 1] = 0.0
        assert not out.any(), m


@pytest.mark.parametrize("B,V,R", [(2, 20, 32), (1, 30, 256)])
def test_parallel_filter_vs_the_fft_path(B, V, R):
    """radon_filter without a geometry against Radon_norm.filter_sinogram on the same sinogram (2 x 20 x 46 and 1 x 30 x 363):
    within 4 x the FFT path's own rel-L2 from the float64 restatement (profiles/fan_fbp.md)."""
    from tfpnp_amd.utils.transforms import Radon_norm
    det = ops.radon_det_count(R)
    y = F.loud_sinogram(B, V, det, 60 + R)
    ref64 = P.fan_filter(y, None, torch.float64)
    fft = Radon_norm(R, V, opnorm=1.0, device=dev()).filter_sinogram(g(y)).cpu()
    out = ops.radon_filter(g(y)).cpu()
    d_fft, d_out, e = F.rel_l2(fft, ref64), F.rel_l2(out, ref64), F.rel_l2(out, fft)
    print(f"  parallel filter {B} x {V} x {det}: FFT path vs float64 {d_fft:.2e}, kernel vs float64 {d_out:.2e}, kernel vs FFT path {e:.2e}")
    assert tuple(out.shape) == (B, 1, V, det) and d_fft > 0
    assert e <= 4 * d_fft
    assert d_out <= bar_of(F.rel_l2(P.fan_filter(y, None, torch.float32), ref64))


def test_one_hot_sinogram_backprojects_onto_its_ray_with_the_fbp_weight():
    """tests/test_gpu_fanbeam.py's impulse test under weight='fbp': pixel (x, y) receives (D_so / U)^2 (1 - |pos - j|) where its
    exact projection pos lies within one bin of j, and nothing elsewhere."""
    R, V = 64, 8
    gm = F.geometry(R, V, 1.2 * R, 0.6 * R)
    c0 = np.arange(R) - (R / 2 - 0.5)
    X, Y = np.meshgrid(c0, c0)                        # Y along rows
    cs = F.view_table(V).astype(np.float64)
    for v, j in ((0, gm.det_count // 2 + 7), (3, gm.det_count // 3), (5, gm.det_count - 30), (6, 40)):
        y = np.zeros((1, 1, V, gm.det_count), np.float32)
        y[0, 0, v, j] = 1.0
        out = ops.fan_backprojection(g(y), R, *geom_args(gm), weight="fbp")[0, 0].cpu().numpy().astype(np.float64)
        pos, _ = F.view_projection(gm, cs[v, 0], cs[v, 1], X, Y)
        U = gm.source_distance + (Y * cs[v, 0] - X * cs[v, 1])
        want = (gm.source_distance / U) ** 2 * np.clip(1.0 - np.abs(pos - j), 0.0, None)
        assert want.max() > 0.5
        # fp32 positions of ~100 bins carry ~1e-5 bins of rounding, times the tent's slope w ~ 1
        assert np.abs(out - want).max() <= 1e-4 * want.max(), (v, j, np.abs(out - want).max())
        assert not out[np.abs(pos - j) >= 1.0 + 1e-3].any(), (v, j)


def test_lds_and_gather_kernels_give_equal_bytes_under_both_weights():
    """The V = 120 / 240 construction of tests/test_gpu_fanbeam.py (the even views of the 2V geometry are the V views, a silent odd
    view adds w * 0) through weight='fbp', which carries no V-dependent scale; and weight='adjoint' is the plain entry, on both
    kernels."""
    R, V, B = 64, 120, 2
    gm = F.geometry(R, V, 0.8 * R, 0.4 * R, det_count=150)
    assert ops.fan_tables(R, V, gm.det_count, *geom_args(gm))[2] > 64
    assert ops.fan_tables(R, 2 * V, gm.det_count, *geom_args(gm))[2] == 0
    y = F.loud_sinogram(B, V, gm.det_count, 77)
    y2 = np.zeros((B, 1, 2 * V, gm.det_count), np.float32)
    y2[:, :, 0::2] = y
    lds = ops.fan_backprojection(g(y), R, *geom_args(gm), weight="fbp")
    gather = ops.fan_backprojection(g(y2), R, *geom_args(gm), weight="fbp")
    r32, r64 = P.fan_backprojection_fbp(y, gm, torch.float32), P.fan_backprojection_fbp(y, gm, torch.float64)
    assert F.rel_l2(lds.cpu(), r64) <= bar_of(F.rel_l2(r32, r64))
    assert float(lds.abs().max()) > 0 and torch.equal(lds, gather)
    for sino in (y, y2):
        plain = ops.fan_backprojection(g(sino), R, *geom_args(gm))
        assert float(plain.abs().max()) > 0 and not torch.equal(plain, lds)
        assert torch.equal(ops.fan_backprojection(g(sino), R, *geom_args(gm), weight="adjoint"), plain)


@pytest.mark.parametrize("a,b,n,ss", P.CHORD_CASES)
def test_kernels_reconstruct_exact_chords(a, b, n, ss):
    """The chord check of tests/test_fan_fbp_host.py on the kernels (360 views: the gather backprojection): the same two
    conditions."""
    gm, gt, y = P.chord_case(a, b, n, ss)
    assert ops.fan_tables(gm.R, gm.n_view, gm.det_count, *geom_args(gm))[2] == 0
    rec = ops.fan_fbp(g(y.astype(np.float32)), gm.R, *geom_args(gm))[0, 0].cpu().numpy().astype(np.float64)
    scale, err = P.lsq_scale(rec, gt), np.linalg.norm(rec - gt) / np.linalg.norm(gt)
    print(f"  HIP fan FBP ({a}, {b}) R, {n} ellipse(s): scale {scale:.4f}, rel-L2 {err:.3e}")
    assert abs(scale - 1.0) <= 1e-2
    assert err <= 1.5 * P.CHORD_REL_L2[(a, b, n)]


def test_refusals_launch_nothing():
    """Aliased filter buffers, a one-bin row, and pnpx_fan_fbp without a geometry: status, message, outputs untouched."""
    R, V, det = 64, 8, 120
    ctx = ops.default_context(dev())
    lib = _lib.lib()
    gm = ops.fan_geom(V, det, 128.0, 64.0, 1.5)
    sino = torch.full((1, 1, V, det), -7.0, device=dev())
    out = torch.full((1, 1, V, det), -5.0, device=dev())
    img = torch.full((1, 1, R, R), -3.0, device=dev())
    P_, s = ops._p, ops._stream(sino)
    calls = [(lambda: lib.pnpx_radon_filter(ctx.handle, P_(sino), P_(sino), gm, 1, V, det, s), 1, "must not be sino_in"),
             (lambda: lib.pnpx_radon_filter(ctx.handle, P_(sino), P_(sino), None, 1, V, det, s), 1, "must not be sino_in"),
             (lambda: lib.pnpx_radon_filter(ctx.handle, P_(sino), P_(out), None, 1, V * det, 1, s), 2, "det must be in"),
             (lambda: lib.pnpx_radon_filter(ctx.handle, P_(sino), P_(out), gm, 1, V, det - 1, s), 1, "the geometry has"),
             (lambda: lib.pnpx_fan_fbp(ctx.handle, P_(sino), P_(img), None, 1, R, s), 1, "PNPX_GEOM_FAN"),
             (lambda: lib.pnpx_fan_backprojection_w(ctx.handle, P_(sino), P_(img), gm, 2, 1, R, s), 1, "weight must be")]
    for k, (call, want, text) in enumerate(calls):
        with torch.cuda.device(dev()):
            status = call()
            msg = lib.pnpx_last_error().decode()
        assert status == want and text in msg, (k, status, msg)
    torch.cuda.synchronize()
    assert bool((sino == -7.0).all()) and bool((out == -5.0).all()) and bool((img == -3.0).all())
    for fn, text in ((lambda: ops.radon_filter(torch.zeros(1, 1, V, 1, device=dev())), "det must be in"),
                     (lambda: ops.fan_fbp(sino, R, 20.0, 64.0, 1.5), "inside the sampled span"),
                     (lambda: ops.fan_backprojection(sino, R, 128.0, 64.0, 1.5, weight="ramp"), "weight must be one of")):
        with pytest.raises(_lib.PnpxError, match=text):
            fn()


def test_torch_ops_have_schemas_and_fakes():
    from tfpnp_amd import torch_ops  # noqa: F401  (registers torch.ops.pnpx.*)
    r = references()[4]
    gm, y = r["geom"], g(r["sino"])
    assert torch.equal(torch.ops.pnpx.fan_fbp(y, gm.R, *geom_args(gm)), ops.fan_fbp(y, gm.R, *geom_args(gm)))
    assert torch.equal(torch.ops.pnpx.radon_filter(y, *geom_args(gm)), ops.radon_filter(y, *geom_args(gm)))
    assert torch.equal(torch.ops.pnpx.radon_filter(y, 0.0, 0.0, 0.0), ops.radon_filter(y))
    tests = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.pnpx.fan_fbp, (y, gm.R, *geom_args(gm)), test_utils=tests)
    torch.library.opcheck(torch.ops.pnpx.radon_filter, (y, *geom_args(gm)), test_utils=tests)


def test_ct_measure_starts_from_fbp_on_request():
    from tfpnp_amd import synth
    from tfpnp_amd.data.synthesis import ct_measure
    from tfpnp_amd.utils.transforms import FanBeam, RadonGenerator
    R, V = 32, 20
    fan, gen = FanBeam(1.5 * R, 0.5 * R), RadonGenerator()
    gt = g(synth.phantom_batch(2, R, R, 512))
    d = ct_measure(gt, V, radon_generator=gen, geometry=fan, x0_from="fbp")
    radon = gen(R, V, device=dev(), geometry=fan)
    assert torch.equal(d["x0"], radon.fbp(d["y0"])) and not torch.equal(d["x0"], d["ATy0"])
    # pnpx_fan_fbp is the two launches: the filter, then the FBP-weighted backprojection
    two = ops.fan_backprojection(radon.filter_fan(d["y0"]), R, *radon.geometry[2:], weight="fbp")
    assert torch.equal(d["x0"], two)
    d0 = ct_measure(gt, V, radon_generator=gen, geometry=fan)
    assert torch.equal(d0["x0"], d0["ATy0"]) and torch.equal(d0["ATy0"], d["ATy0"])
    assert torch.equal(ct_measure(gt, V, radon_generator=gen, geometry=fan, x0_from="aty0")["x0"], d0["x0"])
    # the parallel beam: None is FBP, as before; 'aty0' now chooses the other start
    p = ct_measure(gt, V, radon_generator=gen)
    par = gen(R, V, device=dev())
    assert torch.equal(p["x0"], par.filter_backprojection(p["y0"])) and torch.equal(p["x0"], par.fbp(p["y0"]))
    assert torch.equal(ct_measure(gt, V, radon_generator=gen, x0_from="aty0")["x0"], p["ATy0"])
