"""Fan-beam geometry without a GPU: the host tables and refusals of libpnpx.so against the formulas of include/pnpx.h, and the
restatement (tests/fanbeam_ref.py) against exact ellipse chords and the adjoint identity, in float64."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import fanbeam_ref as F
from tests.golden_inputs import ellipse_phantom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTANCES = [(2.0, 2.0), (1.0, 1.0), (1.5, 0.5)]          # (D_so, D_od) / R
NEW_SYMBOLS = ("pnpx_fan_det_count", "pnpx_fan_forward", "pnpx_fan_backprojection", "pnpx_fan_tables", "pnpx_ct_hqs",
               "pnpx_ct_hqs_train", "pnpx_ct_hqs_backward")


def test_default_det_count_and_host_tables():
    from tfpnp_amd import ops
    assert ops.fan_det_count(256, 512.0, 512.0, 2.0) == 389 == F.geometry(256, 30, 512.0).det_count
    assert ops.fan_det_count(256, 256.0, 256.0, 2.0) == 515 == F.geometry(256, 30, 256.0).det_count
    for R, V, a, b, det, du in [(256, 30, 2.0, 2.0, None, None), (97, 5, 4.0, 0.0, None, None), (48, 6, 1.5, 0.5, 45, 1.7),
                                (64, 8, 0.8, 0.4, None, None), (33, 1, 2.0, 2.0, None, None)]:
        g = F.geometry(R, V, a * R, b * R, det, du)
        if det is None:
            n = math.ceil(math.sqrt(2.0) * R)
            D = g.source_distance + g.det_distance
            want = math.ceil(2 * D * math.tan(math.asin((n / 2) / g.source_distance)) / g.det_spacing)
            assert ops.fan_det_count(R, g.source_distance, g.det_distance, g.det_spacing) == want == g.det_count
        cs, bins, win = ops.fan_tables(R, V, g.det_count, g.source_distance, g.det_distance, g.det_spacing)
        # view table: the angle in double, rounded to fp32; cos / sin in double of that fp32 angle, rounded
        for v in range(V):
            af = float(np.float32(2.0 * math.pi * v / V))
            assert cs[v, 0] == np.float32(math.cos(af)) and cs[v, 1] == np.float32(math.sin(af)), (R, V, v)
        # bin table: u_j = (j - det/2 + 0.5) du, L_j = sqrt(D^2 + u_j^2), (D / L, u / L, D_so u / L) -- D is the fp32 sum the kernels get
        D = float(np.float32(g.source_distance + g.det_distance))
        u = (np.arange(g.det_count) - g.det_count / 2 + 0.5) * g.det_spacing
        L = np.sqrt(D * D + u * u)
        want = np.stack([D / L, u / L, g.source_distance * u / L], 1)
        assert np.abs(bins - want).max() <= 1e-7 * max(1.0, g.source_distance), (R, V)       # one fp32 rounding
        assert np.array_equal(bins, F.bin_table(g)) and np.array_equal(cs, F.view_table(V))
        assert 0 < win <= g.det_count + 12
    # the window grows as the source comes close (the parallel kernel's 64 bins would not hold the tile)
    g = F.geometry(64, 8, 0.8 * 64, 0.4 * 64)
    assert ops.fan_tables(64, 8, g.det_count, g.source_distance, g.det_distance, g.det_spacing)[2] > 64
    # V x window beyond the LDS budget: the gather kernel is announced (0)
    assert ops.fan_tables(64, 400, g.det_count, g.source_distance, g.det_distance, g.det_spacing)[2] == 0


@pytest.mark.parametrize("a,b", DISTANCES)
def test_restatement_reproduces_exact_fan_chords(a, b):
    """256^2, 30 views: the float64 restatement against the exact chords of every fan ray (from its (theta, s)): rel-L2 < 1e-2,
    the bar of the parallel pair's test (measured 4.3e-3 .. 4.7e-3: what bilinear sampling loses at the phantom's sharp edges)."""
    R, V = 256, 30
    g = F.geometry(R, V, a * R, b * R)
    ells = ellipse_phantom.make(1)
    img = ellipse_phantom.raster(ells, R)
    s = F.fan_forward(img[None, None], g, torch.float64)[0, 0].numpy()
    ana = F.ellipse_fan_sinogram(ells, g)
    err = np.linalg.norm(s - ana) / np.linalg.norm(ana)
    print(f"fan ({a}, {b}) R: {g.det_count} bins, forward rel-L2 vs exact chords = {err:.3e}")
    assert err < 1e-2


@pytest.mark.parametrize("a,b", DISTANCES)
def test_weight_makes_the_pair_adjoint_on_a_smooth_phantom(a, b):
    """|<Ax,Ax> - <x,BAx>| / <Ax,Ax> in float64 on the smooth phantom (make(5), ss = 2): below 1e-4 with the weight
    w = sqrt(D^2 + u^2) / (U du), above 1e-3 without it (measured 8e-7 .. 3.6e-6 and 2.7e-3 .. 1.1e-2).  White noise is no gate:
    its inner products sit near zero."""
    R, V = 256, 30
    g = F.geometry(R, V, a * R, b * R)
    x = torch.from_numpy(ellipse_phantom.raster(ellipse_phantom.make(5), R, ss=2))[None, None].double()
    y = F.fan_forward(x, g, torch.float64)
    lhs = float((y * y).sum())
    mis = {w: abs(lhs - float((x * F.fan_backprojection(y, g, torch.float64, weight=w)).sum())) / lhs for w in (True, False)}
    print(f"fan ({a}, {b}) R: adjoint mismatch with w {mis[True]:.3e}, without {mis[False]:.3e}")
    assert mis[True] < 1e-4
    assert mis[False] > 1e-3


def test_fp32_restatement_distance_from_float64():
    """The figure the GPU tests' bar is derived from (tests/test_gpu_fanbeam.py::bar, profiles/fanbeam.md): the fp32
    restatement's rel-L2 from the float64 one on every case, both directions.  fp32 arithmetic on positions of up to a few hundred
    pixels / bins: a few 1e-7 forward, up to a few 1e-6 on a loud random sinogram; anything near 1e-4 would be a mistake in
    one of the two, not rounding."""
    worst = 0.0
    for case in F.CASES:
        g = F.case_geometry(case)
        img, y = F.case_image(case), F.loud_sinogram(case[0], g.n_view, g.det_count, 40 + case[1])
        ef = F.rel_l2(F.fan_forward(img, g, torch.float32), F.fan_forward(img, g, torch.float64))
        eb = F.rel_l2(F.fan_backprojection(y, g, torch.float32), F.fan_backprojection(y, g, torch.float64))
        print(f"case {case}: {g.det_count} bins, fp32 vs float64 restatement: forward {ef:.2e}, backprojection {eb:.2e}")
        worst = max(worst, ef, eb)
    assert 0 < worst < 2e-5


def test_header_and_binding_agree_on_the_new_names():
    from tfpnp_amd import _lib, ops, torch_ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pnpx_[a-z0-9_]+)\s*\(", src))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    m = re.search(r"typedef struct pnpx_radon_geom \{(.*?)\} pnpx_radon_geom;", src, flags=re.S)
    fields = re.findall(r"\b(kind|n_view|det_count|source_distance|det_distance|det_spacing)\b", m.group(1))
    assert fields == [n for n, _ in _lib.RadonGeom._fields_]
    for op in ("fan_forward", "fan_backprojection", "ct_hqs", "ct_hqs_train", "ct_hqs_backward"):
        assert op in torch_ops.ALL_OPS and hasattr(torch.ops.pnpx, op), op
    for fn in ("fan_forward", "fan_backprojection", "fan_det_count", "fan_tables", "ct_hqs", "ct_hqs_train", "ct_hqs_backward"):
        assert callable(getattr(ops, fn)), fn


def test_refused_geometries_and_their_messages():
    """The refusals of include/pnpx.h, through the host-only entry (the device entries resolve the geometry with the same code
    before they touch the device: tests/test_gpu_fanbeam.py)."""
    from tfpnp_amd import ops
    from tfpnp_amd._lib import PnpxError
    R, V = 64, 8
    n = math.ceil(math.sqrt(2.0) * R)                 # 91
    ok = dict(det_count=120, source_distance=n / 2 + 1, det_distance=10.0, det_spacing=1.0)
    ops.fan_tables(R, V, **ok)                        # the closest source that is accepted
    for change, status, text in [(dict(source_distance=n / 2 + 0.9), 2, "inside the sampled span"),
                                 (dict(det_spacing=0.0), 1, "det_spacing must be positive"),
                                 (dict(det_spacing=-1.0), 1, "det_spacing must be positive"),
                                 (dict(det_distance=-0.5), 1, "det_distance must not be negative"),
                                 (dict(det_count=1), 2, "det_count"),
                                 (dict(source_distance=float("nan")), 1, "finite")]:
        with pytest.raises(PnpxError) as e:
            ops.fan_tables(R, V, **{**ok, **change})
        assert f"status {status}" in str(e.value) and text in str(e.value), (change, str(e.value))
    with pytest.raises(PnpxError, match="n_view"):
        ops.fan_tables(R, 0, **ok)
    with pytest.raises(PnpxError, match="bad geometry"):
        ops.fan_det_count(R, 10.0, 10.0, 1.0)


def test_python_surface_without_gpu():
    from tfpnp_amd.tasks.ct import HQSSolver_CT, IADMMSolver_CT, create_solver_ct
    from tfpnp_amd.utils.transforms import FanBeam, FanBeam_norm, RadonGenerator

    class Opt:
        solver = "hqs"
    s = create_solver_ct(Opt(), None)
    assert isinstance(s, HQSSolver_CT) and s.geometry is None and s.hyper_keys == ("sigma_d", "mu") and s.init_vars == ("x0", "x0")
    Opt.solver = "iadmm"
    assert isinstance(create_solver_ct(Opt(), None), IADMMSolver_CT)
    g = FanBeam(2 * 256).resolve(256, 30)
    assert g == F.geometry(256, 30, 512.0)[1:] and g.det_count == 389
    g = FanBeam(72.0, 24.0, 45, 1.7).resolve(48, 6)
    assert g == F.geometry(48, 6, 72.0, 24.0, 45, 1.7)[1:]
    assert FanBeam(72.0).key() != FanBeam(72.0, 24.0).key()
    with pytest.raises(NotImplementedError):
        FanBeam_norm.filter_backprojection(None, None)
    gen = RadonGenerator()
    gen.opnorms[(48, 6)] = 3.0                        # a cached norm: no device call
    gen.opnorms[(48, 6, FanBeam(72.0).key())] = 5.0
    assert gen(48, 6, device="cpu").opnorm == 3.0
    fan = gen(48, 6, device="cpu", geometry=FanBeam(72.0))
    assert isinstance(fan, FanBeam_norm) and fan.opnorm == 5.0 and fan.geometry.det_count == F.geometry(48, 6, 72.0).det_count
