"""Fan-beam filtered backprojection and the geometry-taking CT loops without a GPU: the restatements of tests/fan_fbp_ref.py against
the oracle's loops, the FFT construction of the ramp filter and exact ellipse chords; the new symbols; the Python surface.
The measured figures stand in profiles/fan_fbp.md."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fan_fbp_ref as P
from tests import fanbeam_ref as F
from tests.golden_inputs import csmri_actions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pnpx_radon_filter", "pnpx_fan_backprojection_w", "pnpx_fan_fbp", "pnpx_ct_iadmm_geom", "pnpx_ct_iadmm_geom_train",
               "pnpx_ct_iadmm_geom_backward", "pnpx_ct_pg_geom", "pnpx_ct_pg_geom_train", "pnpx_ct_pg_geom_backward")
NEW_OPS = ("radon_filter", "fan_fbp", "ct_iadmm_geom", "ct_iadmm_geom_train", "ct_iadmm_geom_backward", "ct_pg_geom",
           "ct_pg_geom_train", "ct_pg_geom_backward")

def test_header_and_binding_agree_on_the_new_names():
    from tfpnp_amd import _lib, ops, torch_ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pnpx_[a-z0-9_]+)\s*\(", src))
    lib = _lib.lib()
    assert len(NEW_SYMBOLS) == 9
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"enum \{ PNPX_FAN_W_ADJOINT = 0, PNPX_FAN_W_FBP = 1 \}", src)
    assert (_lib.PNPX_FAN_W_ADJOINT, _lib.PNPX_FAN_W_FBP) == (0, 1)
    for op in NEW_OPS:
        assert op in torch_ops.ALL_OPS and hasattr(torch.ops.pnpx, op) and callable(getattr(ops, op)), op


def test_restated_loops_reproduce_the_oracle_on_its_parallel_pair(unet_params):
    """Handed the oracle's own projector pair, the restated iADMM / PG loops are the oracle's, byte for byte (T = 3, 2 x 32^2):
    what the fan solvers are held against differs from the oracle in the pair alone."""
    from oracle import pnp_oracle as O
    B, R, V, T = 2, 32, 20, 3
    den = O.Denoiser(unet_params)
    angles, det = O.radon_geometry(R, V)
    A, AT = (lambda x: O.radon_forward(x, angles, det)), (lambda y: O.radon_backprojection(y, angles, R))
    rs = np.random.RandomState(11)
    gt = torch.from_numpy(rs.uniform(0, 1, (B, 1, R, R)).astype(np.float32))
    y0 = A(gt) * (1 + 0.05 * torch.from_numpy(rs.standard_normal((B, 1, V, det)).astype(np.float32)))
    opnorm = O.radon_opnorm(R, V)
    x0 = AT(y0) / opnorm ** 2
    a = {k: torch.from_numpy(v) for k, v in csmri_actions(B, T, 83, ("sigma_d", "mu", "tau")).items()}
    v3 = torch.cat([x0, x0, torch.zeros_like(x0)], 1)
    for it in (None, 1):
        assert torch.equal(P.ct_iadmm(den, A, AT, v3, y0, opnorm, a["sigma_d"], a["mu"], a["tau"], it),
                           O.ct_iadmm(den, v3, y0, V, opnorm, a["sigma_d"], a["mu"], a["tau"], it))
        assert torch.equal(P.ct_pg(den, A, AT, x0, y0, opnorm, a["sigma_d"], a["tau"], it),
                           O.ct_pg(den, x0, y0, V, opnorm, a["sigma_d"], a["tau"], it))


@pytest.mark.parametrize("det", [45, 363, 389])
def test_spatial_filter_is_the_zero_padded_fft_filter(det):
    """The float64 spatial sum (centre tap and odd lags) against the zero-padded FFT construction of Radon_norm.filter_sinogram
    restated in numpy: within 1e-7 (measured 4e-9 .. 1.5e-8, the fp32 rounding of ramp_filter's table).  The circular convolution
    of length L >= 2 det wraps nothing into the first det outputs, and the table's spatial kernel is the same h."""
    V = 7
    y = F.loud_sinogram(2, V, det, 300 + det)
    sp = P.fan_filter(y, None, torch.float64).numpy()
    ff = P.fft_filter64(y)
    e = np.linalg.norm(sp - ff) / np.linalg.norm(ff)
    print(f"det {det}: spatial filter vs zero-padded FFT filter, float64 rel-L2 {e:.2e}")
    assert e <= 1e-7


@pytest.mark.parametrize("a,b,n,ss", P.CHORD_CASES)
def test_fbp_of_exact_chords_reconstructs_the_phantom(a, b, n, ss):
    """128^2, 360 views, exact chords of an ellipse phantom -> float64 FBP.  The least-squares scale <rec, gt> / <gt, gt> within 1e-2
    of 1 catches any wrong factor of 2, pi or dp; rel-L2 within 1.5 x the figure this restatement gave when it was committed
    (profiles/fan_fbp.md; the margin covers the raster's sub-sampling choice and nothing else)."""
    g, gt, y = P.chord_case(a, b, n, ss)
    rec = P.fan_fbp(y, g, torch.float64)[0, 0].numpy()
    scale, err = P.lsq_scale(rec, gt), np.linalg.norm(rec - gt) / np.linalg.norm(gt)
    print(f"fan ({a}, {b}) R, {n} ellipse(s) (ss {ss}): {g.det_count} bins, FBP scale {scale:.4f}, rel-L2 {err:.3e}")
    assert abs(scale - 1.0) <= 1e-2
    assert err <= 1.5 * P.CHORD_REL_L2[(a, b, n)]


def test_fp32_restatement_distance_from_float64():
    """The figures the GPU tests' bars come from (tests/test_gpu_fan_fbp.py, profiles/fan_fbp.md): the fp32 restatement's rel-L2
    from the float64 one, for the filter, the FBP-weighted backprojection and FBP, on fanbeam_ref.CASES and the wide case.  The
    filter is a sequential fp32 sum of 45 .. 1500 terms: 2e-7 .. 7e-7.  The backprojection interpolates at fp32 positions, which
    carry ~1e-5 bins of rounding at a few hundred bins and ~1e-4 at 1500 bins of 0.1 pixel, on loud rows that the ramp filter has
    made steeper still: up to 1e-5 on CASES, 8.6e-5 on the wide case.  Ten times that would be a mistake in one of the two."""
    worst_f, worst = 0.0, 0.0
    for case in P.all_cases():
        g = F.case_geometry(case)
        y = F.loud_sinogram(case[0], g.n_view, g.det_count, 40 + case[1])
        ef = F.rel_l2(P.fan_filter(y, g, torch.float32), P.fan_filter(y, g, torch.float64))
        eb = F.rel_l2(P.fan_backprojection_fbp(y, g, torch.float32), P.fan_backprojection_fbp(y, g, torch.float64))
        er = F.rel_l2(P.fan_fbp(y, g, torch.float32), P.fan_fbp(y, g, torch.float64))
        print(f"case {case}: {g.det_count} bins, fp32 vs float64 restatement: filter {ef:.2e}, FBP-weight backprojection {eb:.2e}, "
              f"FBP {er:.2e}")
        worst_f, worst = max(worst_f, ef), max(worst, eb, er)
    assert 0 < worst_f < 2e-6 and 0 < worst < 1e-3


def test_python_surface_without_gpu():
    from tfpnp_amd.data.synthesis import ct_measure
    from tfpnp_amd.tasks.ct import HQSSolver_CT, IADMMSolver_CT, PGSolver_CT, create_solver_ct
    from tfpnp_amd.utils.transforms import FanBeam, FanBeam_norm, Radon_norm
    for cls in (IADMMSolver_CT, PGSolver_CT, HQSSolver_CT):
        assert cls(None).geometry is None
    fan = FanBeam(72.0, 24.0)

    class Opt:
        solver = "iadmm"
    assert create_solver_ct(Opt(), None).geometry is None
    Opt.geometry = fan
    for name, cls in (("iadmm", IADMMSolver_CT), ("pg", PGSolver_CT), ("hqs", HQSSolver_CT)):
        Opt.solver = name
        s = create_solver_ct(Opt(), None)
        assert type(s) is cls and s.geometry is fan
    with pytest.raises(ValueError, match="x0_from"):
        ct_measure(torch.zeros(1, 1, 8, 8), 4, x0_from="fpb")
    with pytest.raises(NotImplementedError):
        FanBeam_norm.filter_backprojection(None, None)
    with pytest.raises(NotImplementedError):
        FanBeam_norm.filter_sinogram(None, None)
    assert Radon_norm.fbp is Radon_norm.filter_backprojection and FanBeam_norm.fbp is not Radon_norm.fbp
    assert callable(FanBeam_norm.filter_fan)
