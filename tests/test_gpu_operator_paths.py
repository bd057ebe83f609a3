"""Every dispatch branch of the measurement operators against a plain high-precision reference (pytest -m gpu):

  B  pnpx_fft2 over the case table of tests/fft_plan_model.py (fast / pow2 / mixed-radix / prime passes, XCD-affine mapping with and
     without a trailing partial group, tile geometry edges, degenerate and maximum lengths) against torch.fft in complex128, PER
     IMAGE; options fft_affine / fft_tile bit-identical, fft_fast = 0 against the same reference; tiles above 64 KiB of LDS.
  C  the fused solver passes (fp32 convolution family, 2 iterations) at the mixed fast / generic shapes, items {0, 7, 8, B-1}
     against the CPU oracle.
  D  pnpx_cdp_forward / pnpx_cdp_backward against complex128 and their adjoint identity.
  E  pnpx_radon_backprojection: both kernels (LDS window, per-pixel gather) over edge-tile shapes against the oracle and an fp64
     restatement.
  F  pnpx_psnr over chunk-edge sizes against fp64.

What the first MI355X run of this module found: the backprojection kernels were NOT the oracle's arithmetic -- the rounded-operation
helpers they were written with compile to FMAs -- and sat 4.56e-6 (max / max) from the oracle at R = 97, V = 13, with the loud last
detector bins at sp > 128 (one ulp of the position, 1.5e-5, times an edge of height 10); every FFT, solver and CDP leg passed its
bound, and the tiles above 64 KiB ran bit-identically with make_fft_plan's clamp to the device's per-block LDS limit.  The kernels
now form their products and sums with contraction off (csrc/tasks.hip: mulx / addx / subx).
"""
import math

import numpy as np
import pytest
import torch

from oracle import pnp_oracle as O
from tests import fft_plan_model as M
from tests.golden_inputs import complex_inputs, csmri_actions
from tests.test_pr_pg_host import pr_pg_restated
from tfpnp_amd import ops, synth

pytestmark = pytest.mark.gpu

FFT_TOL = 2e-6          # the bar of test_fft_general_sizes_vs_oracle; fp32 pocketfft and a sequential fp32 DFT of a 2039-point
                        # line sit 1.6e-8 .. 8.0e-7 from fp64 on these cases
TOL = 1e-4              # solver parity bar (BASELINE.json north_star)
LDS_64K = 64 * 1024


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def g(a):
    return t(a).to(dev())


def per_item_rel(a, b):
    """Relative L2 error of every item of the leading dimension, in float64 -> list of floats."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    n = a.shape[0]
    d = (a - b).reshape(n, -1).norm(dim=1)
    return (d / b.reshape(n, -1).norm(dim=1).clamp_min(1e-30)).tolist()


def assert_per_item(a, b, tol, what):
    errs = per_item_rel(a, b)
    worst = int(np.argmax(errs))
    print(f"  {what}: worst item {worst} of {len(errs)}: {errs[worst]:.2e}")
    bad = [(i, f"{e:.2e}") for i, e in enumerate(errs) if not e <= tol]
    assert not bad, f"{what}: items (index, rel-L2) above {tol:g}: {bad}"
    return errs[worst]


# =========================================================================================================== B: pnpx_fft2
def fft2_ref64(x, inverse, centered):
    """torch.fft in complex128 on the CPU, orthonormal; centered: ifftshift -> transform -> fftshift as oracle.pnp_oracle.fft2c."""
    c = torch.view_as_complex(t(x).double().contiguous())
    if centered:
        c = torch.fft.ifftshift(c, dim=(-2, -1))
    c = (torch.fft.ifft2 if inverse else torch.fft.fft2)(c, dim=(-2, -1), norm="ortho")
    if centered:
        c = torch.fft.fftshift(c, dim=(-2, -1))
    return torch.view_as_real(c)


def fft_input(case):
    n, H, W = case
    return complex_inputs((n, H, W), 1000 + 7 * n + 3 * H + W)


VARIANTS = [(False, True), (True, True), (False, False), (True, False)]      # (inverse, centered)


@pytest.mark.parametrize("case", M.FFT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fft2_case_matrix_vs_fp64(case):
    """Forward and inverse, centered and not, per image: one mis-mapped image of 19 (or one wrong value of 2048^2: 5e-4) fails."""
    p = M.plan(*case)
    print(f"\n  {case}: rows {p.rows} (lines {p.lr}, affine {int(p.rows_affine)}, {p.lds_rows} B)  cols {p.cols} (lines {p.lc}, "
          f"affine {int(p.cols_affine)}, {p.lds_cols} B)  partial group {int(p.partial_group)}")
    x = fft_input(case)
    xd = g(x)
    for inverse, centered in VARIANTS:
        out = ops.fft2(xd, inverse=inverse, centered=centered)
        assert_per_item(out, fft2_ref64(x, inverse, centered), FFT_TOL, f"{case} inverse={int(inverse)} centered={int(centered)}")


class fft_options:
    """Options of the default context (the one ops.fft2 runs on), restored on exit."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.ctx = ops.default_context(dev())
        self.saved = {k: self.ctx.get_option(k) for k in ("fft_affine", "fft_tile", "fft_fast")}
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_option(k, v)


def _lds(shape, tile, fast=1):
    """Dynamic LDS the tile would ask for without the plan's clamp to the device limit."""
    p = M.plan(*shape, tile=tile, fast=fast, lds_limit=0)
    return max(p.lds_rows, p.lds_cols)


@pytest.mark.parametrize("shape", M.FFT_OPTION_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_fft2_affine_and_tile_options_are_bit_identical(shape):
    """fft_affine x fft_tile change the block -> image mapping and the tile geometry of the generic passes, never a value.  Legs
    whose tile needs more than 64 KiB of LDS run in test_fft2_tiles_above_64k_of_lds."""
    x = g(fft_input(shape))
    with fft_options():
        ref = {v: ops.fft2(x, inverse=v[0], centered=v[1]).clone() for v in VARIANTS}
    ran = 0
    for aff in (1, 0):
        for tile in M.FFT_TILES:
            p = M.plan(*shape, tile=tile, affine=aff, lds_limit=0)
            big = _lds(shape, tile) > LDS_64K
            print(f"  {shape} fft_affine={aff} fft_tile={tile}: LDS rows {p.lds_rows} B / cols {p.lds_cols} B, lines {p.lr} / {p.lc}"
                  + ("  (above 64 KiB: separate test)" if big else ""))
            if big:
                continue
            with fft_options(fft_affine=aff, fft_tile=tile):
                for v in VARIANTS:
                    assert torch.equal(ops.fft2(x, inverse=v[0], centered=v[1]), ref[v]), (shape, aff, tile, v)
            ran += 1
    assert ran >= 6


@pytest.mark.parametrize("shape", M.FFT_GENERIC256_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_fft2_generic_256_point_passes_vs_fp64(shape):
    """fft_fast = 0: the 256-point lines on the generic Stockham kernel (four radix-4 stages), same reference, same bound."""
    assert M.plan(*shape, fast=0).rows != "fast256" and M.plan(*shape, fast=0).cols != "fast256"
    x = fft_input(shape)
    with fft_options(fft_fast=0):
        for inverse, centered in VARIANTS:
            out = ops.fft2(g(x), inverse=inverse, centered=centered)
            assert_per_item(out, fft2_ref64(x, inverse, centered), FFT_TOL, f"{shape} fft_fast=0 inverse={int(inverse)} centered={int(centered)}")


def test_fft2_tiles_above_64k_of_lds():
    """Option fft_tile is accepted up to 8192 points; on a generic pass that would be 16 * lines * (N + 1) bytes of dynamic LDS,
    above 64 KiB at the legs below (up to 160 KiB at 3 x 2048 x 4), from kernels that never opt in to more than the default
    per-block limit: make_fft_plan clamps the tile to the device's limit.  Every accepted value must run and, being scheduling
    only, give the default tile's bits."""
    legs = list(M.FFT_OVERSIZE_LEGS) + [(s, tile) for s in M.FFT_OPTION_SHAPES for tile in M.FFT_TILES if _lds(s, tile) > LDS_64K]
    assert len(legs) >= 5
    for shape, tile in legs:
        x = g(fft_input(shape))
        with fft_options():
            ref = {v: ops.fft2(x, inverse=v[0], centered=v[1]).clone() for v in VARIANTS[:2]}
        for aff in (1, 0):
            p, c = M.plan(*shape, tile=tile, affine=aff, lds_limit=0), M.plan(*shape, tile=tile, affine=aff)
            print(f"  {shape} fft_affine={aff} fft_tile={tile}: LDS asked rows {p.lds_rows} B / cols {p.lds_cols} B, on a 64 KiB device "
                  f"clamped to {c.lds_rows} B / {c.lds_cols} B")
            with fft_options(fft_affine=aff, fft_tile=tile):
                for v in VARIANTS[:2]:
                    assert torch.equal(ops.fft2(x, inverse=v[0], centered=v[1]), ref[v]), (shape, aff, tile, v)


# =========================================================================================================== C: fused passes
@pytest.fixture(scope="module")
def den(unet_params):
    from tfpnp_amd.pnp import UNetDenoiser2D
    return UNetDenoiser2D(state_dict=unet_params, conv_mode=0)


@pytest.fixture(scope="module")
def oden(unet_params):
    return O.Denoiser(unet_params)


def probe_items(B):
    """First item, last item of the full XCD group, the plainly mapped trailing items."""
    return sorted({i for i in (0, 7, 8, B - 1) if 0 <= i < B})


CSMRI_KEYS = {"admm": ("sigma_d", "mu"), "hqs": ("sigma_d", "mu"), "pg": ("sigma_d", "tau"), "apg": ("sigma_d", "tau", "beta"),
              "redadmm": ("sigma_d", "mu", "lamda")}
CSMRI_LEGS = [("admm", s) for s in ((9, 48, 256), (9, 256, 48), (10, 50, 39), (19, 128, 128))] + \
             [(n, s) for n in ("hqs", "pg", "apg", "redadmm") for s in ((9, 48, 256), (10, 50, 39))]


def _csmri_solver(name, den):
    from tfpnp_amd.tasks import csmri
    return {"admm": csmri.ADMMSolver_CSMRI, "hqs": csmri.HQSSolver_CSMRI, "pg": csmri.PGSolver_CSMRI,
            "apg": csmri.APGSolver_CSMRI, "redadmm": csmri.REDADMMSolver_CSMRI}[name](den)


def test_oracle_solvers_are_per_item(oden):
    """The legs below run the CPU oracle on a few items of the batch only: an item's result must not depend on its neighbours
    (fp32 CPU convolutions may block differently with the batch size, hence a rounding-level bound instead of torch.equal)."""
    B, H, W = 3, 48, 64
    d = synth.make_csmri_batch(B, H, W, ratio=4, seed=901)
    a = csmri_actions(B, 2, 902)
    run = lambda sl: O.csmri_admm(oden, O.admm_reset(t(d["x0"][sl])), t(d["y0"][sl]), t(d["mask"][sl]), t(a["sigma_d"][sl]),
                                  t(a["mu"][sl]))
    pair = run(slice(1, 3))
    for k, i in enumerate((1, 2)):
        e = per_item_rel(pair[k:k + 1], run(slice(i, i + 1)))[0]
        print(f"  oracle item {i} alone vs in a two-item slice: {e:.2e}")
        assert e <= 1e-6
    dp = synth.make_pr_batch(B, 32, 48, S=3, alpha=9.0, seed=903)
    ap = csmri_actions(B, 2, 904, ("sigma_d", "mu", "tau"))
    runp = lambda sl: O.pr_iadmm(oden, O.pr_reset(t(dp["x0"][sl])), t(dp["y0"][sl]), t(dp["mask"][sl]), t(ap["sigma_d"][sl]),
                                 t(ap["mu"][sl]), t(0.5 * ap["tau"][sl]))
    pair = runp(slice(0, 2))
    for i in (0, 1):
        assert per_item_rel(pair[i:i + 1], runp(slice(i, i + 1)))[0] <= 1e-6


@pytest.mark.parametrize("name,shape", CSMRI_LEGS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_csmri_fused_passes_at_mixed_plans_vs_oracle(den, oden, name, shape):
    """The fused k-space passes (row pass -> forward / blend / inverse column pass -> row pass) where one pass is the register
    radix-16 kernel and the other a generic one, with the XCD-affine mapping on and a trailing partial group."""
    B, H, W = shape
    keys = CSMRI_KEYS[name]
    d = synth.make_csmri_batch(B, H, W, ratio=4, sigma_n=15.0, seed=910 + H)
    a = csmri_actions(B, 2, 911 + W, keys)
    sol = _csmri_solver(name, den)
    v0 = sol.reset({"x0": g(d["x0"])})
    out = sol((v0, (g(d["y0"]), g(d["mask"]))), tuple(g(a[k]) for k in keys))
    idx = probe_items(B)
    ref = getattr(O, "csmri_" + name)(oden, v0.cpu()[idx], t(d["y0"][idx]), t(d["mask"][idx]), *[t(a[k][idx]) for k in keys])
    assert out.shape[0] == B and torch.isfinite(out).all()
    assert_per_item(out.cpu()[idx], ref, TOL, f"csmri_{name} {shape} items {idx}")


PR_LEGS = [(9, 3, 48, 256), (9, 3, 256, 48), (3, 3, 50, 39)]        # (B, S, H, W); B * S >= 8 everywhere


@pytest.mark.parametrize("B,S,H,W", PR_LEGS)
def test_pr_iadmm_at_mixed_plans_vs_oracle(den, oden, B, S, H, W):
    """W = 256 with H != 256: the grouped 256-point inverse row kernel (fft256_rows_group_kernel) with the affine mapping over B = 9
    groups -- one full XCD group and a plainly mapped one; H = 256: generic rows + fast columns; 50 x 39: all generic, B * S = 9."""
    from tfpnp_amd.tasks import pr
    d = synth.make_pr_batch(B, H, W, S=S, alpha=9.0, seed=920 + H)
    a = csmri_actions(B, 2, 921 + W, ("sigma_d", "mu", "tau"))
    a["tau"] = (0.5 * a["tau"]).astype(np.float32)
    sol = pr.IADMMSolver_PR(den)
    out = sol((sol.reset({"x0": g(d["x0"])}), (g(d["y0"]), g(d["mask"]))), (g(a["sigma_d"]), g(a["mu"]), g(a["tau"])))
    idx = probe_items(B)
    ref = O.pr_iadmm(oden, O.pr_reset(t(d["x0"][idx])), t(d["y0"][idx]), t(d["mask"][idx]), t(a["sigma_d"][idx]), t(a["mu"][idx]),
                     t(a["tau"][idx]))
    assert_per_item(out.cpu()[idx], ref, TOL, f"pr_iadmm {(B, S, H, W)} items {idx}")


@pytest.mark.parametrize("B,S,H,W", PR_LEGS)
def test_pr_pg_at_mixed_plans_vs_oracle(den, oden, B, S, H, W):
    from tfpnp_amd.tasks import pr
    d = synth.make_pr_batch(B, H, W, S=S, alpha=9.0, seed=930 + H)
    rs = np.random.RandomState(931 + W)
    sd = rs.uniform(5 / 255.0, 50 / 255.0, (B, 2)).astype(np.float32)
    tau = rs.uniform(0.5, 1.2, (B, 2)).astype(np.float32)
    sol = pr.PGSolver_PR(den)
    v0 = sol.reset({"x0": g(d["x0"])})
    out = sol((v0, (g(d["y0"]), g(d["mask"]))), (g(sd), g(tau)))
    idx = probe_items(B)
    with torch.no_grad():
        ref = pr_pg_restated(oden, v0.cpu()[idx], t(d["y0"][idx]), t(d["mask"][idx]), t(sd[idx]), t(tau[idx]))
    assert_per_item(out.cpu()[idx], ref, TOL, f"pr_pg {(B, S, H, W)} items {idx}")


# =========================================================================================================== D: CDP operators
@pytest.mark.parametrize("B,S,H,W", [(3, 4, 256, 256), (5, 2, 48, 256), (2, 3, 50, 39), (1, 1, 16, 16), (9, 1, 15, 33)])
def test_cdp_operators_vs_fp64_and_adjoint_identity(B, S, H, W):
    """A x = F(mask_s x) (un-centered, orthonormal) and A^H y = mean_s conj(mask_s) F^-1 y_s against complex128, per item; then
    <A x, y> = S <x, A^H y> with both sides summed in float64 (y is correlated with A x so that neither side is a small
    difference of large terms)."""
    seed = 940 + B + S + H
    x, mask = complex_inputs((B, 1, H, W), seed), complex_inputs((B, S, H, W), seed + 1)
    c128 = lambda a: torch.view_as_complex(t(a).double().contiguous())
    Ax_ref = torch.fft.fft2(c128(mask) * c128(x), dim=(-2, -1), norm="ortho")
    y = (complex_inputs((B, S, H, W), seed + 2) + torch.view_as_real(Ax_ref).numpy()).astype(np.float32)
    AHy_ref = (c128(mask).conj() * torch.fft.ifft2(c128(y), dim=(-2, -1), norm="ortho")).mean(1, keepdim=True)
    Ax = ops.cdp_forward(g(x), g(mask))
    AHy = ops.cdp_backward(g(y), g(mask))
    assert tuple(Ax.shape) == (B, S, H, W, 2) and tuple(AHy.shape) == (B, 1, H, W, 2)
    assert_per_item(Ax.reshape(B * S, H, W, 2), torch.view_as_real(Ax_ref).reshape(B * S, H, W, 2), FFT_TOL, f"cdp_forward {(B, S, H, W)} (per mask)")
    assert_per_item(AHy, torch.view_as_real(AHy_ref), FFT_TOL, f"cdp_backward {(B, S, H, W)}")
    lhs = float((Ax.double().cpu() * t(y).double()).sum())
    rhs = S * float((t(x).double() * AHy.double().cpu()).sum())
    print(f"  adjoint identity {(B, S, H, W)}: <Ax,y> {lhs:.9e}  S<x,AHy> {rhs:.9e}  relative {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


# =========================================================================================================== E: Radon backprojection
def backprojection64(sino, angles, R):
    """oracle.pnp_oracle.radon_backprojection in float64: the same formula, cos / sin rounded to fp32 as the device table is."""
    B, _, V, det = sino.shape
    s = torch.as_tensor(sino).double()
    c0 = torch.arange(R, dtype=torch.float64) - (R / 2 - 0.5)
    ys, xs = torch.meshgrid(c0, c0, indexing="ij")
    out = torch.zeros(B, 1, R, R, dtype=torch.float64)
    for v in range(V):
        c, sn = float(np.float32(math.cos(float(angles[v])))), float(np.float32(math.sin(float(angles[v]))))
        sp = xs * c + ys * sn + (det / 2 - 0.5)
        s0 = torch.floor(sp)
        f = sp - s0
        for d in (0, 1):
            si = (s0 + d).long()
            ok = (si >= 0) & (si < det)
            out[:, 0] += s[:, 0, v][:, si.clamp(0, det - 1)] * ((f if d else 1 - f) * ok)[None]
    return out


def loud_sinogram(B, V, det, seed):
    y = np.random.RandomState(seed).standard_normal((B, 1, V, det)).astype(np.float32)
    y[..., :2], y[..., -2:] = 5.0, -3.0          # first / last two detector bins
    y[:, :, 0, 2:-2] = 7.0                       # first view
    if V > 1:
        y[:, :, -1, 2:-2] = -2.0                 # last view
    return y


RADON_CASES = [(16, 1, 1), (17, 3, 2), (31, 7, 1), (33, 30, 2), (50, 11, 3), (97, 13, 1), (128, 60, 1), (300, 5, 1), (40, 6, 11),
               (64, 236, 2), (64, 237, 2), (200, 240, 1)]


@pytest.mark.parametrize("R,V,B", RADON_CASES)
def test_radon_backprojection_sweep_vs_oracle_and_fp64(R, V, B):
    """Both backprojection kernels: the LDS-window kernel (V * 260 B <= 60 KiB, i.e. V <= 236: edge tiles with R no multiple of
    32, clamped pixels, the 64-bin window) and the per-pixel gather kernel above that, on random sinograms with LOUD first / last
    detector bins and first / last views.  The kernels do the oracle's fp32 operations in the oracle's order, hence the forward
    sweep's 2e-6 (max / max) against it; against float64 the device must be no further than the fp32 oracle is (that distance,
    6e-8 .. 2e-5 here, is position rounding times the slope of a random sinogram -- an absolute fp64 bound would be wrong).
    By geometry (det = ceil(sqrt 2 R)) every pixel projects inside [0.2, det - 1.2]: no shape reaches the out-of-range taps, and
    this test does not pretend to."""
    angles, det = O.radon_geometry(R, V)
    assert ((V * 260 <= 60 * 1024) == (V <= 236)) and ops.radon_det_count(R) == det
    y = loud_sinogram(B, V, det, 950 + R + V)
    out = ops.radon_backprojection(g(y), R).cpu()
    ref = O.radon_backprojection(t(y), angles, R)
    r64 = backprojection64(y, angles, R)
    mx = float(ref.abs().max())
    e = float((out - ref).abs().max()) / mx
    e_gpu64 = float((out.double() - r64).abs().max() / r64.abs().max())
    e_or64 = float((ref.double() - r64).abs().max() / r64.abs().max())
    print(f"  R={R} V={V} B={B} ({'LDS window' if V <= 236 else 'gather'} kernel): vs oracle {e:.2e} (bit-identical: {torch.equal(out, ref)})"
          f"   vs fp64 {e_gpu64:.2e}   oracle vs fp64 {e_or64:.2e}")
    assert tuple(out.shape) == (B, 1, R, R)
    assert e <= 2e-6, (R, V, B)
    assert e_gpu64 <= 1.5 * e_or64 + 2e-6, (R, V, B)
    for b in range(B):      # per item: a mis-addressed image must be named
        eb = float((out[b] - ref[b]).abs().max()) / mx
        assert eb <= 2e-6, (R, V, B, b)


def test_radon_backprojection_gather_kernel_equals_lds_kernel():
    """The two kernels on the SAME angles.  The view angles are linspace(0, 179 deg, V), so a 237-view sinogram with a silent last
    view is no 236-view sinogram; what switches kernels at equal V is the batch (grid.z holds 65535 images): B = 65536 copies of
    three sinograms run on the gather kernel, the three alone on the LDS kernel."""
    R, V, reps = 5, 4, 65536 // 4 + 1
    angles, det = O.radon_geometry(R, V)
    y3 = loud_sinogram(4, V, det, 960)
    lds = ops.radon_backprojection(g(y3), R)
    big = ops.radon_backprojection(g(y3).repeat(reps, 1, 1, 1), R)
    assert big.shape[0] > 65535
    ref = O.radon_backprojection(t(y3), angles, R)
    assert float((lds.cpu() - ref).abs().max() / ref.abs().max()) <= 2e-6
    d = (big.view(reps, 4, 1, R, R) - lds[None]).abs().amax(dim=(1, 2, 3, 4)).cpu()
    print(f"  gather vs LDS-window kernel, {big.shape[0]} images: max |diff| {float(d.max()):.2e} (bit-identical: {bool((d == 0).all())})")
    assert float(d.max()) <= 2e-6 * float(ref.abs().max()), int(d.argmax())


# =========================================================================================================== F: PSNR
@pytest.mark.parametrize("B,n", [(1, 1), (3, 7), (2, 31), (5, 50 * 39), (65, 4096), (2, 512 * 512)])
def test_psnr_sweep_vs_fp64(B, n):
    """The reward: 32 chunks per item (some empty for n < 32, ragged for n % 32 != 0), 65 items = two blocks of the final kernel.
    Outputs in [-0.2, 1.2] so that the clamp matters.  A relative error delta of the mean squared error moves the result
    4.3 * delta dB: the suite's bound (rtol 1e-5, atol 1e-4 dB) leaves two orders of margin over fp32 summation."""
    from tfpnp_amd.env import torch_psnr
    rs = np.random.RandomState(970 + n % 1000)
    o = rs.uniform(-0.2, 1.2, (B, 1, n)).astype(np.float32)
    gt = rs.uniform(0, 1, (B, 1, n)).astype(np.float32)
    mse = ((np.clip(o.astype(np.float64), 0, 1) - gt.astype(np.float64)) ** 2).reshape(B, -1).mean(1)
    ref = (10 * np.log10(1.0 / mse))[:, None]
    for name, fn in (("torch_psnr", torch_psnr), ("ops.psnr", ops.psnr)):
        out = fn(g(o), g(gt)).cpu().numpy().astype(np.float64)
        err = np.abs(out - ref)
        print(f"  {name} B={B} n={n}: worst item {int(err.argmax())}: |dPSNR| {err.max():.2e} dB at {float(ref.ravel()[err.argmax()]):.3f} dB")
        assert out.shape == (B, 1)
        assert np.all(err <= 1e-4 + 1e-5 * np.abs(ref)), (name, np.nonzero(err > 1e-4 + 1e-5 * np.abs(ref))[0].tolist())
