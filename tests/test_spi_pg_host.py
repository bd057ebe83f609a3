"""CPU tests of PGSolver_SPI's definition (tests/spi_pg_ref.py): its fixed points, the closed-form VJP of the adjoint kernel against
float64 autograd, the fp32 restatement's distance from float64 on the GPU test's inputs, and the Python surface without a device."""
import os
import re

import numpy as np
import pytest
import torch

from tests import spi_pg_ref as R
from tests.conftest import ROOT

NEW_SYMBOLS = ("pnpx_spi_pg_step", "pnpx_spi_pg", "pnpx_spi_pg_train", "pnpx_spi_pg_backward")
KS = (4, 6, 8, 10)


def iterate(K, tau, start, n):
    """max |x - MLE| over every K1 = 0 .. K^2 after n steps without a denoiser, float64."""
    x0, m = R.mle(K)
    x0 = x0.view(1, 1, 1, -1)
    Kmap = torch.full_like(x0, K / 10.0)
    x = x0.clone() if start == "x0" else torch.zeros_like(x0)
    t = torch.tensor([tau], dtype=torch.float64)
    for _ in range(n):
        x = R.step(x, x0, Kmap, t)
    return float((x.view(-1) - m).abs().max())


@pytest.mark.parametrize("start,tau,bound", [("x0", 0.5, 1e-4), ("x0", 1.0, 1e-4), ("x0", 1.5, 1e-4), ("zeros", 1.0, 1e-6),
                                             ("zeros", 1.5, 1e-6)])
def test_fixed_points_are_the_clamped_mle(start, tau, bound):
    """30 steps from x0 (tau 0.5, 1, 1.5: < 1e-4) and from zeros (tau 1, 1.5: < 1e-6) reach the clamped maximum-likelihood value for
    K in {4, 6, 8, 10} and every K1.  Conditions on the definition: measured 7.4e-6 / < 1e-12 / < 1e-10 and <= 1.4e-9 / 2.9e-9."""
    worst = max(iterate(K, tau, start, 30) for K in KS)
    print(f"start {start}, tau {tau}: max |x - MLE| after 30 iterations {worst:.2e}")
    assert worst < bound


def test_ten_iterations_and_the_edge_of_the_actor_range():
    """The other figures DESIGN.md quotes: 10 iterations from x0 (7.8e-3 / 3.3e-5 / 4e-5 at tau 0.5 / 1 / 1.5), and tau = 2, the edge of
    ResNetActor_PG's range, which ends in a limit cycle (about 3.5e-2) instead of converging: expected of a gradient step."""
    ten = {tau: max(iterate(K, tau, "x0", 10) for K in KS) for tau in (0.5, 1.0, 1.5)}
    edge = max(iterate(K, 2.0, "x0", n) for K in KS for n in (30, 31))
    print(f"10 iterations from x0: {ten};  tau = 2 after 30 / 31: {edge:.2e}")
    assert ten[0.5] < 2e-2 and ten[1.0] < 1e-4 and ten[1.5] < 1e-4
    assert 1e-3 < edge < 1e-1


def vjp_grid():
    """float64 grid: x0 = K1 / K^2 for every K1 of K = 4 (0 and 1 included) against x in [-0.3, 1.4] plus zeros, values below
    x_lo, x_lo itself and tiny values (c >= 1: the Newton branch; large x, small x0: c < 1), at three tau per item row."""
    K = 4
    x0 = torch.arange(K * K + 1, dtype=torch.float64) / (K * K)
    xs = torch.cat([torch.linspace(-0.3, 1.4, 35, dtype=torch.float64),
                    torch.tensor([0.0, 0.003, 0.5 / 16 * 0.5, 0.5 / 16, 0.04, 1.0], dtype=torch.float64)])
    taus = torch.tensor([0.3, 1.0, 2.0], dtype=torch.float64)
    B, H, W = len(taus), len(x0), len(xs)
    x = xs.view(1, 1, 1, W).expand(B, 1, H, W).contiguous()
    a = x0.view(1, 1, H, 1).expand(B, 1, H, W).contiguous()
    return x, a, torch.full_like(x, K / 10.0), taus


def test_closed_form_vjp_equals_float64_autograd():
    """h', d/d tau and the pass / live rules of spi_pg_adjoint_kernel against autograd of `step`, pixel by pixel (the map is
    pointwise: the gradient of sum(z) IS the per-pixel derivative).  The grid holds both branches, both clamp sides, x < x_lo,
    x0 = 0 and x0 = 1."""
    x, x0, Kmap, tau = vjp_grid()
    xg = x.clone().requires_grad_(True)
    tg = tau.view(-1, 1, 1, 1).expand_as(x).contiguous().requires_grad_(True)      # one tau per pixel: per-pixel dz/dtau
    z = R.step(xg, x0, Kmap, tg)
    assert torch.equal(z.detach(), R.step(x, x0, Kmap, tau))
    gx, gt = torch.autograd.grad(z.sum(), (xg, tg))
    ok, live, hh, hp, dzdx, dzdt = R.closed_form(x, x0, Kmap, tau)
    c, x_lo = R.parts(x, x0, Kmap, tau)["c"], R.parts(x, x0, Kmap, tau)["x_lo"]
    # every region is on the grid
    assert bool((c < 1).any()) and bool((c >= 1).any()) and bool((~live).any()) and bool(live.any())
    pre = R.parts(x, x0, Kmap, tau)["pre"]
    assert bool((pre < 0).any()) and bool((pre > 1).any()) and bool(ok.any())
    assert bool((x0 == 0).any()) and bool((x0 == 1).any()) and bool((x == x_lo).any())
    assert torch.isfinite(dzdx).all() and torch.isfinite(dzdt).all()
    ex = float((gx - dzdx).abs().max() / gx.abs().max())
    et = float((gt - dzdt).abs().max() / gt.abs().max())
    print(f"closed form vs float64 autograd: dz/dx {ex:.2e}, dz/dtau {et:.2e} (max-abs over max-abs)")
    assert ex < 1e-12 and et < 1e-12
    # x0 = 0: h = 1, z = x - tau with no special case;  x0 = 1: g < 0 always (the step never moves down)
    assert torch.equal(hh[x0 == 0], torch.ones_like(hh[x0 == 0]))
    assert bool((hh[x0 == 1] < 0).all())


def test_loop_restatement_applies_the_columns_in_order():
    """spi_pg(den, ...) with a recording denoiser: T columns, iter_num, and the state passed through at iter_num = 0."""
    x, x0, Kmap, _ = (torch.from_numpy(a) for a in R.step_case())
    sig = torch.tensor([[0.1, 0.2, 0.3]] * 3)
    tau = torch.tensor([[0.5, 1.0, 1.5]] * 3)
    seen = []

    def den(z, s):
        seen.append(s.clone())
        return z * 0.5
    out = R.spi_pg(den, x, x0, Kmap, sig, tau)
    assert len(seen) == 3 and all(torch.equal(s, sig[:, i]) for i, s in enumerate(seen))
    want = x
    for i in range(3):
        want = 0.5 * R.step(want, x0, Kmap, tau[:, i])
    assert torch.equal(out, want)
    assert R.spi_pg(den, x, x0, Kmap, sig, tau, iter_num=0) is x and len(seen) == 3
    assert torch.equal(R.spi_pg(den, x, x0, Kmap, sig, tau, iter_num=1), 0.5 * R.step(x, x0, Kmap, tau[:, 0]))


def test_fp32_restatement_distance_from_float64():
    """The figure the step kernel's bar is derived from (tests/test_gpu_spi_pg.py, profiles/spi_pg.md): rel-L2 of the fp32 CPU
    restatement from the float64 one on the GPU test's very inputs.  A few 1e-8: one rounding per operation on values of order 1."""
    x, x0, Kmap, tau = (torch.from_numpy(a) for a in R.step_case())
    e = R.rel_l2(R.step(x, x0, Kmap, tau), R.step(x.double(), x0.double(), Kmap.double(), tau.double()))
    print(f"step case: fp32 vs float64 restatement rel-L2 {e:.2e}")
    assert 0 < e < 2.5e-6            # 4 x this figure has to stay under the 1e-5 cap of the bar rule
    x0s, Kmaps = R.synth(3, 24, 40, (4, 6, 8), 11)
    assert x0s.shape == (3, 1, 24, 40) and x0s.min() >= 0 and x0s.max() <= 1
    for b, K in enumerate((4, 6, 8)):
        assert np.allclose(x0s[b] * K * K, np.round(x0s[b] * K * K), atol=1e-4) and Kmaps[b, 0, 0, 0] == np.float32(K / 10.0)


def test_header_and_binding_agree_on_the_new_names():
    from tfpnp_amd import _lib, ops, torch_ops
    from tfpnp_amd.utils import transforms
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pnpx_[a-z0-9_]+)\s*\(", src))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for op in ("spi_pg_step", "spi_pg", "spi_pg_train", "spi_pg_backward"):
        assert op in torch_ops.ALL_OPS and hasattr(torch.ops.pnpx, op) and callable(getattr(ops, op)), op
    assert callable(transforms.spi_pg_step)
    with pytest.raises(_lib.PnpxError, match="no CPU path"):
        transforms.spi_pg_step(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), torch.full((1, 1, 4, 4), 0.6), torch.ones(1))


def test_python_surface_without_gpu():
    from tfpnp_amd.tasks.spi import ADMMSolver_SPI, PGSolver_SPI, create_solver_spi

    class Opt:
        solver = "pg_spi"
    s = create_solver_spi(Opt(), None)
    assert type(s) is PGSolver_SPI and s.num_var == 1 and s.hyper_keys == ("sigma_d", "tau") and s.init_vars == ("x0",)
    x0 = torch.rand(2, 1, 8, 8)
    state = {"x0": x0, "K": torch.full_like(x0, 0.6)}
    v = s.reset(state)
    assert torch.equal(v, x0) and v is not x0 and s.get_output(v) is v
    assert s.filter_aux_inputs(state) == (state["x0"], state["K"])
    assert s.filter_hyperparameter({"sigma_d": 1, "tau": 2, "mu": 3}) == (1, 2)
    Opt.solver = "admm_spi"
    assert type(create_solver_spi(Opt(), None)) is ADMMSolver_SPI
    Opt.solver = "hqs_spi"
    with pytest.raises(NotImplementedError):
        create_solver_spi(Opt(), None)
    # a denoiser without a native context is refused with PnPSolver._ctx's message, before anything native is called
    p = torch.ones(2, 1)
    with pytest.raises(NotImplementedError, match="PGSolver_SPI needs a native denoiser"):
        PGSolver_SPI(torch.nn.Identity())((v, (x0, state["K"])), (p, p))
    with pytest.raises(NotImplementedError, match="PGSolver_SPI needs a native denoiser"):
        PGSolver_SPI(torch.nn.Identity())((v.requires_grad_(True), (x0, state["K"])), (p, p))
