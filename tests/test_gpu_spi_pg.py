"""PGSolver_SPI (pnpx_spi_pg_step, pnpx_spi_pg, _train, _backward): the step kernel against the fp32 and the float64 restatement of
tests/spi_pg_ref.py, the loop against the restatement run with the oracle's denoisers (UNet and DRUNet, both convolution
families), a ragged batch, the fused VJP against the same loop composed from A.denoise and torch pointwise ops, and one SPIEnv
step driven by ResNetActor_PG.  The reference has no PG solver for SPI: the restatement is the definition."""
import numpy as np
import pytest
import torch

from tests import spi_pg_ref as R
from tests.golden_inputs import csmri_actions
from tfpnp_amd import autograd as A
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4              # the project's solver parity bar
KS = (4, 6, 8)


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def g(a, grad=False):
    return t(a).to(dev()).requires_grad_(grad)


rel = R.rel_l2


@pytest.fixture(scope="module", params=[1, 0], ids=["hs_f16x3", "f32_mfma"])
def den(unet_params, request):
    """Both conv_modes: half-split f16 MFMA and plain fp32 MFMA."""
    from tfpnp_amd.pnp import UNetDenoiser2D
    d = UNetDenoiser2D(state_dict=unet_params, conv_mode=request.param)
    d.mode = request.param            # for the printed figures
    return d


@pytest.fixture(scope="module")
def oden(unet_params):
    from oracle import pnp_oracle as O
    return O.Denoiser(unet_params)


def actions(B, T, seed):
    """sigma_d in [5, 50] / 255, tau in [0.1, 1.5] with one entry at 2, the edge of ResNetActor_PG's range."""
    a = csmri_actions(B, T, seed, ("sigma_d", "tau"))
    a["tau"][0, 0] = 2.0
    return a["sigma_d"], a["tau"]


def test_step_kernel_vs_restatement():
    """ops.spi_pg_step on B = 3, K = (4, 6, 8), tau = (0.1, 1, 2), 17 x 15.  Bar (the rule of profiles/fanbeam.md): 4 x the rel-L2 of the
    fp32 CPU restatement from the float64 one on these very inputs, and no more than 1e-5; both of the kernel's distances (from
    the fp32 and from the float64 restatement) stay under it.  profiles/spi_pg.md holds the figures."""
    from tfpnp_amd import ops
    from tfpnp_amd.utils import transforms as Tr
    x, x0, Kmap, tau = (t(a) for a in R.step_case())
    assert x.shape[2] * x.shape[3] % 256 != 0
    ref32 = R.step(x, x0, Kmap, tau)
    ref64 = R.step(x.double(), x0.double(), Kmap.double(), tau.double())
    measured = rel(ref32, ref64)
    bar = min(4 * measured, 1e-5)
    out = ops.spi_pg_step(x.to(dev()), x0.to(dev()), Kmap.to(dev()), tau.to(dev()))
    e32, e64 = rel(out, ref32), rel(out, ref64)
    print(f"  spi_pg_step: fp32 vs float64 restatement {measured:.3e}, bar {bar:.3e}; kernel vs fp32 {e32:.3e}, vs float64 {e64:.3e}")
    assert 0 < measured and e32 < bar and e64 < bar
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0 and bool(torch.isfinite(out).all())
    o = out.cpu()
    assert torch.equal(o[:, 0, 0], torch.clamp(x[:, 0, 0] - tau.view(3, 1), 0, 1))      # x0 = 0: z = x - tau, no special case
    assert bool((o[:, 0, 1] >= torch.clamp(x[:, 0, 1], 0, 1)).all())                    # x0 = 1: the step never moves down
    assert bool((o[:, 0, 2, :5] > 0).all())                                             # a zero with x0 > 0 leaves zero
    # the same bytes through the dispatcher op and with one K value per item
    assert torch.equal(Tr.spi_pg_step(x.to(dev()), x0.to(dev()), Kmap.to(dev()), tau.to(dev())), out)
    assert torch.equal(ops.spi_pg_step(x.to(dev()), x0.to(dev()), Kmap[:, :, :1, :1].to(dev()), tau.view(3, 1).to(dev())), out)


def test_step_refusals():
    from tfpnp_amd import _lib, ops
    from tfpnp_amd._lib import PnpxError
    x = torch.rand(2, 1, 8, 8, device=dev())
    K = torch.full_like(x, 0.6)
    tau = torch.ones(2, device=dev())
    for bad in [(x[:, 0], x, K, tau), (x, x[:1], K, tau), (x, x, K[:, :, :3], tau), (x, x, K, tau[:1]), (x.double(), x, K, tau)]:
        with pytest.raises(PnpxError):
            ops.spi_pg_step(*bad)
    lib = _lib.lib()
    ctx = ops.default_context(dev())
    p = lambda a: a.data_ptr()
    out = torch.empty_like(x)
    assert lib.pnpx_spi_pg_step(ctx.handle, p(x), p(x), p(K), p(tau), p(out), 2, 0, 8, None) == 1          # PNPX_ERR_ARG
    assert lib.pnpx_spi_pg_step(ctx.handle, p(x), None, p(K), p(tau), p(out), 2, 8, 8, None) == 1
    assert b"pnpx_spi_pg_step: bad argument" in lib.pnpx_last_error()
    assert lib.pnpx_spi_pg(ctx.handle, p(x), p(out), p(x), p(K), p(tau), p(tau), 1, 2, 8, 8, 2, None) == 1   # param_stride < T
    assert b"pnpx_spi_pg: bad argument" in lib.pnpx_last_error()


def loop_case(B, H, W, T, seed):
    x0, Kmap = R.synth(B, H, W, KS[:B], seed)
    sd, tau = actions(B, T, seed + 1)
    return x0, Kmap, sd, tau


def test_pg_spi_vs_restatement(den, oden):
    """B = 3, 24 x 40, K = (4, 6, 8), T = 3 columns; iter_num None / 0 / 1 / 2 (2: param_stride > T) against the fp32 restatement
    with the oracle's UNet (which sits 4.6-4.8e-7 from float64 on such a case)."""
    from tfpnp_amd.tasks.spi import PGSolver_SPI
    B, H, W, T = 3, 24, 40, 3
    x0, Kmap, sd, tau = loop_case(B, H, W, T, 31)
    sol = PGSolver_SPI(den)
    v0 = sol.reset({"x0": g(x0)})
    assert tuple(v0.shape) == (B, 1, H, W)
    for it in (None, 0, 1, 2):
        out = sol((v0, (g(x0), g(Kmap))), (g(sd), g(tau)), iter_num=it)
        with torch.no_grad():
            ref = R.spi_pg(oden, t(x0), t(x0), t(Kmap), t(sd), t(tau), iter_num=it)
        e = rel(out, ref)
        print(f"  PGSolver_SPI conv_mode {den.mode} T={T if it is None else it}: rel-L2 vs restatement {e:.2e}")
        assert e < TOL, it
        if it == 0:
            assert torch.equal(out, v0) and out.data_ptr() != v0.data_ptr()


@pytest.mark.parametrize("conv_mode", [None, 1], ids=["f32", "hs_f16x3"])
def test_pg_spi_drunet_vs_restatement(conv_mode):
    """Config #5's pairing: the DRUNet prox in both families, B = 2, 32 x 40, T = 2, against the restatement with the oracle's DRUNet."""
    from oracle import pnp_oracle as O
    from tfpnp_amd.pnp import DRUNetDenoiser2D
    from tfpnp_amd.tasks.spi import PGSolver_SPI
    B, H, W, T = 2, 32, 40, 2
    params = synth.make_drunet_params(0)
    x0, Kmap, sd, tau = loop_case(B, H, W, T, 41)
    sol = PGSolver_SPI(DRUNetDenoiser2D(state_dict=params, conv_mode=conv_mode))
    out = sol((sol.reset({"x0": g(x0)}), (g(x0), g(Kmap))), (g(sd), g(tau)))
    with torch.no_grad():
        ref = R.spi_pg(O.DRUNetDenoiser(params), t(x0), t(x0), t(Kmap), t(sd), t(tau))
    e = rel(out, ref)
    print(f"  PGSolver_SPI + DRUNet conv_mode {conv_mode}: rel-L2 vs restatement {e:.2e}")
    assert e < TOL


def test_pg_spi_ragged_batch_equals_the_full_call(den):
    """Rows [1], then [0, 2] of a B = 3 call: an item's result does not depend on the batch it arrives in."""
    from tfpnp_amd.tasks.spi import PGSolver_SPI
    x0, Kmap, sd, tau = (g(a) for a in loop_case(3, 32, 32, 3, 51))
    sol = PGSolver_SPI(den)
    v0 = sol.reset({"x0": x0})
    full = sol((v0, (x0, Kmap)), (sd, tau))
    for rows in ([1], [0, 2]):
        r = torch.tensor(rows, device=dev())
        part = sol((v0[r].contiguous(), (x0[r].contiguous(), Kmap[r].contiguous())), (sd[r].contiguous(), tau[r].contiguous()))
        assert torch.equal(part, full[r]), rows


def composed_pg(sol, x, x0, Kmap, sigma_d, tau, iter_num):
    """PGSolver_SPI's loop from A.denoise and torch pointwise ops on device tensors: what the fused native VJP is held against."""
    ctx = sol._ctx(x)
    K = Kmap[:, :1, :1, :1] * 10
    x_lo = (0.5 / (K * K)).expand_as(x)
    for i in range(iter_num):
        q = -torch.expm1(-torch.clamp(x, min=x_lo))
        h = (1 - x0 / q) / torch.clamp(x0 * (1 - q) / (q * q), min=1)
        z = torch.clamp(x - tau[:, i].reshape(-1, 1, 1, 1) * h, 0, 1)
        x = A.denoise(ctx, z, sigma_d[:, i])
    return x


def test_pg_spi_fused_vjp_vs_composed_autograd(den):
    """pnpx_spi_pg_train / _backward against the composed loop on a perturbed state, B = 2, 32 x 32, T = 3 of 4 columns: every input's
    gradient within 2e-2 of its norm (the bar of the other fused-vs-composed tests), exact zeros past iter_num, everything finite,
    a non-zero tau gradient for every item (the point of the solver) and equal bytes from two runs."""
    from tfpnp_amd.tasks.spi import PGSolver_SPI
    B, H, T = 2, 32, 3
    x0, Kmap, sd, tau = loop_case(B, H, H, T + 1, 61)
    x0, Kmap = g(x0), g(Kmap)
    sol = PGSolver_SPI(den)
    v0 = sol.reset({"x0": x0})
    v0 = v0 + 0.02 * torch.randn(v0.shape, device=v0.device, generator=torch.Generator(v0.device).manual_seed(10))
    wts = torch.randn(v0.shape, device=v0.device, generator=torch.Generator(v0.device).manual_seed(12))

    def grads(fn):
        leaves = [v0.clone().requires_grad_(True), g(sd, True), g(tau, True)]
        out = fn(*leaves)
        (out * wts).sum().backward()
        return out.detach(), [l.grad for l in leaves]

    out_f, gf = grads(lambda v, s_, t_: sol((v, (x0, Kmap)), (s_, t_), iter_num=T))
    out_c, gc = grads(lambda v, s_, t_: composed_pg(sol, v, x0, Kmap, s_, t_, T))
    with torch.no_grad():
        # the training forward parks the denoiser's activations and runs its network tail unfused, so it is the inference forward
        # to rounding, not to the bit: the claim and the bar of test_hqs_ct_fused_vjp_vs_composed_autograd
        e = rel(out_f, sol((v0, (x0, Kmap)), (g(sd), g(tau)), iter_num=T))
        print(f"  PGSolver_SPI conv_mode {den.mode} training forward vs inference forward: {e:.2e}")
        assert e < 1e-6
    assert rel(out_f, out_c) < 1e-5
    for name, a, b in zip(("variables", "sigma_d", "tau"), gf, gc):
        e = rel(a, b)
        print(f"  PGSolver_SPI conv_mode {den.mode} fused vs composed d/d{name}: {e:.2e}")
        assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0 and a.shape == b.shape and e < 2e-2, name
    for k in (1, 2):
        assert float(gf[k][:, T:].abs().max()) == 0.0
    assert bool((gf[2][:, :T].abs().amax(dim=1) > 0).all())
    _, gf2 = grads(lambda v, s_, t_: sol((v, (x0, Kmap)), (s_, t_), iter_num=T))
    assert all(torch.equal(a, b) for a, b in zip(gf, gf2))


def test_spi_env_step_with_pg_actor(unet_params):
    """One SPIEnv reset and step with PGSolver_SPI at B = 3, 32 x 32: the policy observation has 1 + 3 channels, ResNetActor_PG(3,
    pack) maps it to (sigma_d, tau), the environment's state equals the direct solver call and the reward is finite."""
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.policy import ResNetActor_PG
    from tfpnp_amd.tasks import spi

    class Opt:
        solver = "pg_spi"
    sol = spi.create_solver_spi(Opt(), UNetDenoiser2D(state_dict=unet_params))
    assert type(sol) is spi.PGSolver_SPI
    n, pack = 3, 2
    data = {k: g(v) for k, v in synth.make_spi_batch(n, 32, 32, K=6, seed=71).items()}
    env = spi.SPIEnv(None, sol, max_episode_step=3)
    ob = env.reset(data)
    assert tuple(env.state["solver"].shape) == (n, 1, 32, 32)
    pob = env.get_policy_ob(ob)
    assert tuple(pob.shape) == (n, 4, 32, 32)                           # x, x0, K, T
    actor = ResNetActor_PG(3, pack, state_dict={k: t(v) for k, v in synth.make_policy_params(4, 2 * pack).items()})
    action, _, _, _ = actor(pob, torch.zeros(n, dtype=torch.int64, device=dev()), False, None)
    assert tuple(action["sigma_d"].shape) == tuple(action["tau"].shape) == (n, pack)
    assert float(action["tau"].min()) >= 0 and float(action["tau"].max()) <= 2
    v0 = env.state["solver"].clone()
    want = sol((v0, (data["x0"], data["K"])), (action["sigma_d"], action["tau"]))
    ob, ob_masked, reward, all_done, info = env.step(action)
    assert torch.equal(env.state["solver"], want) and torch.equal(env.state["output"], want) and torch.equal(ob.variables, want)
    assert tuple(reward.shape) == (n, 1) and bool(torch.isfinite(reward).all()) and not all_done
    assert tuple(env.get_policy_ob(ob_masked).shape) == (n, 4, 32, 32)
