"""HQSSolver_CT (pnpx_ct_hqs, _train, _backward) on the parallel pair and on a fan-beam pair: the forward against the restatement
of tests/fanbeam_ref.py run with the oracle's denoiser, the fused VJP against the same loop composed from tfpnp_amd.autograd
blocks, a ragged batch, and one CTEnv episode step driven by ResNetActor_HQS."""
import numpy as np
import pytest
import torch

from tests import fanbeam_ref as F
from tests.golden_inputs import csmri_actions
from tfpnp_amd import autograd as A
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4              # the solver parity bar (test_ct_vs_oracle)
B, R, V, T = 2, 32, 20, 3


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def g(a, grad=False):
    return t(a).to(dev()).requires_grad_(grad)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def fan():
    from tfpnp_amd.utils.transforms import FanBeam
    return FanBeam(1.5 * R, 0.5 * R)


@pytest.fixture(scope="module", params=[1, 0], ids=["hs_f16x3", "f32_mfma"])
def den(unet_params, request):
    """Both conv_modes: half-split f16 MFMA (default) and plain fp32 MFMA."""
    from tfpnp_amd.pnp import UNetDenoiser2D
    return UNetDenoiser2D(state_dict=unet_params, conv_mode=request.param)


@pytest.fixture(scope="module")
def oden(unet_params):
    from oracle import pnp_oracle as O
    return O.Denoiser(unet_params)


def case(geometry, n=B, seed=95):
    """y0 = A gt with 5 % multiplicative noise, x0 = A^T y0 / |A|^2, measured with the package's own projector."""
    from tfpnp_amd.utils import transforms as Tr
    radon = Tr.RadonGenerator()(R, V, device=dev(), geometry=geometry)
    sino = radon.forward(g(synth.phantom_batch(n, R, R, seed)))
    noise = np.random.RandomState(seed + 1).standard_normal(tuple(sino.shape)).astype(np.float32)
    y0 = sino * (1 + 0.05 * g(noise))
    return radon, y0, radon.backprojection_norm(y0), g(np.full((n, 1, R, R), V / 120.0, np.float32))


def cpu_pair(geometry):
    """The CPU projector pair of the reference loop: the oracle's parallel pair, or the fp32 fan restatement."""
    if geometry is None:
        from oracle import pnp_oracle as O
        angles, det = O.radon_geometry(R, V)
        return (lambda x: O.radon_forward(x, angles, det)), (lambda y: O.radon_backprojection(y, angles, R))
    gm = F.Geom(R, *geometry.resolve(R, V))
    return (lambda x: F.fan_forward(x, gm)), (lambda y: F.fan_backprojection(y, gm))


@pytest.mark.parametrize("kind", ["parallel", "fan"])
def test_hqs_ct_vs_restatement(den, oden, kind):
    from tfpnp_amd.tasks import ct
    geometry = fan() if kind == "fan" else None
    radon, y0, x0, view = case(geometry)
    fwd, bwd = cpu_pair(geometry)
    assert rel(radon.forward(x0), fwd(x0.cpu())) < 1e-5 and rel(radon.backprojection(y0), bwd(y0.cpu())) < 1e-5
    a = csmri_actions(B, T, 83, ("sigma_d", "mu"))
    sol = ct.HQSSolver_CT(den, geometry)
    sol.radon_generator.opnorms[(R, V) if geometry is None else (R, V, geometry.key())] = radon.opnorm
    v0 = sol.reset({"x0": x0})
    assert tuple(v0.shape) == (B, 2, R, R)
    for it in (None, 0, 1):
        out = sol((v0, (y0, view)), (g(a["sigma_d"]), g(a["mu"])), iter_num=it)
        ref = F.ct_hqs(oden, fwd, bwd, v0.cpu(), y0.cpu(), radon.opnorm, t(a["sigma_d"]), t(a["mu"]), iter_num=it)
        e = rel(out, ref)
        print(f"  HQSSolver_CT {kind} T={T if it is None else it}: rel-L2 vs restatement {e:.2e}")
        assert e < TOL, (kind, it)
        if it == 0:
            assert torch.equal(out, v0)


@pytest.mark.parametrize("kind", ["parallel", "fan"])
def test_hqs_ct_ragged_batch_equals_the_full_call(den, kind):
    """Rows [1], then [0, 2] of a B = 3 call: an item's result does not depend on the batch it arrives in."""
    from tfpnp_amd.tasks import ct
    geometry = fan() if kind == "fan" else None
    radon, y0, x0, view = case(geometry, n=3, seed=75)
    a = csmri_actions(3, T, 76, ("sigma_d", "mu"))
    sol = ct.HQSSolver_CT(den, geometry)
    v0 = sol.reset({"x0": x0})
    sig, mu = g(a["sigma_d"]), g(a["mu"])
    full = sol((v0, (y0, view)), (sig, mu))
    for rows in ([1], [0, 2]):
        r = torch.tensor(rows, device=dev())
        part = sol((v0[r].contiguous(), (y0[r].contiguous(), view[r].contiguous())), (sig[r].contiguous(), mu[r].contiguous()))
        assert torch.equal(part, full[r]), (kind, rows)


def composed_hqs(sol, variables, y0, sigma_d, mu, iter_num):
    """HQSSolver_CT's loop from the differentiable blocks of tfpnp_amd.autograd: what the fused native VJP is held against."""
    n_view = int(y0.shape[2])
    radon = sol.radon_generator(variables.shape[-1], n_view, device=variables.device, geometry=sol.geometry)
    gm = getattr(radon, "geometry", None)
    fwd = (lambda x: A.radon_forward(x, n_view)) if gm is None else (lambda x: A.fan_forward(x, gm))
    bwd = (lambda y: A.radon_backprojection(y, variables.shape[-1])) if gm is None else \
        (lambda y: A.fan_backprojection(y, variables.shape[-1], gm))
    x, z = torch.split(variables, 1, dim=1)
    n = x.shape[0]
    for i in range(iter_num):
        x = sol.prox_mapping(z, sigma_d[:, i])
        m = mu[:, i].reshape(n, 1, 1, 1)
        z = z - (bwd(fwd(z) - y0) / radon.opnorm ** 2 + m * (z - x)) / (1 + m)
    return torch.cat([x, z], dim=1)


@pytest.mark.parametrize("kind", ["parallel", "fan"])
def test_hqs_ct_fused_vjp_vs_composed_autograd(den, kind):
    """pnpx_ct_hqs_train / _backward against the composed loop on a perturbed state: every input's gradient (variables,
    sigma_d, mu) within 2e-2 of its norm (the tolerance of the other fused-vs-composed tests); hyper-parameter columns past
    iter_num get zeros; the iteration never reads x, so its gradient slot is exactly zero."""
    from tfpnp_amd.tasks import ct
    geometry = fan() if kind == "fan" else None
    radon, y0, x0, view = case(geometry)
    a = csmri_actions(B, T + 1, 97, ("sigma_d", "mu"))
    sol = ct.HQSSolver_CT(den, geometry)
    v0 = sol.reset({"x0": x0})
    v0 = v0 + 0.02 * torch.randn(v0.shape, device=v0.device, generator=torch.Generator(v0.device).manual_seed(10))
    wts = torch.randn(v0.shape, device=v0.device, generator=torch.Generator(v0.device).manual_seed(12))

    def grads(fn):
        leaves = [v0.clone().requires_grad_(True), g(a["sigma_d"], True), g(a["mu"], True)]
        out = fn(*leaves)
        (out * wts).sum().backward()
        return out.detach(), [l.grad for l in leaves]

    out_f, gf = grads(lambda v, s_, m_: sol((v, (y0, view)), (s_, m_), iter_num=T))
    out_c, gc = grads(lambda v, s_, m_: composed_hqs(sol, v, y0, s_, m_, T))
    with torch.no_grad():
        assert rel(out_f, sol((v0, (y0, view)), (g(a["sigma_d"]), g(a["mu"])), iter_num=T)) < 1e-6
    assert rel(out_f, out_c) < 1e-5
    for name, x, y in zip(("variables", "sigma_d", "mu"), gf, gc):
        e = rel(x, y)
        print(f"  HQSSolver_CT {kind} fused vs composed d/d{name}: {e:.2e}")
        assert float(y.abs().max()) > 0 and x.shape == y.shape and e < 2e-2, name
    assert float(gf[0][:, 0].abs().max()) == 0.0
    for k in (1, 2):
        assert float(gf[k][:, T:].abs().max()) == 0.0
    _, gf2 = grads(lambda v, s_, m_: sol((v, (y0, view)), (s_, m_), iter_num=T))
    assert all(torch.equal(x, y) for x, y in zip(gf, gf2))


def test_ct_env_episode_step_with_hqs_actor(unet_params):
    """One CTEnv step on fan-beam measurements: ResNetActor_HQS maps the policy observation to (sigma_d, mu) and HQSSolver_CT
    runs them; create_solver_ct names the class."""
    from tfpnp_amd.data.synthesis import ct_measure
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.policy import ResNetActor_HQS
    from tfpnp_amd.tasks import ct

    class Opt:
        solver = "hqs"
    sol = ct.create_solver_ct(Opt(), UNetDenoiser2D(state_dict=unet_params))
    assert type(sol) is ct.HQSSolver_CT and sol.geometry is None
    sol.geometry = fan()
    n, bundle = 3, 2
    data = ct_measure(g(synth.phantom_batch(n, R, R, 512)), V, radon_generator=sol.radon_generator, geometry=sol.geometry)
    assert torch.equal(data["x0"], data["ATy0"]) and data["y0"].shape[-1] == sol.geometry.resolve(R, V).det_count
    env = ct.CTEnv(None, sol, max_episode_step=3)
    ob = env.reset(data)
    pob = env.get_policy_ob(ob)
    assert tuple(pob.shape) == (n, 6, R, R)                      # x, z, ATy0, view, T, sigma_n
    actor = ResNetActor_HQS(4, bundle, state_dict={k: t(v) for k, v in synth.make_policy_params(6, 2 * bundle).items()})
    action, _, _, _ = actor(pob, torch.zeros(n, dtype=torch.int64, device=dev()), False, None)
    assert tuple(action["sigma_d"].shape) == tuple(action["mu"].shape) == (n, bundle)
    ob, ob_masked, reward, all_done, info = env.step(action)
    assert tuple(reward.shape) == (n, 1) and bool(torch.isfinite(reward).all()) and not all_done
    assert bool(torch.isfinite(env.state["solver"]).all()) and tuple(env.state["solver"].shape) == (n, 2, R, R)
