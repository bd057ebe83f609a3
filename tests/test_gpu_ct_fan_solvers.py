"""IADMMSolver_CT and PGSolver_CT on a fan-beam pair (pnpx_ct_iadmm_geom / pnpx_ct_pg_geom and their training pairs): the forward
against the restatement of tests/fan_fbp_ref.py run with the oracle's denoiser, the unchanged parallel path, a ragged batch, the
fused VJP against the loop composed from tfpnp_amd.autograd blocks, and one CTEnv step that starts from the fan FBP."""
import numpy as np
import pytest
import torch

from tests import fan_fbp_ref as P
from tests import fanbeam_ref as F
from tests.golden_inputs import csmri_actions
from tfpnp_amd import autograd as A
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4              # the solver parity bar (test_ct_vs_oracle, tests/test_gpu_ct_hqs.py)
B, R, V, T = 2, 32, 20, 3
HYPERS = {"iadmm": ("sigma_d", "mu", "tau"), "pg": ("sigma_d", "tau")}


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


def solver(kind, den, geometry):
    from tfpnp_amd.tasks import ct
    return {"iadmm": ct.IADMMSolver_CT, "pg": ct.PGSolver_CT}[kind](den, geometry)


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


@pytest.mark.parametrize("kind", ["iadmm", "pg"])
def test_fan_solver_vs_restatement(den, oden, kind):
    geometry = fan()
    radon, y0, x0, view = case(geometry)
    gm = F.Geom(R, *geometry.resolve(R, V))
    fwd, bwd = (lambda x: F.fan_forward(x, gm)), (lambda y: F.fan_backprojection(y, gm))
    a = csmri_actions(B, T, 83, HYPERS[kind])
    sol = solver(kind, den, geometry)
    sol.radon_generator.opnorms[(R, V, geometry.key())] = radon.opnorm
    v0 = sol.reset({"x0": x0})
    assert tuple(v0.shape) == (B, 3 if kind == "iadmm" else 1, R, R)
    ref_fn = P.ct_iadmm if kind == "iadmm" else P.ct_pg
    for it in (None, 0, 1):
        out = sol((v0, (y0, view)), tuple(g(a[k]) for k in HYPERS[kind]), iter_num=it)
        ref = ref_fn(oden, fwd, bwd, v0.cpu(), y0.cpu(), radon.opnorm, *[t(a[k]) for k in HYPERS[kind]], iter_num=it)
        e = rel(out, ref)
        print(f"  {kind} fan T={T if it is None else it}: rel-L2 vs restatement {e:.2e}")
        assert e < TOL, (kind, it)
        if it == 0:
            assert torch.equal(out, v0)


@pytest.mark.parametrize("kind", ["iadmm", "pg"])
def test_parallel_path_is_unchanged(den, kind):
    """geometry None: the solver's output is, byte for byte, a direct call of the ct_iadmm / ct_pg op, and the _geom op with
    det_count 0 returns the same bytes."""
    from tfpnp_amd import torch_ops  # noqa: F401
    radon, y0, x0, view = case(None)
    a = csmri_actions(B, T, 83, HYPERS[kind])
    sol = solver(kind, den, None)
    assert sol.geometry is None
    sol.radon_generator.opnorms[(R, V)] = radon.opnorm
    v0 = sol.reset({"x0": x0})
    hyp = tuple(g(a[k]) for k in HYPERS[kind])
    cid = sol._ctx(v0).cid
    for it in (-1, 1):
        out = sol((v0, (y0, view)), hyp, iter_num=None if it < 0 else it)
        old = getattr(torch.ops.pnpx, f"ct_{kind}")(v0, y0, V, float(radon.opnorm), *hyp, it, cid)
        new = getattr(torch.ops.pnpx, f"ct_{kind}_geom")(v0, y0, V, float(radon.opnorm), 0, 0.0, 0.0, 0.0, *hyp, it, cid)
        assert float(out.abs().max()) > 0 and torch.equal(out, old) and torch.equal(new, old), (kind, it)


@pytest.mark.parametrize("kind", ["iadmm", "pg"])
def test_fan_solver_ragged_batch_equals_the_full_call(den, kind):
    """Rows [1], then [0, 2] of a B = 3 call: an item's result does not depend on the batch it arrives in."""
    geometry = fan()
    radon, y0, x0, view = case(geometry, n=3, seed=75)
    a = csmri_actions(3, T, 76, HYPERS[kind])
    sol = solver(kind, den, geometry)
    v0 = sol.reset({"x0": x0})
    hyp = tuple(g(a[k]) for k in HYPERS[kind])
    full = sol((v0, (y0, view)), hyp)
    for rows in ([1], [0, 2]):
        r = torch.tensor(rows, device=dev())
        part = sol((v0[r].contiguous(), (y0[r].contiguous(), view[r].contiguous())), tuple(h[r].contiguous() for h in hyp))
        assert torch.equal(part, full[r]), (kind, rows)


def composed(kind, sol, variables, y0, hyp, iter_num):
    """The solver's loop (tasks/ct/solver.py:32-49 and :73-83) from the differentiable blocks of tfpnp_amd.autograd on the fan pair:
    what the fused native VJP is held against."""
    n_view, Rr = int(y0.shape[2]), variables.shape[-1]
    radon = sol.radon_generator(Rr, n_view, device=variables.device, geometry=sol.geometry)
    gm = radon.geometry
    n = variables.shape[0]
    grad = lambda z: A.fan_backprojection(A.fan_forward(z, gm) - y0, Rr, gm) / radon.opnorm ** 2
    col = lambda p, i: p[:, i].reshape(n, 1, 1, 1)
    if kind == "pg":
        sigma_d, tau = hyp
        x = variables
        for i in range(iter_num):
            x = sol.prox_mapping(x - col(tau, i) * grad(x), sigma_d[:, i])
        return x
    sigma_d, mu, tau = hyp
    x, z, u = torch.split(variables, 1, dim=1)
    for i in range(iter_num):
        x = sol.prox_mapping(z - u, sigma_d[:, i])
        z = z - col(tau, i) * (grad(z) + col(mu, i) * (z - (x + u)))
        u = u + x - z
    return torch.cat([x, z, u], dim=1)


@pytest.mark.parametrize("kind", ["iadmm", "pg"])
def test_fan_solver_fused_vjp_vs_composed_autograd(den, kind):
    """pnpx_ct_*_geom_train / _backward against the composed loop on a perturbed state: every input's gradient within 2e-2 of its
    norm (the tolerance of the other fused-vs-composed tests); hyper-parameter columns past iter_num get zeros; two runs give
    equal bytes."""
    geometry = fan()
    radon, y0, x0, view = case(geometry)
    keys = HYPERS[kind]
    a = csmri_actions(B, T + 1, 97, keys)
    sol = solver(kind, den, geometry)
    v0 = sol.reset({"x0": x0})
    v0 = v0 + 0.02 * torch.randn(v0.shape, device=v0.device, generator=torch.Generator(v0.device).manual_seed(10))
    wts = torch.randn(v0.shape, device=v0.device, generator=torch.Generator(v0.device).manual_seed(12))

    def grads(fn):
        leaves = [v0.clone().requires_grad_(True)] + [g(a[k], True) for k in keys]
        out = fn(leaves[0], tuple(leaves[1:]))
        (out * wts).sum().backward()
        return out.detach(), [l.grad for l in leaves]

    fused = lambda v, hyp: sol((v, (y0, view)), hyp, iter_num=T)
    out_f, gf = grads(fused)
    out_c, gc = grads(lambda v, hyp: composed(kind, sol, v, y0, hyp, T))
    with torch.no_grad():
        assert rel(out_f, sol((v0, (y0, view)), tuple(g(a[k]) for k in keys), iter_num=T)) < 1e-6
    assert rel(out_f, out_c) < 1e-5
    for name, x, y in zip(("variables",) + keys, gf, gc):
        e = rel(x, y)
        print(f"  {kind} fan fused vs composed d/d{name}: {e:.2e}")
        assert float(y.abs().max()) > 0 and x.shape == y.shape and e < 2e-2, name
    for k in range(1, len(gf)):
        assert float(gf[k][:, T:].abs().max()) == 0.0
    _, gf2 = grads(fused)
    assert all(torch.equal(x, y) for x, y in zip(gf, gf2))


def test_ct_env_step_with_a_fan_iadmm_solver_from_fbp(unet_params):
    """One CTEnv step on fan-beam measurements: ResNetActor_IADMM drives a fan IADMMSolver_CT that starts from the fan FBP, whose
    PSNR is above that of the A^T y0 start on the same data."""
    from tfpnp_amd.data.synthesis import ct_measure
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.policy import ResNetActor_IADMM
    from tfpnp_amd.tasks import ct

    class Opt:
        solver = "iadmm"
        geometry = fan()
    sol = ct.create_solver_ct(Opt(), UNetDenoiser2D(state_dict=unet_params))
    assert type(sol) is ct.IADMMSolver_CT and sol.geometry is Opt.geometry
    n, bundle = 3, 2
    gt = g(synth.phantom_batch(n, R, R, 512))
    data = {k: ct_measure(gt, V, radon_generator=sol.radon_generator, geometry=sol.geometry, x0_from=k) for k in ("fbp", "aty0")}
    assert torch.equal(data["fbp"]["y0"], data["aty0"]["y0"]) and not torch.equal(data["fbp"]["x0"], data["aty0"]["x0"])
    from tfpnp_amd.env.base import torch_psnr
    baseline = {k: torch_psnr(d["x0"], gt) for k, d in data.items()}      # CPU restatement at this size: ~27 .. 30 dB against 15 .. 23 dB
    print(f"  PSNR of the start image: FBP {baseline['fbp'].flatten().tolist()}, A^T y0 {baseline['aty0'].flatten().tolist()}")
    assert tuple(baseline["fbp"].shape) == (n, 1) and bool((baseline["fbp"] > baseline["aty0"]).all())
    env = ct.CTEnv(None, sol, max_episode_step=3)
    ob = env.reset(data["fbp"])
    assert torch.equal(env.state["solver"][:, :1], data["fbp"]["x0"])        # the solver starts from the FBP image
    pob = env.get_policy_ob(ob)
    assert tuple(pob.shape) == (n, 7, R, R)                      # x, z, u, ATy0, view, T, sigma_n
    actor = ResNetActor_IADMM(4, bundle, state_dict={k: t(v) for k, v in synth.make_policy_params(7, 3 * bundle).items()})
    action, _, _, _ = actor(pob, torch.zeros(n, dtype=torch.int64, device=dev()), False, None)
    assert all(tuple(action[h].shape) == (n, bundle) for h in HYPERS["iadmm"])
    ob, ob_masked, reward, all_done, info = env.step(action)
    assert tuple(reward.shape) == (n, 1) and bool(torch.isfinite(reward).all()) and not all_done
    assert bool(torch.isfinite(env.state["solver"]).all()) and tuple(env.state["solver"].shape) == (n, 3, R, R)
