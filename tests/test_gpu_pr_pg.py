"""Phase-retrieval proximal-gradient solver on the GPU (pnpx_pr_pg / _train / _backward, tfpnp_amd/tasks/pr.py::PGSolver_PR):
parity with the chain of real reference calls (tests/golden/pr_pg_B2_64x64.npz, tools/make_pr_pg_golden.py), with the float64
restatement of tests/test_pr_pg_host.py on the grouped 256-point path and on the generic one, determinism, the complex start,
the fused training path against a composed loop and against reference autograd, the dispatcher registration, the environment
and the DRUNet context."""
import numpy as np
import pytest
import torch

from oracle import pnp_oracle as O
from tests.test_pr_pg_host import pg_case, pg_grad_start, pr_pg_restated
from tfpnp_amd import autograd as A
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

# Parity bound per convolution family: the bar of test_pr_golden and of every solver golden.  conv_mode 1 (half-split f16 x3)
# meets the same bar: measured 7.9e-7 / 7.8e-7 at T = 1 / 5 against the golden (fp32 family: 6.6e-7 / 6.3e-7) on its first run.
GOLD_TOL = {0: 1e-4, 1: 1e-4}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev():
    return torch.device("cuda:0")


def g(a, grad=False):
    x = t(a).to(dev())
    return x.requires_grad_(True) if grad else x


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def pg_actions(B, T, seed):
    """sigma_d within the denoiser's 5/255 .. 50/255, tau in 0.5 .. 1.2 (the golden's ranges)."""
    rs = np.random.RandomState(seed)
    return (rs.uniform(5 / 255.0, 50 / 255.0, (B, T)).astype(np.float32), rs.uniform(0.5, 1.2, (B, T)).astype(np.float32))


@pytest.fixture(scope="module", params=[0, 1], ids=["f32_mfma", "hs_f16x3"])
def den(unet_params, request):
    from tfpnp_amd.pnp import UNetDenoiser2D
    d = UNetDenoiser2D(state_dict=unet_params, conv_mode=request.param)
    d.mode = request.param
    return d


@pytest.fixture(scope="module")
def oden64(unet_params):
    return O.Denoiser(unet_params, dtype=torch.float64)


def _solver(den):
    from tfpnp_amd.tasks.pr import PGSolver_PR
    return PGSolver_PR(den)


def restated64(oden64, v0, d, sd, tau, iter_num=None, trace=None):
    c = lambda a: t(a).double()
    with torch.no_grad():
        return pr_pg_restated(oden64, c(v0), c(d["y0"]), c(d["mask"]), c(sd), c(tau), iter_num, trace)


def composed_pg(self, variables, y0, mask, sigma_d, tau, iter_num):
    """The loop of PGSolver_PR.forward from differentiable building blocks: what the fused native VJP (pnpx_pr_pg_backward) is
    tested against.  cdp_forward / cdp_backward are written as their definitions (transforms.py:282-320) on the differentiable
    fft2 op -- the dispatcher's cdp ops carry no autograd formula; the denoiser is its autograd op (prox_mapping)."""
    x, B, S = variables, variables.shape[0], mask.shape[1]
    for i in range(sigma_d.shape[-1] if iter_num is None else iter_num):
        Ax = A.fft2(A.cmul(x.repeat(1, S, 1, 1, 1), mask), centered=False)                          # cdp_forward
        y_hat = (Ax ** 2).sum(dim=-1).sqrt()                                                        # complex_abs
        q = ((y_hat - y0) / y_hat).unsqueeze(-1)
        grad = A.cmul(A.fft2(q * Ax, inverse=True, centered=False), A.conj(mask)).mean(1, keepdim=True)   # cdp_backward
        z = x - tau[:, i].reshape(B, 1, 1, 1, 1) * grad
        x = A.r2c(self.prox_mapping(A.c2r(z), sigma_d[:, i]))
    return x


@pytest.fixture(scope="module", autouse=True)
def _install_composed():
    from tfpnp_amd.tasks.pr import PGSolver_PR
    PGSolver_PR._forward_autograd = composed_pg
    yield
    del PGSolver_PR._forward_autograd


def test_golden_parity(den):
    d, gold = pg_case()
    sol = _solver(den)
    v0 = sol.reset({"x0": g(d["x0"])})
    for T, key in ((1, "out_T1"), (5, "out_T5")):
        out = sol((v0, (g(d["y0"]), g(d["mask"]))), (g(gold["sigma_d"][:, :T]), g(gold["tau"][:, :T])))
        e = rel(out, gold[key])
        print(f"  conv_mode {den.mode} T={T}: native vs reference golden {e:.2e}")
        assert e <= GOLD_TOL[den.mode], key
        assert tuple(out.shape) == (2, 1, 64, 64, 2) and torch.all(out[..., 1] == 0)
        assert not torch.signbit(out[..., 1]).any()


@pytest.mark.parametrize("B,H,W,seed", [(3, 256, 256, 51), (2, 50, 39, 52)])
def test_against_float64_restatement(den, oden64, B, H, W, seed):
    """256 x 256: the grouped inverse row pass with the real-valued accumulator; 50 x 39: mixed-radix passes + pr_pg_step_kernel."""
    T = 3
    d = synth.make_pr_batch(B, H, W, S=4, alpha=9.0, seed=seed)
    sd, tau = pg_actions(B, T, seed + 1)
    sol = _solver(den)
    v0 = sol.reset({"x0": g(d["x0"])})
    aux = (g(d["y0"]), g(d["mask"]))
    out = sol((v0, aux), (g(sd), g(tau)))
    tr = {}
    ref = restated64(oden64, v0.cpu().numpy(), d, sd, tau, trace=tr)
    e = rel(out, ref)
    print(f"  conv_mode {den.mode} B={B} {H}x{W} T={T}: native vs float64 restatement {e:.2e}  (min |Ax| {tr['min_abs']:.2e})")
    assert tr["min_abs"] > 0
    assert e < 1e-4
    if W == 256:
        # the same call on the generic Stockham passes + pr_pg_step_kernel (option fft_fast = 0): one formula, two FFT
        # factorisations.  Bound: a 256-point transform rounds at about log2(256) * 2^-24 = 5e-7 relative in either
        # factorisation; three transforms per iteration, three iterations, through a denoiser that does not expand: 1e-5.
        ctx = den.context(dev())
        ctx.set_option("fft_fast", 0)
        try:
            slow = sol((v0, aux), (g(sd), g(tau)))
        finally:
            ctx.set_option("fft_fast", 1)
        e2 = rel(slow, out)
        print(f"  conv_mode {den.mode}: grouped 256-point path vs generic path {e2:.2e}")
        assert e2 <= 1e-5 and rel(slow, ref) < 1e-4


def test_iter_num_zero_iterations_determinism_and_batch_independence(den):
    d, gold = pg_case()
    sol = _solver(den)
    v0 = sol.reset({"x0": g(d["x0"])})
    aux = (g(d["y0"]), g(d["mask"]))
    sd, tau = g(gold["sigma_d"]), g(gold["tau"])
    a = sol((v0, aux), (sd, tau), iter_num=2)
    b = sol((v0, aux), (sd[:, :2].contiguous(), tau[:, :2].contiguous()))
    assert torch.equal(a, b)
    vc = v0 + 0.05 * torch.randn(v0.shape, device=dev(), generator=torch.Generator(dev()).manual_seed(3))
    assert torch.equal(sol((vc, aux), (sd, tau), iter_num=0), vc)
    assert torch.equal(sol((v0, aux), (sd, tau)), sol((v0, aux), (sd, tau)))
    # a B = 5 call against per-item calls (64 x 64: both in the small-batch K-split class of the fp32 family)
    B = 5
    d5 = synth.make_pr_batch(B, 64, 64, S=4, alpha=9.0, seed=53)
    s5, t5 = pg_actions(B, 2, 54)
    v5 = sol.reset({"x0": g(d5["x0"])})
    whole = sol((v5, (g(d5["y0"]), g(d5["mask"]))), (g(s5), g(t5)))
    for i in range(B):
        sl = slice(i, i + 1)
        one = sol((v5[sl], (g(d5["y0"][sl]), g(d5["mask"][sl]))), (g(s5[sl]), g(t5[sl])))
        assert rel(whole[sl], one) <= 1e-6, i


def test_complex_start(den, oden64):
    d, gold = pg_case()
    v0 = pg_grad_start(d, gold)
    assert np.abs(v0[..., 1]).max() > 0.01
    sd, tau = gold["sigma_d"][:, :1], gold["tau"][:, :1]
    out = _solver(den)((g(v0), (g(d["y0"]), g(d["mask"]))), (g(sd), g(tau)))
    ref = restated64(oden64, v0, d, sd, tau)
    real_only = v0.copy()
    real_only[..., 1] = 0
    e = rel(out, ref)
    print(f"  conv_mode {den.mode}: complex start, T=1 vs float64 restatement {e:.2e};"
          f" the imaginary part moves the result by {rel(restated64(oden64, real_only, d, sd, tau), ref):.2e}")
    assert e <= 1e-5
    assert torch.all(out[..., 1] == 0)


def test_training_path(den):
    d, gold = pg_case()
    sol = _solver(den)
    y0, m = g(d["y0"]), g(d["mask"])
    T, cols = 2, 4
    v0 = g(pg_grad_start(d, gold))
    sd, tau = gold["sigma_d"][:, :cols], gold["tau"][:, :cols]
    wts = g(np.random.RandomState(int(gold["grad_wts_seed"])).standard_normal(tuple(v0.shape)).astype(np.float32))

    def grads(fn, w=wts):
        leaves = [v0.clone().requires_grad_(True), g(sd, True), g(tau, True)]
        out = fn(*leaves)
        assert out.requires_grad
        (out * w).sum().backward()
        return out.detach(), [l.grad for l in leaves]

    out_f, gf = grads(lambda v, s_, t_: sol((v, (y0, m)), (s_, t_), iter_num=T))
    out_c, gc = grads(lambda v, s_, t_: sol._forward_autograd(v, y0, m, s_, t_, T))
    with torch.no_grad():
        e_inf = rel(out_f, sol((v0, (y0, m)), (g(sd), g(tau)), iter_num=T))
    print(f"  conv_mode {den.mode}: training forward vs inference {e_inf:.2e}, vs composed {rel(out_f, out_c):.2e},"
          f" vs the reference chain {rel(out_f, gold['grad_out']):.2e}")
    assert e_inf < 1e-6
    assert rel(out_f, out_c) < 1e-5
    assert rel(out_f, gold["grad_out"]) <= GOLD_TOL[den.mode]
    for n, x, y in zip(("variables", "sigma_d", "tau"), gf, gc):
        e_c = rel(x, y)
        ref = t(gold[f"grad_{n}"])
        e_r = rel(x if n == "variables" else x[:, :T], ref)
        print(f"  conv_mode {den.mode}: fused VJP d/d{n}: vs composed {e_c:.2e}, vs reference autograd {e_r:.2e}")
        assert x.shape == y.shape
        assert e_c < 2e-2, n          # the kink-flip bound of every *_fused_vjp_vs_composed test
        assert e_r < 2e-2, n          # the bound tests/test_gpu_backward.py holds PR to against reference autograd
    for k in (1, 2):                  # unused parameter columns: exactly zero; used ones: non-zero
        assert float(gf[k][:, T:].abs().max()) == 0.0 and float(gf[k][:, :T].abs().min()) > 0
    # the first iteration reads the imaginary part of the state through the masks
    assert float(gf[0][..., 1].abs().max()) > 0
    e_im = rel(gf[0][..., 1], gc[0][..., 1])
    print(f"  conv_mode {den.mode}: d/d Im(variables) vs composed {e_im:.2e}, vs reference {rel(gf[0][..., 1], gold['grad_variables'][..., 1]):.2e}")
    assert e_im < 2e-2 and rel(gf[0][..., 1], gold["grad_variables"][..., 1]) < 2e-2
    # the output's imaginary part is a constant: its cotangent contributes exactly nothing
    w_re = wts.clone()
    w_re[..., 1] = 0
    _, gr = grads(lambda v, s_, t_: sol((v, (y0, m)), (s_, t_), iter_num=T), w_re)
    assert all(torch.equal(x, y) for x, y in zip(gf, gr))
    _, gf2 = grads(lambda v, s_, t_: sol((v, (y0, m)), (s_, t_), iter_num=T))
    assert all(torch.equal(x, y) for x, y in zip(gf, gf2))
    # no iterations: the identity, cotangent passed through whole
    _, g0 = grads(lambda v, s_, t_: sol((v, (y0, m)), (s_, t_), iter_num=0))
    assert torch.equal(g0[0], wts) and float(g0[1].abs().max()) == 0.0 and float(g0[2].abs().max()) == 0.0


def test_opcheck(den):
    from tfpnp_amd import torch_ops  # noqa: F401
    cid = den.context(dev()).cid
    B = 2
    d = synth.make_pr_batch(B, 32, 32, S=4, alpha=9.0, seed=55)
    sd, tau = pg_actions(B, 3, 56)
    v0 = O.real2complex(g(d["x0"]))
    torch.library.opcheck(torch.ops.pnpx.pr_pg, (v0, g(d["y0"]), g(d["mask"]), g(sd), g(tau), -1, cid))
    torch.library.opcheck(torch.ops.pnpx.pr_pg, (v0, g(d["y0"]), g(d["mask"]), g(sd), g(tau), 2, cid))
    # the training op's ticket output is a fresh number per call by design (tests/test_gpu_torch_ops.py): schema, fake-tensor and
    # autograd-registration checks apply
    parts = ("test_schema", "test_faketensor", "test_autograd_registration")
    lv, ls, lt = (x.clone().requires_grad_(True) for x in (v0, g(sd), g(tau)))
    torch.library.opcheck(torch.ops.pnpx.pr_pg_train, (lv, g(d["y0"]), g(d["mask"]), ls, lt, 2, cid), test_utils=parts)


def test_environment(den, oden64):
    from tfpnp_amd.eval import eval_single
    from tfpnp_amd.policy import ResNetActor_PG
    from tfpnp_amd.tasks.pr import PREnv
    B, H, W, pack = 3, 64, 64, 2
    d = synth.make_pr_batch(B, H, W, S=4, alpha=9.0, seed=57)
    d["sigma_n"] = (np.ones((B, 1, H, W)) * np.random.RandomState(58).uniform(0.02, 0.2, (B, 1, 1, 1))).astype(np.float32)
    env = PREnv(None, _solver(den), max_episode_step=6)
    ob = env.reset(data={k: g(v) for k, v in d.items()})
    assert tuple(env.state["solver"].shape) == (B, 1, H, W, 2)
    assert tuple(env.get_policy_ob(ob).shape) == (B, 15, H, W)           # Re x + y0 [4] + mask [8] + T + sigma_n
    live = [0, 1, 2]
    stops = ([0, 1, 0], [0, 0], [0, 0])                                  # item 1 stops after the first step
    x = O.real2complex(t(d["x0"]).double())
    gt = t(d["gt"]).double()
    for s, stop in enumerate(stops):
        n = len(live)
        sd, tau = pg_actions(n, pack, 60 + s)
        before = env.state["solver"].clone()
        ob, ob_masked, reward, all_done, info = env.step({"sigma_d": g(sd), "tau": g(tau),
                                                          "idx_stop": torch.tensor(stop, device=dev())})
        sub = {k: d[k][live] for k in ("y0", "mask")}
        nxt = x.clone()
        nxt[live] = restated64(oden64, x[live].numpy(), sub, sd, tau)
        want = O.torch_psnr(O.complex2real(nxt), gt) - O.torch_psnr(O.complex2real(x), gt)
        x = nxt
        e = rel(env.state["solver"][live], x[live])
        print(f"  conv_mode {den.mode} step {s}: live rows vs float64 restatement {e:.2e},"
              f" reward diff {float((reward.cpu().double() - want).abs().max()):.2e}")
        assert e < 1e-4
        assert rel(env.get_policy_ob(ob)[:, 0], x[live][:, 0, ..., 0]) < 1e-4
        for row in set(range(B)) - set(live):
            assert torch.equal(env.state["solver"][row], before[row])
        assert tuple(reward.shape) == (B, 1)
        assert np.allclose(reward.cpu().numpy(), want.numpy(), atol=2e-3)
        live = [r for r, st in zip(live, stop) if st == 0]
        assert env.idx_left.cpu().tolist() == live and not all_done
        assert tuple(env.get_policy_ob(ob_masked).shape) == (len(live), 15, H, W)
    # a policy-driven rollout: ResNetActor_PG reads the 15-channel observation and emits (sigma_d, tau) bundles of 5
    actor = ResNetActor_PG(14, action_bundle=5)
    actor.load_state_dict(synth.make_policy_params(15, 10, False, seed=59))
    one = {k: g(v[:1]) for k, v in d.items()}
    p0, p1, (steps, trace, actions, _), imgs = eval_single(PREnv(None, _solver(den), max_episode_step=3), one, actor, 3)
    print(f"  conv_mode {den.mode}: eval_single PSNR {p0:.2f} -> {p1:.2f} in {steps} steps")
    assert 1 <= steps <= 3 and len(trace) == steps + 1 and np.isfinite([p0, p1] + list(trace)).all()
    assert set(actions) == {"sigma_d", "tau"} and len(actions["tau"]) == 5 * steps


def test_drunet_context():
    from tfpnp_amd.pnp import DRUNetDenoiser2D
    params = synth.make_drunet_params(0)
    d, gold = pg_case()
    sol = _solver(DRUNetDenoiser2D(state_dict=params))
    T = 2
    sd, tau = gold["sigma_d"][:, :T], gold["tau"][:, :T]
    v0 = sol.reset({"x0": g(d["x0"])})
    out = sol((v0, (g(d["y0"]), g(d["mask"]))), (g(sd), g(tau)))
    ref = restated64(O.DRUNetDenoiser(params, dtype=torch.float64), v0.cpu().numpy(), d, sd, tau)
    e = rel(out, ref)
    print(f"  DRUNet T={T}: native vs float64 restatement {e:.2e}")
    assert e <= 1e-4
