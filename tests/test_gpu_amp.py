"""CS-MRI AMP solver on the GPU (pnpx_csmri_amp, tfpnp_amd/tasks/csmri.py::AMPSolver_CSMRI): parity with the real
reference's loop (tests/golden/csmri_amp_B2_64x64.npz, tools/make_amp_golden.py), with the float64 restatement of
tests/test_amp_host.py at other sizes, determinism, the single 2B-item denoiser call, the composed training path and
the DRUNet context."""
import numpy as np
import pytest
import torch

from oracle import pnp_oracle as O
from tests.golden_inputs import WEIGHT_SEED
from tests.test_amp_host import amp_case, amp_reset, amp_restated
from tfpnp_amd import synth

pytestmark = pytest.mark.gpu

# Parity bound per convolution family.  conv_mode 0 (fp32) has the bar of the other solver goldens.  conv_mode 1 (half-split
# fp16 x3, fp32-accurate products) measured 2.0e-6 / 1.6e-5 at T = 1 / 5 against the golden and 1.3e-5 against the float64
# restatement at 50x39 on its first run, the same size as the fp32 family's errors: it keeps the same bar.  The divergence
# quotient (D(r + eps delta) - D(r)) / eps divides rounding by eps ~ 1e-3, so a family that rounds coarser would need more.
GOLD_TOL = {0: 1e-4, 1: 1e-4}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev():
    return torch.device("cuda:0")


def g(a, grad=False):
    x = t(a).to(dev())
    return x.requires_grad_(True) if grad else x


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


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
    from tfpnp_amd.tasks.csmri import AMPSolver_CSMRI
    return AMPSolver_CSMRI(den)


def test_golden_parity(den):
    d, gold = amp_case()
    sol = _solver(den)
    v0 = amp_reset(g(d["y0"]))
    probe = g(gold["probe"])
    for T, key in ((1, "out_T1"), (5, "out_T5")):
        out = sol((v0, (g(d["y0"]), g(d["mask"]))), g(gold["sigma_d"][:, :T]), probe=probe)
        e = rel(out, t(gold[key]))
        print(f"  conv_mode {den.mode} T={T}: native vs reference golden {e:.2e}")
        assert e <= GOLD_TOL[den.mode], key


@pytest.mark.parametrize("B,H,W,seed", [(2, 256, 256, 41), (2, 50, 39, 42)])
def test_against_float64_restatement(den, oden64, B, H, W, seed):
    _, gold = amp_case()
    T = 5 if H == 256 else 3
    d = synth.make_csmri_batch(B, H, W, ratio=4, sigma_n=15, seed=seed)
    sd = gold["sigma_d"][:B, :T]
    probe = np.random.RandomState(seed + 1).standard_normal((T, B, 1, H, W)).astype(np.float32)
    out = _solver(den)((amp_reset(g(d["y0"])), (g(d["y0"]), g(d["mask"]))), g(sd), probe=g(probe))
    with torch.no_grad():
        ref = amp_restated(oden64, amp_reset(t(d["y0"]).double()), t(d["y0"]).double(), t(d["mask"]),
                           t(sd).double(), t(probe).double())
    e = rel(out, ref)
    print(f"  conv_mode {den.mode} B={B} {H}x{W} T={T}: native vs float64 restatement {e:.2e}")
    assert e <= GOLD_TOL[den.mode]


def test_determinism(den):
    d, gold = amp_case()
    sol = _solver(den)
    v0, aux = amp_reset(g(d["y0"])), (g(d["y0"]), g(d["mask"]))
    sd, probe = g(gold["sigma_d"]), g(gold["probe"])
    a = sol((v0, aux), sd, probe=probe)
    b = sol((v0, aux), sd, probe=probe)
    assert torch.equal(a, b)
    outs = []
    for _ in range(2):
        torch.manual_seed(1234)
        outs.append(sol((v0, aux), sd))
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], a)          # the drawn probe is not the golden's


def test_prox_and_probe_share_one_2b_denoiser_call(den):
    from tfpnp_amd import ops
    d, gold = amp_case()
    sol = _solver(den)
    ctx = den.context(dev())
    y0, mask = g(d["y0"]), g(d["mask"])
    B, H, W = y0.shape[0], y0.shape[2], y0.shape[3]
    v0 = amp_reset(y0)
    sd, probe = g(gold["sigma_d"][:, :1]), g(gold["probe"][:1])
    out = sol((v0, (y0, mask)), sd, probe=probe)
    nbytes = ctx.bytes()
    for _ in range(3):
        again = sol((v0, (y0, mask)), sd, probe=probe)
    torch.cuda.synchronize()
    assert ctx.bytes() == nbytes and torch.equal(again, out)
    # the stack [r, r + eps delta] built here, denoised in one 2B call
    r = ops.fft2(y0, inverse=True)[..., 0]
    eps = r.max() / 1000 + 1e-8
    s = torch.sqrt((y0 * y0).reshape(B, -1).sum(dim=-1)) / torch.sqrt(torch.tensor(float(H * W), device=dev())) * sd[:, 0]
    dn = ops.unet_denoise(ctx, torch.cat([r, r + probe[0] * eps]), torch.cat([s, s]))
    e = rel(out[:, 0, ..., 0], dn[:B, 0])
    print(f"  conv_mode {den.mode}: x slot vs first half of the 2B call {e:.2e}")
    assert e <= 1e-6
    assert torch.all(out[:, 0, ..., 1] == 0)


def test_training_path(den):
    from tfpnp_amd.tasks.csmri import CSMRIEnv
    d, gold = amp_case()
    sol = _solver(den)
    y0, mask = g(d["y0"]), g(d["mask"])
    v0 = amp_reset(y0)
    sd, probe = gold["sigma_d"][:, :2], g(gold["probe"][:2])
    fused = sol((v0, (y0, mask)), g(sd), probe=probe)
    leaves = [v0.clone().requires_grad_(True), g(sd, True)]
    out = sol((leaves[0], (y0, mask)), leaves[1], probe=probe)
    assert out.requires_grad
    e = rel(out, fused)
    print(f"  conv_mode {den.mode}: composed vs fused forward {e:.2e}")
    # the bar of the other CS-MRI solvers' composed-vs-fused checks (tests/test_gpu_backward.py): the per-item sums of the
    # divergence and of ||z||^2 are reductions in different orders here and there, and the Onsager term divides their
    # rounding by eps ~ 1e-3 (the x slot of the first iteration is bit-identical: test_prox_and_probe_share_one_2b_denoiser_call)
    assert e <= 1e-5
    w = np.random.RandomState(int(gold["grad_wts_seed"])).standard_normal(tuple(v0.shape)).astype(np.float32)
    (out * g(w)).sum().backward()
    for leaf, key in zip(leaves, ("grad_variables", "grad_sigma_d")):
        e = rel(leaf.grad, t(gold[key]))
        print(f"  conv_mode {den.mode}: vs reference autograd {key}: {e:.2e}")
        assert e < 0.25, key          # the bound tests/test_gpu_backward.py uses for the other CS-MRI solvers
    # the environment end to end: reset / step / forward (training path) with a finite reward
    B, H, W = 3, 64, 64
    d2 = synth.make_csmri_batch(B, H, W, ratio=4, sigma_n=15, seed=43)
    env = CSMRIEnv(None, sol, max_episode_step=3)
    ob = env.reset({k: g(v) for k, v in d2.items()})
    sig = torch.full((B, 2), 0.5, device=dev())
    ob, ob_masked, reward, all_done, info = env.step({"sigma_d": sig, "idx_stop": torch.zeros(B, dtype=torch.long,
                                                                                               device=dev())})
    assert torch.isfinite(torch.as_tensor(reward)).all()
    raw = torch.zeros(B, 2, device=dev(), requires_grad=True)
    _, reward = env.forward(ob, {"sigma_d": torch.sigmoid(raw) + 0.1})
    assert torch.isfinite(reward).all()
    reward.sum().backward()
    assert torch.isfinite(raw.grad).all()


def test_drunet_context():
    from tfpnp_amd.pnp import DRUNetDenoiser2D
    params = synth.make_drunet_params(0)
    d, gold = amp_case()
    sol = _solver(DRUNetDenoiser2D(state_dict=params))
    T = 2
    out = sol((amp_reset(g(d["y0"])), (g(d["y0"]), g(d["mask"]))), g(gold["sigma_d"][:, :T]), probe=g(gold["probe"][:T]))
    with torch.no_grad():
        ref = amp_restated(O.DRUNetDenoiser(params, dtype=torch.float64), amp_reset(t(d["y0"]).double()),
                           t(d["y0"]).double(), t(d["mask"]), t(gold["sigma_d"][:, :T]).double(), t(gold["probe"]).double())
    e = rel(out, ref)
    print(f"  DRUNet T={T}: native vs float64 restatement {e:.2e}")
    assert e <= 1e-4
