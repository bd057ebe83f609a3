"""Writes tests/golden/pr_pg_B2_64x64.npz by a chain of REAL REFERENCE calls (reference imported in place through
oracle/ref_shim.py).  Build machine only: it needs the reference checkout and never runs on a GPU box.

    python tools/make_pr_pg_golden.py

The reference's PGSolver_PR.forward (tasks/pr/solver.py:79-112) raises on any PR input: its gradient step was pasted from
CS-MRI.  The step it is meant to take is the one IADMMSolver_PR.forward computes in the same file (:61-68), and the reference
itself executes it here: one IADMMSolver_PR.forward call with iter_num = 1, state cat(x, x, 0) and mu = 0 returns

    z' = x - tau * cdp_backward((|Ax| - y0) / |Ax| * Ax, mask)

in its second slot (the mu term is 0 * finite = 0; the denoiser result of that call, slot 0, is discarded).  One PG iteration
is that call followed by the reference solver's prox_mapping between the reference's complex2real / real2complex.  No
arithmetic of the chain is written here.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tfpnp_amd import synth  # noqa: E402
from tests.golden_inputs import WEIGHT_SEED, sha  # noqa: E402

B, H, W, S, T = 2, 64, 64, 4, 5
DATA_SEED, ACT_SEED, START_SEED, WTS_SEED = 77, 78, 79, 80
OUT = os.path.join(ROOT, "tests", "golden", "pr_pg_B2_64x64.npz")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def actions():
    """sigma_d within the denoiser's 5/255 .. 50/255, tau in 0.5 .. 1.2, [B,T]."""
    rs = np.random.RandomState(ACT_SEED)
    return (rs.uniform(5 / 255.0, 50 / 255.0, (B, T)).astype(np.float32), rs.uniform(0.5, 1.2, (B, T)).astype(np.float32))


def grad_start(x0):
    """x0 as complex plus 0.05 * randn in both parts: the first iteration reads a non-zero imaginary part."""
    v = np.stack([x0, np.zeros_like(x0)], axis=-1)
    return (v + 0.05 * np.random.RandomState(START_SEED).standard_normal(v.shape)).astype(np.float32)


class Chain:
    def __init__(self, mod, sol, y0, mask):
        self.mod, self.sol, self.y0, self.mask = mod, sol, y0, mask
        self.min_abs = float("inf")

    def gradient_step(self, x, tau_i):
        """z' of one reference IADMMSolver_PR iteration from (x, x, 0) with mu = 0."""
        with torch.no_grad():
            self.min_abs = min(self.min_abs, float(self.mod.complex_abs(self.mod.cdp_forward(x, self.mask)).min()))
        state = torch.cat([x, x, torch.zeros_like(x)], dim=1)
        col = lambda v: v.reshape(-1, 1)
        any_sigma = torch.full((x.shape[0], 1), 25 / 255.0)
        out = self.sol((state, (self.y0, self.mask)), (any_sigma, torch.zeros(x.shape[0], 1), col(tau_i)), iter_num=1)
        return out[:, 1:2]

    def run(self, x, sigma_d, tau, n):
        zs = []
        for i in range(n):
            z = self.gradient_step(x, tau[:, i])
            zs.append(z)
            x = self.mod.real2complex(self.sol.prox_mapping(self.mod.complex2real(z), sigma_d[:, i]))
        return x, zs


def main():
    assert ref_shim.available(), "reference not mounted"
    ref_shim.install()
    torch.set_num_threads(8)
    mod = ref_shim.load_task_module("pr", "solver")
    sol = mod.IADMMSolver_PR(ref_shim.make_denoiser(synth.make_unet_params(WEIGHT_SEED), tempfile.mkdtemp()))
    d = synth.make_pr_batch(B, H, W, S=S, alpha=9.0, seed=DATA_SEED)
    sig, tau = actions()
    chain = Chain(mod, sol, t(d["y0"]), t(d["mask"]))
    with torch.no_grad():
        x0 = sol.reset({"x0": t(d["x0"])})[:, 0:1]
        out_T1, zs = chain.run(x0, t(sig), t(tau), 1)
        out_T5, _ = chain.run(x0, t(sig), t(tau), T)
    assert torch.all(out_T5[..., 1] == 0)

    # reference autograd of sum(out * w) wrt (variables, sigma_d, tau) at T = 2, from a complex start
    w = np.random.RandomState(WTS_SEED).standard_normal((B, 1, H, W, 2)).astype(np.float32)
    leaves = [t(grad_start(d["x0"])).requires_grad_(True), t(sig[:, :2]).requires_grad_(True), t(tau[:, :2]).requires_grad_(True)]
    out_g, _ = chain.run(leaves[0], leaves[1], leaves[2], 2)
    (out_g * t(w)).sum().backward()

    print(f"min |Ax| over the run: {chain.min_abs:.3e}")
    assert chain.min_abs > 0, "the residual divides by |Ax|"
    np.savez_compressed(OUT, in_sha=sha(d["y0"], d["mask"], d["x0"]), sigma_d=sig, tau=tau, z_T1=zs[0].numpy(),
                        out_T1=out_T1.numpy(), out_T5=out_T5.numpy(), grad_start_seed=START_SEED, grad_wts_seed=WTS_SEED,
                        grad_out=out_g.detach().numpy(), grad_variables=leaves[0].grad.numpy(),
                        grad_sigma_d=leaves[1].grad.numpy(), grad_tau=leaves[2].grad.numpy(), min_abs_Ax=np.float32(chain.min_abs))
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KB)")


if __name__ == "__main__":
    main()
