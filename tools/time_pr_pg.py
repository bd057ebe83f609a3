"""us per inner iteration of the PR proximal-gradient solver (pnpx_pr_pg) against PR inexact ADMM (pnpx_pr_iadmm) at BASELINE
config #3's shape (36 x 256 x 256, S = 4) in both convolution families, and the data step alone: the iteration minus one denoiser
forward over the same batch, timed in the same process.

    python tools/time_pr_pg.py [--reps 30]

Each figure: device events around one call of T = 10 iterations, divided by T (the once-per-call kernels -- the state's complex
copy in PG, Re(z - u) in iADMM -- are inside, a tenth each); median over --reps rounds after warm-up.  A round times the
denoiser, PG and iADMM one after the other, so a drift of the machine hits the three alike.

The denoiser is 50 times the data step, so "iteration minus denoiser" carries the denoiser's run-to-run spread (a stand-alone
denoiser call is not exactly the one inside the loop); the last column, iADMM minus PG per iteration, has the same denoiser calls
on both sides and is the figure to compare.  Per-kernel times of the data step's three launches come from a kernel trace of this
script:  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/time_pr_pg.py --reps 4 ; python tools/rocpd_stats.py DIR/t_results.db"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfpnp_amd import ops, synth  # noqa: E402
from tfpnp_amd.pnp import UNetDenoiser2D  # noqa: E402
from tfpnp_amd.tasks.pr import IADMMSolver_PR, PGSolver_PR  # noqa: E402

dev = torch.device("cuda:0")
B, H, S, T = 36, 256, 4, 10


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    reps = ap.parse_args().reps
    params = synth.make_unet_params(0)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.make_pr_batch(B, H, H, S=S, alpha=9.0, seed=77).items()}
    aux = (d["y0"], d["mask"])
    sd = torch.full((B, T), 25 / 255.0, device=dev)
    mu = torch.full((B, T), 0.5, device=dev)
    tau = torch.full((B, T), 0.5, device=dev)
    print(f"{B} x {H}x{H}, S = {S}, T = {T}; us per iteration, median of {reps}")
    print(f"{'mode':>4} {'denoiser':>9} {'PG it':>9} {'iADMM it':>9} {'PG data':>9} {'iADMM data':>11} {'PG/iADMM data':>14} {'iADMM - PG':>11}")
    for mode in (0, 1):
        den = UNetDenoiser2D(state_dict=params, conv_mode=mode)
        ctx = den.context(dev)
        pg, admm = PGSolver_PR(den), IADMMSolver_PR(den)
        v_pg, v_admm = pg.reset(d), admm.reset(d)
        x, s1 = d["x0"].contiguous(), sd[:, 0].contiguous()
        legs = {"den": lambda: ops.unet_denoise(ctx, x, s1), "pg": lambda: pg((v_pg, aux), (sd, tau)),
                "admm": lambda: admm((v_admm, aux), (sd, mu, tau))}
        ts = {k: [] for k in legs}
        with torch.no_grad():
            for fn in legs.values():
                fn()
                fn()
            torch.cuda.synchronize()
            for _ in range(reps):
                for k, fn in legs.items():
                    ts[k].append(event_us(fn))
        t_den = float(np.median(ts["den"]))
        t_pg, t_admm = float(np.median(ts["pg"])) / T, float(np.median(ts["admm"])) / T
        print(f"{mode:>4} {t_den:9.1f} {t_pg:9.1f} {t_admm:9.1f} {t_pg - t_den:9.1f} {t_admm - t_den:11.1f} "
              f"{(t_pg - t_den) / (t_admm - t_den):14.3f} {t_admm - t_pg:11.1f}", flush=True)


if __name__ == "__main__":
    main()
