"""ms per inner iteration of the CS-MRI AMP solver (pnpx_csmri_amp) against ADMM (pnpx_csmri_admm) at 48 x 256^2 and at
B = 6, in both convolution families; at B = 6 also one denoiser call over 2B items against two calls over B items (the
two denoiser evaluations of an AMP iteration run as the former).

    python tools/time_amp.py

Each figure: median over 5 runs of (time of T = 5 iterations) / 5 after warm-up, synchronised per run."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfpnp_amd import ops, synth  # noqa: E402
from tfpnp_amd.pnp import UNetDenoiser2D  # noqa: E402
from tfpnp_amd.tasks.csmri import ADMMSolver_CSMRI, AMPSolver_CSMRI  # noqa: E402

dev = torch.device("cuda:0")
T = 5


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    params = synth.make_unet_params(0)
    print(f"{'mode':>4} {'B':>3} {'HxW':>8} {'ADMM ms/it':>11} {'AMP ms/it':>10} {'AMP/ADMM':>9} {'2B call ms':>11} {'2 x B ms':>9}")
    for mode in (0, 1):
        den = UNetDenoiser2D(state_dict=params, conv_mode=mode)
        for B, H in ((48, 256), (6, 256)):
            d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                 for k, v in synth.make_csmri_batch(B, H, H, seed=5).items()}
            aux = (d["y0"], d["mask"])
            admm, amp = ADMMSolver_CSMRI(den), AMPSolver_CSMRI(den)
            sd = torch.full((B, T), 0.1, device=dev)
            mu = torch.full((B, T), 0.5, device=dev)
            probe = torch.randn(T, B, 1, H, H, device=dev)
            v_admm, v_amp = admm.reset(d), amp.reset(d)
            with torch.no_grad():
                t_admm = timed(lambda: admm((v_admm, aux), (sd, mu))) / T
                t_amp = timed(lambda: amp((v_amp, aux), sd, probe=probe)) / T
                extra = ""
                if B == 6:
                    ctx = den.context(dev)
                    x2, s2 = torch.rand(2 * B, 1, H, H, device=dev), torch.full((2 * B,), 0.1, device=dev)
                    t_one = timed(lambda: ops.unet_denoise(ctx, x2, s2))
                    t_two = timed(lambda: (ops.unet_denoise(ctx, x2[:B], s2[:B]), ops.unet_denoise(ctx, x2[B:], s2[B:])))
                    extra = f" {t_one:11.2f} {t_two:9.2f}"
            print(f"{mode:>4} {B:>3} {H:>4}x{H:<3} {t_admm:11.2f} {t_amp:10.2f} {t_amp / t_admm:9.2f}{extra}", flush=True)


if __name__ == "__main__":
    main()
