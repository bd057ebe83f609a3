"""Times the fan-beam and the parallel-beam Radon pair and one CT HQS iteration at BASELINE config #4's shape (32 x 256^2, 30 views)
and writes the record, profiles/fanbeam_times.txt by default.

    python tools/time_fanbeam.py [--out FILE] [--reps N]

Event-timed medians.  A projector call is the whole native entry: the host builds and uploads its small tables (one stream
synchronisation), the forward entries run radon_pad_kernel before the projector kernel; the figures are therefore call times, an
upper bound of the kernel times, taken the same way for both geometries.  One HQS iteration = (t(T = 5) - t(T = 1)) / 4 of
pnpx_ct_hqs: denoiser, forward projector with the fused subtraction, backprojector, update."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfpnp_amd import ops, synth  # noqa: E402
from tfpnp_amd.pnp import UNetDenoiser2D  # noqa: E402
from tfpnp_amd.tasks.ct import HQSSolver_CT  # noqa: E402
from tfpnp_amd.utils import transforms as T  # noqa: E402


def median_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fanbeam_times.txt"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, R, V = 32, 256, 30
    gt = torch.from_numpy(synth.phantom_batch(B, R, R)).to(dev)
    lines = [f"# tools/time_fanbeam.py: {torch.cuda.get_device_name(0)}, B={B} R={R} V={V}, median of {a.reps} event-timed calls (us)",
             "# projector rows are whole native calls (table upload + synchronisation, pad kernel for the forward entries, kernel)"]
    den = UNetDenoiser2D(state_dict=synth.make_unet_params(0))
    sig = torch.full((B, 5), 25 / 255.0, device=dev)
    mu = torch.full((B, 5), 0.5, device=dev)
    view = torch.full((B, 1, R, R), V / 120.0, device=dev)
    for name, geometry in (("parallel", None), ("fan D_so=D_od=2R", T.FanBeam(2.0 * R)), ("fan D_so=D_od=R", T.FanBeam(1.0 * R))):
        radon = T.RadonGenerator()(R, V, device=dev, geometry=geometry)
        y = radon.forward(gt)
        win = "" if geometry is None else f", LDS window {ops.fan_tables(R, *radon.geometry)[2]} bins"
        lines.append(f"{name:18s} det={y.shape[-1]}{win}")
        lines.append(f"  forward call        {median_us(lambda: radon.forward(gt), a.reps):9.1f}")
        lines.append(f"  backprojection call {median_us(lambda: radon.backprojection(y), a.reps):9.1f}")
        sol = HQSSolver_CT(den, geometry)
        sol.radon_generator.opnorms = {(R, V) if geometry is None else (R, V, geometry.key()): radon.opnorm}
        v0 = sol.reset({"x0": radon.backprojection_norm(y)})
        with torch.no_grad():
            t1 = median_us(lambda: sol((v0, (y, view)), (sig, mu), iter_num=1), max(5, a.reps // 3))
            t5 = median_us(lambda: sol((v0, (y, view)), (sig, mu), iter_num=5), max(5, a.reps // 3))
        lines.append(f"  HQS iteration       {(t5 - t1) / 4:9.1f}   (T=1 call {t1:.1f}, T=5 call {t5:.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
