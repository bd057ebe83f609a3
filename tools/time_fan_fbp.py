"""Times the ramp-filter kernel against the FFT filter path, fan-beam filtered backprojection, and one iADMM iteration on the fan
pair against the parallel pair, at BASELINE config #4's shape (32 x 256^2, 30 views), and writes the record,
profiles/fan_fbp_times.txt by default.

    python tools/time_fan_fbp.py [--out FILE] [--reps N]

Event-timed medians of whole calls, taken the same way on both sides of each comparison.  radon_filter without a geometry is one
launch with no table upload; Radon_norm.filter_sinogram is the zero-padding, two native FFT calls, a spectrum multiply, a crop and a
scale in torch.  fan_fbp uploads its small tables (one stream synchronisation) and launches the filter and the backprojection.  One
iADMM iteration = (t(T = 5) - t(T = 1)) / 4 of the solver call: denoiser, forward projector with the fused subtraction,
backprojector, update."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfpnp_amd import ops, synth  # noqa: E402
from tfpnp_amd.pnp import UNetDenoiser2D  # noqa: E402
from tfpnp_amd.tasks.ct import IADMMSolver_CT  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fan_fbp_times.txt"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, R, V = 32, 256, 30
    gt = torch.from_numpy(synth.phantom_batch(B, R, R)).to(dev)
    lines = [f"# tools/time_fan_fbp.py: {torch.cuda.get_device_name(0)}, B={B} R={R} V={V}, median of {a.reps} event-timed calls (us)"]
    gen = T.RadonGenerator()
    par = gen(R, V, device=dev)
    fan_geometry = T.FanBeam(2.0 * R)
    fan = gen(R, V, device=dev, geometry=fan_geometry)
    yp, yf = par.forward(gt), fan.forward(gt)
    lines.append(f"ramp filter, parallel sinogram {tuple(yp.shape)}")
    lines.append(f"  radon_filter (one launch)          {median_us(lambda: ops.radon_filter(yp), a.reps):9.1f}")
    lines.append(f"  Radon_norm.filter_sinogram (FFT)   {median_us(lambda: par.filter_sinogram(yp), a.reps):9.1f}")
    lines.append(f"fan FBP, sinogram {tuple(yf.shape)}, D_so = D_od = 2R, LDS window {ops.fan_tables(R, *fan.geometry)[2]} bins")
    lines.append(f"  filter_fan call                    {median_us(lambda: fan.filter_fan(yf), a.reps):9.1f}")
    lines.append(f"  fbp call (filter + backprojection) {median_us(lambda: fan.fbp(yf), a.reps):9.1f}")
    lines.append(f"  parallel filter_backprojection     {median_us(lambda: par.filter_backprojection(yp), a.reps):9.1f}")
    den = UNetDenoiser2D(state_dict=synth.make_unet_params(0))
    sig = torch.full((B, 5), 25 / 255.0, device=dev)
    mu = torch.full((B, 5), 0.5, device=dev)
    tau = torch.full((B, 5), 0.5, device=dev)
    view = torch.full((B, 1, R, R), V / 120.0, device=dev)
    lines.append("one iADMM iteration")
    for name, geometry, radon, y in (("parallel", None, par, yp), ("fan", fan_geometry, fan, yf)):
        sol = IADMMSolver_CT(den, geometry)
        sol.radon_generator.opnorms = dict(gen.opnorms)
        v0 = sol.reset({"x0": radon.fbp(y)})
        with torch.no_grad():
            t1 = median_us(lambda: sol((v0, (y, view)), (sig, mu, tau), iter_num=1), a.reps)
            t5 = median_us(lambda: sol((v0, (y, view)), (sig, mu, tau), iter_num=5), a.reps)
        lines.append(f"  {name:9s}                          {(t5 - t1) / 4:9.1f}   (T=1 call {t1:.1f}, T=5 call {t5:.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
