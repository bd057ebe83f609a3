"""Time the native critic forward + parameter gradient (pnpx_critic_param_grad) and -- in the same run, as the yardstick --
forward + backward of the torch stand-in module (tests/critic_cases.py::stand_in_module with a forward through F.conv2d) on
the same GPU, which is what a user without the native gradient runs.  HIP events, warm-up, median and spread of interleaved
repetitions.

    python tools/time_critic_grad.py [out_file]        (GPU box; default profiles/critic_grad_times.txt)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import critic_cases as K  # noqa: E402
from tfpnp_amd import synth  # noqa: E402
from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn  # noqa: E402

dev = torch.device("cuda:0")
NUM_INPUTS, WARMUP, REPS, INNER = 9, 3, 7, 5


def stand_in_forward(net, x):
    """forward of the stand-in module (it registers parameters only): critic.py:121-131 through F.conv2d"""
    def conv(m, v):   # (weight_norm's hook fills m.weight only inside m.forward, where the module was built: fold here)
        return F.conv2d(v, torch._weight_norm(m.weight_v, m.weight_g, 0), m.bias, stride=m.stride, padding=m.padding)

    def trelu(m, v):
        return F.relu(v - m.alpha) + m.alpha

    x = trelu(net.relu_1, conv(net.conv1, x))
    for li in range(1, 5):
        for blk in getattr(net, f"layer{li}"):
            out = conv(blk.conv2, trelu(blk.relu_1, conv(blk.conv1, x)))
            x = trelu(blk.relu_2, out + (conv(blk.shortcut[0], x) if len(blk.shortcut) else x))
    return net.fc(F.adaptive_avg_pool2d(x, 1).flatten(1))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "critic_grad_times.txt")
    params = synth.make_critic_params(NUM_INPUTS, 1)
    critic = ResNet_wobn(NUM_INPUTS, 18, 1, state_dict=params)
    torch_net = K.stand_in_module(NUM_INPUTS)
    with torch.no_grad():
        for p, (key, _) in zip(torch_net.parameters(), synth.critic_param_specs(NUM_INPUTS)):
            p.copy_(torch.from_numpy(params[key]))
    torch_net.to(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; num_inputs {NUM_INPUTS}; ms per call, median [min .. max] of {REPS} interleaved "
             f"repetitions of {INNER} calls (HIP events, {WARMUP} warm-up calls)",
             "# native: critic forward + param_grad (the gradient re-computes the forward itself); torch: forward + backward of the",
             "# weight_norm stand-in module through F.conv2d, gradients into .grad.  ratio: native / torch",
             "# B  HxW      native_fwd+param_grad    torch_fwd+bwd            ratio"]
    for (B, H) in [(6, 128), (48, 128), (6, 256), (48, 256)]:
        ob = torch.rand(B, NUM_INPUTS, H, H, device=dev)
        q = torch.randn(B, 1, device=dev)

        def native():
            V = critic(ob)
            return critic.param_grad(ob, 2.0 * (V - q) / B)

        def stand_in():
            torch_net.zero_grad(set_to_none=True)
            ((stand_in_forward(torch_net, ob) - q) ** 2).mean().backward()

        legs = {"native": native, "torch": stand_in}
        for fn in legs.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(REPS):
            for k, fn in legs.items():
                t[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in t.items()}
        col = lambda k: f"{med[k]:8.3f} [{min(t[k]):7.3f} .. {max(t[k]):7.3f}]"
        lines.append(f"{B:3d}  {H}x{H}  {col('native')}  {col('torch')}  {med['native'] / med['torch']:7.3f}")
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
