"""Time what it costs to change the native critic's weights, in one run on one box:
  (a) host reload       ResNet_wobn.load_state_dict + context(): flatten through numpy, weight-norm fold and packing in C++
                        loops on the host, free + allocate + upload (the only way before the device path existed)
  (b) load_flat_        a flat device vector: fold and packing by HIP kernels, refresh in place
  (c) soft_update       from a torch module source (shape check + torch.cat of its 82 parameters + update kernel + (b))
  (d) one critic forward at 48 x 128^2, for scale
(b)-(d): HIP events around each call on the current stream (each refresh ends with its own stream synchronisation, so the
event pair covers the whole call); (a): wall clock around the call with device synchronisation, it is host work.

    python tools/time_critic_update.py [out_file [commit]]        (GPU box; default profiles/critic_update_times.txt)
"""
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from tfpnp_amd import ops, synth  # noqa: E402
from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn  # noqa: E402
from tfpnp_amd.utils.misc import soft_update  # noqa: E402

dev = torch.device("cuda:0")
NUM_INPUTS, WARMUP, REPS, HOST_REPS = 9, 3, 20, 5


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    from target_critic import TorchCritic
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "critic_update_times.txt")
    params = [synth.make_critic_params(NUM_INPUTS, s) for s in (1, 2)]
    flats = [torch.from_numpy(ops.critic_flat_params(p, NUM_INPUTS)).to(dev) for p in params]
    module = TorchCritic(NUM_INPUTS)
    with torch.no_grad():
        for p, (key, _) in zip(module.parameters(), synth.critic_param_specs(NUM_INPUTS)):
            p.copy_(torch.from_numpy(params[1][key]))
    module.to(dev)
    net = ResNet_wobn(NUM_INPUTS, 18, 1, state_dict=params[0])
    ob = torch.rand(48, NUM_INPUTS, 128, 128, device=dev)
    net(ob)
    step = [0]

    def host_reload():
        step[0] += 1
        net.load_state_dict(params[step[0] % 2])
        net.context(dev)

    def load_flat():
        step[0] += 1
        net.load_flat_(flats[step[0] % 2])

    legs = [("a_host_reload", host_reload, wall_ms, HOST_REPS), ("b_load_flat_", load_flat, event_ms, REPS),
            ("c_soft_update_module", lambda: soft_update(net, module, 0.001), event_ms, REPS),
            ("d_forward_48x128x128", lambda: net(ob), event_ms, REPS)]
    rows = {}
    for name, fn, clock, reps in legs:
        for _ in range(WARMUP if clock is event_ms else 1):
            fn()
        torch.cuda.synchronize()
        t = [clock(fn) for _ in range(reps)]
        rows[name] = (float(np.median(t)), min(t), max(t), reps)
        print(f"{name:24s} {rows[name][0]:10.3f} ms", flush=True)
    # where (b) spends its time: the same refresh under wall clock (launch + read-back latency included)
    wall_b = float(np.median([wall_ms(load_flat) for _ in range(REPS)]))
    commit = sys.argv[2] if len(sys.argv) > 2 else ""       # for a tree that travels without its git metadata
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            pass
    a = rows["a_host_reload"][0]
    lines = [f"# {torch.cuda.get_device_name(0)}; commit {commit or 'n/a (no git metadata on this box)'}; num_inputs {NUM_INPUTS} "
             f"({flats[0].numel()} parameters); ms per call, median [min .. max]",
             f"# (a) wall clock with device synchronisation, {HOST_REPS} repetitions after 1 warm-up; (b)-(d) HIP events, {REPS} repetitions "
             f"after {WARMUP} warm-ups",
             "# leg                          median        min        max   reps   (a) / leg"]
    for name, (med, lo, hi, reps) in rows.items():
        lines.append(f"{name:24s} {med:12.3f} {lo:10.3f} {hi:10.3f} {reps:6d} {a / med:11.1f}")
    lines.append(f"# (b) under wall clock: {wall_b:.3f} ms per call")
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    assert rows["b_load_flat_"][0] < a and rows["c_soft_update_module"][0] < a, "the device paths must beat the host reload"


if __name__ == "__main__":
    main()
