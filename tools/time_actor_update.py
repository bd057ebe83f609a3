"""Time what it costs the native ADMM actor (9 inputs, bundle 5) to follow a torch actor, both ways in one run on one box:
  (a) host reload      module.state_dict() -> CPU -> ResNetActorBase.load_state_dict -> first forward: flatten through numpy,
                       BatchNorm fold and three packings in C++ loops on the host, free + allocate + upload, a fresh arena
                       (the only way before the device path existed; it is the existing path, not the code under test)
  (b) device refresh   utils.misc.hard_update(native, module) -> forward: name-based gather + one torch.cat on the device,
                       fold and packing by HIP kernels, refresh in place
Both legs end in the same forward (B x H x W below), so the difference is the refresh.  Wall clock with
torch.cuda.synchronize() before and after each repetition (the host reload is host work; the device refresh ends with its
own stream synchronisation); the two legs alternate repetition by repetition, so drift on a shared box hits both alike.  The
source alternates between two modules, so every repetition really changes the weights.  The figure of merit is the ratio of
the two medians.

    python tools/time_actor_update.py [out_file [commit]]        (GPU box; default profiles/actor_update_times.txt)
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
from tfpnp_amd import ops, policy  # noqa: E402
from tfpnp_amd.utils.misc import hard_update  # noqa: E402

dev = torch.device("cuda:0")
BUNDLE, WARMUP, REPS = 5, 2, 20
B, H, W = 16, 128, 128


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    from follow_actor import seeded_actor
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "actor_update_times.txt")
    host_net, dev_net = policy.ResNetActor_ADMM(6, BUNDLE), policy.ResNetActor_ADMM(6, BUNDLE)
    modules = [seeded_actor(host_net.in_dim, host_net.n_det, s).to(dev).eval() for s in (1, 2)]
    ob = torch.rand(B, host_net.in_dim, H, W, device=dev)
    step = [0]
    outs = {}

    def host_reload():
        m = modules[step[0] % 2]
        host_net.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        outs["a"] = ops.policy_forward(host_net.context(dev), ob)

    def device_refresh():
        hard_update(dev_net, modules[step[0] % 2])
        outs["b"] = ops.policy_forward(dev_net.context(dev), ob)

    def forward_only():
        outs["c"] = ops.policy_forward(dev_net.context(dev), ob)

    legs = [("a_host_reload+forward", host_reload), ("b_device_refresh+forward", device_refresh), ("c_forward_only", forward_only)]
    times = {name: [] for name, _ in legs}
    for rep in range(WARMUP + REPS):
        step[0] = rep
        for name, fn in legs:
            t = wall_ms(fn)
            if rep >= WARMUP:
                times[name].append(t)
        # both paths hold the same weights now: they must compute the same bits
        assert all(torch.equal(x, y) for x, y in zip(outs["a"], outs["b"])), "host reload and device refresh disagree"
    commit = sys.argv[2] if len(sys.argv) > 2 else ""       # for a tree that travels without its git metadata
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            pass
    med = {k: float(np.median(v)) for k, v in times.items()}
    n = int(ops._lib.lib().pnpx_policy_num_params(host_net.in_dim, host_net.n_det, 0))
    lines = [f"# {torch.cuda.get_device_name(0)}; commit {commit or 'n/a (no git metadata on this box)'}; ResNetActor_ADMM, "
             f"{host_net.in_dim} inputs, bundle {BUNDLE} ({n} parameters); forward {B} x {H} x {W}",
             f"# wall clock with device synchronisation around each repetition, legs alternating; {REPS} repetitions after {WARMUP} "
             "warm-ups; ms per call",
             "# leg                              median        min        max   reps"]
    for name, t in times.items():
        lines.append(f"{name:28s} {med[name]:12.3f} {min(t):10.3f} {max(t):10.3f} {len(t):6d}")
    a, b, c = med["a_host_reload+forward"], med["b_device_refresh+forward"], med["c_forward_only"]
    lines.append(f"# ratio of medians (a) / (b): {a / b:.1f}")
    lines.append(f"# without the common forward: host reload {a - c:.3f} ms, device refresh {b - c:.3f} ms, ratio {(a - c) / max(b - c, 1e-9):.1f}")
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
