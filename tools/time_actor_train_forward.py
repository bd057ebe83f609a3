"""Median time of the native actor's train-mode forward (batch-statistics BatchNorm, running statistics moved) against the
native eval-mode forward and against the torch stand-in's train-mode forward (examples/follow_actor.py: MIOpen convolutions,
torch BatchNorm) on the same device, at B = 48, 256 x 256, ResNetActor_ADMM (9 inputs, bundle 5).  Device time by events
around each call, the three legs alternating repetition by repetition.  No threshold is asserted.

    python tools/time_actor_train_forward.py [out_file [commit]]        (GPU box; default profiles/actor_train_forward_times.txt)
"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from tfpnp_amd import ops, policy, synth  # noqa: E402

dev = torch.device("cuda:0")
BUNDLE, WARMUP, REPS = 5, 3, 20
B, H, W = 48, 256, 256


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    from follow_actor import seeded_actor
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "actor_train_forward_times.txt")
    net = policy.ResNetActor_ADMM(6, BUNDLE)
    net.load_state_dict(synth.make_policy_params(net.in_dim, net.n_det, False, seed=1))
    train_ctx, eval_ctx = net.context(dev), ops.Context(dev)
    eval_ctx.load_policy_device(train_ctx.policy_params(), net.in_dim, net.n_det, False)   # its statistics never move
    module = seeded_actor(net.in_dim, net.n_det, 1).to(dev).train()
    ob = torch.rand(B, net.in_dim, H, W, device=dev)

    def torch_train():
        with torch.no_grad():
            module(ob)

    legs = [("native_train_forward", lambda: ops.policy_forward_train(train_ctx, ob)),
            ("native_eval_forward", lambda: ops.policy_forward(eval_ctx, ob)),
            ("torch_train_forward", torch_train)]
    times = {name: [] for name, _ in legs}
    for rep in range(WARMUP + REPS):
        for name, fn in legs:
            t = event_ms(fn)
            if rep >= WARMUP:
                times[name].append(t)
    commit = sys.argv[2] if len(sys.argv) > 2 else ""       # for a tree that travels without its git metadata
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            pass
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"# {torch.cuda.get_device_name(0)}; commit {commit or 'n/a (no git metadata on this box)'}; ResNetActor_ADMM, "
             f"{net.in_dim} inputs, bundle {BUNDLE}; forward {B} x {H} x {W}",
             f"# device time by events around each call, legs alternating; {REPS} repetitions after {WARMUP} warm-ups; ms per call",
             "# leg                              median        min        max   reps"]
    for name, t in times.items():
        lines.append(f"{name:28s} {med[name]:12.3f} {min(t):10.3f} {max(t):10.3f} {len(t):6d}")
    lines.append(f"# native train / native eval: {med['native_train_forward'] / med['native_eval_forward']:.2f}; "
                 f"torch train / native train: {med['torch_train_forward'] / med['native_train_forward']:.2f}")
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
