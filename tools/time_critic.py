"""Time the native critic forward, its input gradient and -- in the same run, as the yardstick -- the native actor forward
with the same num_inputs (the critic runs the actor's convolutions with another epilogue).  HIP events, warm-up, median and
spread of interleaved repetitions.

    python tools/time_critic.py [out_file]        (GPU box; default profiles/critic_times.txt)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tfpnp_amd import synth, ops, policy  # noqa: E402
from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn  # noqa: E402

dev = torch.device("cuda:0")
NUM_INPUTS, WARMUP, REPS, INNER = 9, 5, 7, 10


def timed(fn):
    """ms per call: INNER calls between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "critic_times.txt")
    critic = ResNet_wobn(NUM_INPUTS, 18, 1, state_dict=synth.make_critic_params(NUM_INPUTS, 1))
    actor = policy.ResNetActor_ADMM(6, 5, state_dict=synth.make_policy_params(NUM_INPUTS, 10, False, seed=1))
    cc, ac = critic.context(dev), actor.context(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; num_inputs {NUM_INPUTS}; ms per call, median [min .. max] of {REPS} interleaved "
             f"repetitions of {INNER} calls (HIP events, {WARMUP} warm-up calls)",
             "# actor_1chain: the actor with option chains = 1 (the critic runs one launch chain; the actor's automatic choice is two",
             "# chains at these B = 48 sizes, DESIGN.md section 9).  ratios: critic_fwd / actor_fwd, critic_fwd / actor_1chain, critic_bwd / critic_fwd",
             "# B  HxW      actor_fwd              actor_1chain           critic_fwd             critic_bwd             f/actor  f/actor1  bwd/fwd"]
    for (B, H) in [(6, 128), (48, 128), (6, 256), (48, 256)]:
        ob = torch.rand(B, NUM_INPUTS, H, H, device=dev)
        gv = torch.ones(B, device=dev)
        def actor_one_chain():
            ac.set_option("chains", 1)
            try:
                return ops.policy_forward(ac, ob)
            finally:
                ac.set_option("chains", 0)

        legs = {"actor": lambda: ops.policy_forward(ac, ob), "actor1": actor_one_chain, "fwd": lambda: ops.critic_forward(cc, ob),
                "bwd": lambda: ops.critic_backward(cc, ob, gv)}
        for fn in legs.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(REPS):
            for k, fn in legs.items():
                t[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in t.items()}
        col = lambda k: f"{med[k]:7.3f} [{min(t[k]):6.3f} .. {max(t[k]):6.3f}]"
        lines.append(f"{B:3d}  {H}x{H}  {col('actor')}  {col('actor1')}  {col('fwd')}  {col('bwd')}  {med['fwd'] / med['actor']:7.3f}  "
                     f"{med['fwd'] / med['actor1']:8.3f}  {med['bwd'] / med['fwd']:7.3f}")
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
