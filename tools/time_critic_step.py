"""Time one critic update (tfpnp/trainer/mddpg/trainer.py:180-186, 198, 206-212) on the native path
(trainer/mddpg/critic_step.py::critic_update: one forward for value, loss and gradient; clip + Adam + re-pack inside the native
context) and -- in the same run, as the yardstick -- on the composed path of examples/train_critic.py (critic forward, param_grad
with its own forward, torch's clip_grad_norm_ and Adam on a flat nn.Parameter, load_flat_, soft_update_).  HIP events, warm-up,
median and spread of interleaved repetitions.  Then the optimiser's accuracy: the six synthetic steps of
tests/critic_step_cases.py against its fp64 restatement, worst |error| / bound per quantity.

    python tools/time_critic_step.py [out_file]        (GPU box; default profiles/critic_step_times.txt)
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import critic_step_cases as S  # noqa: E402
from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn  # noqa: E402
from tfpnp_amd.trainer.mddpg.critic_step import critic_update  # noqa: E402

dev = torch.device("cuda:0")
NUM_INPUTS, WARMUP, REPS, INNER = 9, 3, 7, 5
TAU, LR, DISCOUNT = 0.001, 1e-4, 0.99


def example():
    spec = importlib.util.spec_from_file_location("example_train_critic", os.path.join(ROOT, "examples", "train_critic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def accuracy():
    p0 = torch.from_numpy(S.flat_params(NUM_INPUTS)).to(dev)
    net = ResNet_wobn(NUM_INPUTS, 18, 1).load_flat_(p0)
    ref = S.Yardstick(p0)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}
    for k in range(S.STEPS):
        gk = torch.from_numpy(S.synthetic_gradient(p0.numel(), k)).to(dev)
        ref.step(gk)
        norm = net.adam_step_(gk, S.LR, betas=S.BETAS, eps=S.EPS, max_norm=S.MAX_NORM)
        m, v, _ = net.optim_state(dev)
        r = ref.ratios(net.parameters_flat(dev), m, v)
        r["norm"] = abs(float(norm) - ref.norm) / ref.norm / 1e-6
        worst = {q: max(worst[q], r[q]) for q in r}
    return worst


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "critic_step_times.txt")
    ex = example()
    lines = [f"# {torch.cuda.get_device_name(0)}; num_inputs {NUM_INPUTS}; ms per critic update, median [min .. max] of {REPS} interleaved "
             f"repetitions of {INNER} updates (HIP events, {WARMUP} warm-up updates)",
             "# native: critic_update (target forward, value_loss_grad, adam_step_, soft_update); composed: examples/train_critic.py",
             "# composed_step (target forward, critic forward, param_grad, clip_grad_norm_, torch Adam, load_flat_, soft_update_)",
             "# ratio: native / composed",
             "# B  HxW      native                   composed                 ratio"]
    for (B, H) in [(48, 128)]:
        flat, critic, target, ob, ob2, reward = ex.setup(B, H, NUM_INPUTS, 1)
        _, critic_c, target_c, _, _, _ = ex.setup(B, H, NUM_INPUTS, 1)
        stop = torch.zeros(B, 1, device=dev)
        param = nn.Parameter(flat.clone())
        opt = torch.optim.Adam([param], lr=LR)
        legs = {"native": lambda: critic_update(critic, target, ob, ob2, reward, stop, DISCOUNT, TAU, LR),
                "composed": lambda: ex.composed_step(critic_c, target_c, param, opt, ob, ob2, reward, DISCOUNT, TAU)}
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
        lines.append(f"{B:3d}  {H}x{H}  {col('native')}  {col('composed')}  {med['native'] / med['composed']:7.3f}")
        print(lines[-1], flush=True)
    worst = accuracy()
    lines.append(f"# optimiser accuracy: {S.STEPS} synthetic steps (tests/critic_step_cases.py), num_inputs {NUM_INPUTS}, against the fp64 "
                 "restatement; worst |error| / bound after any step")
    lines.append("# parameters {p:.4f}   exp_avg {m:.4f}   exp_avg_sq {v:.4f}   norm (bound 1e-6 relative) {norm:.4f}".format(**worst))
    print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
