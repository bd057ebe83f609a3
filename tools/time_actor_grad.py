"""Time the native actor's train-mode forward + parameter gradient (pnpx_policy_forward_train + pnpx_policy_param_grad) and -- as the
yardstick, on the same GPU -- forward + backward of the torch stand-in module (tests/actor_cases.py::stand_in_actor in `.train()`
mode), which is what a user without the native gradient runs; and the whole-vector relative difference between the two gradients at
those sizes (both fp32: the only place where the gradient-range choice of csrc/policy_grad.hip meets real sizes).

    python tools/time_actor_grad.py [out_file]        (GPU box; default profiles/actor_grad_times.txt)

One GPU process per size, each under its own time limit; a size that fails or runs out of time ends the run.
"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASE, SEED, WARMUP, REPS = (9, 10, False), 3, 3, 20
SIZES = [(48, 128), (48, 256)]
STEP_LIMIT = 240   # seconds per size


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def one_size(B, H):
    from tests import actor_cases as A
    from tfpnp_amd import synth
    dev = torch.device("cuda:0")
    params = synth.make_policy_params(*CASE, seed=SEED)
    actor = A.native_actor(CASE, state_dict=params)
    net = A.load_params(A.stand_in_actor(*CASE), params).to(dev).train()
    r = np.random.RandomState(5)
    ob = torch.from_numpy(r.uniform(0, 1, (B, CASE[0], H, H)).astype(np.float32)).to(dev)
    gp = torch.from_numpy(r.standard_normal((B, 2)).astype(np.float32)).to(dev)
    gd = torch.from_numpy(r.standard_normal((B, CASE[1])).astype(np.float32)).to(dev)
    out = {}

    def native():
        actor.forward_train_raw(ob)
        out["native"] = actor.param_grad(ob, gp, gd)

    def stand_in():
        net.zero_grad(set_to_none=True)
        probs, det = net(ob)
        ((gp * probs).sum() + (gd * det).sum()).backward()

    legs = {"native": native, "torch": stand_in}
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    named = dict(net.named_parameters())
    ref = torch.cat([named[k].grad.reshape(-1) if k in named else torch.zeros(int(np.prod(s)), device=dev)
                     for k, s in synth.policy_param_specs(*CASE)]).double()
    diff = float((out["native"].double() - ref).norm() / ref.norm())
    tripped = actor.context(dev).range_tripped()
    med = {k: float(np.median(v)) for k, v in t.items()}
    col = lambda k: f"{med[k]:8.3f} [{min(t[k]):7.3f} .. {max(t[k]):7.3f}]"
    print(f"RESULT {B:3d}  {H}x{H}  {col('native')}  {col('torch')}  {med['native'] / med['torch']:7.3f}  {diff:.2e}  "
          f"{'TRIPPED' if tripped else 'ok'}", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        return one_size(int(sys.argv[2]), int(sys.argv[3]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "actor_grad_times.txt")
    lines = [f"# actor {CASE}; ms per call, median [min .. max] of {REPS} interleaved single calls (HIP events, {WARMUP} warm-up calls)",
             "# native: forward_train (update_running = 0) + param_grad (the gradient re-computes the forward itself); torch: train-mode",
             "# forward + backward of the stand-in module on the same device, gradients into .grad.  ratio: native / torch.",
             "# diff: whole-vector relative L2 between the two fp32 gradients; guard: the half-split range guard after the run",
             "# B  HxW      native_fwd+param_grad      torch_fwd+bwd              ratio    diff      guard"]
    for B, H in SIZES:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--one", str(B), str(H)],
                           capture_output=True, text=True)
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(p.stdout[-2000:], p.stderr[-2000:], sep="\n")
            lines.append(f"# {B} x {H}x{H}: exit status {p.returncode}; the run ends here")
            break
        lines.append(res[0][len("RESULT "):])
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 0 if len(lines) == 5 + len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
