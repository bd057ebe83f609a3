"""Time one whole actor update three ways on the same GPU:

  (a) native     trainer/mddpg/actor_step.py::actor_update: forward_train_keep (the train-mode forward, once, running statistics
                 moved), the torch head and the toy loss of examples/train_actor.py, param_grad_kept, adam_step_
  (b) composed   what the package offered before: forward_train with the running update, the same head and loss, param_grad (which
                 re-computes the forward), torch clip_grad_norm_ + Adam on a flat nn.Parameter, load_flat_
  (c) torch      the torch stand-in module (tests/actor_cases.py::stand_in_actor in `.train()` mode): forward, the same head and
                 loss, backward, clip_grad_norm_ + Adam on its parameters -- what a user without the native actor runs

    python tools/time_actor_step.py [out_file]        (GPU box; default profiles/actor_step_times.txt)

One GPU process per size, each under its own time limit; a size that fails or runs out of time ends the run.  Wall clock with a
device synchronisation around each update (the native refresh ends with a read-back, so HIP events alone would not see it).
"""
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASE, SEED, WARMUP, REPS, LR, MAX_NORM = (9, 10, False), 3, 3, 20, 1e-4, 50.0
SIZES = [(48, 128), (48, 256)]
STEP_LIMIT = 300   # seconds per size


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one_size(B, H):
    from tests import actor_cases as A
    from tfpnp_amd import synth
    from tfpnp_amd.trainer.mddpg.actor_step import actor_update
    dev = torch.device("cuda:0")
    params = synth.make_policy_params(*CASE, seed=SEED)
    native, composed = A.native_actor(CASE, state_dict=params), A.native_actor(CASE, state_dict=params)
    net = A.load_params(A.stand_in_actor(*CASE), params).to(dev).train()
    r = np.random.RandomState(5)
    ob = torch.from_numpy(r.uniform(0, 1, (B, CASE[0], H, H)).astype(np.float32)).to(dev)
    idx_stop = torch.from_numpy(r.randint(0, 2, B)).to(dev)

    def loss_fn(action, logp, entropy):
        return -(logp.mean() + 0.01 * entropy.mean()) + sum(
            ((action[k] - 0.5 * rng['scale'] - rng['shift']) ** 2).mean() for k, rng in native.action_range.items())

    def leg_native():
        actor_update(native, ob, loss_fn, LR, max_norm=MAX_NORM, idx_stop=idx_stop)

    from tests import actor_train_cases as T
    stat = T.stat_mask(CASE).to(dev).nonzero().squeeze(1)      # an index tensor: no host synchronisation per update
    flat = torch.nn.Parameter(composed.parameters_flat(dev).clone())
    opt_flat = torch.optim.Adam([flat], lr=LR)
    ctx = composed.context(dev)

    def leg_composed():
        from tfpnp_amd import ops
        probs, det = (t.requires_grad_() for t in ops.policy_forward_train(ctx, ob))
        loss_fn(*composed.head(probs, det, idx_stop, True)).backward()
        flat.grad = composed.param_grad(ob, probs.grad, det.grad)
        torch.nn.utils.clip_grad_norm_([flat], MAX_NORM)
        opt_flat.step()
        # the running statistics moved in the context, not in `flat`: carry them over before the vector goes back
        with torch.no_grad():
            flat[stat] = composed.parameters_flat(dev)[stat]
        composed.load_flat_(flat.detach())

    trainable = [p for p in net.parameters()]
    opt_net = torch.optim.Adam(trainable, lr=LR)

    def leg_torch():
        opt_net.zero_grad(set_to_none=True)
        probs, det = net(ob)
        loss_fn(*native.head(probs, det, idx_stop, True)).backward()
        torch.nn.utils.clip_grad_norm_(trainable, MAX_NORM)
        opt_net.step()

    legs = {"native": leg_native, "composed": leg_composed, "torch": leg_torch}
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    t = {k: [] for k in legs}
    for _ in range(REPS):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    tripped = native.context(dev).range_tripped() or composed.context(dev).range_tripped()
    med = {k: float(np.median(v)) for k, v in t.items()}
    col = lambda k: f"{med[k]:8.3f} [{min(t[k]):7.3f} .. {max(t[k]):7.3f}]"
    print(f"RESULT {B:3d}  {H}x{H}  {col('native')}  {col('composed')}  {col('torch')}  {med['native'] / med['composed']:7.3f}  "
          f"{med['native'] / med['torch']:7.3f}  {'TRIPPED' if tripped else 'ok'}", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        return one_size(int(sys.argv[2]), int(sys.argv[3]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "actor_step_times.txt")
    lines = [f"# actor {CASE}; ms per update, median [min .. max] of {REPS} interleaved updates (wall clock, device synchronised around each; "
             f"{WARMUP} warm-up updates)",
             "# (a) native: actor_update = forward_train_keep + torch head / toy loss + param_grad_kept + adam_step_",
             "# (b) composed: forward_train (running update) + head / loss + param_grad (re-computes the forward) + torch clip / Adam on a flat",
             "#     parameter + load_flat_;  (c) torch: the stand-in module's train-mode forward + head / loss + backward + clip / Adam",
             "# a/b, a/c: ratios of the medians; guard: the half-split range guard after the run",
             "# B  HxW      (a) native                 (b) composed               (c) torch                  a/b      a/c      guard"]
    head = len(lines)
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
    return 0 if len(lines) == head + len(SIZES) else 1


if __name__ == "__main__":
    sys.exit(main())
