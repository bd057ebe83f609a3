"""Time one replay-memory cycle (store the observation batch of an env step, then sample an update batch) both ways in one run on
one box, for the CS-MRI observation that CSMRIEnv._observation produces (3-variable solver) plus `hidden`, at B x H x W below:
  (a) host path      the algorithm of save_experience + sample_batch + convert2batch (tfpnp/trainer/mddpg/trainer.py:224-241 over
                     tfpnp/utils/rpm.py:10-36) restated with this package's Batch: every tensor cloned to the host, ob[i] stored row
                     by row in a Python list ring, random.sample over the list, Batch.stack, upload
                     (the way a PnPEnv user had to do it before the device memory existed; not the code under test)
  (b) device path    ReplayMemory.store_batch + ReplayMemory.sample: one ring-store launch, one gather launch, rows never leave
                     the device
Wall clock with torch.cuda.synchronize() before and after each repetition; the two legs alternate repetition by repetition, so
drift on a shared box hits both alike.  Both memories are pre-filled to capacity, so every timed store overwrites (steady
state); the time does not depend on the capacity.  Both legs draw with the same seed and must return the same batch, bit for
bit.  The figure of merit is the ratio of the two medians.

    python tools/time_replay.py [out_file [commit]]        (GPU box; default profiles/replay_times.txt)
"""
import os
import random
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tfpnp_amd.data.batch import Batch  # noqa: E402
from tfpnp_amd.utils.rpm import ReplayMemory  # noqa: E402

dev = torch.device("cuda:0")
WARMUP, REPS = 2, 20
B, H, W = 48, 128, 128
CAPACITY = 288


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


class HostMemory:
    """tfpnp/utils/rpm.py:4-36 restated: a list ring of row Batches on the host."""

    def __init__(self, capacity):
        self.capacity, self.buffer, self.index = capacity, [], 0

    def store(self, row):
        if len(self.buffer) == self.capacity:
            self.buffer[self.index] = row
            self.index = (self.index + 1) % self.capacity
        else:
            self.buffer.append(row)

    def sample_batch(self, env_batch):
        picked = random.sample(list(enumerate(self.buffer)), min(env_batch, len(self.buffer)))
        return [row for _, row in picked]


def observation(step):
    """The keys, shapes and dtypes of CSMRIEnv._observation for a 3-variable solver (mask as float), values from a seed."""
    g = torch.Generator(device=dev).manual_seed(step)
    r = lambda *shape: torch.rand(shape, generator=g, device=dev)
    ob = Batch(gt=r(B, 1, H, W), variables=r(B, 3, H, W, 2), T=r(B, 1, H, W), y0=r(B, 1, H, W, 2), ATy0=r(B, 1, H, W, 2),
               mask=(r(B, 1, H, W) > 0.5).float(), sigma_n=r(B, 1, H, W, 2))
    return ob, r(B)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "replay_times.txt")
    host, device = HostMemory(CAPACITY), ReplayMemory(CAPACITY)
    obs = [observation(s) for s in range(2)]             # two batches alternate, so every repetition stores new values
    step = [0]
    outs = {}

    def host_path():
        ob, hidden = obs[step[0] % 2]
        saved = Batch({k: v.clone().detach().cpu() for k, v in ob.items()})       # save_experience
        saved["hidden"] = hidden.clone().detach().cpu()
        for i in range(B):
            host.store(saved[i])
        random.seed(step[0])
        outs["a"] = Batch.stack(host.sample_batch(B)).to(dev)                     # sample_batch + convert2batch

    def device_path():
        ob, hidden = obs[step[0] % 2]
        device.store_batch(ob, hidden)
        random.seed(step[0])
        outs["b"] = device.sample(B)

    for fill in range(CAPACITY // B):                    # both rings full before anything is timed
        step[0] = fill
        host_path()
        device_path()
    assert len(host.buffer) == device.size() == CAPACITY
    legs = [("a_host_store+sample", host_path), ("b_device_store+sample", device_path)]
    times = {name: [] for name, _ in legs}
    for rep in range(WARMUP + REPS):
        step[0] = rep
        for name, fn in legs:
            t = wall_ms(fn)
            if rep >= WARMUP:
                times[name].append(t)
        assert list(outs["a"].keys()) == list(outs["b"].keys())
        assert all(torch.equal(outs["a"][k], outs["b"][k]) for k in outs["a"].keys()), "host path and device path disagree"
    commit = sys.argv[2] if len(sys.argv) > 2 else ""       # for a tree that travels without its git metadata
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            pass
    med = {k: float(np.median(v)) for k, v in times.items()}
    row_bytes = device.nbytes // CAPACITY
    lines = [f"# {torch.cuda.get_device_name(0)}; commit {commit or 'n/a (no git metadata on this box)'}; CS-MRI observation + hidden, "
             f"{B} x {H} x {W}: {len(device.storage)} keys, {row_bytes} B per row, {B * row_bytes / 1e6:.1f} MB per batch; capacity {CAPACITY}",
             f"# one cycle = store a batch of {B} rows + sample {B} rows; wall clock with device synchronisation around each repetition, legs "
             f"alternating; {REPS} repetitions after {WARMUP} warm-ups; ms per cycle",
             "# leg                              median        min        max   reps"]
    for name, t in times.items():
        lines.append(f"{name:28s} {med[name]:12.3f} {min(t):10.3f} {max(t):10.3f} {len(t):6d}")
    a, b = med["a_host_store+sample"], med["b_device_store+sample"]
    lines.append(f"# ratio of medians (a) / (b): {a / b:.1f}")
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
