"""Writes tests/golden/replay_trace.npz from the EXECUTED reference replay memory (tfpnp/utils/rpm.py, loaded by file path).
Build machine only: it needs the reference checkout and never runs on a GPU box.

    python tools/make_replay_golden.py

Rows are plain integer tags 0, 1, 2, ... in the order they are stored.  Per schedule: `random.seed(SEED)` once, then for every
store of the schedule the rows go in one by one (the loop of trainer/mddpg/trainer.py:232-234) and `sample_batch(ENV_BATCH)` is
called once.  Recorded per stage: the buffer's tags in slot order, size(), index and the sampled tags in order (rows padded
with -1).  The file holds these integers and the schedules only.
"""
import importlib.util
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "replay_trace.npz")
SEED, ENV_BATCH = 7, 4
SCHEDULES = {"s1": (10, (3, 4, 1, 5, 2, 7, 3, 3, 6)),      # fills, wraps in the middle of a store, laps
             "s2": (5, (7, 2))}                            # a store larger than the capacity


def load_reference_rpm():
    path = os.path.join(ref_shim.REF, "tfpnp", "utils", "rpm.py")
    spec = importlib.util.spec_from_file_location("ref_rpm", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def trace(mod, capacity, stores):
    memory = mod.ReplayMemory(capacity)
    random.seed(SEED)
    buf = np.full((len(stores), capacity), -1, np.int64)
    smp = np.full((len(stores), ENV_BATCH), -1, np.int64)
    size, index = np.zeros(len(stores), np.int64), np.zeros(len(stores), np.int64)
    tag = 0
    for s, n in enumerate(stores):
        for _ in range(n):
            memory.store(tag)
            tag += 1
        got = memory.sample_batch(ENV_BATCH)
        buf[s, :memory.size()] = memory.buffer
        smp[s, :len(got)] = got
        size[s], index[s] = memory.size(), memory.index
        print(f"capacity {capacity} stage {s + 1}: +{n} rows  size {size[s]}  index {index[s]}  sampled {got}  buffer {list(memory.buffer)}")
    return dict(capacity=np.int64(capacity), stores=np.asarray(stores, np.int64), buffer=buf, size=size, index=index, sampled=smp)


def main():
    assert ref_shim.available(), "reference not mounted"
    mod = load_reference_rpm()
    res = dict(seed=np.int64(SEED), env_batch=np.int64(ENV_BATCH))
    for name, (capacity, stores) in SCHEDULES.items():
        res.update({f"{name}_{k}": v for k, v in trace(mod, capacity, stores).items()})
    np.savez_compressed(OUT, **res)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
