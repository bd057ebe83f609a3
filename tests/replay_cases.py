"""Shared by tests/test_replay_host.py and tests/test_gpu_replay.py: the schedules of tests/golden/replay_trace.npz (recorded
from the executed reference replay memory by tools/make_replay_golden.py) and rows whose payloads are functions of their tag."""
import os
import random

import numpy as np
import torch

from tfpnp_amd.data.batch import Batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tag", "x", "m")
SHAPES = {"tag": (), "x": (2, 4, 4, 2), "m": (1, 5, 3)}
DTYPES = {"tag": torch.int64, "x": torch.float32, "m": torch.bool}


def trace():
    return np.load(os.path.join(ROOT, "tests", "golden", "replay_trace.npz"))


def rows(tags, device="cpu"):
    """Batch of len(tags) rows: `tag` int64 [n], `x` fp32 [n,2,4,4,2] and `m` bool [n,1,5,3], both determined by the tag."""
    tags = torch.as_tensor(list(tags), dtype=torch.int64)
    n = tags.numel()
    ramp = torch.arange(64, dtype=torch.float32).reshape(1, 2, 4, 4, 2)
    x = tags.reshape(n, 1, 1, 1, 1).float() * 0.5 + ramp / 128
    bits = torch.arange(15, dtype=torch.int64).reshape(1, 1, 5, 3)
    m = ((tags.reshape(n, 1, 1, 1) + 1) * (bits + 3)) % 5 < 2
    return Batch(tag=tags, x=x, m=m).to(device)


def check_payloads(batch):
    """Every row of `batch` carries the payloads of its tag, with dtypes and row shapes intact."""
    want = rows(batch.tag.cpu().tolist())
    for k in KEYS:
        got = batch[k]
        assert got.dtype == DTYPES[k] and tuple(got.shape[1:]) == SHAPES[k], (k, got.dtype, tuple(got.shape))
        assert torch.equal(got.cpu(), want[k]), k


def drive(memory, name, how, device="cpu", on_stage=None):
    """Runs schedule `name` ('s1' | 's2') of the golden trace through `memory` -- how = 'rows': store() row by row, 'batch':
    store_batch() -- and checks storage tags in slot order, size(), index, and the tags sampled by sample() and by
    Batch.stack(sample_batch()) against the trace after every store, and that payloads follow their tags.
    on_stage(stage, sampled Batch) is called with each sample() result."""
    tr = trace()
    env_batch = int(tr["env_batch"])
    assert memory.capacity == int(tr[f"{name}_capacity"])
    random.seed(int(tr["seed"]))
    tag = 0
    for s, n in enumerate(tr[f"{name}_stores"].tolist()):
        ob = rows(range(tag, tag + n), device)
        tag += n
        if how == "rows":
            for i in range(n):
                memory.store(ob[i])
        else:
            memory.store_batch(ob)
        size = int(tr[f"{name}_size"][s])
        assert memory.size() == size and memory.index == int(tr[f"{name}_index"][s]), (s, memory.size(), memory.index)
        assert memory.storage["tag"][:size].cpu().tolist() == tr[f"{name}_buffer"][s][:size].tolist(), s
        check_payloads(Batch({k: v[:size] for k, v in memory.storage.items()}))
        want = [t for t in tr[f"{name}_sampled"][s].tolist() if t >= 0]
        state = random.getstate()
        got = memory.sample(env_batch)
        after = random.getstate()
        assert got.tag.cpu().tolist() == want, (s, got.tag.tolist(), want)
        check_payloads(got)
        random.setstate(state)                                   # the same draw again, through the reference surface
        listed = memory.sample_batch(env_batch)
        assert random.getstate() == after, "sample and sample_batch must consume the same single draw"
        assert isinstance(listed, list) and len(listed) == len(want)
        assert all(tuple(r[k].shape) == SHAPES[k] for r in listed for k in KEYS)
        stacked = Batch.stack(listed)
        assert list(stacked.keys()) == list(got.keys())
        assert all(torch.equal(stacked[k], got[k]) and stacked[k].dtype == got[k].dtype for k in got.keys()), s
        if on_stage is not None:
            on_stage(s, got)
