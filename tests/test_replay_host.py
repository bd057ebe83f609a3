"""Host logic of tfpnp_amd.utils.rpm.ReplayMemory on its CPU-tensor path, against the trace recorded from the executed
reference (tests/golden/replay_trace.npz, tools/make_replay_golden.py): ring rule, sampling order, schema checks."""
import os
import random

import pytest
import torch

from tests import replay_cases as R

ROOT = R.ROOT


def memory(capacity, **kw):
    from tfpnp_amd.utils.rpm import ReplayMemory
    return ReplayMemory(capacity, **kw)


def test_golden_trace_is_the_recorded_one():
    """The values the schedule was specified with: stage -> (size, index, sampled tags)."""
    tr = R.trace()
    assert tr["s1_stores"].tolist() == [3, 4, 1, 5, 2, 7, 3, 3, 6] and int(tr["s1_capacity"]) == 10
    assert tr["s1_size"].tolist() == [3, 7, 8, 10, 10, 10, 10, 10, 10]
    assert tr["s1_index"].tolist() == [0, 0, 0, 3, 5, 2, 5, 8, 4]
    assert tr["s1_sampled"].tolist() == [[1, 0, 2, -1], [5, 0, 6, 4], [5, 4, 0, 6], [3, 10, 11, 9], [6, 11, 13, 10],
                                         [18, 16, 20, 19], [19, 21, 23, 15], [19, 20, 26, 18], [33, 30, 32, 27]]
    assert tr["s2_stores"].tolist() == [7, 2] and int(tr["s2_capacity"]) == 5
    memory(1)          # the module under test exists


@pytest.mark.parametrize("how", ["rows", "batch"])
@pytest.mark.parametrize("name", ["s1", "s2"])
def test_schedules_follow_the_reference_trace(name, how):
    mem = memory(int(R.trace()[f"{name}_capacity"]))
    assert mem.size() == 0 and mem.index == 0 and mem.nbytes == 0 and len(mem.storage) == 0
    R.drive(mem, name, how)
    assert list(mem.storage.keys()) == list(R.KEYS)
    per_row = 8 + 64 * 4 + 15
    assert mem.nbytes == mem.capacity * per_row
    for k in R.KEYS:
        assert mem.storage[k].dtype == R.DTYPES[k] and tuple(mem.storage[k].shape) == (mem.capacity,) + R.SHAPES[k]
    with pytest.raises(TypeError):
        mem.storage["tag"] = torch.zeros(1)


def test_hidden_is_stored_under_its_key_and_empty_batches_are_noops():
    mem = memory(6)
    ob = R.rows(range(4))
    hidden = torch.arange(4, dtype=torch.float32) + 0.25
    mem.store_batch(ob, hidden)
    assert list(mem.storage.keys()) == list(R.KEYS) + ["hidden"]
    mem.store_batch(R.rows([]), hidden[:0])
    assert mem.size() == 4 and mem.index == 0
    got = mem.sample(10)
    assert len(got) == 4 and torch.equal(got.hidden, got.tag.float() + 0.25)
    R.check_payloads(got)
    with pytest.raises(Exception, match="hidden"):
        mem.store_batch(R.rows([9]))                 # the schema now has 'hidden'


def test_private_generator():
    a, b = memory(10, rng=random.Random(3)), memory(10)
    a.store_batch(R.rows(range(10)))
    b.store_batch(R.rows(range(10)))
    state = random.getstate()
    got = a.sample(4).tag.tolist()
    assert random.getstate() == state                # the global generator was not touched
    assert got == random.Random(3).sample(range(10), 4)
    random.seed(3)
    assert b.sample(4).tag.tolist() == got


def test_schema_violations_name_the_key():
    from tfpnp_amd._lib import PnpxError
    from tfpnp_amd.data.batch import Batch

    def fresh():
        mem = memory(5)
        mem.store_batch(R.rows(range(2)))
        return mem

    ob = R.rows(range(2, 4))
    cases = {
        "missing key": (Batch(tag=ob.tag, x=ob.x), "'m'"),
        "extra key": (Batch(tag=ob.tag, x=ob.x, m=ob.m, extra=ob.x), "'extra'"),
        "wrong dtype": (Batch(tag=ob.tag, x=ob.x.double(), m=ob.m), "'x'"),
        "wrong row shape": (Batch(tag=ob.tag, x=ob.x, m=ob.m[:, :, :4]), "'m'"),
        "non-tensor value": (Batch(tag=ob.tag, x=ob.x, m=[True, False]), "'m'"),
        "nested value": (Batch(tag=ob.tag, x=Batch(y=ob.x), m=ob.m), "'x'"),
    }
    for what, (bad, key) in cases.items():
        mem = fresh()
        with pytest.raises(PnpxError, match=key):
            mem.store_batch(bad)
        with pytest.raises(PnpxError, match=key):
            mem.store(bad[0] if what != "non-tensor value" else Batch(tag=ob.tag[0], x=ob.x[0], m=True))
        assert mem.size() == 2 and mem.index == 0, what           # nothing was stored
        R.check_payloads(mem.sample(2))
    with pytest.raises(PnpxError, match="'m'"):                   # also at the first store, before anything is allocated
        memory(5).store_batch(cases["non-tensor value"][0])
    with pytest.raises(PnpxError):
        memory(0)
    with pytest.raises(PnpxError):
        memory(5).sample(1)


def test_store_copies():
    for how in ("rows", "batch"):
        mem = memory(4)
        ob = R.rows(range(3))
        if how == "rows":
            for i in range(3):
                mem.store(ob[i])
        else:
            mem.store_batch(ob)
        ob.tag.add_(100)
        ob.x.zero_()
        ob.m.fill_(True)
        got = mem.sample(3)
        assert sorted(got.tag.tolist()) == [0, 1, 2]
        R.check_payloads(got)
        got.x.zero_()                                             # a sample is a copy as well
        R.check_payloads(mem.sample(3))


def test_header_and_binding_declare_the_ring_store():
    """(That the header stays plain C99 / C++11 with the new prototype is tests/test_c_abi.py's check.)"""
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    assert "int pnpx_ring_store(pnpx_ctx* ctx, int n_tensors, const void* const* src_host, void* const* dst_host," in header
    from tfpnp_amd import _lib
    assert "pnpx_ring_store" in _lib.EXPORTED_SYMBOLS
