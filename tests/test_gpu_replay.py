"""GPU tests of the device-resident replay memory: ops.ring_store (csrc/env.hip ring_store_kernel) against plain indexing on
a CPU twin, ReplayMemory on the device against its CPU-path twin and the trace of the executed reference, and a round trip
through the native CS-MRI environment against the host path of trainer/mddpg/trainer.py:224-241.  Every path is a copy: all
comparisons are bit for bit (torch.equal)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import replay_cases as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def ring_reference(values, storages, first_slot, n_rows):
    """Plain indexing on CPU tensors: storages[k][(first_slot + r) % capacity] = values[k][r]."""
    cap = storages[0].shape[0]
    slots = (torch.arange(n_rows) + first_slot) % cap
    for v, t in zip(values, storages):
        t[slots] = v[:n_rows]


def make_fields(n, g):
    """The access widths of the copy: (name, CPU values [n, ...]) -- 16-byte, 4-byte and byte rows, a 4-byte `hidden`, and two
    sources whose BASE is misaligned (views one row / one byte into a larger buffer)."""
    buf = torch.rand((n + 1, 3), generator=g)                        # 12 B rows: buf[1:] starts 12 B behind a 16-B boundary
    bbuf = torch.rand((n * 16 + 1,), generator=g) > 0.5
    return [("x16", torch.rand((n, 2, 8, 8, 2), generator=g)),       # 1024 B rows
            ("x4", torch.rand((n, 3), generator=g)),                 # 12 B rows
            ("b1", torch.rand((n, 1, 5, 3), generator=g) > 0.5),     # 15 B rows
            ("hidden", torch.rand((n,), generator=g)),               # 4 B rows
            ("x4_off", buf[1:]),
            ("b1_off", bbuf[1:].view(n, 16))]                        # 16 B rows at storage offset 1: byte path


def to_device_keeping_offsets(name, v):
    """Device twin of a CPU value; the *_off fields are rebuilt as views into a larger device buffer so that their base
    pointers are misaligned on the device as well."""
    if name == "x4_off":
        big = torch.empty((v.shape[0] + 1, 3), device=dev())
        big[1:] = v.to(dev())
        out = big[1:]
        assert out.is_contiguous() and out.data_ptr() % 16 == 12
        return out
    if name == "b1_off":
        big = torch.empty((v.numel() + 1,), dtype=torch.bool, device=dev())
        big[1:] = v.reshape(-1).to(dev())
        out = big[1:].view(v.shape)
        assert out.is_contiguous() and out.data_ptr() % 4 == 1
        return out
    return v.to(dev())


def sentinel_like(name, v, cap):
    shape = (cap,) + tuple(v.shape[1:])
    return torch.ones(shape, dtype=torch.bool) if v.dtype == torch.bool else torch.full(shape, -7.0)


def test_ring_store_matches_plain_indexing():
    from tfpnp_amd import _lib, ops
    cap = 7
    g = torch.Generator().manual_seed(11)
    twin = dev_st = None
    for first, n in ((0, 3), (3, 3), (6, 3), (2, 7), (5, 0)):        # fill, fill, wrap mid-batch, full lap, nothing
        fields = make_fields(max(n, 1), g)
        if twin is None:
            twin = [sentinel_like(k, v, cap) for k, v in fields]
            dev_st = [t.to(dev()) for t in twin]
        values = [v[:n] for _, v in fields] if n else [v[:0] for _, v in fields]
        dvals = [to_device_keeping_offsets(k, v)[:n] for k, v in fields]
        before = [v.clone() for v in dvals]
        ring_reference(values, twin, first, n)
        ops.ring_store(dvals, dev_st, first, n)
        for (k, _), t, d, v, b in zip(fields, twin, dev_st, dvals, before):
            assert d.dtype == t.dtype and torch.equal(d.cpu(), t), (k, first, n)
            assert torch.equal(v, b), k                                # sources are only read
    # the C ABI refuses what could make two rows race for a slot or leave the ring, and writes nothing
    lib = _lib.lib()
    ctx = ops.default_context(dev())
    vals = [torch.rand((8,) + tuple(t.shape[1:]), device=dev()) if t.dtype != torch.bool else
            torch.zeros((8,) + tuple(t.shape[1:]), dtype=torch.bool, device=dev()) for t in dev_st]
    nt = len(vals)
    S = (C.c_void_p * nt)(*[v.data_ptr() for v in vals])
    D = (C.c_void_p * nt)(*[t.data_ptr() for t in dev_st])
    RB = (C.c_size_t * nt)(*[(t.numel() // cap) * t.element_size() for t in dev_st])
    stream = C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)
    PNPX_ERR_ARG = 1
    for first, n in ((0, 8), (cap, 1), (-1, 1)):
        assert lib.pnpx_ring_store(ctx.handle, nt, S, D, RB, first, cap, n, stream) == PNPX_ERR_ARG, (first, n)
        assert b"ring_store" in lib.pnpx_last_error()
    assert lib.pnpx_ring_store(ctx.handle, nt, S, D, RB, 0, 0, 0, stream) == PNPX_ERR_ARG
    torch.cuda.synchronize()
    for t, d in zip(twin, dev_st):
        assert torch.equal(d.cpu(), t)
    # ... and so does the binding, with the package's exception
    for first, n in ((0, 8), (cap, 1), (-1, 1)):
        with pytest.raises(_lib.PnpxError):
            ops.ring_store(vals, dev_st, first, n)
    with pytest.raises(_lib.PnpxError):
        ops.ring_store([v.double() if v.dtype != torch.bool else v for v in vals], dev_st, 0, 1)
    with pytest.raises(_lib.PnpxError):
        ops.ring_store([v.cpu() for v in vals], dev_st, 0, 1)
    with pytest.raises(_lib.PnpxError):
        ops.ring_store(vals, [t.cpu() for t in dev_st], 0, 1)
    for t, d in zip(twin, dev_st):
        assert torch.equal(d.cpu(), t)


def test_ring_store_thirteen_fields_in_one_call():
    """More tensors than one launch carries (12): the call is chunked, every field arrives."""
    from tfpnp_amd import ops
    cap, n, first = 5, 4, 3
    g = torch.Generator().manual_seed(13)
    values = [torch.rand((n, k + 1, 3), generator=g) for k in range(13)]
    twin = [torch.full((cap, k + 1, 3), -7.0) for k in range(13)]
    dev_st = [t.to(dev()) for t in twin]
    ring_reference(values, twin, first, n)
    ops.ring_store([v.to(dev()) for v in values], dev_st, first, n)
    for k, (t, d) in enumerate(zip(twin, dev_st)):
        assert torch.equal(d.cpu(), t), k


def test_ring_store_row_longer_than_one_sweep():
    """307 200 B rows: longer than the 64 x 256 x 16 B one sweep of the grid covers, so the grid-stride loop iterates."""
    from tfpnp_amd import ops
    cap, first = 4, 2
    g = torch.Generator().manual_seed(17)
    v = torch.rand((3, 3, 160, 160), generator=g)
    twin = torch.full((cap, 3, 160, 160), -7.0)
    d = twin.to(dev())
    ring_reference([v], [twin], first, 3)
    ops.ring_store([v.to(dev())], [d], first, 3)
    assert torch.equal(d.cpu(), twin)


def test_ring_store_more_rows_than_one_grid():
    """70 000 rows of 4 bytes: more than grid.y holds (65 535), so the entry issues a second launch with its own first slot."""
    from tfpnp_amd import ops
    cap, first, n = 70001, 69990, 70000
    v = torch.arange(n, dtype=torch.float32)
    twin = torch.full((cap,), -7.0)
    d = twin.to(dev())
    ring_reference([v], [twin], first, n)
    ops.ring_store([v.to(dev())], [d], first, n)
    assert torch.equal(d.cpu(), twin)


def test_ring_store_addresses_past_4_gib():
    """Storage of 4100 rows x 1 MiB (4.3 GB, what one field of a replay at the reference's default size and 256 x 256 exceeds):
    slot * row_bytes needs 64 bits.  Two rows at slot 4099 land in slots 4099 and 0; their neighbours keep a sentinel."""
    from tfpnp_amd import ops
    cap, row = 4100, 262144
    st = torch.empty((cap, row), dtype=torch.float32, device=dev())
    for slot in (0, 1, 4098, 4099):
        st[slot].fill_(-7.0)
    g = torch.Generator().manual_seed(19)
    v = torch.rand((2, row), generator=g)
    ops.ring_store([v.to(dev())], [st], 4099, 2)
    assert torch.equal(st[4099].cpu(), v[0]) and torch.equal(st[0].cpu(), v[1])
    sentinel = torch.full((row,), -7.0)
    assert torch.equal(st[1].cpu(), sentinel) and torch.equal(st[4098].cpu(), sentinel)


def test_memory_on_device_equals_cpu_twin_and_reference_trace():
    from tfpnp_amd.utils.rpm import ReplayMemory
    cap = int(R.trace()["s1_capacity"])
    for how in ("batch", "rows"):
        host_samples = []
        R.drive(ReplayMemory(cap), "s1", how, on_stage=lambda s, b: host_samples.append(b))
        mem = ReplayMemory(cap)
        seen = []

        def compare(s, got):
            seen.append(s)
            for k in R.KEYS:
                assert got[k].device == dev() and got[k].dtype == host_samples[s][k].dtype
                assert torch.equal(got[k].cpu(), host_samples[s][k]), (how, s, k)

        R.drive(mem, "s1", how, device=dev(), on_stage=compare)
        assert seen == list(range(9))
        assert all(v.device == dev() for v in mem.storage.values())


def test_sample_reads_nothing_back_and_stores_copy():
    from tfpnp_amd.utils.rpm import ReplayMemory
    mem = ReplayMemory(4)
    ob = R.rows(range(3), dev())
    hidden = torch.zeros(3, device=dev())
    mem.store_batch(ob, hidden)                       # allocation and first launches outside the sync detector
    mem.sample(2)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mem.store_batch(ob, hidden)                   # laps: 3 + 3 rows in a ring of 4
        got = mem.sample(3)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    ob.tag.add_(100)
    ob.x.zero_()
    ob.m.fill_(True)
    hidden.fill_(5.0)
    torch.cuda.synchronize()
    R.check_payloads(got)
    again = mem.sample(4)
    R.check_payloads(again)
    assert sorted(again.tag.tolist()) == [0, 1, 2, 2] and not again.hidden.any()
    assert mem.index == 2 and mem.size() == 4


def test_environment_round_trip(unet_params):
    """store_batch(ob, hidden) at every env step against a host list kept exactly as save_experience keeps it (per-row
    .clone().detach().cpu()); the same draw, then convert2batch on the host rows vs sample() -- equal key by key, equal policy
    observations, and equal next variables / reward from the native one-step model."""
    from tfpnp_amd.data.batch import Batch
    from tfpnp_amd.pnp import UNetDenoiser2D
    from tfpnp_amd.tasks.csmri import ADMMSolver_CSMRI, CSMRIEnv
    from tfpnp_amd import synth
    from tfpnp_amd.utils.rpm import ReplayMemory
    B, H, W, steps, pack = 2, 64, 64, 3, 2
    d = synth.make_csmri_batch(B, H, W, ratio=4, sigma_n=15.0, seed=5)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    env = CSMRIEnv(None, ADMMSolver_CSMRI(UNetDenoiser2D(state_dict=unet_params)), max_episode_step=steps)
    acts = synth.make_actions(B, n_steps=steps, pack=pack)
    stops = [[1, 0], [0], [0]]                                       # row 0 stops after the first step
    mem = ReplayMemory(8)
    host_rows = []
    ob = env.reset({k: g(v) for k, v in d.items()})
    hidden_full = torch.arange(B, dtype=torch.float32, device=dev()) + 0.5
    hidden = hidden_full
    for s in range(steps):
        n = len(ob)
        assert n == len(stops[s])
        action = {"sigma_d": g(acts[s]["sigma_d"][:n]), "mu": g(acts[s]["mu"][:n]), "idx_stop": g(np.array(stops[s], np.int64))}
        _, ob_masked, _, all_done, _ = env.step(action)
        mem.store_batch(ob, hidden)
        saved = Batch({k: v.clone().detach().cpu() for k, v in ob.items()})      # trainer.py:224-234
        saved["hidden"] = hidden.clone().detach().cpu()
        host_rows.extend(saved[i] for i in range(n))
        ob, hidden = ob_masked, hidden_full[env.idx_left, ...]
        if all_done:
            break
    assert mem.size() == len(host_rows) == 4 and mem.index == 0
    k_sample = 3
    random.seed(23)
    picked = random.sample(list(enumerate(host_rows)), k_sample)      # rpm.py:24-36
    host = Batch.stack([row for _, row in picked]).to(dev())          # convert2batch, trainer.py:236-241
    random.seed(23)
    got = mem.sample(k_sample)
    assert list(got.keys()) == list(host.keys())
    for k in host.keys():
        assert got[k].dtype == host[k].dtype and got[k].shape == host[k].shape and torch.equal(got[k], host[k]), k
    assert torch.equal(env.get_policy_ob(got), env.get_policy_ob(host))
    action = {"sigma_d": g(acts[1]["sigma_d"][:1]).expand(k_sample, -1).contiguous(),
              "mu": g(acts[1]["mu"][:1]).expand(k_sample, -1).contiguous()}
    with torch.no_grad():
        nxt_a, rew_a = env.forward(got, action)
        nxt_b, rew_b = env.forward(host, action)
    assert torch.equal(nxt_a.variables, nxt_b.variables) and torch.equal(rew_a, rew_b)
    assert torch.isfinite(rew_a).all()
