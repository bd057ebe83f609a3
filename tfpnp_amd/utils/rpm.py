"""ReplayMemory -- tfpnp/utils/rpm.py:4-36 with the rows kept where the environment produced them.

The reference keeps a Python list of row Batches on the host: `save_experience` (trainer/mddpg/trainer.py:224-234) clones
every observation tensor to the CPU and stores `ob[i]` row by row, `sample_batch` picks rows with `random.sample`, and
`convert2batch` (:236-241) re-stacks and uploads them.  Here the memory is one `[capacity, *row_shape]` tensor per
observation key on the device of the stored tensors:

  store_batch(ob, hidden)   all rows of a batch in ONE launch (ops.ring_store, csrc/env.hip; one per 12 keys)
  sample(env_batch)         the sampled batch in ONE launch (ops.rows_gather with a device slot list): what
                            convert2batch(sample_batch(env_batch)) returns, without a host round trip or a device read

and the reference surface on top of them (`capacity`, `index`, `size()`, `store(row)`, `sample_batch(env_batch)` -> list of
row Batches), so trainer.py:46, :111, :135 and :234 read unchanged.

Ring rule (rpm.py:10-19): while size() < capacity a row goes to slot size() and `index` stays 0; once full, a row goes to slot
`index`, which then advances modulo capacity.  The t-th row ever stored therefore lives in slot t % capacity.  The
reference's "trimming" branch (:11-13) is unreachable and not reproduced.

Sampling draws `random.sample(range(size()), min(env_batch, size()))` from Python's global generator (or the `rng` given to
the constructor): the same positions, from the same generator state, as the reference's
`random.sample(list(enumerate(buffer)), k)` (tests/golden/replay_trace.npz is recorded from the executed reference).
`sample` and `sample_batch` each consume exactly one draw.

Storage is allocated at the first store, which also freezes the schema: ordered keys, per-row shapes, dtypes, device.  A later
store that does not match raises PnpxError naming the key; so does a value that is not a tensor (nested Batches included).
Stores copy.  All device work is issued on the CURRENT STREAM of the storage's device at the time of the call; a consumer on
another stream has to order itself behind it like behind any other torch work.  The head of the ring is a launch argument
of the store, so a store is not capturable into a HIP graph that is replayed with a moving head.

CPU tensors take a plain-indexing path (the convention of env/base.py `_take_rows` / `_put_rows`): host-logic tests and stub
environments run without a GPU.  Device tensors always take the native calls.

Not here: GroupReplayMemory (rpm.py:39-86: abstract key_from_ob, no caller), checkpointing (the reference does not save its
memory either), on-device random sampling.
"""
import random
from types import MappingProxyType

import torch

from .. import ops
from .._lib import PnpxError
from ..data.batch import Batch


class ReplayMemory:
    def __init__(self, capacity, rng=None):
        capacity = int(capacity)
        if capacity <= 0:
            raise PnpxError(f"ReplayMemory: capacity must be positive, got {capacity}")
        self.capacity = capacity
        self.index = 0
        self._size = 0
        self._rng = random if rng is None else rng
        self._storage = None        # key -> [capacity, *row_shape], in the key order of the first store

    # ------------------------------------------------------------------ reference surface
    def size(self):
        return self._size

    def store(self, obj):
        """One row: a Batch (or dict) of tensors WITHOUT the batch dimension, e.g. `ob[i]`."""
        items = self._items(obj)
        self._store_rows([(k, v.unsqueeze(0) if isinstance(v, torch.Tensor) else v) for k, v in items])

    def sample_batch(self, env_batch):
        """List of row Batches (views into one sampled batch): Batch.stack(rows) is sample(env_batch) of the same draw."""
        batch = self.sample(env_batch)
        return [batch[i] for i in range(len(batch))]

    # ------------------------------------------------------------------ fast surface
    def store_batch(self, ob, hidden=None):
        """All rows of `ob` (tensors [B, ...]); `hidden`, when given, is stored under the key 'hidden'
        (trainer.py:229-230).  More rows than the capacity keep the last `capacity` rows, as storing row by row would."""
        items = self._items(ob)
        if hidden is not None:
            if any(k == "hidden" for k, _ in items):
                raise PnpxError("ReplayMemory.store_batch: key 'hidden' given twice (in the batch and as the argument)")
            items.append(("hidden", hidden))
        self._store_rows(items)

    def sample(self, env_batch):
        """Batch of min(env_batch, size()) rows at random.sample positions, on the storage's device.  No device read."""
        if self._storage is None:
            raise PnpxError("ReplayMemory.sample: the memory is empty")
        n = self._size
        slots = self._rng.sample(range(n), min(int(env_batch), n))
        tensors = list(self._storage.values())
        device = tensors[0].device
        if device.type == "cuda":
            # the one small upload of a sample: from pinned memory and asynchronous, so the host does not wait for the stream
            idx = torch.tensor(slots, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
            got = ops.rows_gather(tensors, idx, len(slots))
        else:
            idx = torch.tensor(slots, dtype=torch.int64)
            got = [t[idx] for t in tensors]
        return Batch(dict(zip(self._storage.keys(), got)))

    # ------------------------------------------------------------------ storage
    @property
    def storage(self):
        """Read-only mapping key -> [capacity, *row_shape] tensor (empty before the first store).  Slots >= size() are
        uninitialised."""
        return MappingProxyType(self._storage or {})

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self._storage or {}).values())

    @staticmethod
    def _items(obj):
        if isinstance(obj, Batch):
            return list(obj.items())
        if isinstance(obj, dict):
            return list(obj.items())
        raise PnpxError(f"ReplayMemory: expected a Batch of tensors, got {type(obj).__name__}")

    def _check(self, items):
        """-> number of rows; allocates the storage / freezes the schema on the first store."""
        if not items:
            raise PnpxError("ReplayMemory: a batch without keys cannot be stored")
        for k, v in items:
            if not isinstance(v, torch.Tensor):
                raise PnpxError(f"ReplayMemory: key '{k}' holds a {type(v).__name__}, not a tensor (nested values are not stored)")
            if v.dim() < 1:
                raise PnpxError(f"ReplayMemory: key '{k}' has no batch dimension")
        n = items[0][1].shape[0]
        first_store = self._storage is None
        if first_store:
            device = items[0][1].device
            schema = {k: torch.empty((0,) + tuple(v.shape[1:]), dtype=v.dtype, device=device) for k, v in items}
        else:
            schema = self._storage
            device = next(iter(schema.values())).device
            keys = [k for k, _ in items]
            for k in schema:
                if k not in keys:
                    raise PnpxError(f"ReplayMemory: key '{k}' of the stored schema is missing (got {keys})")
        for k, v in items:
            if k not in schema:
                raise PnpxError(f"ReplayMemory: key '{k}' is not part of the stored schema {list(schema)}")
            s = schema[k]
            if v.dtype != s.dtype:
                raise PnpxError(f"ReplayMemory: key '{k}' has dtype {v.dtype}, the memory holds {s.dtype}")
            if tuple(v.shape[1:]) != tuple(s.shape[1:]):
                raise PnpxError(f"ReplayMemory: key '{k}' has row shape {tuple(v.shape[1:])}, the memory holds {tuple(s.shape[1:])}")
            if v.device != device:
                raise PnpxError(f"ReplayMemory: key '{k}' is on {v.device}, the memory is on {device}")
            if v.shape[0] != n:
                raise PnpxError(f"ReplayMemory: key '{k}' has {v.shape[0]} rows, the batch has {n}")
        if first_store:
            self._storage = {k: torch.empty((self.capacity,) + tuple(s.shape[1:]), dtype=s.dtype, device=device)
                             for k, s in schema.items()}
        return n

    def _store_rows(self, items):
        n = self._check(items)
        if n == 0:
            return
        by_key = dict(items)
        values = [by_key[k].detach() for k in self._storage]       # schema order
        cap = self.capacity
        first = (self._size + self.index) % cap        # slot of the next row: size() while filling, index once full
        skip = max(n - cap, 0)                         # rows that later rows of this very batch would overwrite
        if skip:
            values = [v[skip:] for v in values]
        slot0, rows = (first + skip) % cap, n - skip
        targets = list(self._storage.values())
        if targets[0].device.type == "cuda":
            ops.ring_store(values, targets, slot0, rows)
        else:
            slots = (torch.arange(rows, dtype=torch.int64) + slot0) % cap
            for v, t in zip(values, targets):
                t[slots] = v
        if self._size + n >= cap:
            self.index = (first + n) % cap
            self._size = cap
        else:
            self._size += n
