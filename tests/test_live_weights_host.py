"""The ownership of the live weights (tfpnp_amd/live.py) without a GPU: which copy of an actor's / a critic's weights is the
truth after each call that loads, moves or changes them, on one device and across two.  ops.Context is replaced by a recorder
and device tensors by storage-less stand-ins that only report a device, so every transition is observed through the modules'
public methods."""
import functools

import pytest
import torch

from tfpnp_amd import ops, torch_ops
from tfpnp_amd._lib import PnpxError
from tfpnp_amd.policy import ResNetActor_ADMM
from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn

CUDA0, CUDA1 = torch.device("cuda", 0), torch.device("cuda", 1)


class DeviceVector(torch.Tensor):
    """A float32 vector "on" cuda:<index> without storage: reports its device, and .to(device) gives another one that
    remembers where it came from.  Nothing else is implemented.  (`to` is overridden as a method: torch's own initialises the
    GPU runtime for a ROCm target before it dispatches.)"""

    @staticmethod
    def __new__(cls, index, origin=None):
        t = torch.Tensor._make_wrapper_subclass(cls, (8,), dtype=torch.float32, device=f"cuda:{index}")
        t.origin = origin
        return t

    def to(self, device):
        return type(self)(torch.device(device).index, origin=self)

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        raise NotImplementedError(f"DeviceVector: {func}")


class RecordingContext:
    """ops.Context as the modules use it: a device, a cid, `_policy` / `_critic` set as the real one sets them, every call
    appended to `log`.  fail[method] = unload: the next call of that method raises PnpxError, having unloaded the network
    first or not."""
    log, fail, made = [], {}, []

    def __init__(self, device):
        self.device = torch.device(device)
        self.cid = len(self.made) + 1
        self._policy = self._critic = None
        self.made.append(self)

    def _call(self, name, holds, loads, *args):
        self.log.append((name, self.device.index) + args)
        if name in self.fail:
            if self.fail.pop(name):
                setattr(self, holds, None)
            raise PnpxError(f"{name}: told to fail")
        if loads:
            setattr(self, holds, args[1:])
        return DeviceVector(self.device.index, origin=self) if name.endswith("_params") else None

    load_policy = functools.partialmethod(_call, "load_policy", "_policy", True)
    load_policy_device = functools.partialmethod(_call, "load_policy_device", "_policy", True)
    policy_params = functools.partialmethod(_call, "policy_params", "_policy", False)
    load_critic = functools.partialmethod(_call, "load_critic", "_critic", True)
    load_critic_device = functools.partialmethod(_call, "load_critic_device", "_critic", True)
    critic_params = functools.partialmethod(_call, "critic_params", "_critic", False)
    critic_soft_update = functools.partialmethod(_call, "critic_soft_update", "_critic", False)
    critic_optim_reset = functools.partialmethod(_call, "critic_optim_reset", "_critic", False)

    def critic_adam_step(self, grad, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=50.0):
        self._call("critic_adam_step", "_critic", False, grad, lr)
        return "norm"


@pytest.fixture(autouse=True)
def recorder(monkeypatch):
    RecordingContext.log, RecordingContext.fail, RecordingContext.made = [], {}, []
    monkeypatch.setattr(ops, "Context", RecordingContext)
    return RecordingContext


@pytest.fixture(params=["policy", "critic"])
def net_kind(request):
    return (ResNetActor_ADMM(6, 5), "policy") if request.param == "policy" else (ResNet_wobn(9, 18, 1), "critic")


STATE = {"some.weight": torch.zeros(2)}


def names(log):
    return [(e[0], e[1]) for e in log]


def snapshot(net):
    return dict(net._ctx), net._live, net._state


def test_unloaded_module_has_no_context(net_kind, recorder):
    net, _ = net_kind
    with pytest.raises(ValueError, match="weights were not loaded"):
        net.context(CUDA0)
    assert recorder.made == [] and net.device is None and net.state_dict() == {}


def test_host_load_then_device_load_then_other_device(net_kind, recorder):
    net, kind = net_kind
    shape = net._shape()
    net.load_state_dict(STATE)
    c0 = net.context(CUDA0)
    assert names(recorder.log) == [(f"load_{kind}", 0)] and recorder.log[0][2:] == (net._state,) + shape
    assert net.context(CUDA0) is c0 and len(recorder.log) == 1 and len(recorder.made) == 1
    assert net.device == CUDA0 and net._state is not None

    # a device load on another device: a fresh context there, which is the truth from then on
    flat = DeviceVector(1)
    assert net.load_flat_(flat) is net
    c1 = recorder.made[1]
    assert recorder.log[1][:2] == (f"load_{kind}_device", 1) and recorder.log[1][2] is flat and recorder.log[1][3:] == shape
    assert net._ctx == {("cuda", 1): c1} and net._state is None and net.device == CUDA1

    # the first device again: from cuda:1's vector, moved, not from a state dict
    c0b = net.context(CUDA0)
    assert c0b is recorder.made[2] and c0b is not c0
    assert names(recorder.log[2:]) == [(f"{kind}_params", 1), (f"load_{kind}_device", 0)]
    moved = recorder.log[3][2]
    assert moved.device == CUDA0 and moved.origin.device == CUDA1 and moved.origin.origin is c1
    assert set(net._ctx) == {("cuda", 1), ("cuda", 0)} and net.device == CUDA1 and net._state is None
    assert net.parameters_flat(CUDA0).origin is c0b

    # a second device load on cuda:1 refreshes its context in place and drops the other copy
    net.load_flat_(DeviceVector(1))
    assert len(recorder.made) == 3 and recorder.log[-1][:2] == (f"load_{kind}_device", 1)
    assert net._ctx == {("cuda", 1): c1} and net.device == CUDA1

    # a checkpoint load forgets every context
    net.load_state_dict(STATE)
    assert net._ctx == {} and net._live is None and net._state is not None and net.device is None


def test_failed_refresh_that_unloads_drops_the_context(net_kind, recorder):
    net, kind = net_kind
    net.load_state_dict(STATE)
    net.load_flat_(DeviceVector(1))
    c0 = net.context(CUDA0)
    assert net.device == CUDA1
    recorder.fail[f"load_{kind}_device"] = True
    with pytest.raises(PnpxError, match="told to fail"):
        net.load_flat_(DeviceVector(1))
    assert net._ctx == {("cuda", 0): c0} and net._live is None and net._state is None
    assert net.device == CUDA0                       # falls back to the device that is left
    with pytest.raises(ValueError, match="weights were not loaded"):
        net.context(CUDA1)                           # no silent reload from a stale copy
    assert len(recorder.made) == 2


def test_failed_refresh_that_keeps_the_network_drops_nothing(net_kind, recorder):
    net, kind = net_kind
    net.load_state_dict(STATE)
    net.load_flat_(DeviceVector(1))
    net.context(CUDA0)
    before = snapshot(net)
    recorder.fail[f"load_{kind}_device"] = False
    with pytest.raises(PnpxError, match="told to fail"):
        net.load_flat_(DeviceVector(1))
    assert snapshot(net) == before and net.device == CUDA1


@pytest.mark.parametrize("unload", [False, True])
def test_failed_load_on_a_fresh_context_changes_nothing(net_kind, recorder, unload):
    net, kind = net_kind
    net.load_state_dict(STATE)
    net.context(CUDA0)
    before = snapshot(net)
    recorder.fail[f"load_{kind}_device"] = unload
    with pytest.raises(PnpxError, match="told to fail"):
        net.load_flat_(DeviceVector(1))
    assert snapshot(net) == before and net.device == CUDA0 and net._state is not None
    with pytest.raises(PnpxError, match="cpu"):
        net.load_flat_(torch.zeros(8))
    with pytest.raises(PnpxError, match="torch.Tensor"):
        net.load_flat_([0.0])
    assert snapshot(net) == before


@pytest.mark.parametrize("entry", ["soft_update_", "adam_step_"])
def test_critic_updates_take_the_same_transitions(recorder, entry):
    net = ResNet_wobn(9, 18, 1)
    native = {"soft_update_": "critic_soft_update", "adam_step_": "critic_adam_step"}[entry]
    call = (lambda v: net.soft_update_(v, 0.01)) if entry == "soft_update_" else (lambda v: net.adam_step_(v, 1e-3))
    with pytest.raises(ValueError, match="weights were not loaded"):
        call(DeviceVector(0))
    assert recorder.made == []
    with pytest.raises(PnpxError, match="torch.Tensor"):
        call([0.0])
    net.load_state_dict(STATE)
    c0 = net.context(CUDA0)

    # on a device without a context: one is made there from the current weights, updated, and is the truth
    v = DeviceVector(1)
    out = call(v)
    assert out == "norm" if entry == "adam_step_" else out is net
    c1 = recorder.made[1]
    assert names(recorder.log) == [("load_critic", 0), ("load_critic", 1), (native, 1)] and recorder.log[-1][2] is v
    assert net._ctx == {("cuda", 1): c1} and net._state is None and net.device == CUDA1

    # a failure that keeps the critic drops nothing; one that unloads it drops the context
    c0 = net.context(CUDA0)
    before = snapshot(net)
    recorder.fail[native] = False
    with pytest.raises(PnpxError, match="told to fail"):
        call(DeviceVector(1))
    assert snapshot(net) == before
    recorder.fail[native] = True
    with pytest.raises(PnpxError, match="told to fail"):
        call(DeviceVector(1))
    assert net._ctx == {("cuda", 0): c0} and net._live is None and net.device == CUDA0
    with pytest.raises(ValueError, match="weights were not loaded"):
        net.context(CUDA1)


def test_critic_reset_optim_reaches_every_context(recorder):
    net = ResNet_wobn(9, 18, 1, state_dict=STATE)
    net.load_flat_(DeviceVector(1))
    net.context(CUDA0)
    del recorder.log[:]
    assert net.reset_optim_() is net
    assert sorted(names(recorder.log)) == [("critic_optim_reset", 0), ("critic_optim_reset", 1)]


def test_actor_train_forward_marks_its_context(recorder, monkeypatch):
    calls = []

    def call(name, state, *args):
        calls.append((name, args[-1]))
        return torch.tensor([[0.25, 0.75], [0.5, 0.5]]), torch.full((2, 10), 0.5)

    monkeypatch.setattr(torch_ops, "call", call)
    net = ResNetActor_ADMM(6, 5, state_dict=STATE, bn_follows_mode=True)
    c1, c0 = net.context(CUDA1), net.context(CUDA0)
    ob = DeviceVector(0)
    net.eval()
    action, logp, entropy, _ = net(ob, None, False, None)
    assert calls == [("policy_forward", c0.cid)] and action["idx_stop"].tolist() == [1, 0]
    assert net._live is None and net._state is not None and len(net._ctx) == 2      # the eval forward changes nothing
    net.train()
    net(ob, None, False, None)
    assert calls[-1] == ("policy_forward_train", c0.cid)
    assert net._ctx == {("cuda", 0): c0} and net._live == ("cuda", 0) and net._state is None and net.device == CUDA0
    assert c1 not in net._ctx.values()
    # without bn_follows_mode the mode is ignored
    plain = ResNetActor_ADMM(6, 5, state_dict=STATE)
    plain(DeviceVector(0), None, False, None)
    assert calls[-1][0] == "policy_forward" and plain._live is None and plain._state is not None
