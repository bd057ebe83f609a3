"""Host-side checks of the actor's live-weight entries (no GPU): the C ABI / binding surface, the stand-in module against
synth.policy_param_specs, and the name-based gather of utils.misc.hard_update and its refusals."""
import os
import re

import pytest
import torch

from tests import actor_cases as A
from tfpnp_amd import _lib, synth
from tfpnp_amd._lib import PnpxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pnpx_policy_load_device", "pnpx_policy_params")


def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    from tfpnp_amd import ops, policy
    for name in ("load_policy_device", "policy_params"):
        assert callable(getattr(ops.Context, name)), name
    for name in ("load_flat_", "parameters_flat", "state_dict"):
        assert callable(getattr(policy.ResNetActor_ADMM, name)), name
    assert isinstance(policy.network.ResNetActorBase.device, property)


@pytest.mark.parametrize("case", A.CASES)
def test_stand_in_matches_param_specs(case):
    m = A.stand_in_actor(*case)
    specs = [(k, tuple(s)) for k, s in synth.policy_param_specs(*case)]
    assert A.fp32_entries(m.state_dict()) == specs
    total = sum(v.numel() for v in m.state_dict().values() if v.dtype == torch.float32)
    assert total == _lib.lib().pnpx_policy_num_params(case[0], case[1], int(case[2]))
    # the integer buffers exist in the module and are not part of the vector
    assert sum(k.endswith("num_batches_tracked") for k in m.state_dict()) == 21
    from tfpnp_amd.utils.misc import gather_actor_state
    named = gather_actor_state(m.state_dict(keep_vars=True), *case)
    assert [k for k, _ in named] == [k for k, _ in specs]
    # the native actor of the case has this head
    actor = A.native_actor(case)
    assert actor.state_dict() == {} and actor.device is None


def test_gather_rejects_missing_key_and_changed_shape():
    from tfpnp_amd.utils.misc import gather_actor_state, hard_update
    target = A.native_actor((9, 10, False))
    m = A.stand_in_actor(9, 10, False)
    sd = m.state_dict(keep_vars=True)
    del sd["actor_encoder.layer3.1.bn2.running_mean"]
    with pytest.raises(PnpxError, match=r"actor_encoder\.layer3\.1\.bn2\.running_mean"):
        gather_actor_state(sd, 9, 10, False)
    m.actor_encoder.layer2[0].shortcut[0] = torch.nn.Conv2d(64, 128, 3, 2, 1, bias=False)        # a 3x3 shortcut
    with pytest.raises(PnpxError, match=r"layer2\.0\.shortcut\.0\.weight.*\(128, 64, 3, 3\).*\(128, 64, 1, 1\)"):
        hard_update(target, m)
    with pytest.raises(PnpxError, match=r"actor_encoder\.conv1\.weight.*\(64, 17, 3, 3\)"):
        hard_update(target, A.stand_in_actor(17, 10, False))                                    # another num_inputs
    with pytest.raises(PnpxError, match=r"fc_deterministic\.0\.weight.*\(10, 512\).*\(64, 512\)"):
        hard_update(A.native_actor((6, 10, True)), A.stand_in_actor(6, 10, False))              # not the SPI head
    no_bn = A.stand_in_actor(9, 10, False)
    no_bn.actor_encoder.bn1 = torch.nn.Identity()
    with pytest.raises(PnpxError, match=r"actor_encoder\.bn1\.weight"):
        hard_update(target, no_bn)


def test_updates_refuse_cpu_and_non_fp32_sources():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    from tfpnp_amd.utils.misc import hard_update, soft_update
    target = A.native_actor((9, 10, False))
    source = A.stand_in_actor(9, 10, False)
    with pytest.raises(PnpxError, match=r"actor_encoder\.conv1\.weight.*is on cpu"):
        hard_update(target, source)
    with pytest.raises(PnpxError, match="cpu"):
        target.load_flat_(torch.zeros(8))
    with pytest.raises(PnpxError, match="torch.Tensor"):
        target.load_flat_([0.0])
    with pytest.raises(PnpxError, match=r"actor_encoder\.conv1\.weight.*float64.*float32"):
        hard_update(target, A.stand_in_actor(9, 10, False).double())                            # dtype comes before the device
    # soft_update onto an actor is refused whatever the source
    for src in (source, A.native_actor((9, 10, False))):
        with pytest.raises(PnpxError, match="soft_update onto a native actor is not implemented"):
            soft_update(target, src, 0.001)
    # an unsupported target keeps the critic's message
    with pytest.raises(PnpxError, match="native ResNet_wobn"):
        hard_update(source, source)
    # two native actors that never saw a device: nothing to copy from; mismatched heads
    with pytest.raises(PnpxError, match="device"):
        hard_update(target, A.native_actor((9, 10, False)))
    with pytest.raises(PnpxError, match="actor mismatch"):
        hard_update(target, A.native_actor((17, 15, False)))
    # a critic is no actor source
    with pytest.raises(PnpxError, match=r"actor_encoder\.conv1\.weight"):
        hard_update(target, ResNet_wobn(9, 18, 1))
    assert target.state_dict() == {} and target.device is None

