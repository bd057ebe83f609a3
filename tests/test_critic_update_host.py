"""Host-side checks of the critic's live-weight entries (no GPU): the C ABI / binding surface, the parameter-order check of
utils.misc against a weight-normalised module in both spellings, and the refusal of CPU sources."""
import os
import re

import pytest
import torch

from tests import critic_cases as K
from tfpnp_amd import _lib
from tfpnp_amd._lib import PnpxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pnpx_critic_load_device", "pnpx_critic_soft_update", "pnpx_critic_params")


def _stand_in(num_inputs, spelling):
    """K.stand_in_module with torch.nn.utils.weight_norm (weight_g / weight_v) or with the parametrization that current
    PyTorch offers in its place (parametrizations.weight.original0 / original1)."""
    if spelling == "weight_g":
        return K.stand_in_module(num_inputs)
    old = torch.nn.utils.weight_norm
    torch.nn.utils.weight_norm = torch.nn.utils.parametrizations.weight_norm
    try:
        return K.stand_in_module(num_inputs)
    finally:
        torch.nn.utils.weight_norm = old


def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    from tfpnp_amd import ops
    for name in ("load_critic_device", "critic_soft_update", "critic_params"):
        assert callable(getattr(ops.Context, name)), name


@pytest.mark.parametrize("spelling", ["weight_g", "original0"])
@pytest.mark.parametrize("num_inputs", [1, 9, 17])
def test_param_order_check_accepts_both_spellings(num_inputs, spelling):
    from tfpnp_amd.utils.misc import check_param_order
    m = _stand_in(num_inputs, spelling)
    names = [n for n, _ in m.named_parameters()]
    assert any(spelling in n for n in names), names[:3]
    check_param_order(list(m.parameters()), num_inputs)
    assert sum(p.numel() for p in m.parameters()) == _lib.lib().pnpx_critic_num_params(num_inputs)


def test_param_order_check_rejects_a_changed_shape():
    from tfpnp_amd.utils.misc import check_param_order
    m = K.stand_in_module(9)
    m.layer2[0].shortcut[0] = torch.nn.utils.weight_norm(torch.nn.Conv2d(64, 128, 3, 2, 1, bias=True))   # a 3x3 shortcut
    with pytest.raises(PnpxError, match=r"layer2\.0\.shortcut\.0\.weight_v.*\(128, 64, 1, 1\)"):
        check_param_order(list(m.parameters()), 9)
    with pytest.raises(PnpxError, match="num_inputs"):
        check_param_order(list(K.stand_in_module(17).parameters()), 9)
    short = K.stand_in_module(9)
    del short.layer3[1].relu_2
    with pytest.raises(PnpxError, match="81 parameter tensors"):
        check_param_order(list(short.parameters()), 9)


def test_updates_refuse_cpu_sources():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    from tfpnp_amd.utils.misc import hard_update, soft_update
    target = ResNet_wobn(9, 18, 1)
    source = K.stand_in_module(9)
    with pytest.raises(PnpxError, match="source module is on cpu"):
        hard_update(target, source)
    with pytest.raises(PnpxError, match="source module is on cpu"):
        soft_update(target, source, 0.001)
    with pytest.raises(PnpxError, match="cpu"):
        target.load_flat_(torch.zeros(11177042))
    with pytest.raises(PnpxError, match="native ResNet_wobn"):
        hard_update(source, source)
    # two native critics that never saw a device: nothing to copy from
    with pytest.raises(PnpxError, match="device"):
        hard_update(target, ResNet_wobn(9, 18, 1))
    assert target.state_dict() == {} and target.device is None
