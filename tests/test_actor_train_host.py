"""Host-side checks of the actor's train-mode forward (no GPU): the torch stand-in in `.train()` mode against the golden of the
real reference actor (tools/make_actor_train_golden.py), the C ABI / binding surface, the fake-tensor shapes of the new operator
and the opt-in default of `bn_follows_mode`."""
import inspect
import os
import re

import numpy as np
import torch

from tests import actor_cases as A
from tests import actor_train_cases as T
from tests.conftest import golden
from tfpnp_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pnpx_policy_forward_train", "pnpx_policy_num_bn_channels", "pnpx_policy_bn_stats")


def test_stand_in_reproduces_the_reference_train_golden():
    """Both are fp32 torch on the CPU: outputs and running statistics of two train-mode forwards agree to 1e-6."""
    gd = golden("policy_actor_train")
    case, shape = T.CASES[1]
    assert case == (7, 10, False) and (shape[0], case[0]) + shape[1:] == tuple(gd["shape"])
    assert int(gd["weight_seed"]) == T.WEIGHT_SEED and int(gd["ob_seed"]) == T.OB_SEED
    m = A.load_params(A.stand_in_actor(*case), T.params(case))
    ob = torch.from_numpy(T.observation(case, shape))
    idx_stop = torch.from_numpy(gd["idx_stop"]).view(-1, 1)
    for it in (1, 2):
        probs, det, _, _ = T.train_forward(m, ob)
        dist = torch.distributions.Categorical(probs)
        got = {"probs": probs, "det": det, "logp": dist.log_prob(idx_stop[:, 0]).unsqueeze(1), "entropy": dist.entropy().unsqueeze(1),
               "running": T.running_of(m)}
        for k, v in got.items():
            err = float(np.abs(v.numpy() - gd[f"{k}{it}"]).max())
            print(f"forward {it} {k}: max |stand-in - reference| {err:.2e}")
            assert err <= 1e-6, (it, k, err)
    assert not np.array_equal(gd["running1"], gd["running2"])


def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    from tfpnp_amd import ops
    assert callable(ops.policy_forward_train) and callable(ops.policy_bn_stats)


def test_num_bn_channels():
    n = int(_lib.lib().pnpx_policy_num_bn_channels())
    assert n == T.N_BN == 4864
    for case in A.CASES:
        assert n == sum(int(np.prod(s)) for k, s in synth.policy_param_specs(*case) if k.endswith("running_mean"))
        assert sum(cnt for _, cnt in T.stat_slices(case)) == 2 * n


def test_fake_tensor_shapes_and_registration():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tfpnp_amd import ops, torch_ops

    class Stub:          # the fake formula reads the head of the context only
        _policy = (9, 10, False)

    assert "policy_forward_train" in torch_ops.ALL_OPS and hasattr(torch.ops.pnpx, "policy_forward_train")
    schema = str(torch.ops.pnpx.policy_forward_train.default._schema)
    assert "Tensor ob" in schema and "Tensor(a" not in schema          # mutates the context, none of its tensor arguments
    stub = Stub()
    cid = 1 << 40
    ops._ctx_by_id[cid] = stub
    try:
        with FakeTensorMode():
            ob = torch.empty(3, 9, 64, 32)
            probs, det = torch.ops.pnpx.policy_forward_train(ob, 0.1, True, cid)
            assert probs.shape == (3, 2) and det.shape == (3, 10) and probs.dtype == det.dtype == torch.float32
    finally:
        del ops._ctx_by_id[cid]


def test_bn_follows_mode_is_opt_in():
    from tfpnp_amd import policy
    for name in ("ResNetActor_ADMM", "ResNetActor_HQS", "ResNetActor_PG", "ResNetActor_APG", "ResNetActor_RED", "ResNetActor_IADMM",
                 "ResNetActor_AMP", "ResNetActor_SPI"):
        cls = getattr(policy, name)
        assert inspect.signature(cls.__init__).parameters["bn_follows_mode"].default is False, name
        assert cls(3, 5).bn_follows_mode is False and cls(3, 5, bn_follows_mode=True).bn_follows_mode is True
    assert policy.ResNetActor_ADMM(6, 5).training          # an nn.Module trains by default: hence the opt-in
