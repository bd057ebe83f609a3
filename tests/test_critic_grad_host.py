"""Host-side checks of the critic's parameter gradients (no GPU): the fp64 leaf restatement of tests/critic_grad_cases.py
against the executed reference's autograd (tests/golden/critic_param_grad.npz, tools/make_critic_grad_golden.py), the C ABI /
binding surface, and the fixture itself."""
import os
import re

import numpy as np
import pytest
import torch

from tests import critic_cases as K
from tests import critic_grad_cases as G
from tests.golden_inputs import sha
from tfpnp_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "critic_param_grad.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", G.GOLDEN_CASES)
def test_leaf_restatement_reproduces_the_reference(gold, name):
    """The fp64 leaf restatement against the reference's fp32 autograd: per tensor <= 3e-4 (on the stored sample and on the
    norm), whole vector (all samples) <= 1e-5 -- ten times the reference arithmetic's own fp32-vs-fp64 difference, measured
    with the restatement on the CPU: worst tensor 3.2e-5 (layer3.1.relu_2.alpha, kf9), whole vector 5.8e-7 .. 8.0e-7 over the
    four cases.  No tensor of any case has a zero or negligible gradient, so none is left out.  Sums: a difference d with
    ||d|| <= 3e-4 ||ref|| moves the sum of n entries by at most sqrt(n) ||d||."""
    C = K.CASES[name][0]
    ob, w = K.case_inputs(name, gold[f"{name}_try"])
    _, ref = G.leaf_grads(K.critic_params(C), ob, w, torch.float64)
    keys = [k for k, _ in synth.critic_param_specs(C)]
    assert len(keys) == 82 and gold[f"{name}_norm"].shape == (82,)
    norms = gold[f"{name}_norm"]
    assert norms.min() > 1e-6 * norms.max()          # nothing negligible: every tensor is held to its own norm
    got, want, pos = {}, {}, 0
    for i, k in enumerate(keys):
        idx = G.sample_index(ref[k].size)
        got[k] = ref[k].reshape(-1)[idx]
        want[k] = gold[f"{name}_sample"][pos:pos + idx.size].astype(np.float64)
        pos += idx.size
        n = float(np.linalg.norm(ref[k]))
        assert abs(n - norms[i]) <= 3e-4 * norms[i], (k, n, norms[i])
        assert abs(float(ref[k].sum()) - gold[f"{name}_sum"][i]) <= 3e-4 * norms[i] * np.sqrt(ref[k].size), k
    assert pos == gold[f"{name}_sample"].size
    rel = G.per_tensor_rel(got, want)
    whole = np.linalg.norm(np.concatenate([got[k] - want[k] for k in keys])) / np.linalg.norm(np.concatenate([want[k] for k in keys]))
    print(f"{name}: worst tensor {G.worst(rel)}  whole vector {whole:.2e}")
    assert max(rel.values()) <= 3e-4
    assert whole <= 1e-5


def test_new_symbol_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    name = "pnpx_critic_param_grad"
    assert re.search(r"\b" + name + r"\s*\(", header)
    assert "trainer.py:198,207" in header
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    from tfpnp_amd import ops, torch_ops
    assert "critic_param_grad" in torch_ops.ALL_OPS and callable(ops.critic_param_grad)
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    net = ResNet_wobn(9, 18, 1)
    with pytest.raises(_lib.PnpxError):
        net.param_grad(torch.zeros(1, 9, 32, 32), torch.ones(1))      # CPU tensors: no CPU path, as forward


def test_fixture_is_small_holds_results_only_and_matches_the_generators(gold):
    assert os.path.getsize(GOLDEN) < 1 << 20 and sum(gold[k].nbytes for k in gold.files) < 1 << 20
    assert not any("weight" in k or "param" in k for k in gold.files)
    value = np.load(os.path.join(ROOT, "tests", "golden", "critic_value.npz"))
    for name in G.GOLDEN_CASES:
        assert int(gold[f"{name}_try"]) == int(value[f"{name}_try"])
        assert np.array_equal(sha(*K.case_inputs(name, gold[f"{name}_try"])), gold[f"{name}_in_sha"]), name
        assert np.array_equal(gold[f"{name}_in_sha"], value[f"{name}_in_sha"])
        C = K.CASES[name][0]
        assert gold[f"{name}_sample"].size == sum(G.sample_index(int(np.prod(s))).size for _, s in synth.critic_param_specs(C))


def test_sample_index_is_a_fixed_stride_of_at_most_1024():
    for n in (1, 64, 1024, 1025, 5184, 2359296):
        idx = G.sample_index(n)
        assert idx[0] == 0 and idx[-1] < n and idx.size <= G.SAMPLE_MAX and (idx.size == n or idx.size > G.SAMPLE_MAX // 2)
