"""Host-side checks of the value network (no GPU): the golden from the executed reference critic
(tests/golden/critic_value.npz, tools/make_critic_golden.py) against the plain restatement of tests/critic_cases.py, the
input generators, the C ABI / binding surface, the parameter layout and the unchanged CPU observation path."""
import os
import re

import numpy as np
import pytest
import torch

from tests import critic_cases as K
from tests.golden_inputs import KINK_MARGIN, sha
from tfpnp_amd import _lib, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pnpx_critic_num_params", "pnpx_critic_load", "pnpx_critic_forward", "pnpx_critic_backward",
               "pnpx_policy_ob_unpack")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "critic_value.npz"))


@pytest.mark.parametrize("name", ["kf9", "kf17", "arb", "rect"])
def test_restatement_reproduces_the_reference(gold, name):
    """fp32 and fp64 restatement against the reference's fp32 run.  V: 2e-5 * max(1, |V|) (ten times the reference's own
    fp32-vs-fp64 difference); gradient: 1e-4 relative L2 on the kink-free cases (the project's bound for fp32 arithmetic),
    the kink-flip bound 2e-2 on the arbitrary one."""
    ob, w = K.case_inputs(name, gold[f"{name}_try"])
    params = K.critic_params(K.CASES[name][0])
    for dtype in (torch.float32, torch.float64):
        V, g, margin = K.restate_value_and_grad(params, ob, w, dtype)
        ref = gold[f"{name}_V"].astype(np.float64)
        err = np.abs(V - ref).max()
        print(f"{name} {dtype}: |dV| {err:.2e}  margin {margin:.2e}")
        assert np.all(np.abs(V - ref) <= 2e-5 * np.maximum(1.0, np.abs(ref)))
        if name != "rect":
            rel = K.rel_l2(g, gold[f"{name}_grad"])
            print(f"{name} {dtype}: gradient rel-L2 {rel:.2e}")
            assert rel < (1e-4 if name.startswith("kf") else 2e-2)
        if name.startswith("kf") and dtype == torch.float64:
            assert margin > KINK_MARGIN and float(gold[f"{name}_margin"]) > KINK_MARGIN


def test_arb_case_is_far_from_the_kink_flip_bound(gold):
    assert float(gold["arb_ref_dgrad"]) <= K.ARB_MAX_REF_DIFF


def test_input_generators_reproduce_the_stored_hashes(gold):
    from tests.golden_inputs import GRAD_CASE as C
    for name in K.CASES:
        assert np.array_equal(sha(*K.case_inputs(name, gold[f"{name}_try"])), gold[f"{name}_in_sha"]), name
    d = synth.make_csmri_batch(C.env_B, C.env_H, C.env_W, seed=C.env_data_seed)
    raw = np.random.RandomState(C.env_raw_seed).standard_normal((C.env_B, 10)).astype(np.float32)
    assert np.array_equal(sha(d["y0"], d["mask"], d["x0"], raw), gold["ddpg_in_sha"])
    assert int(gold["critic_weight_seed"]) == K.CRITIC_WEIGHT_SEED and float(gold["ddpg_discount"]) == K.DISCOUNT


def test_golden_holds_no_weights(gold):
    assert sum(gold[k].nbytes for k in gold.files) < 1 << 20
    assert not any("weight" in k and k != "critic_weight_seed" for k in gold.files)


def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pnpx.h")).read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.pnpx_critic_num_params(9) == sum(int(np.prod(s)) for _, s in synth.critic_param_specs(9)) == 11177042
    assert lib.pnpx_critic_num_params(0) == 0 and lib.pnpx_critic_num_params(65) == 0
    from tfpnp_amd import torch_ops
    for op in ("critic_value", "critic_backward", "policy_ob_pack_diff", "policy_ob_unpack"):
        assert op in torch_ops.ALL_OPS


@pytest.mark.parametrize("num_inputs", [9, 17])
def test_param_specs_match_a_weight_norm_module(num_inputs):
    sd = K.stand_in_module(num_inputs).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in synth.critic_param_specs(num_inputs)]
    assert len(sd) == 82


def test_flat_params_accept_both_weight_norm_spellings():
    params = synth.make_critic_params(9, 3)
    flat = ops.critic_flat_params(params, 9)
    assert flat.dtype == np.float32 and flat.size == 11177042
    renamed = {}
    for k, v in params.items():
        k = k.replace(".weight_g", ".parametrizations.weight.original0").replace(".weight_v", ".parametrizations.weight.original1")
        renamed[k] = torch.from_numpy(v)
    assert np.array_equal(ops.critic_flat_params(renamed, 9), flat)
    missing = dict(params)
    del missing["layer2.0.shortcut.0.weight_v"]
    with pytest.raises(_lib.PnpxError, match="layer2.0.shortcut.0.weight_v"):
        ops.critic_flat_params(missing, 9)
    bad = dict(params)
    bad["fc.weight"] = np.zeros((2, 512), np.float32)
    with pytest.raises(_lib.PnpxError, match="fc.weight"):
        ops.critic_flat_params(bad, 9)


def test_make_critic_params_recipe():
    p = synth.make_critic_params(9, 0)
    alphas = np.array([v[0] for k, v in p.items() if k.endswith("alpha")])
    assert alphas.size == 17 and np.all(alphas != 0) and (alphas < 0).any() and (alphas > 0).any()
    g = p["layer1.0.conv1.weight_g"]
    assert g.min() >= 0.5 * np.sqrt(2) - 1e-6 and g.max() <= 1.5 * np.sqrt(2) + 1e-6
    # activations neither die nor blow up on uniform-random observations
    V = K.restate(p, np.random.RandomState(0).uniform(0, 1, (2, 9, 32, 32)).astype(np.float32), torch.float32)
    assert 0.1 < float(V.abs().max()) < 50


def test_critic_module_rejects_other_shapes():
    from tfpnp_amd.trainer.mddpg.critic import ResNet_wobn
    with pytest.raises(NotImplementedError):
        ResNet_wobn(9, 34, 1)
    with pytest.raises(NotImplementedError):
        ResNet_wobn(9, 18, 2)
    net = ResNet_wobn(9, 18, 1)
    with pytest.raises(_lib.PnpxError):
        net(torch.zeros(1, 9, 32, 32))


def test_cpu_policy_ob_keeps_the_cat_graph():
    from tfpnp_amd.data.batch import Batch
    from tfpnp_amd.tasks import csmri
    env = csmri.CSMRIEnv(None, None, max_episode_step=6)
    B, H, W = 2, 8, 8
    cplx = lambda c: torch.randn(B, c, H, W, 2)
    ob = Batch(variables=cplx(3).requires_grad_(True), y0=cplx(1), ATy0=cplx(1), mask=torch.ones(B, 1, H, W),
               T=torch.zeros(B, 1, H, W), sigma_n=cplx(1))
    out = env.get_eval_ob(ob)
    assert out.requires_grad and type(out.grad_fn).__name__ == "CatBackward0"
    assert out.shape[1] == 9
