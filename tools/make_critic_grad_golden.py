"""Writes tests/golden/critic_param_grad.npz from the EXECUTED reference critic's own autograd
(tfpnp/trainer/mddpg/critic.py, loaded by file path as tools/make_critic_golden.py does).  Build machine only: it needs the
reference checkout and never runs on a GPU box.

    python tools/make_critic_grad_golden.py

For the cases kf9, kf17, arb and rect of tests/critic_cases.py, at the tries frozen in tests/golden/critic_value.npz and with
the same weights w of the scalar sum(V * w), the reference runs in fp32 and the file stores, per parameter tensor in
state_dict order: the L2 norm and the sum of d sum(V * w) / d tensor (float64 accumulations of the fp32 gradient) and the
fixed strided sample of at most 1024 entries (tests/critic_grad_cases.py::sample_index).  Plus the input hashes and the
reference's own fp32-vs-fp64 difference per case.  Results only: no weights."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import critic_cases as K  # noqa: E402
from tests import critic_grad_cases as G  # noqa: E402
from tests.golden_inputs import sha  # noqa: E402
from tools.make_critic_golden import build, load_reference_critic, t  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "critic_param_grad.npz")


def run(net, ob, w, dtype):
    """{state_dict key: d sum(V * w) / d parameter} of the reference in `dtype`, as float64 arrays"""
    net.zero_grad()
    V = net(t(ob).to(dtype))
    (V[:, 0] * t(w).to(dtype)).sum().backward()
    named = dict(net.named_parameters())
    return {k: named[k].grad.detach().double().numpy().copy() for k in net.state_dict()}


def main():
    assert ref_shim.available(), "reference not mounted"
    ref_shim.install()
    torch.set_num_threads(8)
    mod = load_reference_critic()
    value = np.load(os.path.join(ROOT, "tests", "golden", "critic_value.npz"))
    res, nets = {}, {}
    for name in G.GOLDEN_CASES:
        C = K.CASES[name][0]
        if C not in nets:
            nets[C] = (build(mod, C, torch.float32).train(), build(mod, C, torch.float64).train())
        k = int(value[f"{name}_try"])
        ob, w = K.case_inputs(name, k)
        assert np.array_equal(sha(ob, w), value[f"{name}_in_sha"]), name
        g32, g64 = run(nets[C][0], ob, w, torch.float32), run(nets[C][1], ob, w, torch.float64)
        keys = list(g32)
        rel = G.per_tensor_rel(g32, g64)
        print(f"{name} try {k}: reference fp32-vs-fp64 worst per tensor {G.worst(rel)}  whole vector {G.whole_rel(g32, g64, C):.2e}", flush=True)
        res[f"{name}_try"] = np.int64(k)
        res[f"{name}_in_sha"] = sha(ob, w)
        res[f"{name}_norm"] = np.array([np.linalg.norm(g32[q]) for q in keys], np.float64)
        res[f"{name}_sum"] = np.array([g32[q].sum() for q in keys], np.float64)
        res[f"{name}_sample"] = np.concatenate([g32[q].reshape(-1)[G.sample_index(g32[q].size)] for q in keys]).astype(np.float32)
        res[f"{name}_ref_worst_tensor"] = np.float64(G.worst(rel)[1])
        res[f"{name}_ref_whole"] = np.float64(G.whole_rel(g32, g64, C))
    np.savez_compressed(OUT, **res)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KB)")


if __name__ == "__main__":
    main()
