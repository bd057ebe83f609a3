"""CPU-only checks of the phase-retrieval proximal-gradient solver: a restatement of the loop on the oracle's functions pinned
to the golden that a chain of real reference calls produced (tests/golden/pr_pg_B2_64x64.npz, tools/make_pr_pg_golden.py), the
C-ABI surface and the solver's wiring."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import pnp_oracle as O
from tests.conftest import ROOT, golden
from tests.golden_inputs import WEIGHT_SEED, sha
from tfpnp_amd import synth

PG_B, PG_H, PG_W, PG_S, PG_DATA_SEED = 2, 64, 64, 4, 77      # tools/make_pr_pg_golden.py
PG_SYMBOLS = ("pnpx_pr_pg", "pnpx_pr_pg_train", "pnpx_pr_pg_backward")


def pr_pg_restated(den, x, y0, mask, sigma_d, tau, iter_num=None, trace=None):
    """PGSolver_PR.forward: the loop of tasks/pr/solver.py:79-112 with the PR gradient step of :61-68.  Runs in the dtype of its
    inputs.  `trace`, a dict, receives the z of every iteration and the smallest |Ax| met."""
    B = x.shape[0]
    T = sigma_d.shape[-1] if iter_num is None else iter_num
    for i in range(T):
        Ax = O.cdp_forward(x, mask)
        y_hat = O.complex_abs(Ax)
        err = y_hat - y0
        r = torch.stack((err / y_hat * Ax[..., 0], err / y_hat * Ax[..., 1]), -1)
        z = x - tau[:, i].view(B, 1, 1, 1, 1) * O.cdp_backward(r, mask)
        x = O.real2complex(den(O.complex2real(z), sigma_d[:, i]))
        if trace is not None:
            trace.setdefault("z", []).append(z)
            trace["min_abs"] = min(trace.get("min_abs", float("inf")), float(y_hat.min()))
    return x


def pg_case():
    """(inputs, golden) of the fixture; the inputs are rebuilt from seeds and checked against the stored sha."""
    gold = golden("pr_pg_B2_64x64")
    d = synth.make_pr_batch(PG_B, PG_H, PG_W, S=PG_S, alpha=9.0, seed=PG_DATA_SEED)
    assert np.array_equal(sha(d["y0"], d["mask"], d["x0"]), gold["in_sha"]), "input generator drifted"
    return d, gold


def pg_grad_start(d, gold):
    """The complex start of the golden's gradient leg: x0 + 0.05 * randn in both parts."""
    v = np.stack([d["x0"], np.zeros_like(d["x0"])], axis=-1)
    return (v + 0.05 * np.random.RandomState(int(gold["grad_start_seed"])).standard_normal(v.shape)).astype(np.float32)


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("dtype,bound", [(torch.float32, 1e-5), (torch.float64, 1e-5)], ids=["f32", "f64"])
def test_restatement_reproduces_reference_golden(dtype, bound):
    d, gold = pg_case()
    c = lambda a: t(a).to(dtype)
    den = O.Denoiser(synth.make_unet_params(WEIGHT_SEED), dtype=dtype)
    x0 = O.real2complex(c(d["x0"]))
    with torch.no_grad():
        for T, key in ((1, "out_T1"), (5, "out_T5")):
            tr = {}
            out = pr_pg_restated(den, x0, c(d["y0"]), c(d["mask"]), c(gold["sigma_d"][:, :T]), c(gold["tau"][:, :T]), trace=tr)
            e = rel(out, gold[key])
            print(f"  {dtype} T={T}: restatement vs reference golden {e:.2e}  (min |Ax| {tr['min_abs']:.2e})")
            assert tr["min_abs"] > 0
            if dtype == torch.float32 or T == 5:
                assert e <= bound, key
            if dtype == torch.float32 and T == 1:
                ez = rel(tr["z"][0], gold["z_T1"])
                print(f"  {dtype}: z of the first step vs the reference's {ez:.2e}")
                assert ez <= bound
            assert torch.all(out[..., 1] == 0)


def test_header_binding_and_library_agree_on_the_three_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpx.h")).read(), flags=re.S)
    from tfpnp_amd import _lib, torch_ops
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in PG_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "pr_pg" in torch_ops.ALL_OPS
    for op in ("pr_pg", "pr_pg_train", "pr_pg_backward"):
        assert hasattr(torch.ops.pnpx, op), op


def test_solver_wiring_without_gpu():
    from tfpnp_amd._lib import PnpxError
    from tfpnp_amd.pnp.solver.base import PGSolver
    from tfpnp_amd.tasks import pr

    class Den:
        pass

    sol = pr.create_solver_pr(type("o", (), {"solver": "pg"})(), Den())
    assert type(sol) is pr.PGSolver_PR and isinstance(sol, PGSolver) and sol.num_var == 1
    x0 = torch.rand(3, 1, 8, 8)
    v = sol.reset({"x0": x0})
    assert tuple(v.shape) == (3, 1, 8, 8, 2) and torch.equal(v[..., 0], x0) and torch.all(v[..., 1] == 0)
    assert torch.equal(sol.get_output(v), x0)
    act = {"sigma_d": 1, "mu": 2, "tau": 3, "beta": 4}
    assert sol.filter_hyperparameter(act) == (1, 3)
    assert sol.filter_aux_inputs({"y0": "a", "mask": "b"}) == ("a", "b")
    inputs = (v, (torch.rand(3, 4, 8, 8), torch.rand(3, 4, 8, 8, 2)))
    hyper = (torch.rand(3, 2), torch.rand(3, 2))
    with pytest.raises(NotImplementedError, match="native denoiser"):        # a denoiser without a native context
        sol(inputs, hyper)

    class Overridden(pr.PGSolver_PR):
        def prox_mapping(self, x, sigma):
            return x

    with pytest.raises(NotImplementedError, match="overrides prox_mapping"):
        Overridden(Den())(inputs, hyper)

    class Native:                                   # gets past _ctx: the forward reaches the op, which has no CPU path
        def context(self, device):
            return type("c", (), {"cid": 0})()

    with pytest.raises(PnpxError, match="no CPU path"):
        pr.PGSolver_PR(Native())(inputs, hyper)
