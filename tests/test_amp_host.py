"""CPU-only checks of the CS-MRI AMP solver: the C-ABI entry, a float64 restatement of the loop pinned to the golden the
real reference produced (tests/golden/csmri_amp_B2_64x64.npz, tools/make_amp_golden.py), and the solver's wiring."""
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

AMP_B, AMP_H, AMP_W, AMP_DATA_SEED = 2, 64, 64, 91      # tools/make_amp_golden.py


def amp_restated(den, variables, y0, mask, sigma_d, probe, iter_num=None):
    """AMPSolver_CSMRI.forward (tasks/csmri/solver.py:211-250) with prox_fun = the denoiser prox and complex_norm = the
    per-item L2 norm, written on the oracle's denoiser and centered FFTs.  Runs in the dtype of its inputs (float64 for the
    yardstick); eps = max(r) / 1000 + 1e-8 over the whole batch."""
    x, z = torch.split(variables, variables.shape[1] // 2, dim=1)
    B, _, H, W, _ = x.shape
    T = sigma_d.shape[-1] if iter_num is None else iter_num
    m = mask.bool().unsqueeze(-1)
    M = mask.reshape(B, -1).sum(dim=-1).to(x.dtype).view(B, 1, 1, 1, 1)
    sqrt_n = torch.sqrt(torch.tensor(float(H * W), dtype=x.dtype))
    for i in range(T):
        r = O.complex2real(x + O.ifft2c(z))
        s = torch.sqrt((z * z).reshape(B, -1).sum(dim=-1)) / sqrt_n * sigma_d[:, i]
        xr = den(r, s)
        eps = r.max() / 1000 + 1e-8
        d = probe[i].to(x.dtype)
        div = (d * (den(r + d * eps, s) - xr)).reshape(B, -1).sum(dim=-1) / eps
        o = z * div.view(B, 1, 1, 1, 1) / M
        x = O.real2complex(xr)
        z = torch.where(m, y0 - O.fft2c(x), torch.zeros_like(y0)) + o
    return torch.cat([x, z], dim=1)


def amp_case():
    """(inputs, golden) of the fixture; the inputs are rebuilt from seeds and checked against the stored sha."""
    gold = golden("csmri_amp_B2_64x64")
    d = synth.make_csmri_batch(AMP_B, AMP_H, AMP_W, ratio=4, sigma_n=15, seed=AMP_DATA_SEED)
    assert np.array_equal(sha(d["y0"], d["mask"], d["x0"]), gold["in_sha"]), "input generator drifted"
    return d, gold


def amp_reset(y0):
    """AMPSolver.reset: cat([0, y0])"""
    return torch.cat([torch.zeros_like(y0), y0], dim=1)


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def test_header_declares_and_library_exports_amp():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pnpx_csmri_amp\s*\(", src)
    from tfpnp_amd import _lib
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pnpx_csmri_amp")
    assert "pnpx_csmri_amp" in _lib.EXPORTED_SYMBOLS


def test_float64_restatement_reproduces_reference_golden():
    d, gold = amp_case()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    den = O.Denoiser(synth.make_unet_params(WEIGHT_SEED), dtype=torch.float64)
    v0 = amp_reset(t(d["y0"]))
    probe = t(gold["probe"])
    with torch.no_grad():
        for T, key in ((1, "out_T1"), (5, "out_T5")):
            out = amp_restated(den, v0, t(d["y0"]), torch.from_numpy(d["mask"]), t(gold["sigma_d"][:, :T]), probe)
            e = rel(out, gold[key])
            print(f"  T={T}: float64 restatement vs reference golden {e:.2e}")
            assert e <= 1e-5, key


def test_solver_wiring_without_gpu():
    from tfpnp_amd.pnp.solver.base import PnPSolver
    from tfpnp_amd.tasks.csmri import AMPSolver_CSMRI, _solver_map

    class Den:
        pass

    sol = AMPSolver_CSMRI(Den())
    assert _solver_map["amp"] is AMPSolver_CSMRI
    assert sol.num_var == 2
    sd = torch.rand(3, 4)
    assert sol.filter_hyperparameter({"sigma_d": sd, "mu": torch.rand(3, 4)}) is sd
    y0 = torch.randn(3, 1, 8, 8, 2)
    v = sol.reset({"y0": y0, "x0": torch.randn(3, 1, 8, 8, 2)})
    assert torch.equal(v[:, 0], torch.zeros_like(y0[:, 0])) and torch.equal(v[:, 1], y0[:, 0])
    mask = torch.ones(3, 1, 8, 8, dtype=torch.bool)
    for bad in (torch.randn(4, 3, 8, 8), torch.randn(3, 3, 1, 8, 8), torch.randn(4, 2, 1, 8, 8),
                torch.randn(4, 3, 1, 8, 4)):
        with pytest.raises(ValueError, match="probe"):
            sol((v, (y0, mask)), sd, probe=bad)
    with pytest.raises(NotImplementedError, match="native denoiser"):     # a denoiser without a native context
        sol((v, (y0, mask)), sd, probe=torch.randn(4, 3, 1, 8, 8))
    assert PnPSolver.prox_mapping is AMPSolver_CSMRI.prox_mapping
