"""CS-MRI solvers on MI355X -- drop-in for tasks/csmri/solver.py (same class names / call surface).

solver(inputs, parameters, iter_num=None) with inputs = (variables, (y0, mask)), parameters the tuple from
filter_hyperparameter(action); returns the next state tensor.  Each forward is ONE native call that runs all
iter_num inner iterations (denoiser prox + masked-FFT data prox + dual update) on the caller's stream.
"""
import torch

from .. import autograd as A
from .. import torch_ops as T
from ..env.base import PnPEnv
from ..pnp.solver.base import ADMMSolver, HQSSolver, PGSolver, APGSolver, REDADMMSolver, AMPSolver
from ..utils import transforms


class CSMRIMixin:
    """tasks/csmri/solver.py:15-21"""

    def get_output(self, state):
        return transforms.complex2real(super().get_output(state))

    def filter_aux_inputs(self, state):
        return (state['y0'], state['mask'])


class ADMMSolver_CSMRI(CSMRIMixin, ADMMSolver):
    """tasks/csmri/solver.py:24-57"""

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, mask) = inputs
        sigma_d, mu = parameters
        if A.needs_grad(variables, sigma_d, mu):      # training path: native forward + native VJP (csmri.hip)
            return T.call("csmri_admm_train", variables, y0, mask, sigma_d, mu, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("csmri_admm", variables, y0, mask, sigma_d, mu, -1 if iter_num is None else iter_num, self._ctx(variables).cid)

class HQSSolver_CSMRI(CSMRIMixin, HQSSolver):
    """tasks/csmri/solver.py:60-89"""

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, mask) = inputs
        sigma_d, mu = parameters
        if A.needs_grad(variables, sigma_d, mu):      # training path: native forward + fused native VJP (csmri.hip)
            return T.call("csmri_hqs_train", variables, y0, mask, sigma_d, mu, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("csmri_hqs", variables, y0, mask, sigma_d, mu, -1 if iter_num is None else iter_num, self._ctx(variables).cid)

class PGSolver_CSMRI(CSMRIMixin, PGSolver):
    """tasks/csmri/solver.py:92-120"""

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, mask) = inputs
        sigma_d, tau = parameters
        if A.needs_grad(variables, sigma_d, tau):      # training path: native forward + fused native VJP (csmri.hip)
            return T.call("csmri_pg_train", variables, y0, mask, sigma_d, tau, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("csmri_pg", variables, y0, mask, sigma_d, tau, -1 if iter_num is None else iter_num, self._ctx(variables).cid)

class APGSolver_CSMRI(CSMRIMixin, APGSolver):
    """tasks/csmri/solver.py:123-165"""

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, mask) = inputs
        sigma_d, tau, beta = parameters
        if A.needs_grad(variables, sigma_d, tau, beta):      # training path: native forward + fused native VJP (csmri.hip)
            return T.call("csmri_apg_train", variables, y0, mask, sigma_d, tau, beta, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("csmri_apg", variables, y0, mask, sigma_d, tau, beta, -1 if iter_num is None else iter_num, self._ctx(variables).cid)

class REDADMMSolver_CSMRI(CSMRIMixin, REDADMMSolver):
    """tasks/csmri/solver.py:168-204"""

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, mask) = inputs
        sigma_d, mu, lamda = parameters
        if A.needs_grad(variables, sigma_d, mu, lamda):      # training path: native forward + fused native VJP (csmri.hip)
            return T.call("csmri_redadmm_train", variables, y0, mask, sigma_d, mu, lamda,
                          -1 if iter_num is None else iter_num, self._ctx(variables).cid)[0]
        return T.call("csmri_redadmm", variables, y0, mask, sigma_d, mu, lamda, -1 if iter_num is None else iter_num, self._ctx(variables).cid)

class AMPSolver_CSMRI(CSMRIMixin, AMPSolver):
    """tasks/csmri/solver.py:207-250.  The reference's loop calls two names that do not exist; they are supplied as
        self.prox_fun (:238)            = self.prox_mapping: the context's native denoiser (UNet, or DRUNet when loaded)
        transforms.complex_norm(z) (:230) = per item sqrt(sum of z[b]^2 over its [1,H,W,2] entries), shape [B]
    and otherwise the loop runs in the reference's operation order, per iteration i with N = H*W, M[b] = mask count:
        r = Re(x + ifft2(z));  s = ||z|| / sqrt(N) * sigma_d[:, i];  x = r2c(D(r, s))
        eps = max(r) / 1000 + 1e-8;  div = sum(delta_i * (D(r + eps delta_i, s) - Re x)) / eps
        z = (y0 - fft2(x))[mask] (0 elsewhere) + z * div / M
    eps is ONE scalar over all items of the call (the reference's r.max()): under PnPEnv, over the rows still running, so
    an item's result depends on the other items of the call.  The Monte-Carlo probe delta (the reference's
    torch.randn_like(r) at :235) is an input: forward(..., probe=[T,B,1,H,W]); when it is None the class draws it with
    torch.randn on the state's device (governed by the caller's torch.manual_seed).  Given the probe, a call is bitwise
    deterministic.  Inference is one native call (pnpx_csmri_amp: both denoiser evaluations of an iteration as one 2B-item
    denoiser call); under autograd the same loop is composed from the differentiable native blocks (tfpnp_amd.autograd)."""

    def forward(self, inputs, parameters, iter_num=None, *, probe=None):
        variables, (y0, mask) = inputs
        sigma_d = parameters[0] if isinstance(parameters, (tuple, list)) else parameters
        T_ = sigma_d.shape[-1] if iter_num is None else iter_num
        B, _, H, W, _ = variables.shape
        if probe is None:
            probe = torch.randn(T_, B, 1, H, W, device=variables.device)
        elif probe.dim() != 5 or probe.shape[0] < T_ or tuple(probe.shape[1:]) != (B, 1, H, W):
            raise ValueError(f'AMPSolver_CSMRI: probe must be [{T_}, {B}, 1, {H}, {W}], got {tuple(probe.shape)}')
        ctx = self._ctx(variables)
        if A.needs_grad(variables, sigma_d):      # training path: the same loop from differentiable native blocks
            return self._forward_autograd(ctx, variables, y0, mask, sigma_d, probe, T_)
        return T.call("csmri_amp", variables, y0, mask, sigma_d, probe, -1 if iter_num is None else iter_num, ctx.cid)

    @staticmethod
    def _forward_autograd(ctx, variables, y0, mask, sigma_d, probe, iter_num):
        x, z = torch.split(variables, variables.shape[1] // 2, dim=1)
        B, _, H, W, _ = x.shape
        m = (mask != 0).unsqueeze(-1)
        M = mask.reshape(B, -1).sum(dim=-1).float().view(B, 1, 1, 1, 1)
        sqrt_n = torch.sqrt(torch.tensor(float(H * W), device=x.device))
        for i in range(iter_num):
            r = A.c2r(x + A.fft2(z, inverse=True))
            s = torch.sqrt((z * z).reshape(B, -1).sum(dim=-1)) / sqrt_n * sigma_d[:, i]
            eps = r.max() / 1000 + 1e-8
            dn = A.denoise(ctx, torch.cat([r, r + probe[i] * eps]), torch.cat([s, s]))
            x = A.r2c(dn[:B])
            div = (probe[i] * (dn[B:] - dn[:B])).reshape(B, -1).sum(dim=-1) / eps
            o = z * div.view(B, 1, 1, 1, 1) / M
            z = torch.where(m, y0 - A.fft2(x), torch.zeros_like(y0)) + o
        return torch.cat([x, z], dim=1)


_solver_map = {
    'admm': ADMMSolver_CSMRI,
    'hqs': HQSSolver_CSMRI,
    'pg': PGSolver_CSMRI,
    'apg': APGSolver_CSMRI,
    'redadmm': REDADMMSolver_CSMRI,
    'amp': AMPSolver_CSMRI,
}


def create_solver_csmri(opt, denoiser):
    """tasks/csmri/solver.py:262-270"""
    if opt.solver in _solver_map:
        return _solver_map[opt.solver](denoiser)
    raise NotImplementedError


class CSMRIEnv(PnPEnv):
    """tasks/csmri/env.py:7-56.  Policy observation (9 channels for 3-variable solvers): Re(variables), y0 as 2
    channels, Re(ATy0), mask, T, Re(sigma_n)."""
    ob_base_dim = 6
    ob_keys = ('y0', 'ATy0', 'mask', 'sigma_n')
    float_keys = ('mask',)
    policy_layout = (('variables', 'real'), ('y0', 'channel'), ('ATy0', 'real'), ('mask', 'raw'), ('T', 'raw'),
                     ('sigma_n', 'real'))
    input_key = 'ATy0'
    aux_keys = ('y0', 'mask')
    aux_bool = ('mask',)
