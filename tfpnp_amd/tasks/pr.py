"""Phase-retrieval solvers -- drop-in for tasks/pr/solver.py."""
import torch

from .. import autograd as A
from .. import torch_ops as T
from ..env.base import PnPEnv
from ..pnp.solver.base import IADMMSolver, PGSolver
from ..utils.transforms import complex2real, real2complex


class PRMixin:
    """tasks/pr/solver.py:15-21"""

    def get_output(self, state):
        return complex2real(super().get_output(state))

    def filter_aux_inputs(self, state):
        return (state['y0'], state['mask'])


class IADMMSolver_PR(PRMixin, IADMMSolver):
    """tasks/pr/solver.py:24-76"""

    def reset(self, data):
        x = real2complex(data['x0'].clone().detach())
        z = x.clone().detach()
        u = torch.zeros_like(x)
        return torch.cat([x, z, u], dim=1)

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, mask) = inputs
        sigma_d, mu, tau = parameters
        if A.needs_grad(variables, sigma_d, mu, tau):      # training path: native forward + fused native VJP (tasks.hip)
            return T.call("pr_iadmm_train", variables, y0, mask, sigma_d, mu, tau, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("pr_iadmm", variables, y0, mask, sigma_d, mu, tau, -1 if iter_num is None else iter_num, self._ctx(variables).cid)

class PGSolver_PR(PRMixin, PGSolver):
    """tasks/pr/solver.py:79-112, proximal gradient on the PR data term.

    The reference's gradient step (:102-103) was pasted from CS-MRI -- `fft2(x) - y0` and `temp[~mask, :] = 0` on the float
    coded-diffraction mask -- and raises on any PR input; it stays broken there.  Here those two lines are replaced by the
    gradient of the PR data term as the same file computes it in IADMMSolver_PR.forward (:61-68):

        Ax = cdp_forward(x, mask);  r = (|Ax| - y0) / |Ax| * Ax;  z = x - tau_i * cdp_backward(r, mask)
        x  = real2complex(prox_mapping(complex2real(z), sigma_d_i))

    The substitution is pinned by executed reference code: one reference IADMMSolver_PR.forward call with iter_num = 1, state
    cat(x, x, 0) and mu = 0 returns exactly this z in its second slot, and tests/golden/pr_pg_B2_64x64.npz is that call chained
    with the reference's denoiser prox (tools/make_pr_pg_golden.py).  All iterations run in one native call (pnpx_pr_pg)."""

    def reset(self, data):
        return real2complex(data['x0'].clone().detach())

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, mask) = inputs
        sigma_d, tau = parameters
        if A.needs_grad(variables, sigma_d, tau):          # training path: native forward + fused native VJP (tasks.hip)
            return T.call("pr_pg_train", variables, y0, mask, sigma_d, tau, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("pr_pg", variables, y0, mask, sigma_d, tau, -1 if iter_num is None else iter_num, self._ctx(variables).cid)


_solver_map = {'iadmm': IADMMSolver_PR, 'pg': PGSolver_PR}


def create_solver_pr(opt, denoiser):
    """tasks/pr/solver.py:120-128"""
    if opt.solver in _solver_map:
        return _solver_map[opt.solver](denoiser)
    raise NotImplementedError


class PREnv(PnPEnv):
    """tasks/pr/env.py:7-56.  Observation: Re(variables), y0 [S], mask as 2S channels, T, sigma_n  (S = 4 -> 14 + 3)."""
    ob_base_dim = 14
    ob_keys = ('y0', 'x0', 'mask', 'sigma_n')
    float_keys = ('mask',)
    policy_layout = (('variables', 'real'), ('y0', 'raw'), ('mask', 'channel'), ('T', 'raw'), ('sigma_n', 'raw'))
    input_key = 'x0'
    aux_keys = ('y0', 'mask')
