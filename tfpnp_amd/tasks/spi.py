"""Single-photon-imaging solver -- drop-in for tasks/spi/solver.py."""
from .. import autograd as A
from .. import torch_ops as T
from ..env.base import PnPEnv
from ..pnp.solver.base import ADMMSolver, PGSolver


class SPIMixin:
    """tasks/spi/solver.py:8-10"""

    def filter_aux_inputs(self, state):
        return (state['x0'], state['K'])


class ADMMSolver_SPI(SPIMixin, ADMMSolver):
    """tasks/spi/solver.py:13-52"""

    def forward(self, inputs, parameters, iter_num=None):
        variables, (x0, K) = inputs
        sigma_d, mu = parameters
        if A.needs_grad(variables, sigma_d, mu):      # training path: native forward + fused native VJP (tasks.hip)
            return T.call("spi_admm_train", variables, x0, K, sigma_d, mu, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("spi_admm", variables, x0, K, sigma_d, mu, -1 if iter_num is None else iter_num, self._ctx(variables).cid)


class PGSolver_SPI(SPIMixin, PGSolver):
    """Proximal gradient on the SPI data term (BASELINE config #5 as named).  The reference has no such class --
    tasks/spi/solver.py stops at ADMM -- so the step is this package's own, on the likelihood behind spi_inverse
    (transforms.py:404-439, func) divided by K^2, f(x) = (1 - x0) x - x0 log(1 - e^-x), K = 10 K_map[b,0,0,0]:

        x_c = max(x, 0.5 / K^2);  q = -expm1(-x_c);  g = 1 - x0 / q;  c = x0 (1 - q) / q^2
        z = clamp(x - tau_i * g / max(c, 1), 0, 1);  x = prox_mapping(z, sigma_d_i)

    g = f' and c = f'' (unbounded as x -> 0): the gradient step where c < 1, the damped Newton step where c >= 1, so tau in
    (0, 1.5] converges to the maximum-likelihood value; tau = 2, the edge of ResNetActor_PG's range, ends in a limit cycle of
    about 3.5e-2.  Unlike the bisection of ADMMSolver_SPI the step is differentiable everywhere, so tau
    receives a gradient from every pixel.  All iterations run in one native call (pnpx_spi_pg), the VJP in another."""

    def forward(self, inputs, parameters, iter_num=None):
        variables, (x0, K) = inputs
        sigma_d, tau = parameters
        if A.needs_grad(variables, sigma_d, tau):          # training path: native forward + fused native VJP (tasks.hip)
            return T.call("spi_pg_train", variables, x0, K, sigma_d, tau, -1 if iter_num is None else iter_num,
                          self._ctx(variables).cid)[0]
        return T.call("spi_pg", variables, x0, K, sigma_d, tau, -1 if iter_num is None else iter_num, self._ctx(variables).cid)


_solver_map = {'admm_spi': ADMMSolver_SPI, 'pg_spi': PGSolver_SPI}


def create_solver_spi(opt, denoiser):
    """tasks/spi/solver.py:58-66"""
    if opt.solver in _solver_map:
        return _solver_map[opt.solver](denoiser)
    raise NotImplementedError


class SPIEnv(PnPEnv):
    """tasks/spi/env.py:7-52.  Observation: variables, x0, K, T."""
    ob_base_dim = 3
    ob_keys = ('x0', 'K')
    policy_layout = (('variables', 'raw'), ('x0', 'raw'), ('K', 'raw'), ('T', 'raw'))
    input_key = 'x0'
    aux_keys = ('x0', 'K')
