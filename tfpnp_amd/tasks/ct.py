"""Sparse-view CT solvers -- drop-in for tasks/ct/solver.py (own Radon pair instead of torch_radon)."""
import torch

from .. import autograd as A
from .. import torch_ops as T
from ..env.base import PnPEnv
from ..pnp.solver.base import HQSSolver, IADMMSolver, PGSolver
from ..utils.transforms import RadonGenerator


class CTMixin:
    """tasks/ct/solver.py:7-9"""

    def filter_aux_inputs(self, state):
        return (state['y0'], state['view'])


def _geometry_args(radon):
    """The geometry tail of the ct_*_geom / ct_hqs ops from a resolved projector pair."""
    g = radon.geometry
    return (g.det_count, g.source_distance, g.det_distance, g.det_spacing)


class IADMMSolver_CT(CTMixin, IADMMSolver):
    """tasks/ct/solver.py:12-53.  geometry: None = the reference's parallel pair, or a utils.transforms.FanBeam (the reference's
    solvers take none; the native loop is the same, on the fan pair)."""

    def __init__(self, denoiser, geometry=None):
        super().__init__(denoiser)
        self.radon_generator = RadonGenerator()
        self.geometry = geometry

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, view) = inputs
        sigma_d, mu, tau = parameters
        # The reference recovers the view count from the observation map, int(view[0,0,0,0] * 120) (:26): a host sync,
        # and the float32 round trip truncates many counts by one (50 -> 49, 100 -> 99), which torch_radon then rejects
        # with a shape error.  The sinogram itself carries the count, exactly and without a sync.
        n_view = int(y0.shape[2])
        it = -1 if iter_num is None else iter_num
        train = A.needs_grad(variables, sigma_d, mu, tau)      # training path: native forward + fused native VJP (tasks.hip)
        if self.geometry is not None:
            radon = self.radon_generator(variables.shape[-1], n_view, device=variables.device, geometry=self.geometry)
            out = T.call("ct_iadmm_geom_train" if train else "ct_iadmm_geom", variables, y0, n_view, float(radon.opnorm),
                         *_geometry_args(radon), sigma_d, mu, tau, it, self._ctx(variables).cid)
            return out[0] if train else out
        radon = self.radon_generator(variables.shape[-1], n_view, device=variables.device)
        if train:
            return T.call("ct_iadmm_train", variables, y0, n_view, float(radon.opnorm), sigma_d, mu, tau, it,
                          self._ctx(variables).cid)[0]
        return T.call("ct_iadmm", variables, y0, n_view, float(radon.opnorm), sigma_d, mu, tau, it, self._ctx(variables).cid)


class PGSolver_CT(CTMixin, PGSolver):
    """tasks/ct/solver.py:56-87.  geometry: as for IADMMSolver_CT."""

    def __init__(self, denoiser, geometry=None):
        super().__init__(denoiser)
        self.radon_generator = RadonGenerator()
        self.geometry = geometry

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, view) = inputs
        sigma_d, tau = parameters
        n_view = int(y0.shape[2])                        # see IADMMSolver_CT.forward
        it = -1 if iter_num is None else iter_num
        train = A.needs_grad(variables, sigma_d, tau)      # training path: native forward + fused native VJP (tasks.hip)
        if self.geometry is not None:
            radon = self.radon_generator(variables.shape[-1], n_view, device=variables.device, geometry=self.geometry)
            out = T.call("ct_pg_geom_train" if train else "ct_pg_geom", variables, y0, n_view, float(radon.opnorm),
                         *_geometry_args(radon), sigma_d, tau, it, self._ctx(variables).cid)
            return out[0] if train else out
        radon = self.radon_generator(variables.shape[-1], n_view, device=variables.device)
        if train:
            return T.call("ct_pg_train", variables, y0, n_view, float(radon.opnorm), sigma_d, tau, it, self._ctx(variables).cid)[0]
        return T.call("ct_pg", variables, y0, n_view, float(radon.opnorm), sigma_d, tau, it, self._ctx(variables).cid)


class HQSSolver_CT(CTMixin, HQSSolver):
    """HQS for CT: state cat(x, z) = (x0, x0), hyper-parameters (sigma_d, mu) -- ResNetActor_HQS drives it.  Per iteration
    x = D(z, sigma_d_i), then z <- z - (A^T(A z - y0) / |A|^2 + mu_i (z - x)) / (1 + mu_i): the inexact data step of
    tasks/ct/solver.py:46-49 without the dual.  geometry: None = the parallel pair, or a utils.transforms.FanBeam."""

    def __init__(self, denoiser, geometry=None):
        super().__init__(denoiser)
        self.radon_generator = RadonGenerator()
        self.geometry = geometry

    def forward(self, inputs, parameters, iter_num=None):
        variables, (y0, view) = inputs
        sigma_d, mu = parameters
        n_view = int(y0.shape[2])                        # see IADMMSolver_CT.forward
        radon = self.radon_generator(variables.shape[-1], n_view, device=variables.device, geometry=self.geometry)
        g = getattr(radon, "geometry", None)
        geom = (g.det_count, g.source_distance, g.det_distance, g.det_spacing) if g is not None else (0, 0.0, 0.0, 0.0)
        name = "ct_hqs_train" if A.needs_grad(variables, sigma_d, mu) else "ct_hqs"   # training: native forward + fused native VJP
        out = T.call(name, variables, y0, n_view, float(radon.opnorm), *geom, sigma_d, mu, -1 if iter_num is None else iter_num,
                     self._ctx(variables).cid)
        return out[0] if name == "ct_hqs_train" else out


_solver_map = {'iadmm': IADMMSolver_CT, 'pg': PGSolver_CT, 'hqs': HQSSolver_CT}


def create_solver_ct(opt, denoiser):
    """tasks/ct/solver.py:95-103"""
    if opt.solver in _solver_map:
        return _solver_map[opt.solver](denoiser, getattr(opt, 'geometry', None))      # None, or a utils.transforms.FanBeam
    raise NotImplementedError


class CTEnv(PnPEnv):
    """tasks/ct/env.py:6-55.  Observation: variables, ATy0, view, T, sigma_n."""
    ob_base_dim = 4
    ob_keys = ('y0', 'ATy0', 'view', 'sigma_n')
    policy_layout = (('variables', 'raw'), ('ATy0', 'raw'), ('view', 'raw'), ('T', 'raw'), ('sigma_n', 'raw'))
    input_key = 'ATy0'
    aux_keys = ('y0', 'view')
