"""Helpers of the critic optimiser tests (pnpx_critic_adam_step): clip_grad_norm_ + torch's single-tensor Adam restated in numpy
float64 (the yardstick) and in float32 with another operation order (the check that the bounds are sound), the synthetic
gradient sequence, and the bounds themselves.  No GPU, no reference import.

Bounds, against the fp64 restatement fed the same fp32 inputs, after k steps:
    parameters     |p - p64| <= k * (8e-6 * lr + ulp32(|p64|))    half an ulp per step from the final rounding; the lr term is about
                                                                  ten fp32 roundings times the (1 - b1) / sqrt(1 - b2) ~ 3.2 worst-case
                                                                  update factor, plus the clip coefficient's relative error
    first moment   |m - m64| <= 4e-6 * max_t |c_t g_t|            the moments are convex combinations of the clipped gradients
    second moment  |v - v64| <= 4e-6 * max_t (c_t g_t)^2          (relative to |m| it would not hold: m cancels)
"""
import functools

import numpy as np
import torch

from tests import critic_cases as K
from tfpnp_amd import synth

LR, BETAS, EPS, MAX_NORM, STEPS = 1e-3, (0.9, 0.999), 1e-8, 50.0, 6
M_TOL, V_TOL, P_LR_TOL = 4e-6, 4e-6, 8e-6


def flat_params(num_inputs):
    """critic_cases.critic_params as the flat float32 vector of synth.critic_param_specs order"""
    params = K.critic_params(num_inputs)
    return np.concatenate([params[k].reshape(-1) for k, _ in synth.critic_param_specs(num_inputs)]).astype(np.float32)


def _f64(a):
    return a.to(torch.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)


def clip_coef(g, max_norm):
    """(norm, c) of clip_grad_norm_ in float64: c = min(1, max_norm / (norm + 1e-6))"""
    g = _f64(g)
    norm = float((g * g).sum()) ** 0.5 if isinstance(g, torch.Tensor) else float(np.sqrt(np.dot(g, g)))
    return norm, min(1.0, max_norm / (norm + 1e-6))


def adam_ref(p, m, v, t, g, lr, betas=BETAS, eps=EPS, max_norm=MAX_NORM):
    """Step number t (1, 2, ...) of clip_grad_norm_(max_norm) + Adam (no weight decay, no amsgrad) in float64.
    p, m, v: the state before the step; g: the raw gradient -- numpy arrays, or torch tensors (then the same float64 arithmetic
    runs on their device).  -> (p, m, v, norm before clipping, clip coefficient)"""
    p, m, v, g = (_f64(a) for a in (p, m, v, g))
    b1, b2 = betas
    norm, c = clip_coef(g, max_norm)
    g = g * c
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    bc2_sqrt = (1.0 - b2 ** t) ** 0.5
    p = p - step_size * (m / (v ** 0.5 / bc2_sqrt + eps))
    return p, m, v, norm, c


def adam_f32(p, m, v, t, g, lr, betas=BETAS, eps=EPS, max_norm=MAX_NORM):
    """The same step in float32 throughout, in the textbook order (m = b1 m + (1 - b1) g, the bias correction inside the root),
    which is not the order the kernel or torch use.  The norm is summed in double and rounded once, as the kernel does."""
    f = np.float32
    p, m, v, g = (np.asarray(a, f) for a in (p, m, v, g))
    b1, b2 = betas
    norm = f(np.sqrt(np.dot(g.astype(np.float64), g.astype(np.float64))))
    c = min(f(1.0), f(max_norm) / (norm + f(1e-6)))
    g = g * f(c)
    m = f(b1) * m + f(1.0 - b1) * g
    v = f(b2) * v + f(1.0 - b2) * (g * g)
    vhat = v / f(1.0 - b2 ** t)
    p = p - (f(lr / (1.0 - b1 ** t)) * m) / (np.sqrt(vhat) + f(eps))
    return p, m, v, norm, c


@functools.lru_cache(maxsize=2)
def _scales(n, seed):
    return np.logspace(-9, 0, n)[np.random.RandomState(seed).permutation(n)]


def synthetic_gradient(n, k, seed=0):
    """Gradient of step index k (0, 1, ...): randn(n) * logspace(-9, 0, n)[perm], every 97th entry zero; even steps times 200
    (norm >> 50: the clip is active), odd steps times 0.01 (inactive).  float32."""
    g = np.random.RandomState(seed + 1000 * (k + 1)).standard_normal(n) * _scales(n, seed)
    g[::97] = 0.0
    return (g * (200.0 if k % 2 == 0 else 0.01)).astype(np.float32)


def ulp32(x):
    """spacing of float32 at |x| (x float64: numpy array or torch tensor), as float64"""
    if isinstance(x, torch.Tensor):
        a = x.abs().to(torch.float32)
        return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(torch.float64)
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


class Yardstick:
    """Runs the fp64 restatement alongside a sequence of steps and measures a candidate state against the three bounds.  numpy
    arrays, or torch tensors (the same arithmetic in float64 on their device)."""

    def __init__(self, p0, lr=LR, betas=BETAS, eps=EPS, max_norm=MAX_NORM):
        self.p = _f64(p0) + 0.0
        self.m = self.p * 0.0
        self.v = self.p * 0.0
        self.t = 0
        self.cg_max = self.p * 0.0     # max_t |c_t g_t|, per element
        self.hyper = (lr, betas, eps, max_norm)
        self.norm = None

    def step(self, g):
        lr, betas, eps, max_norm = self.hyper
        self.t += 1
        self.p, self.m, self.v, self.norm, c = adam_ref(self.p, self.m, self.v, self.t, g, lr, betas, eps, max_norm)
        cg = abs(_f64(g) * c)
        self.cg_max = torch.maximum(self.cg_max, cg) if isinstance(cg, torch.Tensor) else np.maximum(self.cg_max, cg)
        return self

    def ratios(self, p, m, v, k=None):
        """worst |candidate - fp64| / bound per quantity (0 / 0 counts as 0; NaN if the candidate is not finite)"""
        k = self.t if k is None else k
        return bound_ratios(_f64(p) - self.p, _f64(m) - self.m, _f64(v) - self.v, self.p, self.cg_max, k, self.hyper[0])


def bound_ratios(dp, dm, dv, p64, cg_max, k, lr):
    """{'p', 'm', 'v'}: worst |difference| / bound over the elements, for the bounds in the module docstring after k steps"""
    def worst(err, bound):
        err = abs(err)
        if isinstance(err, torch.Tensor):
            r = torch.where(err == 0.0, torch.zeros_like(err), err / bound.clamp_min(np.finfo(np.float64).tiny))
            return float("nan") if bool(torch.isnan(r).any()) else float(r.max())
        return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, np.finfo(np.float64).tiny))))
    return {"p": worst(dp, k * (P_LR_TOL * lr + ulp32(p64))), "m": worst(dm, M_TOL * cg_max), "v": worst(dv, V_TOL * cg_max ** 2)}
