"""PGSolver_SPI restated in torch, generic in dtype: what the native step (tasks.hip spi_pg_step_px) and loop (pnpx_spi_pg) are
held against, in fp32 and in float64, and what autograd differentiates for the VJP tests.  The reference has no counterpart (its
tasks/spi/solver.py stops at ADMM); the definition is this package's own:

    f(x) = (1 - x0) x - x0 log(1 - e^-x)      the Poisson / threshold likelihood behind spi_inverse, divided by K^2
    f'   = 1 - x0 / q,  f'' = x0 (1 - q) / q^2,  q = 1 - e^-x
"""
import numpy as np
import torch


def item_K(Kmap):
    """K = 10 * K_map[b, 0, 0, 0] as [B,1,1,1], the way spi_step_kernel reads it."""
    return Kmap[:, :1, :1, :1] * 10


def parts(x, x0, Kmap, tau):
    """Every intermediate of one step.  tau: one value per item (or, for per-pixel derivatives, a tensor of x's shape).  Written
    with torch.clamp throughout: its closed intervals pass the gradient, so `live` is x >= x_lo, the Newton branch is c >= 1 and
    `pass` is 0 <= x - tau h <= 1."""
    K = item_K(Kmap)
    t = tau if tau.dim() == 4 else tau.reshape(-1, 1, 1, 1)
    x_lo = 0.5 / (K * K)
    x_c = torch.clamp(x, min=x_lo.expand_as(x))
    q = -torch.expm1(-x_c)
    g = 1 - x0 / q
    c = x0 * (1 - q) / (q * q)
    h = g / torch.clamp(c, min=1)
    pre = x - t * h
    return dict(x_lo=x_lo, q=q, g=g, c=c, h=h, pre=pre, z=torch.clamp(pre, 0, 1))


def step(x, x0, K, tau):
    """z = clamp(x - tau h(x), 0, 1); K is the K / 10 map of the solver state."""
    return parts(x, x0, K, tau)["z"]


def spi_pg(den, x, x0, Kmap, sigma_d, tau, iter_num=None):
    """The loop on a passed-in denoiser den(x, sigma): x <- den(step(x, x0, Kmap, tau_i), sigma_d_i)."""
    T = sigma_d.shape[-1] if iter_num is None else iter_num
    for i in range(T):
        x = den(step(x, x0, Kmap, tau[:, i]), sigma_d[:, i])
    return x


def closed_form(x, x0, Kmap, tau):
    """The VJP pieces as the adjoint kernel forms them: (pass, live, h, h', dz/dx, dz/dtau) per pixel."""
    p = parts(x, x0, Kmap, tau)
    q, c, h = p["q"], p["c"], p["h"]
    t = tau.reshape(-1, 1, 1, 1)
    ok = (p["pre"] >= 0) & (p["pre"] <= 1)
    live = x >= p["x_lo"]
    newton = (2 * q - q * q - x0) / (x0 * (1 - q))
    hp = torch.where(c < 1, c, newton)
    zero = torch.zeros_like(x)
    dzdx = torch.where(ok, 1 - t * torch.where(live, hp, zero), zero)
    dzdt = torch.where(ok, -h, zero)
    return ok, live, h, hp, dzdx, dzdt


def mle(K):
    """float64: every x0 = K1 / K^2, K1 = 0 .. K^2, and the minimiser of f clamped to [0, 1] (-log(1 - x0), 1 at x0 = 1)."""
    x0 = torch.arange(K * K + 1, dtype=torch.float64) / (K * K)
    with np.errstate(divide="ignore"):
        m = torch.clamp(-torch.log1p(-x0), 0, 1)
    return x0, m


def synth(B, H, W, Ks, seed):
    """x0 = binomial counts of a phantom: the fraction of ones among the K^2 binary pixels of each cell, per-item K
    (synth.make_spi_batch's measurement at one K).  -> (x0 [B,1,H,W] float32, Kmap [B,1,H,W] float32)."""
    from tfpnp_amd import synth as S
    gt = S.phantom_batch(B, H, W, seed).astype(np.float64)
    rs = np.random.RandomState(seed + 9)
    x0 = np.empty((B, 1, H, W), np.float32)
    Kmap = np.empty((B, 1, H, W), np.float32)
    for b, K in enumerate(Ks):
        ones = rs.binomial(K * K, 1.0 - np.exp(-gt[b]))
        x0[b] = (ones / float(K * K)).astype(np.float32)
        Kmap[b] = np.float32(K / 10.0)
    return x0, Kmap


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# the inputs of the step-kernel test (tests/test_gpu_spi_pg.py), whose fp32-vs-float64 distance tests/test_spi_pg_host.py measures on
# the CPU (profiles/spi_pg.md)
STEP_KS, STEP_TAU, STEP_H, STEP_W = (4, 6, 8), (0.1, 1.0, 2.0), 17, 15


def step_case():
    """B = 3, 17 x 15 (255 pixels an item: no multiple of 256).  x uniform in [-0.5, 1.5] with planted zeros and values below x_lo
    (and one at x_lo); x0 the fractions K1 / K^2 with a row of 0 and a row of 1.  float32 numpy: x, x0, Kmap, tau."""
    B = len(STEP_KS)
    rs = np.random.RandomState(2025)
    x = rs.uniform(-0.5, 1.5, (B, 1, STEP_H, STEP_W)).astype(np.float32)
    x0 = np.empty_like(x)
    Kmap = np.empty_like(x)
    for b, K in enumerate(STEP_KS):
        x0[b] = (rs.randint(0, K * K + 1, (1, STEP_H, STEP_W)) / float(K * K)).astype(np.float32)
        Kmap[b] = np.float32(K / 10.0)
        x_lo = np.float32(0.5) / (np.float32(Kmap[b, 0, 0, 0] * np.float32(10)) ** 2)
        x[b, 0, 2, :5] = 0.0
        x0[b, 0, 2, :5] = (np.arange(1, 6) / float(K * K)).astype(np.float32)      # zeros that have to leave zero
        x[b, 0, 3, :5] = x_lo * np.float32([0.1, 0.5, 0.9, 0.999, 1.0])
        x[b, 0, 4, :3] = [1.0, 0.0, 1e-6]
    x0[:, 0, 0, :] = 0.0
    x0[:, 0, 1, :] = 1.0
    return x, x0, Kmap, np.asarray(STEP_TAU, np.float32)
