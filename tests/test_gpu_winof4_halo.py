"""GPU tests of the halo fetch of the four Winograd F(4x4,3x3) instances (csrc/conv3x3_winof4.hip; the plan itself:
tests/test_winof4_halo_host.py): probe kinds 4, 8, 11 and 12 against the float64 reference of one layer, at each kind's smallest shape, at
a shape with an odd chunk count, 2 x 2 regions and two images (region edges both ways, the batch stride, both halo buffers in steady
state; kinds 4 and 12 with the fused pool) and, kind 4, at a shape with more work items than workgroups (the tile boundary and the
surplus-load tail).  Random normal inputs and impulses at the image corners and either side of a region boundary, in the first and last
channel of the first and last chunk of each source.  Measure and bars are the existing classes' (tests/conv_layer_cases.py,
winof4_entry_cases.py, winof4_fuse_up_cases.py, winof4_c32_cases.py).  Every launch is repeated and must give the same bytes: a gather
the counted waits do not cover shows there."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_layer_cases as CL
from tests import winof4_c32_cases as C32
from tests import winof4_entry_cases as EC
from tests import winof4_fuse_up_cases as FU
from tests.test_gpu_conv_layers import Launch, _check_borders

pytestmark = pytest.mark.gpu

K_PLAIN, K_ENTRY, K_UPS, K_C32 = CL.WINOF4, EC.WINOF4_2SRC, FU.FUSE_UP, C32.WINOF4_C32
BAR = {K_PLAIN: lambda: CL.bar("f4"), K_ENTRY: EC.bar, K_UPS: EC.bar, K_C32: C32.bar}
REGION_W = {K_PLAIN: 32, K_ENTRY: 32, K_UPS: 32, K_C32: 64}

# (kind, images, case)
RUNS = (
    (K_PLAIN, 1, CL._c("fwd", 16, 0, 64, 16, 32)), (K_ENTRY, 1, CL._c("fwd", 8, 8, 64, 16, 32)), (K_UPS, 1, CL._c("ups", 16, 16, 64, 16, 32)),
    (K_C32, 1, CL._c("fwd", 16, 0, 32, 16, 64)),
    (K_PLAIN, 2, CL._c("fwd", 24, 0, 64, 32, 64, pool=True)), (K_ENTRY, 2, CL._c("fwd", 8, 16, 64, 32, 64)),
    (K_UPS, 2, CL._c("ups", 16, 8, 64, 32, 64)), (K_C32, 2, CL._c("fwd", 24, 0, 32, 32, 128, pool=True)),
    (K_PLAIN, 9, CL._c("fwd", 16, 0, 128, 64, 128)),
)
IDS = [f"kind{k}_{B}x{c.name}" for k, B, c in RUNS]
IMPULSE_RUNS = RUNS[4:8]          # the 2 x 2 region shapes, without the pool


@pytest.fixture(scope="module")
def ctx():
    from tfpnp_amd import ops
    return ops.Context("cuda:0")


@functools.lru_cache(maxsize=None)
def _random_case(i):
    """(operands, (ref, denom)) of RUNS[i]; never modified"""
    _, B, c = RUNS[i]
    rs = np.random.RandomState(9300 + 17 * i)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    cin = c.C0 + c.C1
    d = {"w": t(rs.standard_normal((c.cout, cin, 3, 3)) / np.sqrt(9.0 * cin)), "bias": t(0.1 * rs.standard_normal(c.cout)),
         "in0": t(rs.standard_normal((B, c.C0, c.H, c.W)))}
    if c.C1:
        hw = (c.H // 2, c.W // 2) if c.op == "ups" else (c.H, c.W)
        d["in1"] = t(rs.standard_normal((B, c.C1) + hw))
    return d, CL.reference(c, d)


def _bits(t):
    return t.view(torch.int32)


def _twice(L):
    out, pool = L.run()
    out2, pool2 = L.run()
    assert torch.equal(_bits(out2), _bits(out)), "second launch differs"
    assert pool is None or torch.equal(_bits(pool2), _bits(pool)), "second launch differs (pool)"
    _check_borders(out, "out")
    return out, pool


@pytest.mark.parametrize("i", range(len(RUNS)), ids=IDS)
def test_random_inputs_against_float64(ctx, i):
    kind, B, c = RUNS[i]
    d, (ref, den) = _random_case(i)
    L = Launch(ctx, kind, c, d, 0, B)
    L.set_tails(False)
    out, pool = _twice(L)
    err = CL.measure(CL.interior(out), ref, den)
    print(f"{IDS[i]}: measure {err:.3e}, bar {BAR[kind]():.3e}")
    assert err < BAR[kind](), err
    if c.pool:
        _check_borders(pool, "pool_out")
        assert torch.equal(CL.interior(pool), F.max_pool2d(CL.interior(out), 2)), "fused pool != max_pool2d of the kernel's own output"


def _sites(kind, c):
    """[(source, channel, y, x)], one per image: the image corners and the pixels either side of the region boundaries (rows 15 | 16,
    columns RW - 1 | RW), the first and last channel of the first and last chunk of each source in turn; then every such channel at
    one corner and at the two pixels across the regions' common corner.  A low-resolution second source has its sites at half the
    coordinates."""
    rw = REGION_W[kind]
    ys, xs = (0, 15, 16, c.H - 1), (0, rw - 1, rw, c.W - 1)
    chans = []
    for src, C in (("in0", c.C0), ("in1", c.C1)):
        if C:
            chans += [(src, ch) for ch in sorted({0, 7, C - 8, C - 1})]
    low = lambda src, v: v // 2 if (c.op == "ups" and src == "in1") else v
    sites = []
    for n, (y, x) in enumerate((y, x) for y in ys for x in xs):
        src, ch = chans[n % len(chans)]
        sites.append((src, ch, low(src, y), low(src, x)))
    for src, ch in chans:
        sites += [(src, ch, low(src, y), low(src, x)) for y, x in ((c.H - 1, c.W - 1), (15, rw - 1), (16, rw))]
    return sites


@pytest.mark.parametrize("i", range(len(IMPULSE_RUNS)), ids=[f"kind{k}_{c.name}" for k, _, c in IMPULSE_RUNS])
def test_impulses(ctx, i):
    kind, _, c = IMPULSE_RUNS[i]
    c = c._replace(pool=False)
    sites = _sites(kind, c)
    d = CL.impulse_inputs(c, sites)
    ref, _ = CL.reference(c, d, slope=CL.IMPULSE_SLOPE)
    L = Launch(ctx, kind, c, d, 0, len(sites), slope=CL.IMPULSE_SLOPE)
    L.set_tails(False)
    out, _ = _twice(L)
    # an impulse's output is one weight (a low-resolution one: a blend of weights): the absolute error at the scale of the largest
    # weight keeps the zero outputs (no tap of the site) in the check (tests/test_gpu_winof4_c32.py)
    err = float((CL.interior(out).double() - ref).abs().max() / d["w"].double().abs().max())
    print(f"impulses kind {kind} {c.name}: {len(sites)} sites, max |y - ref| / max |w| = {err:.3e}, bar {BAR[kind]():.3e}")
    assert err < BAR[kind](), err
