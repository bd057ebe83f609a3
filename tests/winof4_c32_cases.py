"""Cases, inputs, float64 references, the fp32 emulation's bar and the reference mutants of the F(4x4,3x3) kernel's 32-cout instance
(csrc/conv3x3_winof4.hip, probe kind 12), shared by tests/test_winof4_c32_host.py and tests/test_gpu_winof4_c32.py.  Measure, emulation
and bar factor are tests/conv_layer_cases.py's; the bar is 8 x the largest measure the fp32 CPU emulation of F(4x4) reaches on THESE
cases, recorded in profiles/winof4_c32.md.  No GPU."""
import functools
import os
import re

import numpy as np
import torch

from tests import conv_layer_cases as CL

WINOF4_C32 = 12                       # include/pnpx.h: PNPX_PROBE_WINOF4_C32
PROFILE_NOTE = os.path.join(CL.ROOT, "profiles", "winof4_c32.md")
REGION_H, REGION_W = 16, 64           # one workgroup's region

# (B, case): one region and two chunks (the pipeline's minimum); an odd chunk count and two regions in x; region boundaries both ways, the
# batch stride and the fused pool; 288 regions on 256 workgroups (a workgroup walks two tiles, the XCD-grouped walk, the surplus-load tail)
CASES = (
    (1, CL._c("fwd", 16, 0, 32, 16, 64)),
    (1, CL._c("fwd", 24, 0, 32, 16, 128)),
    (2, CL._c("fwd", 32, 0, 32, 32, 128, pool=True)),
    (9, CL._c("fwd", 32, 0, 32, 128, 256)),
)
CASE_BY_NAME = {c.name: (B, c) for B, c in CASES}
# geometries the instance refuses: W no multiple of 64, H no multiple of 16, one chunk, 12 channels, a 64-cout tile, a second source
REFUSED = ((32, 0, 32, 16, 32), (32, 0, 32, 16, 96), (32, 0, 32, 24, 64), (8, 0, 32, 16, 64), (12, 0, 32, 16, 64), (32, 0, 64, 16, 64),
           (32, 0, 128, 16, 64), (32, 0, 48, 16, 64), (32, 32, 32, 16, 64))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp32 operands of a case (never modified by the callers)"""
    B, c = CASE_BY_NAME[name]
    rs = np.random.RandomState(7100 + 13 * [n for n in CASE_BY_NAME].index(name))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    return {"w": t(rs.standard_normal((c.cout, c.C0, 3, 3)) / np.sqrt(9.0 * c.C0)), "bias": t(0.1 * rs.standard_normal(c.cout)),
            "in0": t(rs.standard_normal((B, c.C0, c.H, c.W)))}


@functools.lru_cache(maxsize=None)
def case_reference(name):
    return CL.reference(CASE_BY_NAME[name][1], inputs(name))


@functools.lru_cache(maxsize=None)
def emulation_maximum():
    """(largest measure of the fp32 F(4x4) emulation over the cases, the case it was found at); one thread: an fp32 sum must not move with
    the number of threads the host happens to have"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        worst, where = 0.0, None
        for _, c in CASES:
            ref, den = case_reference(c.name)
            e = CL.measure(CL.emulate32(c, inputs(c.name), "f4"), ref, den)
            if e > worst:
                worst, where = e, c.name
        return worst, where
    finally:
        torch.set_num_threads(threads)


def recorded_bar():
    """(emulation maximum, bar) as profiles/winof4_c32.md records them (table row `| f4 c32 | max | bar | ...`)"""
    for line in open(PROFILE_NOTE):
        m = re.match(r"\|\s*f4 c32\s*\|\s*([0-9.eE+-]+)\s*\|\s*([0-9.eE+-]+)\s*\|", line)
        if m:
            return float(m.group(1)), float(m.group(2))
    raise AssertionError(f"{PROFILE_NOTE}: the bar's row is missing")


def bar():
    return recorded_bar()[1]


def mutants(name):
    """[(name, mutated float64 reference)]: one weight zeroed; the result shifted by one pixel in x inside one 4 x 4 tile; the two 16-cout
    blocks of the tile swapped inside one region of one image"""
    B, c = CASE_BY_NAME[name]
    d = inputs(name)
    ref = case_reference(name)[0]
    rs = np.random.RandomState(99 + len(name))
    out = []
    w2 = d["w"].clone()
    w2[rs.randint(c.cout), rs.randint(c.C0), rs.randint(3), rs.randint(3)] = 0.0
    out.append(("weight_zeroed", CL.reference(c, dict(d, w=w2))[0]))
    sh = ref.clone()
    b, y0, x0 = rs.randint(B), 4 * rs.randint(c.H // 4), 4 * rs.randint(c.W // 4)
    sh[b, :, y0:y0 + 4, x0 + 1:x0 + 4] = ref[b, :, y0:y0 + 4, x0:x0 + 3]
    out.append(("tile_shifted", sh))
    sw = ref.clone()
    b, y0, x0 = rs.randint(B), REGION_H * rs.randint(c.H // REGION_H), REGION_W * rs.randint(c.W // REGION_W)
    reg = (b, slice(None), slice(y0, y0 + REGION_H), slice(x0, x0 + REGION_W))
    sw[reg] = torch.cat([ref[reg][16:], ref[reg][:16]], 0)
    out.append(("cout_block_swapped", sw))
    return out
