"""Cases, inputs, float64 references, fp32 emulation and reference mutants of the F(4x4,3x3) kernel's decoder-entry instance (probe kind
PNPX_PROBE_WINOF4_2SRC, csrc/conv3x3_winof4.hip), in the manner of tests/conv_layer_cases.py, whose helpers they use.  The measure is
conv_layer_cases.measure; the bar is BAR_FACTOR x the largest value the fp32 CPU emulation of "bilinear x2, then F(4x4) over both sources"
reaches on these cases (profiles/winof4_entries.md records it; tests/test_winof4_entry_host.py re-derives it).  No GPU."""
import functools
import os
import re

import numpy as np
import torch

from tests import conv_layer_cases as CL

PROFILE_NOTE = os.path.join(CL.ROOT, "profiles", "winof4_entries.md")
WINOF4_2SRC, WINOF4_UPS = 8, 9          # include/pnpx.h: enum pnpx_probe_kind
MIN_C0 = 8                              # conv3x3_winof4_entry_ok: one chunk of the first source

# (images, case).  The second source of the reference is the LOW-resolution tensor (H/2 x W/2), as the network has it; the kernel under test
# takes it up-sampled (upsample32: the separate up-sampling kernel's own arithmetic), so the reference covers both steps.
#   1 x (16+16) -> 64 @ 16 x 32: one region, the fewest chunks (two per source)
#   2 x (24+40) -> 128 @ 32 x 64: four regions per image (every interior region edge), two cout tiles, odd chunk counts: the source switch
#       falls on the other halo buffer than in the even cases
#   1 x (64+128) -> 64 @ 16 x 64: the network's 1:2 channel ratio
ENTRY_CASES = ((1, CL._c("ups", 16, 16, 64, 16, 32)), (2, CL._c("ups", 24, 40, 128, 32, 64)), (1, CL._c("ups", 64, 128, 64, 16, 64)))
B_ALL = 2                               # every case's inputs hold two images: an image alone against the image in a batch


@functools.lru_cache(maxsize=None)
def inputs(i):
    """fp32 operands of case i at B_ALL images; in1 is the low-resolution second source.  Never modified by the callers."""
    _, c = ENTRY_CASES[i]
    rs = np.random.RandomState(4100 + 13 * i)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    cin = c.C0 + c.C1
    return {"w": t(rs.standard_normal((c.cout, cin, 3, 3)) / np.sqrt(9.0 * cin)), "bias": t(0.1 * rs.standard_normal(c.cout)),
            "in0": t(rs.standard_normal((B_ALL, c.C0, c.H, c.W))), "in1": t(rs.standard_normal((B_ALL, c.C1, c.H // 2, c.W // 2)))}


def full_res(c, d):
    """The operands as the two-source kernel takes them: op "fwd", in1 up-sampled in fp32 by the up-sampling kernel's arithmetic."""
    return c._replace(op="fwd"), dict(d, in1=CL.upsample32(d["in1"], c.H, c.W))


@functools.lru_cache(maxsize=None)
def case_reference(i):
    """(ref, denom) in float64 from the low-resolution operands."""
    return CL.reference(ENTRY_CASES[i][1], inputs(i))


@functools.lru_cache(maxsize=None)
def emulation_maximum():
    """(largest measure of the fp32 emulation "bilinear x2, then F(4x4)" over the cases at their own batch, index of the case)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        worst, where = 0.0, None
        for i, (B, c) in enumerate(ENTRY_CASES):
            ref, den = case_reference(i)
            e = CL.measure(CL.emulate32(c, inputs(i), "f4")[:B], ref[:B], den[:B])
            if e > worst:
                worst, where = e, i
        return worst, where
    finally:
        torch.set_num_threads(threads)


def recorded_bar():
    """(emulation maximum, bar) as profiles/winof4_entries.md records them (table row `| f4_entry | max | bar | ...`)."""
    for line in open(PROFILE_NOTE):
        m = re.match(r"\|\s*f4_entry\s*\|\s*([0-9.eE+-]+)\s*\|\s*([0-9.eE+-]+)\s*\|", line)
        if m:
            return float(m.group(1)), float(m.group(2))
    raise AssertionError(f"{PROFILE_NOTE}: the f4_entry bar is missing")


def bar():
    return recorded_bar()[1]


def mutants(i):
    """[(name, mutated float64 reference)]: one weight zeroed, one element of either source zeroed, the result shifted by one pixel in x
    inside one 16-wide tile (conv_layer_cases.mutants' three), and the low-resolution source shifted by one pixel in x; each within the
    case's own first B images."""
    B, c = ENTRY_CASES[i]
    d = inputs(i)
    rs = np.random.RandomState(4200 + 13 * i)
    out = []
    w2 = d["w"].clone()
    w2[rs.randint(w2.shape[0]), rs.randint(w2.shape[1]), rs.randint(3), rs.randint(3)] = 0.0
    out.append(("weight_zeroed", CL.reference(c, dict(d, w=w2))[0]))
    src = "in1" if rs.randint(2) else "in0"
    x2 = d[src].clone()
    x2[rs.randint(B), rs.randint(x2.shape[1]), rs.randint(x2.shape[2]), rs.randint(x2.shape[3])] = 0.0
    out.append(("input_zeroed", CL.reference(c, dict(d, **{src: x2}))[0]))
    ref = CL.reference(c, d)[0]
    sh = ref.clone()
    b, y0, x0 = rs.randint(B), 16 * rs.randint(c.H // 16), 16 * rs.randint(c.W // 16)
    sh[b, :, y0:y0 + 16, x0 + 1:x0 + 16] = ref[b, :, y0:y0 + 16, x0:x0 + 15]
    out.append(("tile_shifted", sh))
    out.append(("low_source_shifted", CL.reference(c, dict(d, in1=torch.roll(d["in1"], 1, dims=3)))[0]))
    return out
