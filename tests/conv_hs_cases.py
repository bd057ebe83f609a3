"""Cases, inputs, float64 references and the fp32 emulation of the half-split single-layer probe (pnpx_conv_hs_probe, csrc/conv_hs_probe.hip).

One CASE is one launch_conv_hs call: a geometry, an epilogue with its operands, and the conv_hs_kernel instance the launcher is expected to
pick for it (the plan, pnpx_conv_hs_probe_plan, is the authority: tests/test_conv_hs_host.py holds every case's `expect` against it).
Inputs are seeded, no fixture files; everything here is torch code that runs on whatever device its operands live on (the host tests: CPU;
tests/test_gpu_conv_hs.py: the references of the large cases on the GPU, in float64 matrix products).  No library and no GPU at import.

Layout "HS8": f16 tensor [B][C/8][H + 2][W + 2][16], a record = hi[8] | lo[8] with hi = f16(16 v), lo = f16(16 v - hi), zero border.
The float64 reference works on the DECODED inputs (hi + lo) / 16 and the fp32 weights.  The error measure is that of
tests/conv_layer_cases.py, per element:

    |y - ref| / (conv(|in|, |w|) + |bias| + |res|)

The bar of a class is BAR_FACTOR x the largest value the plain fp32 emulation of the half-split arithmetic reaches in that measure on the
first EMU_IMAGES images of the class's cases (profiles/conv_hs_probe.md records them; the host test re-derives them)."""
import collections
import os
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE_NOTE = os.path.join(ROOT, "profiles", "conv_hs_probe.md")
BAR_FACTOR = 8.0          # tests/conv_layer_cases.py: an fp32 sum moves with the summation order, and the MFMA's order is not the emulation's
EMU_IMAGES = 2            # images of a case the emulation runs on (fewer samples can only lower a maximum: the bar gets no wider)
ASCALE = 16.0             # csrc/conv_hs.h: HS_ASCALE
RANGE_LIMIT = 4095.0      # |value| the range guard reports (16 * 4095 rounds to the f16 infinity)

# csrc/conv_hs_kernel.h: enum HsEpi
EPI_CODE = {"act": 0, "outc": 1, "dmask": 2, "res": 3, "trelu": 4, "dthr": 5}
CLASSES = ("act", "outc", "dmask", "res", "trelu", "dthr", "ups", "first")

Case = collections.namedtuple(
    "Case", "name cls epi taps cin G0 G1 in0_groups cout H W B share pool wreg ups first res res_groups dmask slope alpha expect")


def _c(epi, cout, H, W, B, base, share=1, taps=0x1FF, cin=16, G1=0, in0_groups=0, pool=False, wreg=2, ups=False, first=False, res=False,
       res_groups=0, dmask=None, slope=0.2, alpha=0.0, tag=""):
    """base = (MT, NBW, MBW, NW, w_mt, plain_walk[, WREG]) the launcher is expected to pick; the rest of the instance follows the case."""
    G0 = (cin + 15) // 16 * 2 - G1
    dmask = (epi in ("dmask", "dthr")) if dmask is None else dmask
    cls = "ups" if ups else ("first" if first else epi)
    name = f"{epi}{taps:03x}_{cin}" + (f"+{G1 * 8}" if G1 else "") + f"to{cout}_{H}x{W}_B{B}" + (f"_s{share}" if share != 1 else "") + \
        ("_pool" if pool else "") + ("_ups" if ups else "") + ("_first" if first else "") + ("_res" if res else "") + \
        (f"_rg{res_groups}" if res_groups else "") + (f"_g{in0_groups}" if in0_groups else "") + (f"_w{wreg}" if wreg != 2 else "") + \
        (f"_sl{slope:g}" if slope != 0.2 else "") + (f"_a{alpha:g}" if epi in ("trelu", "dthr") else "") + \
        ("_nomask" if epi in ("dmask", "dthr") and not dmask else "") + tag
    wr = base[6] if len(base) > 6 else 0
    expect = base[:4] + (EPI_CODE[epi], int(ups), wr, taps, base[4], base[5])
    return Case(name, cls, epi, taps, cin, G0, G1, in0_groups, cout, H, W, B, share, pool, wreg, ups, first, res, res_groups, dmask, slope,
                alpha, expect)


# ---------------------------------------------------------------------------------------------------------------------------------
# The table.  Every row was written down from pnpx_conv_hs_probe_plan (the launcher's own decision), not from a restatement of its cost model.
#
# COVERAGE: the cheapest geometry of the sweep grid (sweep_grid) for each (MT, NBW, MBW, NW) the launcher can pick there; every
# epilogue / tap-mask combination runs on each of them, which is what makes "every instance the sweep finds" a run case.
#   (cout, H, W, B, share, pool) -> (MT, NBW, MBW, NW, w_mt, plain_walk)
COVERAGE = (
    ((32, 4, 4, 1, 1), (32, 2, 8, 4, 32, 1)),   # grid 1, 1 tiles
    ((32, 4, 4, 1, 2), (32, 1, 8, 8, 32, 1)),   # grid 1, 1 tiles
    ((32, 4, 16, 1, 1), (32, 2, 16, 4, 32, 1)),   # grid 1, 1 tiles
    ((32, 4, 16, 1, 2), (32, 1, 16, 8, 32, 1)),   # grid 1, 1 tiles
    ((32, 4, 32, 1, 1), (32, 2, 32, 4, 32, 1)),   # grid 1, 1 tiles
    ((32, 4, 32, 1, 2), (32, 1, 32, 8, 32, 1)),   # grid 1, 1 tiles
    ((32, 32, 40, 32, 2), (32, 2, 32, 8, 32, 1)),   # grid 128, 128 tiles
    ((32, 40, 40, 32, 1), (32, 4, 32, 4, 32, 1)),   # grid 192, 192 tiles
    ((32, 64, 24, 32, 2), (32, 2, 16, 8, 32, 1)),   # grid 128, 128 tiles
    ((32, 40, 24, 64, 1), (32, 4, 16, 4, 32, 1)),   # grid 128, 128 tiles
    ((32, 40, 12, 96, 1), (32, 4, 8, 4, 32, 1)),   # grid 192, 192 tiles
    ((64, 4, 4, 1, 1), (32, 1, 8, 4, 64, 1)),   # grid 2, 2 tiles
    ((64, 4, 16, 1, 1), (32, 1, 16, 4, 64, 1)),   # grid 2, 2 tiles
    ((64, 4, 32, 1, 1), (32, 1, 32, 4, 64, 1)),   # grid 2, 2 tiles
    ((64, 64, 40, 32, 1), (64, 4, 32, 4, 64, 1)),   # grid 256, 256 tiles
    ((128, 64, 4, 32, 2), (32, 2, 8, 8, 64, 1)),   # grid 128, 128 tiles
    ((128, 64, 24, 32, 1), (64, 4, 16, 4, 64, 1)),   # grid 256, 256 tiles
    ((192, 4, 24, 32, 1), (64, 1, 16, 4, 64, 1)),   # grid 192, 192 tiles
    ((192, 12, 24, 32, 1), (64, 2, 16, 4, 64, 1)),   # grid 192, 192 tiles
    ((192, 12, 24, 32, 2), (64, 1, 16, 8, 64, 1)),   # grid 192, 192 tiles
    ((192, 12, 40, 8, 1), (64, 1, 32, 4, 64, 1)),   # grid 144, 144 tiles
    ((192, 12, 40, 16, 1), (64, 2, 32, 4, 64, 1)),   # grid 192, 192 tiles
    ((192, 16, 40, 32, 2), (64, 2, 32, 8, 64, 1)),   # grid 192, 192 tiles
    ((192, 24, 40, 8, 2), (64, 1, 32, 8, 64, 1)),   # grid 144, 144 tiles
    ((192, 32, 24, 32, 2), (64, 2, 16, 8, 64, 1)),   # grid 192, 192 tiles
    ((192, 40, 4, 32, 1), (64, 2, 8, 4, 64, 1)),   # grid 192, 192 tiles
    ((192, 64, 4, 32, 2), (64, 1, 8, 8, 64, 1)),   # grid 192, 192 tiles
    ((512, 4, 4, 32, 1), (64, 1, 8, 4, 64, 1)),   # grid 256, 256 tiles
    ((512, 64, 4, 32, 1), (64, 4, 8, 4, 64, 1)),   # grid 256, 256 tiles
    ((512, 64, 4, 32, 2), (64, 2, 8, 8, 64, 1)),   # grid 256, 256 tiles
)
# epilogue / tap-mask combinations of the coverage rows (csrc/conv_hs_taps.hip, conv_hs_trelu.hip, conv_hs_dthr.hip: the compiled masks);
# the fused out-conv exists for 32-cout layers only
COMBOS = (("act", 0x1FF), ("act", 0x010), ("act", 0x01B), ("outc", 0x1FF), ("dmask", 0x1FF), ("res", 0x1FF), ("trelu", 0x1FF),
          ("trelu", 0x01B), ("dthr", 0x1FF), ("dthr", 0x1B0))
CRITIC_ALPHA = 0.3


def _coverage_cases():
    out = []
    for (cout, H, W, B, share), base in COVERAGE:
        for epi, taps in COMBOS:
            if epi == "outc" and cout != 32:
                continue
            out.append(_c(epi, cout, H, W, B, base, share=share, taps=taps, res=(epi == "res"),
                          alpha=CRITIC_ALPHA if epi in ("trelu", "dthr") else 0.0))
    return out


# EXTRAS: the persistent launches of every tile shape (cin stays 16 for the walk cases), the nct = 3 grid rounding (240 workgroups),
# a persistent launch with fewer than 32 regions, the pool cases, partial tiles both ways and heights below one tile, two sources,
# in0_groups above G0, zero-padded K, the weights-in-registers / folded-first / up-sampling instances, slopes, thresholds, wide K.
EXTRAS = (
    _c("act", 32, 40, 40, 32, (32, 1, 32, 8, 32, 0), share=2),   # grid 256, 320 tiles
    _c("act", 256, 24, 40, 3, (64, 1, 32, 4, 64, 1)),   # grid 144, 144 tiles
    _c("act", 128, 64, 40, 32, (64, 2, 32, 8, 64, 0)),   # grid 256, 512 tiles
    _c("act", 512, 4, 24, 32, (64, 1, 16, 4, 64, 0)),   # grid 256, 512 tiles
    _c("act", 512, 64, 12, 32, (64, 2, 8, 8, 64, 0)),   # grid 256, 512 tiles
    _c("act", 512, 4, 12, 32, (64, 1, 8, 4, 64, 0)),   # grid 256, 512 tiles
    _c("act", 192, 64, 40, 32, (64, 2, 32, 8, 64, 0)),   # grid 240, 768 tiles
    _c("act", 1024, 4, 4, 17, (64, 1, 8, 4, 64, 0)),   # grid 256, 272 tiles
    _c("act", 32, 4, 32, 1, (32, 2, 32, 4, 32, 1), pool=True),   # grid 1, 1 tiles
    _c("act", 32, 4, 32, 1, (32, 2, 32, 4, 32, 1), pool=True, share=2),   # grid 1, 1 tiles
    _c("act", 64, 4, 32, 1, (32, 2, 32, 4, 64, 1), pool=True),   # grid 2, 2 tiles
    _c("act", 32, 6, 40, 2, (32, 2, 32, 4, 32, 1), pool=True),   # grid 4, 4 tiles
    _c("act", 32, 40, 40, 32, (32, 4, 32, 4, 32, 1), pool=True),   # grid 192, 192 tiles
    _c("act", 64, 64, 40, 32, (64, 4, 32, 4, 64, 1), pool=True),   # grid 256, 256 tiles
    _c("act", 64, 12, 40, 32, (32, 2, 32, 8, 64, 1), pool=True, share=2),   # grid 128, 128 tiles
    _c("act", 192, 4, 40, 32, (64, 2, 32, 4, 64, 1), pool=True),   # grid 192, 192 tiles
    _c("act", 128, 64, 40, 32, (64, 2, 32, 8, 64, 0), pool=True),   # grid 256, 512 tiles
    _c("act", 32, 32, 40, 32, (32, 2, 32, 8, 32, 1), pool=True, share=2),   # grid 128, 128 tiles
    _c("act", 32, 5, 40, 2, (32, 2, 32, 4, 32, 1)),   # grid 4, 4 tiles
    _c("act", 64, 3, 40, 3, (32, 1, 32, 4, 64, 1)),   # grid 12, 12 tiles
    _c("act", 32, 13, 40, 3, (32, 1, 32, 8, 32, 1), share=2),   # grid 12, 12 tiles
    _c("act", 64, 7, 24, 2, (32, 1, 16, 4, 64, 1)),   # grid 8, 8 tiles
    _c("act", 64, 5, 12, 3, (32, 1, 8, 4, 64, 1)),   # grid 12, 12 tiles
    _c("act", 128, 9, 40, 2, (32, 1, 32, 4, 64, 1)),   # grid 48, 48 tiles
    _c("res", 64, 5, 40, 2, (32, 1, 32, 4, 64, 1), res=True),   # grid 16, 16 tiles
    _c("dmask", 32, 7, 40, 2, (32, 2, 32, 4, 32, 1)),   # grid 4, 4 tiles
    _c("trelu", 64, 3, 24, 2, (32, 1, 16, 4, 64, 1)),   # grid 8, 8 tiles
    _c("dthr", 64, 5, 12, 2, (32, 1, 8, 4, 64, 1)),   # grid 8, 8 tiles
    _c("act", 32, 8, 40, 2, (32, 2, 32, 4, 32, 1), cin=48, G1=2),   # grid 4, 4 tiles
    _c("act", 64, 8, 24, 2, (32, 1, 16, 4, 64, 1), cin=48, G1=4),   # grid 8, 8 tiles
    _c("act", 128, 5, 12, 2, (32, 1, 8, 4, 64, 1), cin=48, G1=2),   # grid 16, 16 tiles
    _c("act", 32, 8, 40, 2, (32, 2, 32, 4, 32, 1), in0_groups=4),   # grid 4, 4 tiles
    _c("trelu", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), in0_groups=6, taps=0x1b),   # grid 8, 8 tiles
    _c("act", 32, 8, 40, 2, (32, 2, 32, 4, 32, 1), cin=24),   # grid 4, 4 tiles
    _c("act", 64, 8, 16, 2, (32, 1, 16, 4, 64, 1), cin=8),   # grid 4, 4 tiles
    _c("act", 64, 8, 8, 2, (32, 1, 8, 4, 64, 1), cin=40, taps=0x10),   # grid 4, 4 tiles
    _c("act", 32, 20, 40, 64, (32, 4, 32, 4, 32, 1), cin=32, wreg=0),   # grid 256, 256 tiles
    _c("act", 32, 20, 40, 64, (32, 4, 32, 4, 32, 1, 1), cin=32, wreg=1),   # grid 256, 256 tiles
    _c("act", 32, 20, 40, 64, (32, 2, 32, 8, 32, 1, 1), cin=32, wreg=2),   # grid 256, 256 tiles
    _c("outc", 32, 20, 40, 64, (32, 4, 32, 4, 32, 1, 1), cin=32, wreg=1),   # grid 256, 256 tiles
    _c("outc", 32, 20, 40, 64, (32, 2, 32, 8, 32, 1, 1), cin=32, wreg=2),   # grid 256, 256 tiles
    _c("outc", 32, 20, 40, 64, (32, 4, 32, 4, 32, 1), cin=32, wreg=0),   # grid 256, 256 tiles
    _c("act", 32, 20, 40, 64, (32, 2, 32, 8, 32, 1, 2), cin=32, first=True),   # grid 256, 256 tiles
    _c("act", 32, 20, 40, 64, (32, 2, 32, 8, 32, 1, 2), cin=32, wreg=1, first=True),   # grid 256, 256 tiles
    _c("act", 32, 20, 40, 64, (32, 2, 32, 8, 32, 1, 1), cin=32, share=2),   # grid 256, 256 tiles
    _c("act", 32, 20, 40, 64, (32, 2, 32, 8, 32, 1, 1), cin=32, pool=True),   # grid 256, 256 tiles
    _c("outc", 32, 5, 40, 2, (32, 2, 32, 4, 32, 1)),   # grid 4, 4 tiles
    _c("outc", 32, 4, 8, 1, (32, 2, 8, 4, 32, 1)),   # grid 1, 1 tiles
    _c("act", 32, 2, 32, 1, (32, 2, 32, 8, 32, 1), cin=48, G1=2, ups=True),   # grid 1, 1 tiles
    _c("act", 64, 2, 32, 1, (64, 1, 32, 8, 64, 1), cin=48, G1=2, ups=True),   # grid 1, 1 tiles
    _c("act", 32, 18, 40, 2, (32, 2, 32, 8, 32, 1), cin=48, G1=2, ups=True),   # grid 8, 8 tiles
    _c("act", 64, 10, 40, 2, (64, 1, 32, 8, 64, 1), cin=64, G1=4, ups=True),   # grid 8, 8 tiles
    _c("act", 128, 18, 72, 3, (64, 1, 32, 8, 64, 1), cin=48, G1=2, ups=True),   # grid 54, 54 tiles
    _c("act", 32, 5, 40, 2, (32, 2, 32, 4, 32, 1), slope=0.0),   # grid 4, 4 tiles
    _c("dmask", 32, 7, 40, 2, (32, 2, 32, 4, 32, 1), slope=0.0),   # grid 4, 4 tiles
    _c("res", 64, 5, 40, 2, (32, 1, 32, 4, 64, 1), res=True, slope=0.0),   # grid 16, 16 tiles
    _c("act", 32, 5, 40, 2, (32, 2, 32, 4, 32, 1), slope=1.0),   # grid 4, 4 tiles
    _c("dmask", 32, 7, 40, 2, (32, 2, 32, 4, 32, 1), slope=1.0),   # grid 4, 4 tiles
    _c("res", 64, 5, 40, 2, (32, 1, 32, 4, 64, 1), res=True, slope=1.0),   # grid 16, 16 tiles
    _c("trelu", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=-0.25),   # grid 8, 8 tiles
    _c("dthr", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=-0.25),   # grid 8, 8 tiles
    _c("trelu", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.0),   # grid 8, 8 tiles
    _c("dthr", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.0),   # grid 8, 8 tiles
    _c("trelu", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.3),   # grid 8, 8 tiles
    _c("dthr", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.3),   # grid 8, 8 tiles
    _c("trelu", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.3, res=True),   # grid 8, 8 tiles
    _c("trelu", 128, 9, 40, 2, (32, 1, 32, 4, 64, 1), alpha=-0.25, res=True, taps=0x1b),   # grid 48, 48 tiles
    _c("dthr", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.3, res=True),   # grid 8, 8 tiles
    _c("dthr", 128, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.3, res=True, res_groups=8),   # grid 16, 16 tiles
    _c("dthr", 128, 9, 40, 2, (32, 1, 32, 4, 64, 1), alpha=-0.25, res=True, res_groups=4, taps=0x1b0),   # grid 48, 48 tiles
    _c("dthr", 64, 6, 24, 2, (32, 1, 16, 4, 64, 1), alpha=0.3, dmask=False),   # grid 8, 8 tiles
    _c("dthr", 512, 64, 4, 32, (64, 4, 8, 4, 64, 1), alpha=0.3, res=True, res_groups=16),   # grid 256, 256 tiles
    _c("act", 32, 8, 8, 1, (32, 2, 8, 4, 32, 1), cin=512),   # grid 1, 1 tiles
    _c("act", 64, 8, 8, 1, (32, 1, 8, 4, 64, 1), cin=512),   # grid 2, 2 tiles
    # the packing tiles and walks of the plain convolution the coverage rows leave out, and the out-conv's (2, 8) blocks of 8 pixels
    _c("act", 64, 24, 4, 64, (32, 1, 8, 8, 64, 1), share=2),   # grid 128, 128 tiles
    _c("act", 32, 40, 16, 96, (32, 1, 16, 8, 32, 0), share=2),   # grid 256, 288 tiles
    _c("act", 64, 12, 24, 32, (32, 1, 16, 8, 64, 1), share=2),   # grid 128, 128 tiles
    _c("act", 64, 4, 32, 1, (32, 1, 32, 8, 64, 1), share=2),   # grid 2, 2 tiles
    _c("act", 32, 40, 4, 128, (32, 2, 8, 8, 32, 1), share=2),   # grid 128, 128 tiles
    _c("act", 32, 64, 24, 96, (32, 2, 16, 8, 32, 0), share=2),   # grid 256, 384 tiles
    _c("act", 64, 32, 24, 32, (32, 2, 16, 8, 64, 1), share=2),   # grid 128, 128 tiles
    _c("act", 32, 40, 40, 32, (32, 2, 32, 4, 32, 0), share=2, pool=True),   # grid 256, 320 tiles
    _c("act", 32, 32, 40, 96, (32, 2, 32, 8, 32, 0), share=2),   # grid 256, 384 tiles
    _c("act", 192, 24, 4, 96, (64, 1, 8, 8, 64, 0), share=2),   # grid 240, 288 tiles
    _c("act", 128, 12, 24, 96, (64, 1, 16, 8, 64, 0), share=2),   # grid 256, 384 tiles
    _c("act", 192, 12, 40, 16, (64, 1, 32, 4, 64, 0), share=2),   # grid 240, 288 tiles
    _c("act", 192, 24, 40, 16, (64, 1, 32, 8, 64, 0), share=2),   # grid 240, 288 tiles
    _c("act", 64, 64, 24, 96, (64, 2, 16, 8, 64, 0), share=2),   # grid 256, 384 tiles
    _c("act", 128, 4, 40, 96, (64, 2, 32, 4, 64, 0), pool=True),   # grid 256, 384 tiles
    _c("outc", 32, 40, 4, 128, (32, 2, 8, 8, 32, 1), share=2),   # grid 128, 128 tiles
    # the persistent walk under the other epilogues
    _c("dmask", 512, 4, 12, 32, (64, 1, 8, 4, 64, 0)), _c("res", 512, 4, 12, 32, (64, 1, 8, 4, 64, 0), res=True),
    _c("trelu", 512, 4, 12, 32, (64, 1, 8, 4, 64, 0), alpha=0.3), _c("dthr", 512, 4, 12, 32, (64, 1, 8, 4, 64, 0), alpha=0.3),
)
CASES = tuple(_coverage_cases()) + EXTRAS
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES), [c.name for c in CASES if sum(k.name == c.name for k in CASES) > 1]
# instances no geometry can select, one line of reason each (tests/test_conv_hs_host.py: the sweep may skip only these)
EXEMPT = {}
FIRST_SLOPE = 0.2

# (B, H, W, ...) combinations the launcher itself refuses: PNPX_ERR_SHAPE, its own message, nothing launched, plan 0
REFUSED = (
    ("taps_with_res", dict(epi="act", cout=64, H=8, W=8, B=1, taps=0x010, res=True), "sparse-tap layers support"),
    ("critic_two_sources", dict(epi="trelu", cout=64, H=8, W=8, B=1, cin=32, G1=2), "the critic epilogues take one source"),
    ("outc_on_64_couts", dict(epi="outc", cout=64, H=8, W=8, B=1), "fused out-conv needs a 32-channel layer"),
    ("odd_G0", dict(epi="act", cout=32, H=8, W=8, B=1, cin=32, G1=1), "incompatible with packed layer"),
    ("ups_at_odd_H", dict(epi="act", cout=32, H=9, W=32, B=1, cin=48, G1=2, ups=True), "fused up-sampling is not available"),
)


def refused_case(kw):
    kw = dict(kw)
    return _c(kw.pop("epi"), kw.pop("cout"), kw.pop("H"), kw.pop("W"), kw.pop("B"), (0, 0, 0, 0, 0, 0), **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# HS8 encode / decode

def split(v):
    """fp32 (already scaled) -> (hi, lo) f16: hi = f16(v), lo = f16(v - hi)."""
    hi = v.half()
    return hi, (v - hi.float()).half()


def hs8_encode(x):
    """fp32 [B][C][H][W], C % 8 == 0 -> f16 [B][C/8][H + 2][W + 2][16] records with a zero border."""
    B, C, H, W = x.shape
    hi, lo = split(x.float() * ASCALE)
    r = torch.cat([hi.view(B, C // 8, 8, H, W), lo.view(B, C // 8, 8, H, W)], 2).permute(0, 1, 3, 4, 2)
    return F.pad(r, (0, 0, 1, 1, 1, 1)).contiguous()


def hs8_decode(r, dtype=torch.float64):
    """The interior of an HS8 tensor as values (hi + lo) / 16: [B][C][H][W]."""
    B, G, Hp, Wp, _ = r.shape
    ri = r[:, :, 1:-1, 1:-1]
    v = (ri[..., :8].to(dtype) + ri[..., 8:].to(dtype)) / ASCALE
    return v.permute(0, 1, 4, 2, 3).reshape(B, G * 8, Hp - 2, Wp - 2)


def hs8_border(r):
    """Every border record of an HS8 tensor, flat."""
    return torch.cat([r[:, :, 0].reshape(-1), r[:, :, -1].reshape(-1), r[:, :, :, 0].reshape(-1), r[:, :, :, -1].reshape(-1)])


def quantize(x, dtype=torch.float64):
    """What a kernel reads back from the HS8 encoding of x."""
    hi, lo = split(x.float() * ASCALE)
    return (hi.to(dtype) + lo.to(dtype)) / ASCALE


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

def inputs(c):
    """fp32 operands of a case in plain layouts (CPU): the HS8 operands are what hs8_encode is given.  Seeded by the case's name."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
    ntaps = bin(c.taps).count("1")
    d = {"w": rn(c.cout, c.cin, 3, 3) / float(np.sqrt(ntaps * c.cin))}
    if c.epi not in ("dmask", "dthr"):
        d["bias"] = 0.1 * rn(c.cout)
    h1, w1 = (c.H // 2, c.W // 2) if c.ups else (c.H, c.W)
    if c.first:
        d["first_x"] = ru(0.0, 1.0, c.B, c.H, c.W)
        d["first_sigma"] = ru(0.05, 0.2, c.B)
        d["first_w"] = rn(32, 2, 3, 3) / float(np.sqrt(18.0))
        d["first_b"] = 0.1 * rn(32)
    else:
        d["in0"] = rn(c.B, max(c.G0, c.in0_groups) * 8, c.H, c.W)
    if c.G1:
        d["in1"] = rn(c.B, c.G1 * 8, h1, w1)
    if c.res:
        d["res"] = rn(c.B, (c.res_groups or c.cout // 8) * 8, c.H, c.W)
    if c.dmask:
        # saved activations: nothing near the decision but the cells that sit exactly on it (the threshold itself, +0 and -0)
        centre = c.alpha if c.epi == "dthr" else 0.0
        sign = torch.where(torch.rand(c.B, c.cout, c.H, c.W, generator=g) < 0.5, -1.0, 1.0)
        m = centre + sign * ru(0.1, 1.0, c.B, c.cout, c.H, c.W)
        flat = m.view(c.B, -1)
        idx = torch.randint(0, flat.shape[1], (9,), generator=g)
        flat[:, idx[:3]] = centre
        flat[:, idx[3:6]] = 0.0
        flat[:, idx[6:]] = -0.0
        flat[:, 0], flat[:, 1], flat[:, 2] = centre, 0.0, -0.0
        d["dmask"] = m
    if c.epi == "outc":
        d["outc_w"] = rn(32) / float(np.sqrt(32.0))
        d["outc_b"] = 0.05 * rn(1)
        d["x_in"] = ru(0.0, 1.0, c.B, c.H, c.W)
    return d


def take(d, lo, hi):
    """The operands of images [lo, hi)."""
    per_image = ("in0", "in1", "res", "dmask", "x_in", "first_x", "first_sigma")
    return {k: (v[lo:hi] if k in per_image else v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference and the error measure

def conv3x3(x, w, taps=0x1FF, shift_tap=None):
    """Cross-correlation, zero padding 1, only the taps of the mask (bit dy * 3 + dx), as one matrix product per tap in the operands' own
    dtype and on their device.  shift_tap (a mutant): that tap reads one pixel further right."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (2, 2, 2, 2))
    out = None
    for t in range(9):
        if (taps >> t) & 1:
            dy, dx = divmod(t, 3)
            dx += 1 if shift_tap == t else 0
            term = torch.einsum("oc,bchw->bohw", w[:, :, t // 3, t % 3], xp[:, :, dy + 1:dy + 1 + H, dx + 1:dx + 1 + W])
            out = term if out is None else out + term
    return out


def _leaky(t, slope):
    return torch.where(t > 0, t, t * slope)


def threshold(alpha):
    """The kernel's TReLU threshold as the gradient epilogue reconstructs it: the value a stored split(16 alpha) reads back as."""
    return float(quantize(torch.tensor([alpha], dtype=torch.float32))[0])


def reference(c, d, device="cpu", shift_tap=None, swap_rows=None):
    """float64 results of a case on the operands d: {"out", "den"} (+ "pre", "img", "den_img" for the fused out-conv), computed from the
    DECODED HS8 operands and the fp32 weights.  shift_tap / swap_rows: the mutants."""
    dd = lambda k: d[k].to(device).double()
    q = lambda k: quantize(d[k].to(device))
    w = dd("w")
    if swap_rows:
        i, j = swap_rows
        w = w.clone()
        w[[i, j]] = w[[j, i]]
    if c.first:
        xs = torch.stack([dd("first_x"), dd("first_sigma").view(-1, 1, 1).expand(-1, c.H, c.W)], 1)
        fw = dd("first_w")
        x = _leaky(conv3x3(xs, fw) + dd("first_b").view(1, -1, 1, 1), FIRST_SLOPE)
        xa = conv3x3(xs.abs(), fw.abs()) + dd("first_b").abs().view(1, -1, 1, 1)
    else:
        x = q("in0")[:, :c.G0 * 8]
        xa = x.abs()
    if c.G1:
        x1 = q("in1")
        x1a = x1.abs()
        if c.ups:
            x1 = F.interpolate(x1, scale_factor=2, mode="bilinear", align_corners=True)
            x1a = F.interpolate(x1a, scale_factor=2, mode="bilinear", align_corners=True)
        x, xa = torch.cat([x, x1], 1), torch.cat([xa, x1a], 1)
    x, xa = x[:, :c.cin], xa[:, :c.cin]                 # K is zero-padded: channels past cin meet zero weights
    lin = conv3x3(x, w, c.taps, shift_tap)
    den = conv3x3(xa, w.abs(), c.taps)
    if "bias" in d:
        lin = lin + dd("bias").view(1, -1, 1, 1)
        den = den + dd("bias").abs().view(1, -1, 1, 1)
    if c.res:
        r = q("res")
        r = F.pad(r, (0, 0, 0, 0, 0, c.cout - r.shape[1]))       # res_groups below the output's: the first groups only
        lin, den = lin + r, den + r.abs()
    if c.epi in ("act", "res"):
        return {"out": _leaky(lin, float(np.float32(c.slope))), "den": den}
    if c.epi == "trelu":
        return {"out": torch.clamp(lin, min=float(np.float32(c.alpha))), "den": den + abs(c.alpha)}
    if c.epi == "dmask":
        f = torch.where(q("dmask") > 0, 1.0, float(np.float32(c.slope))) if c.dmask else 1.0
        return {"out": lin * f, "den": den}
    if c.epi == "dthr":
        f = (q("dmask") > threshold(c.alpha)).double() if c.dmask else 1.0
        return {"out": lin * f, "den": den}
    v = _leaky(lin, float(np.float32(c.slope)))
    ow = dd("outc_w").view(1, -1, 1, 1)
    pre = dd("x_in") + (v * ow).sum(1) + dd("outc_b")
    den_img = dd("x_in").abs() + (den * ow.abs()).sum(1) + dd("outc_b").abs()
    return {"out": v, "den": den, "pre": pre, "img": pre.clamp(0.0, 1.0), "den_img": den_img}


def measure(y, ref, den):
    """The per-element error measure; NaN anywhere = inf."""
    e = (y.double() - ref).abs() / den
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


def case_measure(c, got, ref):
    """The measure of a case's outputs (`got`: {"out"} or {"pre", "img"}, decoded) against reference(): the largest over its outputs."""
    if c.epi == "outc":
        return max(measure(got["pre"], ref["pre"], ref["den_img"]), measure(got["img"], ref["img"], ref["den_img"]))
    return measure(got["out"], ref["out"], ref["den"])


# ---------------------------------------------------------------------------------------------------------------------------------
# plain fp32 emulation of the half-split arithmetic (CPU)

def weight_halves(w):
    """pack_conv_weights_hs: the power-of-two scale s with s max|w| in [2^13, 2^14), and the f16 halves of s w as fp32 tensors."""
    mx = float(w.abs().max())
    s = 2.0 ** (14 - int(np.frexp(mx)[1])) if mx > 0 else 1.0
    hi, lo = split(w.float() * s)
    return s, hi.float(), lo.float()


def _halves(x):
    hi, lo = split(x.float() * ASCALE)
    return hi.float(), lo.float()


def _upsample32(v, H, W):
    from tests import conv_layer_cases as CL            # the kernels' own fp32 bilinear x2
    return CL.upsample32(v, H, W)


def emulate32(c, d, drop_cross_term=False):
    """The case in fp32 by the kernel's scheme: operands split in f16 halves, the three f16 x f16 products (exact in fp32) of every
    16-channel chunk and tap added into an fp32 accumulator in the kernel's K order, the fp32 epilogue, the output split again.
    Returns decoded outputs like the probe's.  drop_cross_term (a mutant): without the w_lo x_hi products."""
    f32 = torch.float32
    if c.first:
        xs = torch.stack([d["first_x"], d["first_sigma"].view(-1, 1, 1).expand(-1, c.H, c.W)], 1)
        a = F.conv2d(xs, d["first_w"], d["first_b"], padding=1)
        xh, xl = split(torch.maximum(a, a * FIRST_SLOPE) * ASCALE)
        xh, xl = xh.float(), xl.float()
    else:
        xh, xl = _halves(d["in0"][:, :c.G0 * 8])
    if c.G1:
        h1, l1 = _halves(d["in1"])
        if c.ups:                                       # interpolated in fp32 from hi + lo, split again
            h1, l1 = split(_upsample32(h1 + l1, c.H, c.W))
            h1, l1 = h1.float(), l1.float()
        xh, xl = torch.cat([xh, h1], 1), torch.cat([xl, l1], 1)
    s, wh, wl = weight_halves(d["w"])
    kpad = xh.shape[1] - c.cin
    wh, wl = F.pad(wh, (0, 0, 0, 0, 0, kpad)), F.pad(wl, (0, 0, 0, 0, 0, kpad))
    B, K, H, W = xh.shape
    xhp, xlp = F.pad(xh, (1, 1, 1, 1)), F.pad(xl, (1, 1, 1, 1))
    acc = torch.zeros(B, c.cout, H, W, dtype=f32)
    for k0 in range(0, K, 16):
        for t in range(9):
            if (c.taps >> t) & 1:
                dy, dx = divmod(t, 3)
                sl = (slice(None), slice(k0, k0 + 16), slice(dy, dy + H), slice(dx, dx + W))
                a_h, a_l = wh[:, k0:k0 + 16, dy, dx], wl[:, k0:k0 + 16, dy, dx]
                acc = acc + torch.einsum("oc,bchw->bohw", a_h, xhp[sl])
                acc = acc + torch.einsum("oc,bchw->bohw", a_h, xlp[sl])
                if not drop_cross_term:
                    acc = acc + torch.einsum("oc,bchw->bohw", a_l, xhp[sl])
    t = acc * (1.0 / s)                                 # a power of two: exact
    if "bias" in d:
        t = (t.double() + (d["bias"] * ASCALE).double().view(1, -1, 1, 1)).float()      # one fused multiply-add
    if c.res:
        rh, rl = _halves(d["res"])
        r = F.pad(rh + rl, (0, 0, 0, 0, 0, c.cout - rh.shape[1]))
        t = t + r
    if c.epi in ("act", "res", "outc"):
        v = torch.maximum(t, t * c.slope)
    elif c.epi == "trelu":
        v = torch.maximum(t, torch.tensor(c.alpha, dtype=f32) * ASCALE)
    elif c.epi == "dmask":
        v = torch.where(_halves(d["dmask"])[0] > 0, t, t * c.slope) if c.dmask else t
    else:
        mh, ml = _halves(d["dmask"]) if c.dmask else (None, None)
        v = torch.where(mh + ml > threshold(c.alpha) * ASCALE, t, torch.zeros_like(t)) if c.dmask else t
    if c.epi == "outc":
        ow = d["outc_w"]
        parts = []
        for half in (0, 16):                            # a lane's 16 channels in order, the two lane halves added last
            p = torch.zeros(B, H, W, dtype=f32)
            for r_ in range(16):
                p = p + ow[half + r_] * v[:, half + r_]
            parts.append(p)
        pre = d["x_in"] + ((parts[0] + parts[1]) * (1.0 / ASCALE) + d["outc_b"])
        return {"pre": pre, "img": pre.clamp(0.0, 1.0)}
    hi, lo = split(v)
    return {"out": (hi.double() + lo.double()) / ASCALE}


def emulation_maxima():
    """{class: (largest measure of the emulation over the first EMU_IMAGES images of the class's cases, the case it was found at)}."""
    out = {cls: (0.0, None) for cls in CLASSES}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)       # an fp32 sum must not move with the number of threads the host happens to have
    try:
        for c in CASES:
            d = take(inputs(c), 0, EMU_IMAGES)
            e = case_measure(c, emulate32(c, d), reference(c, d))
            if e > out[c.cls][0]:
                out[c.cls] = (e, c.name)
    finally:
        torch.set_num_threads(threads)
    return out


def recorded_bars():
    """{class: (emulation maximum, bar)} as profiles/conv_hs_probe.md records them (table rows `| class | max | bar | ...`)."""
    out = {}
    for line in open(PROFILE_NOTE):
        m = re.match(r"\|\s*(" + "|".join(CLASSES) + r")\s*\|\s*([0-9.eE+-]+)\s*\|\s*([0-9.eE+-]+)\s*\|", line)
        if m:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    assert set(out) == set(CLASSES), f"{PROFILE_NOTE}: bars of {sorted(set(CLASSES) - set(out))} missing"
    return out


def bar(cls):
    return recorded_bars()[cls][1]


# mutants the bars must catch (tests/test_conv_hs_host.py), each on one small case of the class
MUTANT_CASES = {"act": "act1ff_16to32_5x40_B2", "outc": "outc1ff_16to32_5x40_B2", "dmask": "dmask1ff_16to32_7x40_B2",
                "res": "res1ff_16to64_5x40_B2_res", "trelu": "trelu1ff_16to64_6x24_B2_a0.3", "dthr": "dthr1ff_16to64_6x24_B2_a0.3",
                "ups": "act1ff_48+16to32_18x40_B2_ups", "first": "act1ff_32to32_20x40_B64_first"}
SWAPPED_ROWS = (4, 16)     # hs_row_channel(4) = 16: the pair a packer that ignored the permutation would exchange


def mutants(c, d):
    """[(name, outputs)]: the emulation without its w_lo x_hi products; the reference with one tap of the layer shifted by a pixel; the
    reference with two weight rows exchanged."""
    tap = [t for t in range(9) if (c.taps >> t) & 1][0]
    return [("cross_term_dropped", emulate32(c, d, drop_cross_term=True)), ("tap_shifted", reference(c, d, shift_tap=tap)),
            ("rows_exchanged", reference(c, d, swap_rows=SWAPPED_ROWS))]


# ---------------------------------------------------------------------------------------------------------------------------------
# the probe's descriptor and the plan

def descriptor(c, ptr, B=None):
    """pnpx_conv_hs_probe_desc of a case; ptr: operand name -> address (device tensors, host arrays).  An operand the case has but ptr
    lacks is an error; one the case lacks stays null."""
    from tfpnp_amd import _lib
    D = _lib.ConvHsProbeDesc()
    names = ["w"] + (["bias"] if c.epi not in ("dmask", "dthr") else []) + ([] if c.first else ["in0"]) + (["in1"] if c.G1 else []) + \
        (["res"] if c.res else []) + (["dmask"] if c.dmask else []) + (["pool_out"] if c.pool else []) + \
        (["outc_w", "outc_b", "x_in", "out_img", "out_pre"] if c.epi == "outc" else ["out"]) + \
        (["first_x", "first_sigma", "first_w", "first_b"] if c.first else [])
    for n in names:
        setattr(D, n, ptr[n])
    D.cin, D.cout, D.G0, D.G1, D.B, D.H, D.W = c.cin, c.cout, c.G0, c.G1, (c.B if B is None else B), c.H, c.W
    D.slope, D.taps, D.in0_groups, D.wreg, D.share = c.slope, c.taps, c.in0_groups, c.wreg, c.share
    D.ups_h, D.ups_w = (c.H // 2, c.W // 2) if c.ups else (0, 0)
    D.critic_epi = {"trelu": 1, "dthr": 2}.get(c.epi, 0)
    D.alpha, D.res_groups = c.alpha, c.res_groups
    D.first_sigma_stride, D.first_slope = (1, FIRST_SLOPE) if c.first else (0, 0.0)
    return D


class _Present(dict):
    def __missing__(self, key):
        return 1           # the plan dereferences nothing: non-null = present


def plan(c, B=None, H=None, W=None):
    """What the probe's call would launch, from the library's host-only plan: (MT, NBW, MBW, NW, EPI, UPS, WREG, TAPS, w_mt, grid, tiles,
    plain_walk), or None when the probe or the launcher refuses."""
    import ctypes as C
    from tfpnp_amd import _lib
    if H is not None or W is not None:
        c = c._replace(H=c.H if H is None else H, W=c.W if W is None else W)
    D = descriptor(c, _Present(), B)
    out = (C.c_int * _lib.PNPX_CONV_HS_PLAN_INTS)()
    ok = _lib.lib().pnpx_conv_hs_probe_plan(C.byref(D), D.B, D.H, D.W, out)
    return tuple(out) if ok else None


def expected(p):
    """A plan in the form of Case.expect: (MT, NBW, MBW, NW, EPI, UPS, WREG, TAPS, w_mt, plain_walk)."""
    return p[:9] + (p[11],)


SWEEP_B = (1, 2, 3, 4, 8, 16, 32, 64, 96, 128)       # (4, 4) blocks of the 8- and 16-pixel 32-cout tiles need more than 64 images
SWEEP_HW = (4, 8, 12, 16, 24, 32, 40, 64)
SWEEP_COUT = (32, 64, 128, 192, 256, 512)


def sweep_grid():
    """The coverage condition's grid: every epilogue / tap-mask combination x cout x H x W x B x share x pool (where a pool can be fused),
    cin 16; and, for the instances only wider layers reach, the 32 -> 32 layers with each `wreg` (plain, out-conv, folded first
    convolution) and the two-source layers with the second source up-sampled, over the same B x H x W."""
    for epi, taps in COMBOS:
        for cout in SWEEP_COUT:
            if epi == "outc" and cout != 32:
                continue
            for H in SWEEP_HW:
                for W in SWEEP_HW:
                    for B in SWEEP_B:
                        for share in (1, 2):
                            for pool in ((False, True) if (epi, taps) == ("act", 0x1FF) and W >= 32 else (False,)):
                                yield _c(epi, cout, H, W, B, (0,) * 6, share=share, taps=taps, pool=pool, res=(epi == "res"))
    for H in SWEEP_HW:
        for W in SWEEP_HW:
            for B in SWEEP_B:
                for wreg in (0, 1, 2):
                    yield _c("act", 32, H, W, B, (0,) * 6, cin=32, wreg=wreg)
                    yield _c("outc", 32, H, W, B, (0,) * 6, cin=32, wreg=wreg)
                    if wreg:
                        yield _c("act", 32, H, W, B, (0,) * 6, cin=32, wreg=wreg, first=True)
                for cout in (32, 64, 128):
                    yield _c("act", cout, H, W, B, (0,) * 6, cin=48, G1=2, ups=True)
