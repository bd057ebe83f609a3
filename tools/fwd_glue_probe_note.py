"""Writes profiles/fwd_glue_probe.md: the derived bars of the probe of the launches between the denoisers' forward convolutions from the fp32
emulations (CPU), and the largest measures of a GPU run.

  python tools/fwd_glue_probe_note.py [GPU_LOG]

GPU_LOG: the output of `pytest tests/test_gpu_fwd_glue.py -s` (its `fwd_glue_probe <key> <case> ... measure <m> bar <b>` lines); without it
the GPU columns of an existing note are kept."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fwd_glue_cases as FG  # noqa: E402

FIXED = (("ups_f32_a", FG.UPS_TIER_A, "6 x 2^-24: at most 5 roundings on the longest path of hy (hx v00 + lx v01) + ly (hx v10 + lx v11), one for second order"),
         ("ups_hs_a", FG.UPS_TIER_A_HS, "11 x 2^-24: the same, the hi + lo split of the record (4 x 2^-24) and lo's subnormal step"),
         ("impulse_f32", FG.IMPULSE_BAR, "3 x 2^-24 of w_y w_x: one product (a clamped end adds hx + lx); zeros of the tables are exact zeros"),
         ("impulse_hs", FG.IMPULSE_BAR_HS, "7 x 2^-24 beyond an absolute 2^-29: the same plus the record's split and the f16 subnormal half-step"),
         ("sigma_part", None, "k x 2^-24 of the sum of abs(terms), k = serial + 6 + 2 (`sigma_depth`); the column holds the largest error / bar"),
         ("sigma_final", None, "k x 2^-24 of the sum of abs(terms), k = serial + 6 + 2 + 64; the column holds the largest error / bar"))


def gpu_maxima(path):
    out = {}
    for line in open(path):
        m = re.search(r"fwd_glue_probe (\w+) (\S+) .*measure ([0-9.eE+-]+) bar", line)
        if m and float(m.group(3)) >= out.get(m.group(1), (-1.0, ""))[0]:
            out[m.group(1)] = (float(m.group(3)), m.group(2))
    return out


def kept_gpu_column():
    out = {}
    if os.path.exists(FG.PROFILE_NOTE):
        for line in open(FG.PROFILE_NOTE):
            m = re.match(r"\|\s*(\w+)\s*\|.*\|\s*([0-9.eE+-]+)\s*\|\s*(\S+)\s*\|\s*$", line)
            if m and m.group(3) != "-":
                out[m.group(1)] = (float(m.group(2)), m.group(3))
    return out


def main(argv):
    gpu = gpu_maxima(argv[1]) if len(argv) > 1 else kept_gpu_column()
    emu = FG.emulation_maxima()
    L = []
    w = L.append
    col = lambda k: ("%.4e | %s" % gpu[k]) if k in gpu else "- | -"
    w("# Forward glue of the denoisers: the single-launch probe (`pnpx_fwd_glue_probe`)\n")
    w("Written by `tools/fwd_glue_probe_note.py`; read by `tests/fwd_glue_cases.py` (`recorded_bars`), re-derived by")
    w("`tests/test_fwd_glue_host.py`.  Measures are per element.  `first_*` (the first convolution on the vector ALU): `|y - ref| / (sum |w f| +")
    w("|b|)` against float64 `leaky_relu(conv2d)`.  `outc_*` (1 x 1 out-conv + residual, before the clamp; the clamped image takes the same")
    w("bar, the clamp being a contraction): `|y - ref| / (sum |w f| + |b| + |x|)`.  `ups_*` (bilinear x2, tier (b)): `|y - ref| / sum |w_y w_x v|`")
    w("against float64 `F.interpolate(align_corners=True)`.  Each bar = `BAR_FACTOR` (%g) x the largest measure of the fp32 CPU emulation of the" % FG.BAR_FACTOR)
    w("kernel (its fma chain in its order; half-split: the records' hi + lo rounding of the output, inputs decoded from records) over the")
    w("class's cases.  No bar was set from a GPU figure.  The up-sampling weights mirror each kernel as compiled (`ups_contracted`): the")
    w("scalar fp32 kernel and the half-split instances get `l = s * d - i0` as one fma from the build's default contraction, the")
    w("four-outputs-per-thread fp32 kernel keeps `l = fp32(s * d) - i0`; the tables (`weight_table` of `tests/vjp_glue_cases.py`) differ by")
    w("up to 2^-24 per unit of the index, which is what sets `ups_f32` apart from `ups_hs`.\n")
    w("GPU columns: the largest measure in `tests/test_gpu_fwd_glue.py` on an MI355X over every form run (`-` = not run yet).\n")
    w("| key | emulation max | bar | emulation case | GPU max | GPU case |")
    w("|---|---|---|---|---|---|")
    for k in FG.BAR_KEYS:
        mx, where = emu[k]
        w(f"| {k} | {mx:.4e} | {FG.BAR_FACTOR * mx:.4e} | {where} | {col(k)} |")
    w("\nBars that are not derived from an emulation:\n")
    w("| key | bar | from | GPU max | GPU case |")
    w("|---|---|---|---|---|")
    for k, b, why in FIXED:
        w(f"| {k} | {'%.4e' % b if b else 'k x 2^-24'} | {why} | {col(k)} |")
    w("\nThe exact ops (input preparation, pooling, both re-layouts, the skip sum, the fp32 tail's output and mask, the image half of the")
    w("DRUNet's input gradient) carry no measure: the GPU result is bit-identical to a torch restatement (half-split pooling: equal decoded")
    w("values; the sign of a zero that comes out of a clamp, and of a zero lo half of a prepared input record, is not compared).")
    open(FG.PROFILE_NOTE, "w").write("\n".join(L) + "\n")
    print(f"{FG.PROFILE_NOTE}: " + ", ".join(f"{k} {FG.BAR_FACTOR * emu[k][0]:.3e}" for k in FG.BAR_KEYS))


if __name__ == "__main__":
    main(sys.argv)
