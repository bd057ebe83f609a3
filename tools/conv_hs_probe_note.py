"""Writes profiles/conv_hs_probe.md: the class bars of the half-split single-layer probe from the fp32 emulation (CPU), the largest measure
of each class in a GPU run, and the instance-to-case coverage table.

  python tools/conv_hs_probe_note.py [GPU_LOG]

GPU_LOG: the output of `pytest tests/test_gpu_conv_hs.py -s` (its `conv_hs_probe <class> <case> ... measure <m> bar <b>` lines); without
it the GPU column of an existing note is kept."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import conv_hs_cases as HS  # noqa: E402

EPI = {v: k for k, v in HS.EPI_CODE.items()}


def gpu_maxima(path):
    out = {}
    for line in open(path):
        m = re.search(r"conv_hs_probe (\w+) (\S+) instance .* measure ([0-9.eE+-]+) bar", line)
        if m and float(m.group(3)) >= out.get(m.group(1), (-1.0, ""))[0]:
            out[m.group(1)] = (float(m.group(3)), m.group(2))
    return out


def kept_gpu_column():
    out = {}
    if os.path.exists(HS.PROFILE_NOTE):
        for line in open(HS.PROFILE_NOTE):
            m = re.match(r"\|\s*(\w+)\s*\|[^|]*\|[^|]*\|[^|]*\|[^|]*\|\s*([0-9.eE+-]+)\s*\|\s*(\S+)\s*\|", line)
            if m and m.group(1) in HS.CLASSES:
                out[m.group(1)] = (float(m.group(2)), m.group(3))
    return out


def main(argv):
    gpu = gpu_maxima(argv[1]) if len(argv) > 1 else kept_gpu_column()
    emu = HS.emulation_maxima()
    L = []
    w = L.append
    w("# Half-split convolution: the single-layer probe (`pnpx_conv_hs_probe`)\n")
    w("Written by `tools/conv_hs_probe_note.py`; read by `tests/conv_hs_cases.py` (`recorded_bars`), re-derived by")
    w("`tests/test_conv_hs_host.py`.  Measure: per element `|y - ref| / (conv(|in|, |w|) + |bias| + |res|)` against a float64 reference of")
    w("the decoded HS8 operands.  Bar of a class = `BAR_FACTOR` (%g) x the largest measure of the plain fp32 emulation of the half-split" % HS.BAR_FACTOR)
    w("arithmetic (operand split, three f16 x f16 products, fp32 accumulation in the kernel's K order, fp32 epilogue, output split) on the")
    w("first %d images of the class's cases, on the CPU.  No bar was changed after a GPU run; no class needed a lower factor for its" % HS.EMU_IMAGES)
    w("mutants (a dropped `w_lo x_hi` term, a tap shifted by a pixel, two weight rows exchanged: 40 x the bar and more).\n")
    w("GPU column: the largest measure of the class in `tests/test_gpu_conv_hs.py` on an MI355X (`-` = not run yet).\n")
    w("| class | emulation max | bar | emulation case | cases | GPU max | GPU case |")
    w("|---|---|---|---|---|---|---|")
    for cls in HS.CLASSES:
        mx, where = emu[cls]
        g = gpu.get(cls)
        n = sum(c.cls == cls for c in HS.CASES)
        w(f"| {cls} | {mx:.4e} | {HS.BAR_FACTOR * mx:.4e} | {where} | {n} | {'%.4e' % g[0] if g else '-'} | {g[1] if g else '-'} |")
    w("\n## Coverage\n")
    w("Sweep (`tests/conv_hs_cases.py: sweep_grid`): B in %s, H and W in %s, cout in %s, share 1 / 2, fused pool on / off, every" % (HS.SWEEP_B, HS.SWEEP_HW, HS.SWEEP_COUT))
    w("epilogue and tap mask at cin 16; plus the 32 -> 32 layers with each `wreg` (plain, out-conv, folded first convolution) and the")
    w("two-source layers with the second source up-sampled.  Every instance the sweep finds is run by the case below (the cheapest one")
    w("of the table that selects it; `tests/test_conv_hs_host.py` asserts the inclusion).  Before this probe none of them was compared to")
    w("a reference on its own.\n")
    w("Exemptions (instances the launcher provably cannot select): %s.\n" % ("none" if not HS.EXEMPT else ""))
    for k, why in HS.EXEMPT.items():
        w(f"- `{k}`: {why}")
    by = collections.OrderedDict()
    for c in sorted(HS.CASES, key=lambda c: c.cout * c.H * c.W * c.B):
        by.setdefault(c.expect[:8], []).append(c)
    w("| MT | NBW | MBW | NW | EPI | UPS | WREG | TAPS | case | packing tiles, walks run |")
    w("|---|---|---|---|---|---|---|---|---|---|")
    for k in sorted(by):
        cs = by[k]
        walks = sorted({(c.expect[8], "plain" if c.expect[9] else "persistent") for c in cs})
        w("| %d | %d | %d | %d | %s | %d | %d | 0x%03x | %s | %s |" % (k[0], k[1], k[2], k[3], EPI[k[4]], k[5], k[6], k[7], cs[0].name,
                                                                ", ".join(f"{a} {b}" for a, b in walks)))
    w(f"\n{len(by)} instances, {len(HS.CASES)} cases.")
    open(HS.PROFILE_NOTE, "w").write("\n".join(L) + "\n")
    print(f"{HS.PROFILE_NOTE}: {len(by)} instances, {len(HS.CASES)} cases")


if __name__ == "__main__":
    main(sys.argv)
