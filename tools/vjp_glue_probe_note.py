"""Writes profiles/vjp_glue_probe.md: the derived bars of the probe of the launches between the UNet VJP's adjoint convolutions from the fp32
emulations (CPU), and the largest measures of a GPU run.

  python tools/vjp_glue_probe_note.py [GPU_LOG]

GPU_LOG: the output of `pytest tests/test_gpu_vjp_glue.py -s` (its `vjp_glue_probe <key> <case> ... measure <m> bar <b>` lines); without it
the GPU columns of an existing note are kept."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vjp_glue_cases as VG  # noqa: E402

FIXED = (("ups_f32_a", VG.UPS_TIER_A, "12 x 2^-24: at most 9 terms of two products, 8 additions, the final factor"),
         ("ups_hs_a", VG.UPS_TIER_A, "the same, on the decoded records"),
         ("sigma_part", None, "k x 2^-24 of the sum of abs(terms), k = serial + 6 + 2 (`sigma_depth`); the column holds the largest error / bar"),
         ("sigma_final", None, "k x 2^-24 of the sum of abs(terms), k = serial + 6 + 2 + 64; the column holds the largest error / bar"))


def gpu_maxima(path):
    out = {}
    for line in open(path):
        m = re.search(r"vjp_glue_probe (\w+) (\S+) .*measure ([0-9.eE+-]+) bar", line)
        if m and float(m.group(3)) >= out.get(m.group(1), (-1.0, ""))[0]:
            out[m.group(1)] = (float(m.group(3)), m.group(2))
    return out


def kept_gpu_column():
    out = {}
    if os.path.exists(VG.PROFILE_NOTE):
        for line in open(VG.PROFILE_NOTE):
            m = re.match(r"\|\s*(\w+)\s*\|.*\|\s*([0-9.eE+-]+)\s*\|\s*(\S+)\s*\|\s*$", line)
            if m and m.group(3) != "-":
                out[m.group(1)] = (float(m.group(2)), m.group(3))
    return out


def main(argv):
    gpu = gpu_maxima(argv[1]) if len(argv) > 1 else kept_gpu_column()
    emu = VG.emulation_maxima()
    L = []
    w = L.append
    col = lambda k: ("%.4e | %s" % gpu[k]) if k in gpu else "- | -"
    w("# Denoiser VJP glue: the single-launch probe (`pnpx_vjp_glue_probe`)\n")
    w("Written by `tools/vjp_glue_probe_note.py`; read by `tests/vjp_glue_cases.py` (`recorded_bars`), re-derived by")
    w("`tests/test_vjp_glue_host.py`.  Up-sampling adjoint: per element `|y - ref| / sum |w_y w_x g|` over the contributing destination")
    w("pixels.  Tier (b) (`ups_f32`, `ups_hs`): ref = float64 autograd of the forward op; bar = `BAR_FACTOR` (%g) x the largest measure of" % VG.BAR_FACTOR)
    w("the fp32 CPU emulation of the kernel (the 7 x 7 candidate loop in its order; half-split: 16 x the decoded values, the result split")
    w("into hi + lo) over `UPS_CASES`.  `adjoint`: `|<up(x), g> - <x, up_bwd(g)>| / <|up(x)|, |g|>` with both inner products in float64;")
    w("bar = `BAR_FACTOR` x what the fp32 emulations of the two sides show over `UPS_ADJOINT_CASES`.  No bar was set from a GPU figure.  The")
    w("weight table of the references and the emulation (`weight_table`) mirrors the kernels as compiled: the build's default contraction")
    w("fuses `l = s * d - i0` into one fma, so `l` is rounded once.  A build without contraction would sit an absolute 2^-24 per unit of")
    w("the index from that table (14 x the tier-(a) bar at 130 columns) and is told apart by `weight_table(n, contracted=False)`.\n")
    w("GPU columns: the largest measure in `tests/test_gpu_vjp_glue.py` on an MI355X over every form run (`-` = not run yet).\n")
    w("| key | emulation max | bar | emulation case | GPU max | GPU case |")
    w("|---|---|---|---|---|---|")
    for k in VG.BAR_KEYS:
        mx, where = emu[k]
        w(f"| {k} | {mx:.4e} | {VG.BAR_FACTOR * mx:.4e} | {where} | {col(k)} |")
    w("\nBars that are not derived from an emulation:\n")
    w("| key | bar | from | GPU max | GPU case |")
    w("|---|---|---|---|---|")
    for k, b, why in FIXED:
        w(f"| {k} | {'%.4e' % b if b else 'k x 2^-24'} | {why} | {col(k)} |")
    w("\nThe single-product ops (out-conv tail, both fp32 skip / pool forms, the image half of the input gradient, and their half-split")
    w("forms) carry no measure: the GPU result is bit-identical to the fp32 restatement, which the host test holds within 3 x 2^-24 of the")
    w("float64 autograd reference.  The gradient scale is compared bit for bit with the pair `frexp` gives.")
    open(VG.PROFILE_NOTE, "w").write("\n".join(L) + "\n")
    print(f"{VG.PROFILE_NOTE}: " + ", ".join(f"{k} {VG.BAR_FACTOR * emu[k][0]:.3e}" for k in VG.BAR_KEYS))


if __name__ == "__main__":
    main(sys.argv)
