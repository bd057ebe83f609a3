"""Writes profiles/net_train_probe.md: the derived bars of the probe of the actor's and the critic's training kernels from the fp32
emulations (CPU), the fixed bars with their rounding counts, and the largest measures of a GPU run.

  python tools/net_train_probe_note.py [GPU_LOG]

GPU_LOG: the output of `pytest tests/test_gpu_net_train.py -s` (its `net_train_probe <key> <case> ... measure <m> bar <b>` lines); without
it the GPU columns of an existing note are kept."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import net_train_cases as NT  # noqa: E402


def gpu_maxima(path):
    out = {}
    for line in open(path):
        m = re.search(r"net_train_probe (\w+) (\S+) .*measure ([0-9.eE+-]+) bar", line)
        if m and float(m.group(3)) >= out.get(m.group(1), (-1.0, ""))[0]:
            out[m.group(1)] = (float(m.group(3)), m.group(2))
    return out


def kept_gpu_column():
    out = {}
    if os.path.exists(NT.PROFILE_NOTE):
        for line in open(NT.PROFILE_NOTE):
            m = re.match(r"\|\s*(\w+)\s*\|.*\|\s*([0-9.eE+-]+)\s*\|\s*(\S+)\s*\|\s*$", line)
            if m and m.group(3) != "-":
                out[m.group(1)] = (float(m.group(2)), m.group(3))
    return out


def main(argv):
    gpu = gpu_maxima(argv[1]) if len(argv) > 1 else kept_gpu_column()
    emu = NT.emulation_maxima()
    L = []
    w = L.append
    col = lambda k: ("%.4e | %s" % gpu[k]) if k in gpu else "- | -"
    w("# Training kernels of the actor and the critic: the single-launch probe (`pnpx_net_train_probe`)\n")
    w("Written by `tools/net_train_probe_note.py`; read by `tests/net_train_cases.py` (`recorded_bars`), re-derived by")
    w("`tests/test_net_train_host.py`.  Measures are per element: `|y - ref|` over the sum of the magnitudes of the terms the output was added")
    w("up from, against float64 references (autograd through `F.batch_norm(training=True)` behind the ReLU mask, through `conv2d` and")
    w("weight-norm, through the heads).  Each derived bar = `BAR_FACTOR` (%g) x the largest measure of the fp32 CPU emulation of the kernel in" % NT.BAR_FACTOR)
    w("its own operation order over the class's cases: `bn_apply` `(z - mean) * scale + beta` in that order; `bn_bwd_dz` the coefficients")
    w("from the fp32 statistics in double, `A dy - c1 - c2 (z - mean)` in fp32; `wgrad*` fp32 fma chains per K-split piece in pixel order")
    w("(the gradient operand times `gv[b]` rounded first), the pieces added in double, the finishing kernel in double; `head_*` the fma")
    w("chains of `pol_head_grad_kernel`; HS8 outputs through `hs8_encode`.  No bar was set from a GPU figure.  `wgrad_wn_*` and `head_param`")
    w("are sums in double OF fp32-chain values (the slab, the head rows), so they inherit those values' error and are derived, not fixed.\n")
    w("GPU columns: the largest measure in `tests/test_gpu_net_train.py` on an MI355X (`-` = not run yet).\n")
    w("| key | emulation max | bar | emulation case | GPU max | GPU case |")
    w("|---|---|---|---|---|---|")
    for k in NT.DERIVED_KEYS:
        mx, where = emu[k]
        w(f"| {k} | {mx:.4e} | {NT.BAR_FACTOR * mx:.4e} | {where} | {col(k)} |")
    w("\nFixed bars (accumulation in double, one store to fp32), in units of 2^-24:\n")
    w("| key | bar | roundings on the longest path | GPU max | GPU case |")
    w("|---|---|---|---|---|")
    for k, (n, why) in NT.FIXED_BARS.items():
        w(f"| {k} | {n} x 2^-24 = {n * NT.U:.4e} | {why} | {col(k)} |")
    w(f"| double_out | 2^-40 = {NT.DOUBLE_BAR:.4e} | outputs left in double (`ALPHA_DOT`, the head threshold's shares of `FC_GRAD`): at most 2^12 "
      f"exact products, 2^-53 a step | {col('double_out')} |")
    w("\nThe exact ops carry no measure: `CLIP_MASK`, `dy_out`, the space-to-depth copy against `out`, the zeros in the running-statistics")
    w("slots of a BatchNorm gradient, and the slot and `gv` of `GRAD_SEED` are bit-identical to a torch restatement.")
    open(NT.PROFILE_NOTE, "w").write("\n".join(L) + "\n")
    print(f"{NT.PROFILE_NOTE}: " + ", ".join(f"{k} {NT.BAR_FACTOR * emu[k][0]:.3e}" for k in NT.DERIVED_KEYS))


if __name__ == "__main__":
    main(sys.argv)
