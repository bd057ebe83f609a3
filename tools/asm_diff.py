"""Per-kernel comparison of two device-assembly files of one translation unit (parent, new): instruction count, VGPR count, SGPR spills,
VGPR spills, scratch size, and every opcode whose count differs as opcode (parent, new), grouped by opcode class.  CPU only.

  asm_diff.py PARENT.s NEW.s [kernel-name substring]

The .s files come from the Makefile's compile line of the translation unit with `--cuda-device-only -S` in place of `-c`, e.g. from
tfpnp_amd/csrc:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include -Wall -Wno-unused-function \\
        -Xclang -target-feature -Xclang -packed-fp32-ops --cuda-device-only -S conv3x3_winof4.hip -o NEW.s
(and the same line in a checkout of the parent commit for PARENT.s)."""
import collections
import re
import sys

META = ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")


def kernels(path):
    """kernel name -> (opcode histogram, metadata)"""
    text = open(path).read()
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in META}
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M).group(1)
        ops = collections.Counter(m.group(1) for m in re.finditer(r"^\t([a-z][a-z0-9_]*)(?:\s|$)", body, re.M))
        out[name] = (ops, meta)
    return out


def klass(op):
    """the first two words of an opcode, `v_mfma`, `ds_read`, `global_load`, `s_waitcnt`: enough to tell vector, matrix, memory and scalar apart"""
    return "_".join(op.split("_")[:2])


def main(pa, pb, only=""):
    a, b = kernels(pa), kernels(pb)
    assert sorted(a) == sorted(b), set(a) ^ set(b)
    for name in sorted(a):
        if only not in name:
            continue
        (oa, ma), (ob, mb) = a[name], b[name]
        print(name)
        print(f"  instructions ({sum(oa.values())}, {sum(ob.values())})  " + "  ".join(f"{k} ({ma[k]}, {mb[k]})" for k in META))
        by = collections.defaultdict(list)
        for op in sorted(set(oa) | set(ob)):
            if oa[op] != ob[op]:
                by[klass(op)].append(f"{op} ({oa[op]}, {ob[op]})")
        for c in sorted(by):
            print(f"  {c}: " + ", ".join(by[c]))
        if not by:
            print("  every opcode count equal")
        same = sum(1 for c in set(map(klass, set(oa) | set(ob))) if c not in by)
        print(f"  opcode classes with equal counts: {same}; with a difference: {len(by)}")


if __name__ == "__main__":
    main(*sys.argv[1:4])
