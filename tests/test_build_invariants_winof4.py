"""Invariants of the Winograd F(4x4,3x3) kernels' device code (csrc/conv3x3_winof4.hip), checked on the CPU in libpnpx.so's gfx950 code
objects, in the manner of tests/test_build_invariants.py: two waves per SIMD need at most 256 registers per wave (VGPRs + AGPRs) and
no scratch, and the library-wide ban on packed-fp32 VALU instructions holds in these kernels too.  All four kernels by name: the three
instances of the 64-cout kernel and the 32-cout kernel."""
import re
import subprocess

import pytest

from tests.test_build_invariants import _tool, code_objects, disassembly  # noqa: F401  (module-scoped fixtures)

# mangled-name fragment -> least number of 16-byte LDS-DMA instructions (the weight slices: 3 stages x 3 per role of the 64-cout kernel;
# the 32-cout kernel's count is the one its first build had)
KERNELS = {
    "conv3x3_winof4_f32_kernelILb0ELb0E": 9,
    "conv3x3_winof4_f32_kernelILb1ELb0E": 9,
    "conv3x3_winof4_f32_kernelILb1ELb1E": 9,
    "conv3x3_winof4_c32_f32_kernel": 12,
}


def _which(name):
    hits = [k for k in KERNELS if k in name]
    assert len(hits) <= 1, name
    return hits[0] if hits else None


def test_winof4_kernel_fits_two_waves_per_simd_without_scratch(code_objects):  # noqa: F811
    readelf = _tool("llvm-readelf")
    if not readelf:
        pytest.skip("llvm-readelf not available")
    seen = set()
    for co in code_objects:
        notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if not _which(name):
                continue
            seen.add(_which(name))
            agpr = int(blk.split()[0])
            vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
            spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
            lds_static = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
            wg = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", blk).group(1))
            assert scratch == 0 and spill == 0, (name, scratch, spill)
            # .vgpr_count is the unified total on gfx950 (architectural VGPRs, then the AGPRs behind them)
            assert max(vgpr, agpr) <= 256 and (vgpr >= agpr) and vgpr <= 256, (name, vgpr, agpr)
            assert wg == 512 and lds_static == 0, (name, wg, lds_static)
    assert seen == set(KERNELS), sorted(set(KERNELS) - seen)


def test_winof4_kernel_instructions(disassembly):  # noqa: F811
    seen = set()
    for text in disassembly:
        for m in re.finditer(r"<(_ZN4pnpx\S*conv3x3_winof4_\S*f32_kernel\S*)>:\n(.*?)s_endpgm", text, re.S):
            which = _which(m.group(1))
            if not which:
                continue
            seen.add(which)
            body = m.group(2)
            assert not re.search(r"v_pk_\w+_f32", body), m.group(1)
            assert "scratch_" not in body, m.group(1)
            assert body.count("v_mfma_f32_16x16x4_f32") >= 144 and "v_mfma_f32_32x32x2_f32" not in body      # 72 per role
            assert body.count("global_load_lds_dwordx4") >= KERNELS[which] and "global_load_lds_dword " in body + " ", m.group(1)
    assert seen == set(KERNELS), sorted(set(KERNELS) - seen)
