"""Invariants of the Winograd F(4x4,3x3) kernel's device code (csrc/conv3x3_winof4.hip), checked on the CPU in libpnpx.so's gfx950 code
objects, in the manner of tests/test_build_invariants.py: two waves per SIMD need at most 256 registers per wave (VGPRs + AGPRs) and
no scratch, and the library-wide ban on packed-fp32 VALU instructions holds in this kernel too."""
import re
import subprocess

import pytest

from tests.test_build_invariants import _tool, code_objects, disassembly  # noqa: F401  (module-scoped fixtures)

KERNEL = "conv3x3_winof4_f32_kernel"


def test_winof4_kernel_fits_two_waves_per_simd_without_scratch(code_objects):  # noqa: F811
    readelf = _tool("llvm-readelf")
    if not readelf:
        pytest.skip("llvm-readelf not available")
    seen = 0
    for co in code_objects:
        notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if KERNEL not in name:
                continue
            seen += 1
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
    assert seen >= 1, "no conv3x3_winof4_f32_kernel instance in libpnpx.so"


def test_winof4_kernel_instructions(disassembly):  # noqa: F811
    n = 0
    for text in disassembly:
        for m in re.finditer(r"<(_ZN4pnpx\S*" + KERNEL + r"\S*)>:\n(.*?)s_endpgm", text, re.S):
            n += 1
            body = m.group(2)
            assert not re.search(r"v_pk_\w+_f32", body), m.group(1)
            assert "scratch_" not in body, m.group(1)
            assert body.count("v_mfma_f32_16x16x4_f32") >= 144 and "v_mfma_f32_32x32x2_f32" not in body      # 72 per role
            assert body.count("global_load_lds_dwordx4") >= 9 and "global_load_lds_dword " in body + " "
    assert n >= 1
