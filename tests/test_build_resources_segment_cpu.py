"""Build-time guard for the kernels of `segment` (csrc/s2s_segment.h), of the kind tests/test_build_resources_resquiggle_cpu.py keeps
for `resquiggle`: no scratch memory, no spilled registers, and the LDS include/s2s_hip.h states for the flag pass -- static, pinned by a
static_assert next to the kernel.  hipcc cross-compiles for gfx950 without a GPU."""
import os
import re

from seq2squiggle_amd import _build

KERNELS = ("s2s_segment_flags_kernel", "s2s_segment_scan_kernel", "s2s_segment_compact_kernel")
TILE, MAX_WINDOW = 2048, 32


def lds_bytes():
    ext = TILE + 2 * 3 * MAX_WINDOW                  # the tile and a halo of max(2 w_l, 3 w_s) on each side
    return 2 * ext * 8 + (TILE // 64) * 8 + ext * (2 + 1 + 1 + 1)


def test_segment_kernels_have_no_scratch_and_the_stated_lds(tmp_path):
    usage = _build.compile_to(str(tmp_path / "libcheck.so"), report=True)
    lds = {}
    for name in KERNELS:
        mine = {k: v for k, v in usage.items() if name in k}
        assert len(mine) == 1, (name, sorted(usage))
        (u,) = mine.values()
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        lds[name] = u["LDS Size [bytes/block]"]
    assert lds_bytes() == 47296 <= 65536              # what one workgroup may ask for
    assert lds[KERNELS[0]] == lds_bytes() and lds[KERNELS[1]] == 16 * 8 and lds[KERNELS[2]] == 0, lds
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "s2s_hip.h")).read()
    seg = open(os.path.join(_build.HERE, "csrc", "s2s_segment.h")).read()
    assert "S2S_SEG_LDS_BYTES\n *                 = 47,296 B" in header and "#define S2S_SEG_TILE 2048" in header
    assert re.search(r"#define S2S_SEG_LDS_BYTES 47296", seg)
    assert re.search(r"static_assert\(sizeof\(S2SSegLds\) == S2S_SEG_LDS_BYTES && S2S_SEG_LDS_BYTES <= 65536", seg)
