"""Build-time guards on the kernels of `preprocess` (csrc/s2s_chunk.h), from the compiler's kernel-resource-usage remarks (the
fixture of tests/test_build_resources_cpu.py: hipcc cross-compiles for gfx950 without a GPU): no scratch memory, no spilled registers,
and the LDS include/s2s_hip.h states -- a tile's 32 flag words and four wave counts in the flag kernel, which the host entry pins with
a static_assert; none in the other three (a wave holds a chunk's rows in its lanes); the scans are the in-place instance of s2s_scan_kernel
(csrc/s2s_prims.h)."""
import os
import re

from seq2squiggle_amd import _build
from test_build_resources_cpu import scan_instances, usage  # noqa: F401

KERNELS = ("s2s_chunk_flags_kernel", "s2s_chunk_compact_kernel", "s2s_chunk_lengths_kernel", "s2s_chunk_write_kernel")


def test_chunk_kernels_have_no_scratch_and_the_stated_lds(usage):  # noqa: F811
    lds, regs = {}, {}
    for name in KERNELS:
        mine = {k: v for k, v in usage.items() if name in k}
        assert len(mine) == 1, (name, sorted(usage))
        (u,) = mine.values()
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        lds[name], regs[name] = u["LDS Size [bytes/block]"], u["VGPRs"]
    assert lds == {KERNELS[0]: 32 * 8 + 4 * 4, KERNELS[1]: 0, KERNELS[2]: 0, KERNELS[3]: 0}, lds
    assert (1, "S2SScanNext") in scan_instances(usage)         # the four scans: no scratch, no spills, 16 * 8 B of LDS
    assert max(regs[k] for k in KERNELS) <= 64, regs           # eight waves per SIMD: the chunk kernels hide their searches' latency by occupancy
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "s2s_hip.h")).read()
    hip = open(_build.SRC).read()
    assert "Static LDS: 272 B in (1), 128 B in the scans, none elsewhere." in header and "#define S2S_CHUNK_MAX_TE 64" in header
    assert re.search(r"static_assert\(S2S_CHK_LDS_BYTES == 272", hip)
