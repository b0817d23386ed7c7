"""Build-time guards on the kernels of `eventalign` (csrc/s2s_eventalign.h), from the compiler's kernel-resource-usage remarks (the
fixture of tests/test_build_resources_cpu.py: hipcc cross-compiles for gfx950 without a GPU): no scratch memory, no spilled registers,
and the LDS include/s2s_hip.h states -- the sweep's is dynamic, 3 (W + 2) 8 + 2 (W + 256) 2 bytes, which the header gives for W = 128
and 1024 and the host entry pins with a static_assert; the scan of the event counts holds 16 wave sums."""
import os
import re

from seq2squiggle_amd import _build
from test_build_resources_cpu import scan_instances, usage  # noqa: F401

KERNELS = ("s2s_event_means_fill_kernel", "s2s_eventalign_kernel", "s2s_eventalign_trace_kernel")


def lds_bytes(W):
    return 3 * (W + 2) * 8 + 2 * (W + 256) * 2


def test_eventalign_kernels_have_no_scratch_and_the_stated_lds(usage):  # noqa: F811
    lds, regs = {}, {}
    for name in KERNELS:
        mine = {k: v for k, v in usage.items() if name in k}
        assert len(mine) == 1, (name, sorted(usage))
        (u,) = mine.values()
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        lds[name], regs[name] = u["LDS Size [bytes/block]"], u["VGPRs"]
    assert lds == {KERNELS[0]: 0, KERNELS[1]: 0, KERNELS[2]: 0}, lds     # no static LDS in the sweep: it is asked for at launch
    assert regs[KERNELS[1]] <= 64, regs              # 1,024 threads are four waves per SIMD, and two such workgroups fit a CU's LDS
    scan = scan_instances(usage)[(1, "S2SEvaCounts")]    # the scan of the event counts: no scratch, no spills, 16 * 8 B of LDS
    assert scan["VGPRs"] <= 128, scan                # one workgroup of 1,024 threads
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "s2s_hip.h")).read()
    hip = open(_build.SRC).read()
    assert lds_bytes(1024) == 29744 <= 65536 and lds_bytes(128) == 4656
    assert "29,744 B at W = 1024, 4,656 B\n *                 at W = 128." in header and "#define S2S_EVA_MAX_WIDTH 1024" in header
    assert re.search(r"static_assert\(S2S_EVA_LDS_BYTES\(S2S_EVA_MAX_WIDTH\) == 29744 && S2S_EVA_LDS_BYTES\(128\) == 4656", hip)
