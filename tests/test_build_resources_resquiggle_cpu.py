"""Build-time guard for the kernels of `resquiggle` (csrc/s2s_resquiggle.h), of the kind tests/test_build_resources_cpu.py keeps for the
production kernels: no scratch memory, no spilled registers, and the LDS include/s2s_hip.h states -- none of it static: the sweep's LDS
is dynamic, 1024 c + 2 (64 c + 128) bytes for c = ceil((2 band + 1) / 64) word pairs per row, which the header gives for bands 512 and
1024 and the host entry pins with a static_assert.  hipcc cross-compiles for gfx950 without a GPU."""
import os
import re

from seq2squiggle_amd import _build

KERNELS = ("s2s_resquiggle_kernel", "s2s_resquiggle_trace_kernel", "s2s_event_sums_kernel")


def lds_bytes(band):
    c = -(-(2 * band + 1) // 64)
    return 2 * 64 * c * 8 + (64 * c + 128) * 2


def test_resquiggle_kernels_have_no_scratch_and_the_stated_lds(tmp_path):
    usage = _build.compile_to(str(tmp_path / "libcheck.so"), report=True)
    for name in KERNELS:
        mine = {k: v for k, v in usage.items() if name in k}
        assert len(mine) == 1, (name, sorted(usage))
        (u,) = mine.values()
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size [bytes/block]"] == 0, (name, u)          # no static LDS: the sweep asks for S2S_RSQ_LDS_BYTES(band) at launch
    sweep = next(v for k, v in usage.items() if KERNELS[0] in k)
    assert sweep["VGPRs"] <= 128, sweep                             # 1024 threads are four waves per SIMD: 512 / 4 registers each
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "s2s_hip.h")).read()
    hip = open(_build.SRC).read()
    assert lds_bytes(1024) == 38272 and lds_bytes(512) == 19840
    assert "38,272 B at S2S_DTW_MAX_BAND, 19,840 B at band 512" in header
    assert re.search(r"static_assert\(S2S_RSQ_LDS_BYTES\(S2S_DTW_MAX_BAND\) == 38272 && S2S_RSQ_LDS_BYTES\(512\) == 19840", hip)
    assert lds_bytes(1024) <= 65536                                 # what one workgroup may ask for
