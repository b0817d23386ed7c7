"""Build-time guard for the kernel of `compare --open-ends` (s2s_sdtw_kernel, csrc/s2s_sdtw.h), of the kind
tests/test_build_resources_cpu.py keeps for the production kernels: no scratch memory, no spilled registers, and the static LDS
include/s2s_hip.h states -- 57,904 B, so that two workgroups share a CU's 160 KB.  hipcc cross-compiles for gfx950 without a GPU."""
from seq2squiggle_amd import _build


def test_sdtw_kernel_has_no_scratch_and_the_stated_lds(tmp_path):
    usage = _build.compile_to(str(tmp_path / "libcheck.so"), report=True)
    mine = {k: v for k, v in usage.items() if "s2s_sdtw_kernel" in k}
    assert len(mine) == 1, sorted(usage)
    (u,) = mine.values()
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["LDS Size [bytes/block]"] == 3 * (2048 + 2) * 8 + 2048 * 2 + (2048 + 256) * 2 == 57904, u
    assert u["VGPRs"] <= 64, u                      # 1024 threads are four waves per SIMD; the LDS admits two such workgroups per CU:
                                                    # eight waves per SIMD share its 512 registers
