"""Build-time guards on the kernel of `--kmer-model-out` (csrc/s2s_kmer_model_events.h), from the compiler's kernel-resource-usage
remarks (the fixture of tests/test_build_resources_cpu.py: hipcc cross-compiles for gfx950 without a GPU): no scratch memory, no
spilled registers, and as static LDS the write-combining cache alone -- the 45,100 B include/s2s_hip.h states, pinned by a
static_assert next to the kernel; and s2s_kmer_model_kernel, whose cache rules the new kernel copies, compiles to the figures it had
before that kernel was written (both instances: registers, LDS, occupancy)."""
import os
import re

from seq2squiggle_amd import _build
from test_build_resources_cpu import usage  # noqa: F401

SLOTS, FIELDS = 1025, 5
# s2s_kmer_model_kernel<TD> on the commit before s2s_kmer_model_events: TD -> its figures
BEFORE = {250: {"TotalSGPRs": 86, "VGPRs": 62, "AGPRs": 0, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 3, "SGPRs Spill": 0,
                "VGPRs Spill": 0, "LDS Size [bytes/block]": 45112},
          0: {"TotalSGPRs": 84, "VGPRs": 68, "AGPRs": 0, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 3, "SGPRs Spill": 0,
              "VGPRs Spill": 0, "LDS Size [bytes/block]": 45112}}


def test_events_kernel_has_no_scratch_and_the_stated_lds(usage):  # noqa: F811
    mine = {k: v for k, v in usage.items() if "s2s_kmer_model_events_kernel" in k}
    assert len(mine) == 1, sorted(usage)
    (u,) = mine.values()
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["LDS Size [bytes/block]"] == SLOTS * 4 + FIELDS * SLOTS * 8 == 45100, u
    assert u["VGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 3, u          # three workgroups of four waves per CU by LDS: three waves per SIMD
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "s2s_hip.h")).read()
    src = open(os.path.join(_build.HERE, "csrc", "s2s_kmer_model_events.h")).read()
    assert "Static LDS: the cache's 45,100 B, nothing else." in header
    assert f"#define S2S_KMER_MODEL_SLOTS           {SLOTS}" in header and f"#define S2S_KMER_MODEL_FIELDS          {FIELDS}" in header
    assert re.search(r"static_assert\(S2S_KME_LDS_BYTES == 45100", src) and re.search(r"static_assert\(sizeof\(lds\) == S2S_KME_LDS_BYTES", src)
    assert "asm" not in re.sub(r"//.*", "", src)                                # plain C++ / HIP


def test_kmer_model_kernel_is_what_it_was(usage):  # noqa: F811
    got = {}
    for name, u in usage.items():
        m = re.match(r"_Z21s2s_kmer_model_kernelILi(\d+)EE", name)
        if m:
            got[int(m.group(1))] = {k: u[k] for k in BEFORE[0]}
    assert got == BEFORE, got
