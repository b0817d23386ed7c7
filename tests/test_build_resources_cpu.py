"""Build-time guards on the compiler's kernel-resource-usage remarks, one test per family of kernels; the library is compiled ONCE for
all of them (the module-scoped `usage`): hipcc cross-compiles for gfx950 without a GPU (about 35 s).
- The predict kernel: every PRODUCTION instance (s2s_fused_kernel<MODE, TEST = false, EXACT>) must compile without
  scratch memory or spilled vector registers -- round 4's key interleave pushed the exact instance to 32 B of scratch per lane and 7
  spills without anybody noticing until a review ran the compiler with remarks on.
- The kernel of `compare --open-ends` (s2s_sdtw_kernel, csrc/s2s_sdtw.h): no scratch memory, no spilled registers, and the static LDS
  include/s2s_hip.h states -- 57,904 B, so that two workgroups share a CU's 160 KB.
- The kernels of `resquiggle` (csrc/s2s_resquiggle.h): no scratch memory, no spilled registers, and the LDS include/s2s_hip.h states --
  none of it static: the sweep's LDS is dynamic, 1024 c + 2 (64 c + 128) bytes for c = ceil((2 band + 1) / 64) word pairs per row,
  which the header gives for bands 512 and 1024 and the host entry pins with a static_assert.
- The kernels of `segment` (csrc/s2s_segment.h): no scratch memory, no spilled registers, and the LDS include/s2s_hip.h states for the
  flag pass -- static, pinned by a static_assert next to the kernel.
- The instances of the one scan kernel (s2s_scan_kernel<ITEMS, VALUE>, csrc/s2s_prims.h): exactly the three that the entries launch,
  each without scratch memory or spilled registers and with the 16 wave sums, 128 B, as its static LDS (scan_instances, which the
  modules of `preprocess` and `eventalign` use too)."""
import os
import re

import pytest

from seq2squiggle_amd import _build

SCAN_INSTANCES = {(8, "S2SScanInts"): "s2s_export_reads, s2s_svb_encode", (1, "S2SScanNext"): "s2s_segment, s2s_chunk_pack",
                  (1, "S2SEvaCounts"): "s2s_event_means"}


def scan_instances(usage):
    """{(ITEMS, VALUE): resource usage} of every s2s_scan_kernel<ITEMS, VALUE> the library holds, after asserting that they are exactly
    SCAN_INSTANCES -- a missing or an extra instance fails here -- and that each has no scratch, no spills and 128 B of static LDS."""
    inst = {}
    for name, u in usage.items():
        if "s2s_scan_kernel" not in name:
            continue
        m = re.match(r"_Z15s2s_scan_kernelILi(\d+)E\d+([A-Za-z0-9]+?)EvT0_xPx$", name)      # <int ITEMS, class VALUE>(VALUE, long long, long long*)
        assert m and (int(m.group(1)), m.group(2)) not in inst, name
        inst[(int(m.group(1)), m.group(2))] = u
    assert set(inst) == set(SCAN_INSTANCES), sorted(inst)
    for k, u in inst.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["LDS Size [bytes/block]"] == 16 * 8, (k, u)
    return inst


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _build.compile_to(str(tmp_path_factory.mktemp("build_resources") / "libcheck.so"), report=True)


def test_production_kernel_instances_have_no_scratch(usage):
    fused = {k: v for k, v in usage.items() if "s2s_fused_kernel" in k}
    # _Z16s2s_fused_kernelILi<MODE>ELb<TEST>ELb<EXACT>EE...
    inst = {}
    for name, u in fused.items():
        m = re.match(r"_Z16s2s_fused_kernelILi(\d)ELb([01])ELb([01])EE", name)
        assert m, name
        inst[(int(m.group(1)), bool(int(m.group(2))), bool(int(m.group(3))))] = u
    production = {k: u for k, u in inst.items() if not k[1]}
    assert set(production) == {(0, False, False), (1, False, False), (3, False, False), (1, False, True), (3, False, True)}, sorted(inst)
    for k, u in production.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (k, u)
        assert u["Occupancy [waves/SIMD]"] == 2 and u["VGPRs"] <= 256, (k, u)            # 512 threads per CU: two waves per SIMD
        # 256 B of static LDS (the production counters) in front of the dynamic region: together they must fit the CU's 160 KB
        assert u["LDS Size [bytes/block]"] == 256, (k, u)
    # the export / codec kernels as well
    for name, u in usage.items():
        if "s2s_fused_kernel" not in name:
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (name, u)


def test_sdtw_kernel_has_no_scratch_and_the_stated_lds(usage):
    mine = {k: v for k, v in usage.items() if "s2s_sdtw_kernel" in k}
    assert len(mine) == 1, sorted(usage)
    (u,) = mine.values()
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["LDS Size [bytes/block]"] == 3 * (2048 + 2) * 8 + 2048 * 2 + (2048 + 256) * 2 == 57904, u
    assert u["VGPRs"] <= 64, u                      # 1024 threads are four waves per SIMD; the LDS admits two such workgroups per CU:
                                                    # eight waves per SIMD share its 512 registers


def test_resquiggle_kernels_have_no_scratch_and_the_stated_lds(usage):
    KERNELS = ("s2s_resquiggle_kernel", "s2s_resquiggle_trace_kernel", "s2s_event_sums_kernel")

    def lds_bytes(band):
        c = -(-(2 * band + 1) // 64)
        return 2 * 64 * c * 8 + (64 * c + 128) * 2

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


def test_segment_kernels_have_no_scratch_and_the_stated_lds(usage):
    KERNELS = ("s2s_segment_flags_kernel", "s2s_segment_compact_kernel")
    TILE, MAX_WINDOW = 2048, 32

    def lds_bytes():
        ext = TILE + 2 * 3 * MAX_WINDOW                  # the tile and a halo of max(2 w_l, 3 w_s) on each side
        return 2 * ext * 8 + (TILE // 64) * 8 + ext * (2 + 1 + 1 + 1)

    lds = {}
    for name in KERNELS:
        mine = {k: v for k, v in usage.items() if name in k}
        assert len(mine) == 1, (name, sorted(usage))
        (u,) = mine.values()
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        lds[name] = u["LDS Size [bytes/block]"]
    assert lds_bytes() == 47296 <= 65536              # what one workgroup may ask for
    assert lds[KERNELS[0]] == lds_bytes() and lds[KERNELS[1]] == 0, lds
    assert (1, "S2SScanNext") in scan_instances(usage)        # launch 2: no scratch, no spills, 16 * 8 B of LDS
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "s2s_hip.h")).read()
    seg = open(os.path.join(_build.HERE, "csrc", "s2s_segment.h")).read()
    assert "S2S_SEG_LDS_BYTES\n *                 = 47,296 B" in header and "#define S2S_SEG_TILE 2048" in header
    assert re.search(r"#define S2S_SEG_LDS_BYTES 47296", seg)
    assert re.search(r"static_assert\(sizeof\(S2SSegLds\) == S2S_SEG_LDS_BYTES && S2S_SEG_LDS_BYTES <= 65536", seg)
