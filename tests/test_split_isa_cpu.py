"""What the compiler made of the hi/lo split (csrc/s2s_device_h.h: split2, split2x2), read from a cross-compile of the library for gfx950 with
the ISA kept (no GPU needed; one compile for the module, about a minute):
- every PRODUCTION instance of the predict kernel (s2s_fused_kernel<MODE, TEST = false, EXACT>) has 0 B of scratch and no spilled
  vector register, from the compiler's resource remarks;
- in every f16x3 instance (MODE = 1: production and TEST, fast and exact) the attention code -- the basic blocks that issue the
  32x32x16 MFMA -- holds no v_fma_mixlo_f16 / v_fma_mixhi_f16: the lo half of P comes from fp32 residuals (v_fma_mix_f32) and a second
  v_cvt_pk_f16_f32 since round 35 (LABNOTES), and a compiler that folds fma + conversion back into the f16-destination form would
  put the kernel back on the 8-cycle instructions without any test of the results noticing: the bits are the same."""
import os
import re
import subprocess

import pytest

from seq2squiggle_amd import _build

MIX_F16 = ("v_fma_mixlo_f16", "v_fma_mixhi_f16")
KERNEL = re.compile(r"^_Z16s2s_fused_kernelILi(\d)ELb([01])ELb([01])EE\S*:")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    # the device side of _build.compile_to's command, stopped at the ISA listing, with the resource remarks on
    listing = str(tmp_path_factory.mktemp("split_isa") / "s2s_hip_gfx950.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                        "-S", "--cuda-device-only", "-o", listing, _build.SRC], check=True, capture_output=True, text=True)
    return _build.resource_usage(r.stderr), open(listing).read().split("\n")


def kernel_blocks(lines):
    """{(MODE, TEST, EXACT): [[opcode, ...] per basic block]} of the s2s_fused_kernel instances in an ISA listing."""
    out, cur = {}, None
    for line in lines:
        m = KERNEL.match(line)
        if m:
            cur = out.setdefault((int(m.group(1)), bool(int(m.group(2))), bool(int(m.group(3)))), [[]])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if re.match(r"^\.LBB\S+:", line):
            cur.append([])
            continue
        t = line.strip()
        if t and not t.startswith((";", ".")):
            cur[-1].append(t.split()[0])
    return out


def test_production_instances_have_no_scratch(compiled):
    usage, _ = compiled
    production = {k: u for k, u in usage.items() if re.match(r"_Z16s2s_fused_kernelILi\dELb0ELb[01]EE", k)}
    assert len(production) == 5, sorted(usage)
    for k, u in production.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (k, u)


def test_f16x3_attention_holds_no_f16_destination_mix(compiled):
    _, lines = compiled
    kernels = kernel_blocks(lines)
    f16x3 = {k: b for k, b in kernels.items() if k[0] == 1}
    assert set(f16x3) == {(1, False, False), (1, False, True), (1, True, False), (1, True, True)}, sorted(kernels)
    for k, blocks in f16x3.items():
        attention = [b for b in blocks if "v_mfma_f32_32x32x16_f16" in b]
        assert attention, k
        split_blocks = 0
        for b in attention:
            assert not any(op in MIX_F16 for op in b), (k, {op: b.count(op) for op in MIX_F16})
            n_exp = sum(op.startswith("v_exp_f32") for op in b)
            if n_exp >= 64:                                   # a block that turns scores into P: one fp32 residual per exponential
                split_blocks += 1
                assert b.count("v_fma_mix_f32") >= min(n_exp, 128), (k, n_exp, b.count("v_fma_mix_f32"))
                assert b.count("v_cvt_pk_f16_f32") >= min(n_exp, 128), (k, n_exp, b.count("v_cvt_pk_f16_f32"))
        assert split_blocks >= 1, k
