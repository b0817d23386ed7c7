"""The compiler's resource report of the trainer's kernels (csrc/s2s_train.h; the `usage` fixture of tests/test_build_resources_cpu.py:
hipcc cross-compiles for gfx950 without a GPU): no scratch memory, no spilled registers, the attention-backward kernel's static LDS
as the header states it, and no inline assembly in the header."""
import os
import re

from seq2squiggle_amd import _build
from test_build_resources_cpu import usage  # noqa: F401

KERNELS = ("train_mm_kernel", "train_colsum_kernel", "train_reduce_kernel", "train_copy_kernel", "train_relu_mask_kernel",
           "train_onehot_kernel", "train_layernorm_bwd_kernel", "train_attention_bwd_kernel", "train_lenreg_bwd_kernel",
           "train_heads_bwd_kernel", "train_emit_bwd_kernel", "train_sumsq_kernel", "train_norm_kernel", "train_loss_stats_kernel",
           "train_adam_kernel", "train_gather_kernel")
HEADER = os.path.join(_build.HERE, "csrc", "s2s_train.h")


def test_train_kernels_have_no_scratch_and_no_spills(usage):  # noqa: F811
    for name in KERNELS:
        mine = {k: v for k, v in usage.items() if name in k}
        assert mine, f"{name}: not in the build"
        for k, v in mine.items():
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert len({k for k in usage if "train_mm_kernel" in k}) == 4        # weight gradients, and the three input-gradient epilogues


def test_attention_backward_lds_is_the_stated_figure(usage):  # noqa: F811
    text = open(HEADER).read()
    stated = int(re.search(r"TRAIN_ATTN_LDS_BYTES = ([\d,]+) B", text).group(1).replace(",", ""))
    assert stated == (3 * 1024 + 4 * (2 * 512 + 2 * 1024)) * 4
    (v,) = [v for k, v in usage.items() if "train_attention_bwd_kernel" in k]
    assert v["LDS Size [bytes/block]"] == stated


def test_header_has_no_inline_assembly():
    assert not re.search(r"\basm\b|__asm", open(HEADER).read())
