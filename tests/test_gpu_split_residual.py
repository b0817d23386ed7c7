"""The hi/lo split of the f16x3 mode takes its residual in fp32 since round 35 (csrc/s2s_device_h.h: split2, split2x2 -- v_cvt_pk_f16_f32,
v_fma_mix_f32, v_cvt_pk_f16_f32) where rounds 1-34 rounded x * 1 - hi straight to f16 (v_fma_mix{lo,hi}_f16).  The two are the same
bits by construction -- the fp32 residual is exact -- and tools/probes/split_residual_check.hip holds them to it on the GPU: a
stand-alone program, built here with the library's own flags, that runs both on every fp32 bit pattern of the exponents where they
could part (all 2^23 mantissas, both signs, at the unbiased exponents -25, -15, -14, -4, -3, 0, 1, 15 and 16, the fp32 subnormals with
the zeros, inf and the NaNs: 369 M values, each in the low and in the high half of a pair) and, in a second kernel, the two round-35
candidates that did NOT ship against the code that stayed (the phantom-key mask as a bit-field select, the pass-0 row maximum as a
tree of three-input maxima) on score tiles holding +0, -0, -inf and the largest finite value.  One run of the program, under its own
time limit, serves both tests."""
import os
import re
import subprocess

import pytest

from seq2squiggle_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "probes", "split_residual_check.hip")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split_residual") / "split_residual_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of _build.compile_to: the float mode (denormals, contraction) and -fno-slp-vectorize are part of what is checked
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-w", "-I", os.path.join(_build.HERE, "csrc"),
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode in (0, 1), (r.returncode, r.stdout[-400:], r.stderr[-400:])      # 1: a mismatch, reported below; else the run failed
    return r.stdout


def count(report, pattern):
    m = re.search(pattern, report)
    assert m, (pattern, report)
    return [int(g) for g in m.groups()]


def test_fp32_residual_split_is_bit_equal_to_the_f16_destination_mix(report):
    ran, want, bad = count(report, r"split finite inputs: values (\d+) \(expected (\d+)\) mismatches (\d+)")
    assert ran == want == 11 * (1 << 23) * 4                      # 11 exponent fields x 2^23 mantissas x 2 signs x 2 halves of a pair
    assert bad == 0, report                                       # hi and lo bit-equal for every finite input
    assert count(report, r"split infinite inputs: mismatches (\d+)") == [0], report
    assert count(report, r"split NaN inputs without NaN hi and lo: mismatches (\d+)") == [0], report


def test_mask_select_and_max_tree_are_bit_equal_to_the_code_that_stayed(report):
    ran, want, bad = count(report, r"mask select: lane-cases (\d+) \(expected (\d+)\) mismatches (\d+)")
    assert ran == want == 64 << 16 and bad == 0, report
    assert count(report, r"row maximum: mismatches (\d+)") == [0], report
