"""The references of tests/test_gpu_sampler_counters.py held to what they restate, without a GPU: the numpy Philox4x32-10 to the
Random123 known answers (the vectors test_gpu_parity.py::test_philox_known_answers holds the kernel to), the float64 normal to its
law, and the Gamma restatement to its law and to itself in float32 -- the share of draws on which float32 and float64 take another
path through the rejection loop bounds what a float32 kernel may differ from the float64 reference by."""
import numpy as np
import pytest
from scipy import stats

import _philox_ref as P


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32-10: all zeros, all ones."""
    r = P.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [hex(int(x)) for x in r] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    m = 0xFFFFFFFF
    r = P.philox4x32_10(m, m, m, m, m, m)
    assert [hex(int(x)) for x in r] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    # vectorised = one by one, and the layout of words(): chunk split into two words, position | kind << 16, the seed's two words
    chunk = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 123456789012, 2 ** 64 - 1], dtype=np.uint64)
    seed = 0x0123456789ABCDEF
    got = np.stack(P.words(chunk[:, None], np.arange(3)[None, :], P.KIND_NOISE, 5, seed), -1)
    for i, ch in enumerate(chunk.tolist()):
        for t in range(3):
            one = P.philox4x32_10(ch & m, ch >> 32, t | (3 << 16), 5, 0x89ABCDEF, 0x01234567)
            assert [int(x) for x in one] == got[i, t].tolist()
    assert len({tuple(w) for w in got.reshape(-1, 4).tolist()}) == got.shape[0] * got.shape[1] and got.max() < 2 ** 32


def test_uniforms_and_normal():
    assert P.u01_open0(0) == 2.0 ** -24 and P.u01_open0(0xFFFFFFFF) == 1.0 and P.u01_open1(0) == 0.0
    assert P.u01_open1(0xFFFFFFFF) == 1.0 - 2.0 ** -24 and P.u01_open1(0xFF) == 0.0
    assert P.normal(0xFFFFFFFF, 12345) == 0.0                                       # u1 = 1: radius 0
    assert abs(P.normal(0, 0) - np.sqrt(48 * np.log(2.0))) < 1e-12                  # u1 = 2^-24, u2 = 0: the largest draw
    assert abs(P.normal(0, 1 << 31) + np.sqrt(48 * np.log(2.0))) < 1e-12            # u2 = 1/2
    z = P.ref_normal(np.arange(400, dtype=np.uint64)[:, None] + np.uint64(2 ** 32 - 200), np.arange(250)[None, :], P.KIND_NOISE, 77)
    assert stats.kstest(z.ravel(), "norm").pvalue > 1e-3 and abs(z.std() - 1) < 0.01
    assert abs(np.corrcoef(z[:, :-1].ravel(), z[:, 1:].ravel())[0, 1]) < 0.01 and abs(np.corrcoef(z[:-1].ravel(), z[1:].ravel())[0, 1]) < 0.01
    z2 = P.ref_normal(np.arange(400, dtype=np.uint64)[:, None] + np.uint64(2 ** 32 - 200), np.arange(250)[None, :], P.KIND_DWELL, 77)
    assert abs(np.corrcoef(z.ravel(), z2.ravel())[0, 1]) < 0.01                     # another kind: other draws


# conc and rate as tests/test_gpu_samplers.py::test_gamma_dwell_distribution meets them: softplus of the head biases
@pytest.mark.parametrize("conc,rate", [(9.0, 0.8), (0.5, 2.5e-3), (0.13, 1.2e-4)], ids=["conc9", "conc0.5", "conc0.13"])
def test_gamma_restatement_in_float32_and_float64(conc, rate):
    n = 100_000
    chunk = (np.arange(n, dtype=np.uint64) // np.uint64(16)) + np.uint64(2 ** 32 - 1000)
    pos = np.arange(n) % 16
    alpha = np.full(n, conc, np.float32)
    s64 = P.ref_standard_gamma(alpha, chunk, pos, 11, np.float64)
    s32 = P.ref_standard_gamma(alpha, chunk, pos, 11, np.float32)
    assert s64.dtype == np.float64 and s32.dtype == np.float32
    assert stats.kstest(s64, stats.gamma(a=conc).cdf).pvalue > 1e-3                 # the restatement draws Gamma(conc, 1)
    g64, g32 = P.dwell_of_gamma(s64, np.float32(rate)), P.dwell_of_gamma(s32, np.float32(rate))
    share, counted = P.agreement(g32, g64)
    assert counted > n // 2
    print(f"conc {conc}: float32 and float64 disagree on {(1 - share) * counted:.0f} of {counted} draws above the clamp")
    assert 1 - share < 1e-4                                                         # an accept / reject decision flipped
    assert P.ref_standard_gamma(np.float32(0.0), 5, 3, 11) == 0.0
