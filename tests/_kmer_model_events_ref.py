"""The definition of s2s_kmer_model_events (include/s2s_hip.h) in Python integers, shared by tests/test_kmer_model_events_cpu.py,
tests/test_kmer_model_events_cli_cpu.py and tests/test_gpu_kmer_model_events.py: the fixed-point event by its stated formula, the
conversion to 2^-8 pA by a record's gain and shift, the three drop rules, the five sums per row.  Nothing here calls the library."""
import math

import numpy as np

FIELDS = 5
MAX_LEN = 1024
GAIN_ONE = 1 << 24
LIMIT = 1 << 23
DROPPED = ("overlong", "out_of_range", "bad_code", "counted")


def event_fixed(n: int, S: int, Q: int):
    """s2s_event_fixed as the header states it: M = round-half-even(256 S / n), D = isqrt(floor(max(n Q - S^2, 0) 2^16 / n^2))."""
    q, r = divmod(256 * S, n)                                  # floor division: 0 <= r < n
    if 2 * r > n or (2 * r == n and q % 2 == 1):
        q += 1
    return q, math.isqrt((max(n * Q - S * S, 0) << 16) // (n * n))


def gain_shift(digitisation: float, offset: float, signal_range: float):
    """(gain, shift) of a record, formed in double; gain 0 for a calibration outside 1 .. 2^30 / |shift| <= 2^30."""
    digitisation, offset, signal_range = float(digitisation), float(offset), float(signal_range)
    if digitisation == 0 or not all(math.isfinite(x) for x in (digitisation, offset, signal_range)):
        return 0, 0
    g, s = float(np.rint(signal_range / digitisation * GAIN_ONE)), float(np.rint(offset * 256))
    if not 1 <= g <= 1 << 30 or abs(s) > 1 << 30:
        return 0, 0
    return int(g), int(s)


def to_pa(M: int, D: int, gain: int, shift: int):
    """-> (Mp, Dp): round-half-even((M + shift) gain / 2^24), floor(D gain / 2^24)."""
    q, r = divmod((M + shift) * gain, GAIN_ONE)
    if 2 * r > GAIN_ONE or (2 * r == GAIN_ONE and q % 2 == 1):
        q += 1
    return q, (D * gain) // GAIN_ONE


def ref_events(codes, ev_len, S, Q, l_offs, gain, shift, k: int, table=None, dropped=None):
    """-> (table int64 [4^k + 1, 5], dropped int64 [4]), added to the ones given."""
    rows = 4 ** k + 1
    table = [[0] * FIELDS for _ in range(rows)] if table is None else [[int(x) for x in row] for row in table]
    dropped = [0, 0, 0, 0] if dropped is None else [int(x) for x in dropped]
    for p in range(len(l_offs) - 1):
        g, s = int(gain[p]), int(shift[p])
        if g == 0:
            continue
        for j in range(int(l_offs[p]), int(l_offs[p + 1])):
            n, c = int(ev_len[j]), int(codes[j])
            if n < 1:
                continue
            if n > MAX_LEN:
                dropped[0] += 1
                continue
            if c < 0 or c >= rows:
                dropped[2] += 1
                continue
            Sj = int(S[j])
            assert -2 ** 31 <= Sj < 2 ** 31, "the definition takes (int32)S: the tests stay inside it"
            Mp, Dp = to_pa(*event_fixed(n, Sj, int(Q[j])), g, s)
            if abs(Mp) > LIMIT or Dp > LIMIT:
                dropped[1] += 1
                continue
            for f, v in enumerate((1, Mp, Mp * Mp, Dp, Dp * Dp)):
                table[c][f] += v
            dropped[3] += 1
    assert all(-2 ** 63 <= v < 2 ** 63 for row in table for v in row)
    return np.array(table, np.int64).reshape(rows, FIELDS), np.array(dropped, np.int64)


def sums(x):
    """(n, S, Q) of the samples x."""
    x = [int(v) for v in x]
    return len(x), sum(x), sum(v * v for v in x)


def cache_slot(code: int, c: dict) -> int:
    """The home slot of a code on the hashed path, as the header states it (c: _kmer_model_ref.header_constants)."""
    return (((code * c["HASH_MUL"]) & 0xFFFFFFFF) * c["SLOTS"]) >> 32


def codes_with_home(home: int, count: int, k: int, c: dict):
    """The first `count` codes of the 4^k whose home slot is `home`; asserts that there are that many."""
    found = []
    for code in range(4 ** k):
        if cache_slot(code, c) == home:
            found.append(code)
            if len(found) == count:
                break
    assert len(found) == count, (home, count, found)
    return found
