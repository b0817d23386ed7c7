"""s2s_kmer_model_events_host -- the definition the kernel must equal -- against tests/_kmer_model_events_ref.py, which restates
include/s2s_hip.h in Python integers.  The slots are planted directly, no alignment: every rule of the definition at its edges (event
lengths 0, 1, 2, 1024, 1025; full-scale samples; the half-way cases of the rounding with both signs; |Mp| = 2^23 and one past it; the
codes around the table's ends; gains 1, 2^24, 2^30 and 0; negative shifts; empty records), every k that takes another path in the
kernel, the error returns, and the identity that ties the table to s2s_kmer_model_accumulate's."""
import ctypes as C

import numpy as np
import pytest

import _kmer_model_events_ref as REF
from seq2squiggle_amd import _lib

ONE = REF.GAIN_ONE


def pooled(records):
    """records: [(gain, shift, [(n, S, Q, code), ...]), ...] -> the arrays of the entry."""
    slots = [s for _, _, ss in records for s in ss]
    col = lambda i, dt: np.array([s[i] for s in slots], dt).reshape(-1)      # noqa: E731
    l_offs = np.concatenate([[0], np.cumsum([len(ss) for _, _, ss in records])]).astype(np.int64)
    return dict(codes=col(3, np.int32), ev_len=col(0, np.int32), S=col(1, np.int64), Q=col(2, np.int64), l_offs=l_offs,
                gain=np.array([r[0] for r in records], np.int64), shift=np.array([r[1] for r in records], np.int64))


def host(a, k, table=None, dropped=None, threads=1, P=None):
    table = np.zeros((4 ** min(max(k, 1), 10) + 1, REF.FIELDS), np.int64) if table is None else table.copy()
    dropped = np.zeros(4, np.int64) if dropped is None else dropped.copy()
    ptr = lambda x: x.ctypes.data if x is not None else None                 # noqa: E731
    rc = _lib.lib().s2s_kmer_model_events_host(ptr(a["codes"]), ptr(a["ev_len"]), ptr(a["S"]), ptr(a["Q"]), ptr(a["l_offs"]),
                                               len(a["l_offs"]) - 1 if P is None else P, ptr(a["gain"]), ptr(a["shift"]), k, ptr(table), ptr(dropped), threads)
    return rc, table, dropped


def check(records, k, **kw):
    a = pooled(records)
    rc, table, dropped = host(a, k, **kw)
    want_t, want_d = REF.ref_events(a["codes"], a["ev_len"], a["S"], a["Q"], a["l_offs"], a["gain"], a["shift"], k)
    assert rc == 0
    assert np.array_equal(table, want_t), np.argwhere(table != want_t)[:5]
    assert dropped.tolist() == want_d.tolist(), (dropped, want_d)
    return table, dropped


def slot(x, code):
    return (*REF.sums(x), code)


def rim_records(c0, c1):
    """|Mp| = 2^23 exactly (counted) and one past it (dropped), below and above."""
    return [(ONE, 0, [slot([-32768] * 4, c0)]), (ONE, -1, [slot([-32768] * 4, c0)]),
            (ONE, 2 ** 23 - 256 * 100, [slot([100] * 3, c1)]), (ONE, 2 ** 23 - 256 * 100 + 1, [slot([100] * 3, c1)])]


def edge_records(k, rng):
    """Every rule at its edges, for a table of 4^k + 1 rows."""
    top = 4 ** k
    code = lambda: int(rng.integers(0, top))                                 # noqa: E731
    noisy = lambda n: rng.integers(-500, 1500, n)                            # noqa: E731
    lengths = [(0, 0, 0, code())] + [slot(noisy(n), code()) for n in (1, 2, 1024)] + [(1025, 1025 * 400, 1025 * 400 * 400, code())]
    full = [slot([v] * 1024, code()) for v in (32767, -32767, -32768)] + [slot([32767, -32768] * 512, code())]
    codes = [slot(noisy(5), c) for c in (-1, top, top + 1, 0, top - 1, -2 ** 31, 2 ** 31 - 1)]
    # the half-way cases: gain 2^23 makes (M + shift) / 2 of it; n = 1 and sample x give M = 256 x, the shift the rest
    halves = [(1 << 23, t - 256 * 7, [(1, 7, 49, code())]) for t in (3, 1, -1, -3, 5, -5, 2, -2)]
    rim = rim_records(code(), code())
    # Dp past 2^23 by the gain alone, the mean in range
    wide = [(1 << 30, 0, [slot([2000, -2000] * 8, code())])]
    gains = [(g, s, [slot(noisy(n), code()) for n in (1, 3, 17, 1024)] + lengths[:1] + lengths[-1:])
             for g in (1, ONE, 1 << 30, 0, 2914461) for s in (0, -2560, 2 ** 30, -2 ** 30, 53)]
    return ([(ONE, 0, lengths), (2914461, 2560, full), (ONE, 0, full), (ONE, -77, codes), (0, 0, codes + full), (ONE, 0, [])] + halves +
            [(5, 5, [])] + rim + wide + [(ONE, 0, []), (ONE, 0, [])] + gains)


@pytest.mark.parametrize("k", [1, 5, 6, 10])
def test_host_twin_equals_the_definition_at_every_edge(k):
    rng = np.random.default_rng(k)
    records = edge_records(k, rng)
    table, dropped = check(records, k)
    assert dropped[0] > 0 and dropped[1] > 0 and dropped[2] > 0 and dropped[3] > 0


def test_the_rim_of_the_range_counts_and_one_past_it_drops():
    t, d = check(rim_records(0, 3), 1)
    assert d.tolist() == [0, 2, 0, 2]
    assert t[0].tolist() == [1, -2 ** 23, 2 ** 46, 0, 0] and t[3].tolist() == [1, 2 ** 23, 2 ** 46, 0, 0]


def test_halfway_cases_round_to_even_with_both_signs():
    got = {}
    for t in (3, 1, -1, -3, 5, -5, 2, -2):
        table, _ = check([(1 << 23, t - 256 * 7, [(1, 7, 49, 2)])], 1)
        got[t] = int(table[2, 1])
    assert got == {3: 2, 1: 0, -1: 0, -3: -2, 5: 2, -5: -2, 2: 1, -2: -1}
    assert REF.to_pa(3, 0, 1 << 23, 0) == (2, 0) and REF.to_pa(-3, 0, 1 << 23, 0) == (-2, 0)


def test_identity_calibration_gives_the_sums_of_event_fixed():
    """gain = 2^24, shift = 0: Mp = M and Dp = D, the events of s2s_kmer_model_accumulate."""
    rng = np.random.default_rng(2)
    L = _lib.lib()
    slots, want = [], np.zeros((4 ** 3 + 1, REF.FIELDS), np.int64)
    for _ in range(300):
        x = rng.integers(-3000, 3000, int(rng.integers(1, 60)))
        c = int(rng.integers(0, 65))
        n, S, Q = REF.sums(x)
        M, D = C.c_int64(), C.c_int64()
        assert L.s2s_event_fixed(n, S, Q, C.addressof(M), C.addressof(D)) == 0 and (M.value, D.value) == REF.event_fixed(n, S, Q)
        want[c] += (1, M.value, M.value ** 2, D.value, D.value ** 2)
        slots.append((n, S, Q, c))
    table, dropped = check([(ONE, 0, slots[:100]), (ONE, 0, []), (ONE, 0, slots[100:])], 3)
    assert np.array_equal(table, want) and dropped.tolist() == [0, 0, 0, 300]


def test_adds_to_what_is_there_and_ignores_batching_and_threads():
    rng = np.random.default_rng(4)
    recs = [(int(rng.integers(1, 1 << 26)), int(rng.integers(-5000, 5000)),
             [slot(rng.integers(-800, 1800, int(rng.integers(0, 40))) if rng.random() > 0.1 else [], int(rng.integers(-1, 4 ** 4 + 2)))
              for _ in range(int(rng.integers(0, 50)))]) for _ in range(12)]
    recs = [(g, s, [x if x[0] else (0, 0, 0, x[3]) for x in ss]) for g, s, ss in recs]
    whole, d_whole = check(recs, 4)
    t, d = None, None
    for part in (recs[:5], recs[5:6], recs[6:]):
        rc, t, d = host(pooled(part), 4, t, d, threads=3)
        assert rc == 0
    assert np.array_equal(t, whole) and d.tolist() == d_whole.tolist()


def test_no_work_and_the_error_returns():
    L = _lib.lib()
    a = pooled([(ONE, 0, [slot([5, 6], 1)])])
    assert host(a, 2)[0] == 0
    assert L.s2s_kmer_model_events_host(None, None, None, None, None, 0, None, None, 3, None, None, 1) == 0          # P = 0
    empty = pooled([(ONE, 0, []), (ONE, 0, [])])
    rc, t, d = host(empty, 2)
    assert rc == 0 and not t.any() and not d.any()                                                                   # no slots
    for k in (0, 11, -1):
        assert host(a, k)[0] == -1
    assert host(a, 2, P=-1)[0] == -1
    for missing in ("codes", "ev_len", "S", "Q", "l_offs", "gain", "shift"):
        assert host({**a, missing: None}, 2, P=1)[0] == -1
    ptrs = [a[n].ctypes.data for n in ("codes", "ev_len", "S", "Q", "l_offs")]
    table, dropped = np.zeros((17, 5), np.int64), np.zeros(4, np.int64)
    tail = [a["gain"].ctypes.data, a["shift"].ctypes.data, 2]
    assert L.s2s_kmer_model_events_host(*ptrs, 1, *tail, None, dropped.ctypes.data, 1) == -1
    assert L.s2s_kmer_model_events_host(*ptrs, 1, *tail, table.ctypes.data, None, 1) == -1
    assert L.s2s_kmer_model_events_host(*ptrs, 1, *tail, table.ctypes.data, dropped.ctypes.data, 0) == -1            # threads < 1
    assert not table.any() and not dropped.any()
    down = {**pooled([(ONE, 0, [slot([5], 1)] * 3), (ONE, 0, [])]), "l_offs": np.array([0, 3, 2], np.int64)}         # offsets that decrease
    assert host(down, 2)[0] == -1
    assert host({**a, "l_offs": np.array([-1, 1], np.int64)}, 2)[0] == -1
