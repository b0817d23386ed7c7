"""Identities that hold the two sweeps of `compare` to each other, on the host entries (tests/test_gpu_compare_identities.py runs
the same checks with the kernels).  The banded sweep (s2s_dtw_banded: int64, a ring, band bookkeeping) and the subsequence sweep
(s2s_sdtw: int32 (E, S), dense) are two independent programs; subsequence DTW has an exhaustive definition that uses the banded
entry only: its cost is the minimum over all intervals t[s:e) of the full-matrix DTW of q against that interval, `end` is the
smallest e at which that minimum is reached, and the reported interval itself reaches it.  At band R = L the band
|i m - j n| <= R max(n, m) covers the whole matrix of every such pair (i m < L m and j n < m L, both <= L max(L, m)), which a few
pairs are held to by the unbanded restatement.  None of it shares a line with tests/_sdtw_ref.py.
  Then the banded sweep and the path at extreme slopes (thousands of samples against one, two or three), where lo(d) and hi(d) move
with every diagonal and the column window barely moves: host entries against the restatements, values in -3 .. 3 so that ties
abound.  Every check is an equality of integers."""
import numpy as np
import pytest

from seq2squiggle_amd import compare as CMP
from _dtw_ref import ref_dtw, ref_dtw_full
from _dtw_path_ref import check_path, ref_path
from test_compare_cpu import dtw_pair
from test_compare_open_ends_cpu import KINDS, make

BRUTE_SHAPES = ((1, 40), (5, 40), (12, 40), (40, 12), (7, 1))
SLOPES = ((4000, 1, 1), (1, 4000, 1), (3000, 2, 1), (2, 3000, 2), (5000, 37, 1), (37, 5000, 3), (513, 3, 7), (3, 513, 300), (256, 1, 1),
          (257, 1, 64), (1, 256, 1024))


# ------------------------------------------------------------------ B1: subsequence DTW by brute force over the intervals
def interval_costs(q, t, cpu):
    """{(s, e): full-matrix DTW of q against t[s:e)} for every 0 <= s < e <= H: one s2s_dtw_banded launch of H (H + 1) / 2 pairs at
    band L."""
    H = len(t)
    iv = [(s, e) for s in range(H) for e in range(s + 1, H + 1)]
    cost = CMP.dtw_banded([q] * len(iv), [t[s:e] for s, e in iv], len(q), cpu=cpu)
    assert len(iv) == H * (H + 1) // 2 and cost.dtype == np.int64 and int(cost.min()) >= 0
    return dict(zip(iv, cost.tolist()))


def check_brute_force(kind, L, H, cpu):
    """s2s_sdtw (forward and reverse) against the minimum over the intervals; the reverse problem is the forward one on reversed
    copies with start = H - end', end = H - start'."""
    q, t = make(kind, L, H)
    for rev in (False, True):
        cost, start, end = (int(v[0]) for v in CMP.sdtw([q], [t], reverse=rev, cpu=cpu))
        q1, t1 = (q[::-1].copy(), t[::-1].copy()) if rev else (q, t)
        s1, e1 = (H - end, H - start) if rev else (start, end)
        C = interval_costs(q1, t1, cpu)
        best = min(C.values())
        assert cost == best, (kind, L, H, rev)
        assert e1 == min(e for (_, e), c in C.items() if c == best), (kind, L, H, rev)
        assert 0 <= s1 < e1 <= H and C[(s1, e1)] == cost, (kind, L, H, rev)
        # the interval alone, through a launch of one pair
        assert int(CMP.dtw_banded([q1], [t1[s1:e1]], L, cpu=cpu)[0]) == cost


@pytest.mark.parametrize("L,H", BRUTE_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_sdtw_is_the_minimum_over_all_intervals(kind, L, H):
    check_brute_force(kind, L, H, cpu=True)


def test_band_L_covers_the_matrix_of_every_interval():
    """The premise of the brute force: at band L the banded cost of q against an interval is the unbanded one."""
    for kind, L, H, iv in (("squiggle", 5, 40, ((0, 40), (3, 4), (17, 29))), ("three", 12, 40, ((0, 40), (39, 40), (0, 11), (5, 18))),
                           ("extreme", 40, 12, ((0, 12), (4, 5), (2, 9))), ("three", 1, 40, ((0, 40), (8, 9))), ("squiggle", 7, 1, ((0, 1),))):
        q, t = make(kind, L, H)
        for s, e in iv:
            assert ref_dtw_full(q, t[s:e]) == ref_dtw(q, t[s:e], L) == int(CMP.dtw_banded([q], [t[s:e]], L, cpu=True)[0]), (kind, L, H, s, e)


# ------------------------------------------------------------------ B2: extreme slopes
def slope_pair(n, m):
    return dtw_pair(n, m, lo=-3, hi=4)


def check_slopes(cpu):
    """Every sloped shape alone and all of one band in one launch against the host entries: cost of s2s_dtw_banded; cost, ops and steps
    of s2s_dtw_path, with the invariants of the definition on every path.  (cpu=True: the host entries against themselves across
    the batchings.)"""
    by_band = {}
    for n, m, R in SLOPES:
        by_band.setdefault(R, []).append(slope_pair(n, m))
    for R, pairs in sorted(by_band.items()):
        al, bl = [p[0] for p in pairs], [p[1] for p in pairs]
        host_cost = CMP.dtw_banded(al, bl, R, cpu=True).tolist()
        host_path = CMP.dtw_path(al, bl, R, cpu=True)
        assert host_path[0].tolist() == host_cost
        assert CMP.dtw_banded(al, bl, R, cpu=cpu).tolist() == host_cost, R
        cost, ops = CMP.dtw_path(al, bl, R, cpu=cpu)
        assert cost.tolist() == host_cost and [o.tolist() for o in ops] == [o.tolist() for o in host_path[1]], R
        for k, (a, b) in enumerate(pairs):
            assert int(CMP.dtw_banded([a], [b], R, cpu=cpu)[0]) == host_cost[k], (len(a), len(b), R)
            c1, o1 = CMP.dtw_path([a], [b], R, cpu=cpu)
            assert int(c1[0]) == host_cost[k] and o1[0].dtype == np.uint8 and np.array_equal(o1[0], host_path[1][k]), (len(a), len(b), R)
            check_path(a, b, R, int(c1[0]), o1[0])


@pytest.mark.parametrize("n,m,R", SLOPES)
def test_host_entries_equal_the_restatement_at_extreme_slopes(n, m, R):
    a, b = slope_pair(n, m)
    want_cost, want_ops = ref_path(a, b, R)
    assert want_cost == ref_dtw(a, b, R)
    assert int(CMP.dtw_banded([a], [b], R, cpu=True)[0]) == want_cost == int(CMP.dtw_banded([b], [a], R, cpu=True)[0])
    cost, ops = CMP.dtw_path([a], [b], R, cpu=True)
    assert (int(cost[0]), ops[0].tolist()) == (want_cost, want_ops)
    check_path(a, b, R, want_cost, want_ops)
    # against a single sample the path has no choice and the cost is a plain sum
    if min(n, m) == 1:
        long_, one = (a, b) if m == 1 else (b, a)
        assert want_cost == int(np.abs(long_.astype(np.int64) - int(one[0])).sum())
        assert want_ops == [1 if m == 1 else 2] * (max(n, m) - 1)


def test_host_slopes_alone_and_in_one_launch():
    check_slopes(cpu=True)
