"""The definition of `resquiggle` (include/s2s_hip.h, next to s2s_resquiggle) restated in Python integers over the full matrix, the
invariants of a solved read, and the shapes and kinds of input the tests of the host twin and of the kernels share."""
import numpy as np

UNKNOWN, UNREACHED, EMPTY, TOO_LONG = -32768, -3, -1, -2
INF = 1 << 62


def solve(q, l, R, skip_penalty, unknown_cost):
    """-> (cost, start [K], len [K]) by the definition: full matrix, Python integers."""
    q, l = [int(x) for x in q], [int(x) for x in l]
    n, K = len(q), len(l)
    none = ([-1] * K, [0] * K)
    if n == 0 or K == 0:
        return (EMPTY, *none)
    if K > 2 * n:
        return (UNREACHED, *none)

    def cost(i, j):
        return unknown_cost if l[j] == UNKNOWN else abs(q[i] - l[j])

    def inside(i, j):
        return 0 <= j < K and abs(i * K - j * n) <= R * n

    D = [[INF] * K for _ in range(n)]
    D[0][0] = cost(0, 0)

    def terms(i, j):
        """The terms of the minimum in the order of the tie rule: advance, stay, skip."""
        out = []
        for dj, add in ((1, 0), (0, 0), (2, skip_penalty)):
            jj = j - dj
            out.append(D[i - 1][jj] + add if inside(i - 1, jj) and D[i - 1][jj] < INF else INF)
        return out

    for i in range(1, n):
        for j in range(K):
            if inside(i, j):
                best = min(terms(i, j))
                if best < INF:
                    D[i][j] = best + cost(i, j)
    if not inside(n - 1, K - 1) or D[n - 1][K - 1] >= INF:
        return (UNREACHED, *none)
    start, length = [-1] * K, [0] * K
    i, j = n - 1, K - 1
    while True:
        length[j] += 1
        if i == 0:
            assert j == 0
            start[0] = 0
            break
        t = terms(i, j)
        dj = (1, 0, 2)[t.index(min(t))]                 # index(): the first of equal terms
        if dj:
            start[j] = i
            j -= dj
        i -= 1
    return D[n - 1][K - 1], start, length


def check_invariants(q, l, R, skip_penalty, unknown_cost, cost, start, length):
    """The invariants of a solved read (include/s2s_hip.h)."""
    q, l = np.asarray(q, np.int64), np.asarray(l, np.int64)
    start, length = np.asarray(start, np.int64), np.asarray(length, np.int64)
    n, K = len(q), len(l)
    assert cost >= 0
    assert int(length.sum()) == n and start[0] == 0
    kept = np.flatnonzero(length > 0)
    skipped = np.flatnonzero(length == 0)
    assert (start[skipped] == -1).all()
    assert kept[0] == 0 and kept[-1] == K - 1
    assert (np.diff(kept) <= 2).all()                   # no two neighbours skipped
    assert (start[kept][1:] == start[kept][:-1] + length[kept][:-1]).all()      # ascend and abut
    total = skip_penalty * len(skipped)
    for j in kept:
        i = np.arange(start[j], start[j] + length[j])
        assert (np.abs(i * K - j * n) <= R * n).all()   # every visited cell is in the band
        total += unknown_cost * len(i) if l[j] == UNKNOWN else int(np.abs(q[i] - l[j]).sum())
    assert total == cost


SMALL = [(1, 1, 1), (5, 1, 1), (1, 2, 1), (2, 3, 2), (3, 7, 4), (7, 7, 1), (64, 64, 1), (65, 9, 1), (300, 40, 1), (300, 40, 3),
         (300, 290, 8), (200, 260, 16), (129, 64, 31), (129, 64, 32), (500, 70, 32), (1000, 200, 96),
         (100, 199, 31), (150, 299, 63)]     # K = 2 n - 1 past a ring of exactly 2 R + 2 slots: a slot's old column is active a row before its new one
LARGE = [(5000, 3, 1), (5000, 600, 31), (5000, 600, 32), (4097, 2100, 512), (3000, 2900, 1024), (2500, 4000, 1024), (20000, 1, 1024)]
EXTREME = (70000, 6000, 64)                             # samples 32767 against levels -32767: the cost passes 2^32
KINDS = ("planted", "noisy", "zeros", "unknown")
SKIP, UNK = 128, 64


def planted(n, K, R, rng):
    """-> (q, l, start, len) or None: samples that are exactly each level repeated by a drawn dwell >= 1, neighbouring levels distinct,
    the planted path inside the band.  Zero cost is then reached by one path only: a skip costs skip_penalty > 0, and in every row
    exactly one of `stay` (q[i] == l[j]) and `advance` (q[i] == l[j + 1] != l[j]) keeps the cost at zero."""
    if K > n:
        return None
    base = np.arange(K + 1, dtype=np.int64) * n // K            # strictly increasing: n >= K
    room = np.minimum(np.diff(base) - 1, (R - 1) * n // K)       # start[j] = base[j] + jitter stays below start[j + 1]
    for jitter in (rng.integers(0, room + 1), np.zeros(K, np.int64)):
        start = base[:K] + jitter
        start[0] = 0
        length = np.diff(np.concatenate([start, [n]]))
        j = np.repeat(np.arange(K), length)
        if (length >= 1).all() and (np.abs(np.arange(n) * K - j * n) <= R * n).all():
            break
    else:
        return None
    lev = np.where(np.arange(K) % 2 == 0, 1, -1) * rng.integers(1, 300, K)      # alternating signs: neighbours differ
    return lev[j].astype(np.int16), lev.astype(np.int16), start.astype(np.int32), length.astype(np.int32)


def case(n, K, R, kind, seed=0):
    """-> (q int16 [n], l int16 [K], planted (start, len) or None)."""
    rng = np.random.default_rng([n, K, R, KINDS.index(kind), seed])
    if kind == "planted":
        pl = planted(n, K, R, rng)
        if pl is not None:
            return pl[0], pl[1], (pl[2], pl[3])
        kind = "noisy"                                  # no planted path fits this shape (K > n, or a band too narrow)
    if kind == "zeros":
        return np.zeros(n, np.int16), np.zeros(K, np.int16), None
    lev = rng.integers(-300, 300, K).astype(np.int16)
    j = np.minimum(np.arange(n) * K // max(n, 1), K - 1) if K else np.zeros(n, np.int64)
    q = (lev[j].astype(np.int64) + rng.integers(-40, 41, n)).astype(np.int16) if K else rng.integers(-300, 300, n).astype(np.int16)
    if kind == "unknown":
        lev = lev.copy()
        lev[2::3] = UNKNOWN
    return q, lev, None
