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
         (100, 199, 31), (150, 299, 63)]     # K = 2 n - 1 past a ring of exactly 2 R + 2 slots: a slot's old column is active TWO rows before its new one (one row: K = 2 n, band_shapes)
LARGE = [(5000, 3, 1), (5000, 600, 31), (5000, 600, 32), (4097, 2100, 512), (3000, 2900, 1024), (2500, 4000, 1024), (20000, 1, 1024)]
EXTREME = (70000, 6000, 64)                             # samples 32767 against levels -32767: the cost passes 2^32
KINDS = ("planted", "noisy", "zeros", "unknown")
SKIP, UNK = 128, 64


MAX_WAVES = 16


def chunks(R):
    """Word pairs of a decision row (csrc/s2s_resquiggle.h): 64 slots each, ring = 64 chunks > 2 R + 1."""
    return (2 * R + 1 + 63) // 64


def per_wave(R):
    """The chunks are dealt out evenly over at most 16 waves: ceil(chunks / 16) to a wave."""
    return -(-chunks(R) // MAX_WAVES)


def waves(R):
    return -(-chunks(R) // per_wave(R))


# the smallest and the largest band of every chunk count 1 .. 33; the largest one has the tightest ring, 64 c == 2 R + 2
BANDS_BY_CHUNKS = [1, 31] + [R for c in range(2, 33) for R in (32 * (c - 1), 32 * c - 1)] + [1024]


def band_shapes(R):
    """-> [(n, K, kind)] of a band.  K = ring + 200 < n: the level window and the slots both wrap.  K = 2 n - 1 past the ring: the row's
    window moves by two columns, a slot's old column is active one row before its new one -- `zeros` as well: there every row but the
    first must skip and a skip is the only cost.  K = 2 n: i K mod n is 0 in every row, so a row holds all 2 R + 1 columns and its
    window moves by two -- with ring == 2 R + 2 the only case in which a slot's old column, jlo(i - 1), is active one row before its
    new one, jhi(i) = jlo(i - 1) + ring (at K = 2 n - 1 a row holds 2 R columns and the two are never a row apart).  No path covers
    2 n columns in n rows, so the answer is `unreached`; a value left over from the old column would make it a cost."""
    ring = 64 * chunks(R)
    K1, n2 = ring + 200, ring // 2 + 120
    return [(K1 + 150, K1, "planted"), (K1 + 150, K1, "noisy"), (n2, 2 * n2 - 1, "noisy"), (n2, 2 * n2 - 1, "unknown"),
            (n2, 2 * n2 - 1, "zeros"), (n2, 2 * n2, "noisy"), (n2, 2 * n2, "zeros")]


# (n, K, R) at which pressed() is solved along both edges of the band (tests/test_resquiggle_cpu.py asserts it on the host twin)
PRESSED_SMALL = [(7, 7, 1), (64, 64, 1), (65, 9, 1), (300, 40, 1), (300, 40, 3), (300, 290, 8), (200, 260, 16)]     # held to solve()
PRESSED = PRESSED_SMALL + [(5000, 600, 31), (5000, 600, 32), (4097, 2100, 512), (2600, 2400, 480), (2600, 2400, 511),
                           (4400, 4200, 992), (4400, 4200, 1023), (4400, 4200, 1024)]


def pressed(n, K, R):
    """-> (q, l) whose optimum is pressed against both edges of the band: noisy levels and samples, but the first third of the samples
    is exactly the first level and the last third exactly the last one, both far from every other level.  The path stays on k-mer 0 as
    long as the band lets it (the cells with jlo = ceil(i K / n) - R) and reaches k-mer K - 1 as soon as the band lets it (jhi =
    floor(i K / n) + R, then the clamp at K - 1).  Not one of KINDS: case() seeds by KINDS.index."""
    rng = np.random.default_rng([n, K, R, len(KINDS)])
    lev = rng.integers(-300, 300, K).astype(np.int16)
    lev[0], lev[K - 1] = 3000, -3000
    j = np.minimum(np.arange(n) * K // n, K - 1)
    q = (lev[j].astype(np.int64) + rng.integers(-40, 41, n)).astype(np.int16)
    q[:n // 3], q[n - n // 3:] = lev[0], lev[K - 1]
    return q, lev


def edge_contact(n, K, R, start, length):
    """-> (lower, upper): has the path a cell with i K - j n > (R - 1) n (no room for one more row on column j: the lower edge), and
    one with i K - j n < -(R - 1) n (the upper edge)?"""
    length = np.asarray(length, np.int64)
    j = np.repeat(np.arange(K, dtype=np.int64), length)
    d = np.arange(n, dtype=np.int64) * K - j * n
    assert len(j) == n
    return bool((d > (R - 1) * n).any()), bool((d < -(R - 1) * n).any())


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
