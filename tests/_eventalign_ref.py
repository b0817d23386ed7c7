"""The definitions of `eventalign` (include/s2s_hip.h, next to s2s_event_means and s2s_eventalign) restated in plain Python integers:
the event means, the adaptive-band alignment of normalised event means to normalised levels with its walk back, the consequences a
solved read is held to, the full chain segment -> means -> normalise -> align, and the planted reads the tests share."""
import numpy as np

import _segment_ref as SR

UNKNOWN, UNREACHED, EMPTY, TOO_LONG = -32768, -3, -1, -2
INF = 1 << 62
DIAG, STAY, SKIP, START = 0, 1, 2, 3
SKIP_PENALTY, TRIM_PENALTY, UNKNOWN_COST = 128, 64, 64
SCALE = 64


# ------------------------------------------------------------------ event means
def round_half_even_div(S: int, n: int) -> int:
    """round-half-even(S / n) for n >= 1, in integers."""
    q, r = divmod(int(S), int(n))                       # floor division: 0 <= r < n
    if 2 * r > n or (2 * r == n and q % 2):
        q += 1
    return q


def event_means(S, ev_len, ev_offs, n_events):
    """-> (m_offs [R + 1], means): record r gives n_events[r] means when 0 < n_events[r] <= its slot, else none; an event of no
    samples has mean 0; a mean is clamped to int16 (a sum of n int16 samples never needs it)."""
    m_offs, means = [0], []
    for r, ne in enumerate(n_events):
        ne = int(ne)
        if ne < 0 or ev_offs[r] < 0 or ne > ev_offs[r + 1] - ev_offs[r]:
            ne = 0
        for e in range(ne):
            n = int(ev_len[ev_offs[r] + e])
            x = round_half_even_div(S[ev_offs[r] + e], n) if n >= 1 else 0
            means.append(max(-32768, min(32767, x)))
        m_offs.append(m_offs[-1] + ne)
    return m_offs, means


# ------------------------------------------------------------------ the alignment
def solve(m, l, W, skip_penalty, trim_penalty, unknown_cost, ev_start=None, ev_len=None):
    """-> dict(cost, first, end, kmer [E], k_start [K], k_len [K], k_events [K]) by the definition.  ev_start / ev_len: the events'
    samples (default: event e is sample e)."""
    m, l = [int(x) for x in m], [int(x) for x in l]
    E, K = len(m), len(l)
    ev_start = list(range(E)) if ev_start is None else [int(x) for x in ev_start]
    ev_len = [1] * E if ev_len is None else [int(x) for x in ev_len]
    out = dict(cost=EMPTY, first=0, end=0, kmer=[-1] * E, k_start=[-1] * K, k_len=[0] * K, k_events=[0] * K)
    if E == 0 or K == 0:
        return out

    def cost(e, j):
        return unknown_cost if l[j] == UNKNOWN else abs(m[e] - l[j])

    bands = E + K - 1
    lk = [-(W // 2)]
    D = []                                              # D[b][o], INF: unreached or outside the matrix
    code = []
    best, best_e = INF, -1
    for b in range(bands):
        if b >= 1:
            ll, ur = D[b - 1][0], D[b - 1][W - 1]
            right = (b % 2 == 1) if (ll >= INF and ur >= INF) else ll > ur
            lk.append(lk[b - 1] + (1 if right else 0))
        row, crow = [INF] * W, [START] * W

        def at(bb, j):
            """D of k-mer j in band bb: only a cell inside its own band that is reached counts."""
            if bb < 0:
                return INF
            o = j - lk[bb]
            return D[bb][o] if 0 <= o < W else INF
        for o in range(W):
            j = lk[b] + o
            e = b - j
            if not (0 <= j < K and 0 <= e < E):
                continue
            c = cost(e, j)
            cand = [INF] * 4
            if j >= 1 and at(b - 2, j - 1) < INF:
                cand[DIAG] = at(b - 2, j - 1) + c
            if at(b - 1, j) < INF:                      # (e - 1, j) lies in band b - 1
                cand[STAY] = at(b - 1, j) + c
            if j >= 1 and at(b - 1, j - 1) < INF:       # (e, j - 1) too
                cand[SKIP] = at(b - 1, j - 1) + skip_penalty
            if j == 0:
                cand[START] = e * trim_penalty + c
            v = min(cand)
            if v < INF:
                row[o], crow[o] = v, cand.index(v)      # index(): the first of equal candidates
                if j == K - 1:
                    f = v + (E - 1 - e) * trim_penalty
                    if f < best:                        # bands ascend, so e does: '<' keeps the smallest e
                        best, best_e = f, e
        D.append(row)
        code.append(crow)
    if best >= INF:
        out["cost"] = UNREACHED
        return out
    out["cost"], out["end"] = best, best_e + 1
    e, j, run, hi = best_e, K - 1, 0, -1
    for _ in range(E + K + 1):
        b = e + j
        c = code[b][j - lk[b]]
        if c == SKIP:
            assert run == 0 and j >= 1
            j -= 1
            continue
        out["kmer"][e] = j
        if run == 0:
            hi = e
        run += 1
        if c == STAY:
            e -= 1
            continue
        out["k_start"][j], out["k_len"][j], out["k_events"][j] = ev_start[e], ev_start[hi] + ev_len[hi] - ev_start[e], run
        run = 0
        if c == START:
            assert j == 0
            out["first"] = e
            break
        e, j = e - 1, j - 1
    else:
        raise AssertionError("the walk did not end")
    return out


def check_consequences(m, l, skip_penalty, trim_penalty, unknown_cost, r, ev_start=None, ev_len=None):
    """The consequences include/s2s_hip.h holds a solved read to; r: a result like solve()'s."""
    m, l = np.asarray(m, np.int64), np.asarray(l, np.int64)
    E, K = len(m), len(l)
    kmer = np.asarray(r["kmer"], np.int64)
    first, end = int(r["first"]), int(r["end"])
    assert r["cost"] >= 0 and 0 <= first < end <= E
    assert (kmer[first:end] >= 0).all() and (kmer[:first] == -1).all() and (kmer[end:] == -1).all()
    a = kmer[first:end]
    assert (np.diff(a) >= 0).all() and a[0] == 0 and a[-1] <= K - 1
    used = np.unique(a)
    lev = l[a]
    cell = np.where(lev == UNKNOWN, unknown_cost, np.abs(m[first:end] - lev))
    assert int(cell.sum()) + skip_penalty * (K - len(used)) + trim_penalty * (first + E - end) == r["cost"]
    ev_start = np.arange(E) if ev_start is None else np.asarray(ev_start, np.int64)
    ev_len = np.ones(E, np.int64) if ev_len is None else np.asarray(ev_len, np.int64)
    ks, kl, ke = (np.asarray(r[k], np.int64) for k in ("k_start", "k_len", "k_events"))
    gone = np.setdiff1d(np.arange(K), used)
    assert (ks[gone] == -1).all() and (kl[gone] == 0).all() and (ke[gone] == 0).all()
    assert (ke[used] == np.bincount(a, minlength=K)[used]).all() and int(ke.sum()) == end - first
    fe = first + np.concatenate([[0], np.cumsum(ke[used])[:-1]])            # every unskipped k-mer's first event
    le = fe + ke[used] - 1
    assert (ks[used] == ev_start[fe]).all() and (kl[used] == ev_start[le] + ev_len[le] - ev_start[fe]).all()
    if (ev_start[1:] == ev_start[:-1] + ev_len[:-1]).all():                  # abutting events: the unskipped k-mers' intervals abut
        assert (ks[used][1:] == ks[used][:-1] + kl[used][:-1]).all()


def scratch_bytes(E, K, W):
    """s2s_eventalign_scratch_bytes: per band W / 64 word pairs of 16 bytes and one int32, rounded up to 16."""
    if E < 1 or K < 1 or E > (1 << 22) or K > (1 << 22):
        return 0
    bands = E + K - 1
    return (bands * (W // 64) * 16 + bands * 4 + 15) // 16 * 16


# ------------------------------------------------------------------ normalisation and the chain
def median_mad(x):
    """The lower median and the lower median of |x - med| (include/s2s_hip.h, compare); 0, 0 for no values."""
    x = sorted(int(v) for v in x)
    if not x:
        return 0, 0
    med = x[(len(x) - 1) // 2]
    return med, sorted(abs(v - med) for v in x)[(len(x) - 1) // 2]


def normalise(x, med, mad, scale=SCALE):
    d = max(mad, 1)
    return [max(-32767, min(32767, (2 * (int(v) - med) * scale + d) // (2 * d))) for v in x]


def chain(signal, levels, known, W, skip_penalty=SKIP_PENALTY, trim_penalty=TRIM_PENALTY, unknown_cost=UNKNOWN_COST,
          seg=(3, 6, 501, 20736)):
    """segment -> means -> normalise -> align of one record, all in Python integers.  levels: int [K] (64 x pA); known: bool [K].
    seg: (w_short, w_long, T_short, T_long), default the thresholds 1.4 and 9.0.  -> solve()'s dict plus ev_start / ev_len / m / lq."""
    x = [int(v) for v in signal]
    st, ln = SR.events(x, *seg)
    S = [sum(x[a:a + n]) for a, n in zip(st, ln)]
    _, means = event_means(S, ln, [0, len(st)], [len(st)])
    m = normalise(means, *median_mad(means))
    lv = [int(v) for v in levels]
    lmed, lmad = median_mad([v for v, k in zip(lv, known) if k])
    lq = [q if k else UNKNOWN for q, k in zip(normalise(lv, lmed, lmad), known)]
    r = solve(m, lq, W, skip_penalty, trim_penalty, unknown_cost, st, ln)
    r.update(ev_start=st, ev_len=ln, m=m, lq=lq)
    return r


# ------------------------------------------------------------------ shared inputs
PLANTED = [(30, 0, 100), (70, 200, 0), (150, 400, 300), (150, 900, 900), (300, 1500, 0), (40, 250, 250)]     # (K, head, tail) samples


def planted_read(K, head, tail, seed=0):
    """-> (adc int16 [n], levels_pA float [K], bounds int [K + 1]): k-mer j holds the samples [bounds[j], bounds[j + 1]) of the record,
    head junk in front and tail junk behind.  Levels uniform in 60-120 pA with neighbours at least 4 pA apart, dwell 12-40 samples, no
    noise; junk in runs of 12-40 samples around 190 +- 6 pA (head) and 10 +- 6 pA (tail); ADC = rint(pA 8192 / 1400 - 200)."""
    rng = np.random.default_rng([K, head, tail, seed])
    lev = np.zeros(K)
    for j in range(K):
        while True:
            lev[j] = rng.uniform(60, 120)
            if j == 0 or abs(lev[j] - lev[j - 1]) >= 4:
                break
    dwell = rng.integers(12, 41, K)

    def junk(n, centre):
        out = []
        while len(out) < n:
            out += [centre + rng.uniform(-6, 6)] * int(rng.integers(12, 41))
        return out[:n]
    pa = np.array(junk(head, 190.0) + list(np.repeat(lev, dwell)) + junk(tail, 10.0))
    adc = np.rint(pa * 8192 / 1400 - 200).astype(np.int16)
    bounds = head + np.concatenate([[0], np.cumsum(dwell)])
    return adc, lev, bounds


def random_case(E, K, kind, seed=0):
    """-> (m int16 [E], l int16 [K]) of a kind: `noisy` (event means that follow the levels with a random dwell, junk at both ends),
    `zeros`, `unknown` (every third level unknown), `extreme` (int16 extremes)."""
    rng = np.random.default_rng([E, K, ("noisy", "zeros", "unknown", "extreme").index(kind), seed])
    if kind == "zeros":
        return np.zeros(E, np.int16), np.zeros(K, np.int16)
    if kind == "extreme":
        return rng.choice(np.array([-32767, 32767, -32768, 0], np.int16), E), rng.choice(np.array([-32767, 32767], np.int16), K)
    lev = rng.integers(-200, 200, K).astype(np.int16)
    if K and E:
        head = int(rng.integers(0, E // 3 + 1))
        tail = int(rng.integers(0, E // 3 + 1))
        j = np.minimum(np.arange(E - head - tail) * K // max(E - head - tail, 1), K - 1)
        m = np.concatenate([rng.integers(250, 400, head), lev[j].astype(np.int64) + rng.integers(-25, 26, len(j)),
                            rng.integers(-400, -250, tail)]).astype(np.int16)
    else:
        m = rng.integers(-200, 200, E).astype(np.int16)
    if kind == "unknown":
        lev = lev.copy()
        lev[2::3] = UNKNOWN
    return m, lev
