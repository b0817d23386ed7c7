"""The definition of `segment` (include/s2s_hip.h, next to s2s_segment) restated in plain Python integers -- arbitrary precision, no
numpy arithmetic in the score -- and the formatting of its table.  Written from the definition, not from the C++."""
import math

COLUMNS = ("read_name", "event_index", "start_idx", "end_idx", "event_level_mean", "event_stdv")
MAX_SAMPLES = 1 << 22


def ints(x):
    return [int(v) for v in x]


def scores(x, w):
    """score_w(i) for i = 0 .. n as Python ints."""
    x = ints(x)
    n = len(x)
    sc = [0] * (n + 1)
    for i in range(w, n - w + 1):
        L, R = x[i - w:i], x[i:i + w]
        SL, SR, QL, QR = sum(L), sum(R), sum(v * v for v in L), sum(v * v for v in R)
        d = SR - SL
        V = w * (QL + QR) - SL * SL - SR * SR
        assert V >= 0 and 256 * w * d * d < 1 << 56 and V < 1 << 42
        sc[i] = (256 * w * d * d) // max(V, 1)
    return sc


def peaks(sc, w, T):
    """The peaks of one detector: positions i of sc [n + 1]."""
    n = len(sc) - 1
    out = []
    for i in range(n + 1):
        if sc[i] < T:
            continue
        if all(sc[i] > sc[j] for j in range(max(0, i - w), i)) and all(sc[i] >= sc[j] for j in range(i + 1, min(n, i + w) + 1)):
            out.append(i)
    return out


def boundaries(x, w_s, w_l, T_s, T_l):
    short = peaks(scores(x, w_s), w_s, T_s)
    long_ = peaks(scores(x, w_l), w_l, T_l)
    keep = set(short)
    for p in long_:
        if not any(abs(p - q) <= w_s for q in short):
            keep.add(p)
    return sorted(keep)


def events(x, w_s, w_l, T_s, T_l):
    """-> (starts, lengths) of the record's events."""
    n = len(x)
    if n == 0:
        return [], []
    cuts = [0] + boundaries(x, w_s, w_l, T_s, T_l) + [n]
    return cuts[:-1], [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def capacity(n, w_s):
    return 0 if n == 0 else max(1, n // w_s)


def check_consequences(n, starts, lengths, w_s):
    """What the definition implies for any record: the events abut, sum to n, respect the minimum lengths and the capacity."""
    assert len(starts) == len(lengths) <= capacity(n, w_s)
    if n == 0:
        assert not starts
        return
    at = 0
    for k, (s, l) in enumerate(zip(starts, lengths)):
        assert s == at and l >= 1
        at += l
        if len(starts) > 1:
            assert l >= (w_s if k in (0, len(starts) - 1) else w_s + 1), (k, l)
    assert at == n


def threshold_int(t):
    return int(math.floor(256.0 * float(t) * float(t)))


def rows(rid, x, starts, lengths, cal):
    """The rows of one record: levels in pA from the record's own (digitisation, offset, range), the formulas of compare --events-out."""
    digitisation, offset, signal_range = cal
    x = ints(x)
    out = []
    for k, (s, n) in enumerate(zip(starts, lengths)):
        S, Q = sum(x[s:s + n]), sum(v * v for v in x[s:s + n])
        mean = (float(S) / n + offset) * signal_range / digitisation
        stdv = math.sqrt(float(max(n * Q - S * S, 0))) / n * signal_range / digitisation
        out.append(f"{rid}\t{k}\t{s}\t{s + n}\t{'%.4f' % mean}\t{'%.4f' % stdv}\n")
    return "".join(out)


def table(records, w_s, w_l, T_s, T_l):
    """records: [(read id, int16 samples, (digitisation, offset, range))] -> (the event table, the summary table) as text; a record of
    more than 2^22 samples gives no rows and 0 events."""
    out, summary = ["\t".join(COLUMNS) + "\n"], ["read_name\tn_samples\tn_events\n"]
    for rid, x, cal in records:
        st, ln = events(x, w_s, w_l, T_s, T_l) if len(x) <= MAX_SAMPLES else ([], [])
        out.append(rows(rid, x, st, ln, cal))
        summary.append(f"{rid}\t{len(x)}\t{len(st)}\n")
    return "".join(out), "".join(summary)
