"""The warping path of `compare --path` (include/s2s_hip.h, next to s2s_dtw_banded) restated in Python integers: every in-band D in
a dict of cells, the walk back with the tie rule, the boundary map and the transfer of an event table.  Slow and obvious on purpose;
what the host entry (s2s_dtw_path_host) and the kernels are held to, bit for bit."""
import math

import numpy as np

from _dtw_ref import INF, in_band

OPS = "MAB"                      # op codes 0, 1, 2


def ref_path(a, b, R):
    """-> (cost, ops): cost as ref_dtw (-1 for an empty member, INF for an unreached corner); ops the list of op codes forward from
    (0, 0), [] for a pair without path."""
    a = [int(v) for v in np.asarray(a).reshape(-1)]
    b = [int(v) for v in np.asarray(b).reshape(-1)]
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return -1, []
    D = {}
    for i in range(n):
        for j in range(m):
            if not in_band(i, j, n, m, R):
                continue
            best = 0 if i == 0 and j == 0 else INF
            for p in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if p in D:
                    best = min(best, D[p])
            D[(i, j)] = INF if best >= INF else best + abs(a[i] - b[j])
    cost = D.get((n - 1, m - 1), INF)
    if cost >= INF:
        return cost, []
    back = []
    i, j = n - 1, m - 1
    while (i, j) != (0, 0):
        best = None
        for op, p in ((0, (i - 1, j - 1)), (1, (i - 1, j)), (2, (i, j - 1))):          # the order of preference: '<' keeps the earlier
            if p in D and D[p] < INF and (best is None or D[p] < best[0]):
                best = (D[p], op, p)
        back.append(best[1])
        i, j = best[2]
    return cost, back[::-1]


def ref_cells(ops):
    """-> the list of cells (i, j) a path visits, (0, 0) first."""
    cells = [(0, 0)]
    for op in ops:
        i, j = cells[-1]
        cells.append((i + (op != 2), j + (op != 1)))
    return cells


def check_path(a, b, R, cost, ops):
    """The invariants of the definition, for a pair of non-empty signals with a reached corner."""
    n, m = len(a), len(b)
    ops = [int(o) for o in ops]
    assert set(ops) <= {0, 1, 2}
    assert max(n, m) - 1 <= len(ops) <= n + m - 2
    assert ops.count(0) + ops.count(1) == n - 1 and ops.count(0) + ops.count(2) == m - 1
    cells = ref_cells(ops)
    assert cells[-1] == (n - 1, m - 1)
    assert all(in_band(i, j, n, m, R) for i, j in cells)
    assert sum(abs(int(a[i]) - int(b[j])) for i, j in cells) == cost


def ref_boundary_map(ops, n, m):
    """g[0] = 0, g[n] = m, else the smallest j with (i, j) on the path."""
    g = [None] * (n + 1)
    for i, j in ref_cells(ops):
        if g[i] is None or j < g[i]:
            g[i] = j
    g[0], g[n] = 0, m
    assert None not in g and all(x <= y for x, y in zip(g, g[1:]))
    return g


def ref_path_string(ops):
    if not len(ops):
        return "*"
    out, k = [], 0
    ops = [int(o) for o in ops]
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append(f"{e - k}{OPS[ops[k]]}")
        k = e
    return "".join(out)


def ref_transfer_events(rid, rows, g, b, digitisation, offset, signal_range):
    """rows: (position, model_kmer, start_idx, end_idx) of one read of A -> (lines, dropped): [start, end) through g, the level and
    deviation of the event table from b's stored samples in [g[start], g[end])."""
    lines, dropped = [], 0
    for pos, kmer, s, e in rows:
        s2, e2 = g[s], g[e]
        if e2 <= s2:
            dropped += 1
            continue
        x = [int(v) for v in b[s2:e2]]
        n, S, Q = len(x), sum(x), sum(v * v for v in x)
        mean = (float(S) / n + offset) * signal_range / digitisation
        stdv = math.sqrt(float(n * Q - S * S)) / n * signal_range / digitisation
        lines.append(f"{rid}\t{pos}\t{kmer}\t{s2}\t{e2}\t{'%.4f' % mean}\t{'%.4f' % stdv}\n")
    return lines, dropped
