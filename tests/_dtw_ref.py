"""The definitions of `compare` (include/s2s_hip.h, next to s2s_dtw_banded) restated in numpy and Python integers: what the host
entries and the kernels are held to, bit for bit.  Slow on purpose (a plain double loop over the band's cells)."""
import numpy as np

SCALE = 64
INF = 1 << 62


def ref_median_mad(x):
    """-> (med, mad) of one int16 record: the elements of rank (n - 1) // 2 of the sorted samples and of the sorted |x - med|."""
    x = np.asarray(x, np.int64)
    n = len(x)
    if n == 0:
        return 0, 0
    k = (n - 1) // 2
    med = int(np.sort(x)[k])
    mad = int(np.sort(np.abs(x - med))[k])
    return med, mad


def ref_normalise(x, med, mad, scale=SCALE):
    """q = clamp(floor((2 (x - med) scale + d) / (2 d)), -32767, 32767), d = max(mad, 1) (numpy's // on int64 is a floor division)."""
    x = np.asarray(x, np.int64)
    d = max(int(mad), 1)
    q = (2 * (x - int(med)) * int(scale) + d) // (2 * d)
    return np.clip(q, -32767, 32767).astype(np.int16)


def in_band(i, j, n, m, R):
    return abs(i * m - j * n) <= R * max(n, m)


def ref_dtw(a, b, R):
    """D(n - 1, m - 1) over the cells with |i m - j n| <= R max(n, m); -1 when a or b is empty; INF when the corner is not reached."""
    a = [int(v) for v in np.asarray(a).reshape(-1)]
    b = [int(v) for v in np.asarray(b).reshape(-1)]
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return -1
    T = R * max(n, m)
    prev, prev_lo = [], 0
    for i in range(n):
        # the in-band columns of a row are contiguous: ceil((i m - T) / n) .. floor((i m + T) / n)
        jlo = max(0, -((T - i * m) // n))
        jhi = min(m - 1, (i * m + T) // n)
        assert jlo == 0 or not in_band(i, jlo - 1, n, m, R)
        assert jhi == m - 1 or not in_band(i, jhi + 1, n, m, R)
        cur = []
        for j in range(jlo, jhi + 1):
            best = 0 if i == 0 and j == 0 else INF
            for pj in (j, j - 1):                              # (i - 1, j), (i - 1, j - 1)
                if 0 <= pj - prev_lo < len(prev):
                    best = min(best, prev[pj - prev_lo])
            if j - 1 >= jlo:                                   # (i, j - 1)
                best = min(best, cur[j - 1 - jlo])
            cur.append(INF if best >= INF else best + abs(a[i] - b[j]))
        prev, prev_lo = cur, jlo
    return prev[m - 1 - prev_lo] if 0 <= m - 1 - prev_lo < len(prev) else INF


def ref_dtw_full(a, b):
    """Unbanded DTW: the same recurrence over the whole matrix."""
    a = [int(v) for v in np.asarray(a).reshape(-1)]
    b = [int(v) for v in np.asarray(b).reshape(-1)]
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return -1
    prev = None
    for i in range(n):
        cur = [0] * m
        for j in range(m):
            c = abs(a[i] - b[j])
            if i == 0 and j == 0:
                cur[j] = c
                continue
            best = INF
            if prev is not None:
                best = min(best, prev[j])
                if j:
                    best = min(best, prev[j - 1])
            if j:
                best = min(best, cur[j - 1])
            cur[j] = best + c
        prev = cur
    return prev[m - 1]


def ref_dtw_rows(a, b, R):
    """ref_dtw for the few large shapes, a row at a time in int64 numpy: entering row i at column k from above (up[k] = min(D(i-1, k),
    D(i-1, k-1))) and walking right to j costs up[k] + c[k] + ... + c[j], so D(i, j) = C[j] + min over k <= j of (up[k] - C[k] + c[k])
    with C the running sum of the row's costs.  Held to ref_dtw on the small shapes by tests/test_compare_cpu.py."""
    a = np.asarray(a, np.int64).reshape(-1)
    b = np.asarray(b, np.int64).reshape(-1)
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return -1
    T = R * max(n, m)
    prev, plo = np.zeros(0, np.int64), 0                       # D(i - 1, plo ...)
    for i in range(n):
        jlo = max(0, -((T - i * m) // n))
        jhi = min(m - 1, (i * m + T) // n)
        pv = np.full(jhi - jlo + 2, INF, np.int64)             # D(i - 1, jlo - 1 .. jhi), +infinity outside the previous row's range
        lo, hi = max(jlo - 1, plo), min(jhi, plo + len(prev) - 1)
        if lo <= hi:
            pv[lo - (jlo - 1):hi - (jlo - 1) + 1] = prev[lo - plo:hi - plo + 1]
        up = np.minimum(pv[1:], pv[:-1])
        if i == 0:
            up[0] = 0
        c = np.abs(a[i] - b[jlo:jhi + 1])
        C = np.cumsum(c)
        cur = C + np.minimum.accumulate(up - C + c)
        prev, plo = np.where(cur >= INF // 2, INF, cur), jlo
    return int(prev[m - 1 - plo]) if 0 <= m - 1 - plo < len(prev) else INF
