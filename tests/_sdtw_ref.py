"""The definition of subsequence DTW (include/s2s_hip.h, next to s2s_sdtw) restated in Python integers: full rows of (E, S), plain
loops, for small shapes only.  What s2s_sdtw_host and the kernel are held to, bit for bit."""
import numpy as np


def ref_sdtw_forward(q, t):
    """-> (cost, start, end) of q inside t, front to back; (-1, 0, 0) when either is empty."""
    q = [int(v) for v in np.asarray(q).reshape(-1)]
    t = [int(v) for v in np.asarray(t).reshape(-1)]
    L, H = len(q), len(t)
    if L == 0 or H == 0:
        return -1, 0, 0
    E = [abs(q[0] - t[j]) for j in range(H)]                   # row 0 starts anywhere: no horizontal predecessor
    S = list(range(H))
    for i in range(1, L):
        pe, ps = E, S
        E, S = [0] * H, [0] * H
        for j in range(H):
            best = None                                        # (E, S) of the chosen predecessor
            if j > 0:
                best = (pe[j - 1], ps[j - 1])                  # (i - 1, j - 1)
            if best is None or pe[j] < best[0]:
                best = (pe[j], ps[j])                          # (i - 1, j)
            if j > 0 and E[j - 1] < best[0]:
                best = (E[j - 1], S[j - 1])                    # (i, j - 1)
            E[j], S[j] = best[0] + abs(q[i] - t[j]), best[1]
    js = min(range(H), key=lambda j: (E[j], j))                # the smallest j among the minima
    return E[js], S[js], js + 1


def ref_sdtw(q, t, reverse=False):
    """reverse: the same problem on q and t read back to front, the interval in forward coordinates of t."""
    if not reverse:
        return ref_sdtw_forward(q, t)
    q, t = np.asarray(q).reshape(-1), np.asarray(t).reshape(-1)
    cost, s, e = ref_sdtw_forward(q[::-1], t[::-1])
    return (cost, len(t) - e, len(t) - s) if cost >= 0 else (cost, 0, 0)
