"""Restatements of the base-to-signal alignment in numpy / plain Python, shared by tests/test_alignment_cpu.py and
tests/test_gpu_alignment.py: `ref_align` is the definition of s2s_align_chunks (include/s2s_hip.h), `py_format` the PAF line
of s2s_paf_format, `parse_line` the inverse used for the per-line invariants."""
import re

import numpy as np


def ref_align(signal: np.ndarray, dur: np.ndarray) -> np.ndarray:
    """signal float32 [B, ts], dur int32 [B, te] -> uint16 [B, te+1]: c[j] = min(ts, sum_{i<=j} max(dur[i], 0)) (int64: 64 dwells of
    2^31 - 1 do not wrap), segment j = rows [c[j-1], c[j]), the tail [c[te-1], ts); every entry counts the rows != 0.0 (numpy: -0.0
    is zero, a subnormal is not)."""
    B, ts = signal.shape
    te = dur.shape[1]
    c = np.minimum(np.cumsum(np.maximum(dur.astype(np.int64), 0), axis=1), ts)
    P = np.zeros((B, ts + 1), np.int64)                       # P[b, x] = non-zero rows in [0, x)
    np.cumsum(signal != 0.0, axis=1, out=P[:, 1:])
    Pc = np.take_along_axis(P, c, axis=1)
    out = np.empty((B, te + 1), np.int64)
    out[:, :te] = np.diff(Pc, axis=1, prepend=0)
    out[:, te] = P[:, ts] - Pc[:, -1]
    assert out.min() >= 0 and out.max() <= 1024
    return out.astype(np.uint16)


def py_format(seg, te, read_first, read_kmers, read_offs, ids, rna) -> bytes:
    """The PAF text of s2s_paf_format, from its column table, one read at a time."""
    seg = np.asarray(seg).reshape(-1, te + 1)
    lines, rec = [], 0
    for r in range(len(read_first) - 1):
        n = int(read_offs[r + 1] - read_offs[r])
        if n == 0:                                            # no samples: no record, no line
            continue
        rid, K = ids[rec], int(read_kmers[r])
        rec += 1
        events = []                                           # (belongs to a real k-mer, samples) in forward order
        for i, c in enumerate(range(int(read_first[r]), int(read_first[r + 1]))):
            events += [(i * te + j < K, int(seg[c, j])) for j in range(te)]
            events.append((False, int(seg[c, te])))
        assert sum(c for _, c in events) == n
        if rna:                                               # the stored signal is reversed per read
            events.reverse()
        kpos = [i for i, (km, _) in enumerate(events) if km]
        first, last = kpos[0], kpos[-1]
        sig_start = sum(c for _, c in events[:first])
        sig_end = n - sum(c for _, c in events[last + 1:])
        toks = []                                             # [kind, value]; adjacent D / I merge
        for km, c in events[first:last + 1]:
            kind = ("," if c else "D") if km else ("I" if c else None)
            if kind is None:
                continue
            val = 1 if kind == "D" else c
            if kind != "," and toks and toks[-1][0] == kind:
                toks[-1][1] += val
            else:
                toks.append([kind, val])
        ss = "".join(f"{v}{k}" for k, v in toks)
        mapped = sum(1 for km, c in events if km and c)
        ks, ke = (K, 0) if rna else (0, K)
        lines.append("\t".join(map(str, [rid, n, sig_start, sig_end, "+", rid, K, ks, ke, mapped, K, 255, "ss:Z:" + ss])) + "\n")
    assert rec == len(ids)
    return "".join(lines).encode()


def parse_line(line: str) -> dict:
    """One PAF line -> its columns and the `ss` tokens [(count, kind)]; checks the three invariants every line must hold."""
    f = line.rstrip("\n").split("\t")
    assert len(f) == 13 and f[4] == "+" and f[11] == "255" and f[12].startswith("ss:Z:") and f[0] == f[5] and f[6] == f[10], line
    ss = f[12][5:]
    toks = [(int(n), k) for n, k in re.findall(r"(\d+)([,DI])", ss)]
    assert "".join(f"{n}{k}" for n, k in toks) == ss and all(n >= 1 for n, _ in toks), ss
    for (_, a), (_, b) in zip(toks, toks[1:]):
        assert not (a == b and a in "DI"), ss                 # runs are merged
    assert toks[0][1] != "I" and toks[-1][1] != "I", ss       # end insertions are trimmed, k-mers never
    d = dict(read_id=f[0], n=int(f[1]), sig_start=int(f[2]), sig_end=int(f[3]), K=int(f[6]), kmer_start=int(f[7]),
             kmer_end=int(f[8]), mapped=int(f[9]), toks=toks)
    n_match = sum(1 for _, k in toks if k == ",")
    assert n_match + sum(n for n, k in toks if k == "D") == d["K"], line
    assert sum(n for n, k in toks if k in ",I") == d["sig_end"] - d["sig_start"], line
    assert d["mapped"] == n_match and 0 <= d["sig_start"] <= d["sig_end"] <= d["n"], line
    return d


def kmer_counts(d: dict) -> list:
    """Samples of every k-mer in the order of the line's walk (0 for the k-mers of a D run)."""
    out = []
    for n, k in d["toks"]:
        if k == ",":
            out.append(n)
        elif k == "D":
            out += [0] * n
    return out
