"""Restatements of `predict --events` in numpy / plain Python, shared by tests/test_events_cpu.py and tests/test_gpu_events.py:
`ref_dac` is the int16 the export stores for a sample, `ref_event_stats` the definition of s2s_event_stats, `py_events` the text of
s2s_events_format (include/s2s_hip.h states all three)."""
import math

import numpy as np

from _alignment_ref import ref_align

HEADER = ["read_name", "position", "model_kmer", "start_idx", "end_idx", "event_level_mean", "event_stdv"]


def ref_dac(signal: np.ndarray, digitisation, signal_range, offset) -> np.ndarray:
    """float32 pA -> the int16 s2s_export_reads stores (as int64): rint(v * dig / range - offset), every step rounded to float32,
    halves to even, clamped to what fits an int32, then wrapped to 16 bits."""
    v = np.asarray(signal, np.float32)
    with np.errstate(all="ignore"):                           # (a product beyond float32 is inf and clamps)
        raw = np.rint((v * np.float32(digitisation)) / np.float32(signal_range) - np.float32(offset))
    assert raw.dtype == np.float32
    i = np.clip(raw, np.float32(-2147483648.0), np.float32(2147483520.0)).astype(np.int64)
    return (i + 32768) % 65536 - 32768


def ref_event_stats(signal: np.ndarray, dur: np.ndarray, digitisation, signal_range, offset):
    """-> (seg uint16, sum int32, sumsq int64), each [B, te+1]: sample t of chunk b falls into slot #{j : c[j] <= t} (the tail is
    slot te), c as in ref_align; the sums run over the stored samples (signal != 0) in np.int64."""
    B, ts = signal.shape
    te = dur.shape[1]
    c = np.minimum(np.cumsum(np.maximum(dur.astype(np.int64), 0), axis=1), ts)
    q = ref_dac(signal, digitisation, signal_range, offset)
    q[signal == 0.0] = 0
    t = np.arange(ts)
    n = np.zeros((B, te + 1), np.int64)
    s = np.zeros((B, te + 1), np.int64)
    ss = np.zeros((B, te + 1), np.int64)
    for b in range(B):
        slot = np.searchsorted(c[b], t, side="right")
        np.add.at(n[b], slot, (signal[b] != 0.0).astype(np.int64))
        np.add.at(s[b], slot, q[b])
        np.add.at(ss[b], slot, q[b] * q[b])
    assert np.array_equal(n, ref_align(signal, dur).astype(np.int64))
    assert np.abs(s).max(initial=0) <= 2 ** 25 and ss.max(initial=0) <= 2 ** 40
    return n.astype(np.uint16), s.astype(np.int32), ss


def py_events(seg, sums, sumsq, te, read_first, read_kmers, read_offs, ids, seqs, k, digitisation, signal_range, offset, rna,
              dac=None, with_header=False) -> bytes:
    """The text of s2s_events_format from its column table, one read at a time.  seqs: the letters of every read; the calibration is
    the float32 the library is handed, widened to double."""
    seg = np.asarray(seg).reshape(-1, te + 1)
    sums = np.asarray(sums).reshape(-1, te + 1)
    sumsq = np.asarray(sumsq).reshape(-1, te + 1)
    dig, rng, off = (float(np.float32(x)) for x in (digitisation, signal_range, offset))
    lines, rec = [], 0
    if with_header:
        lines.append("\t".join(HEADER + (["samples"] if dac is not None else [])) + "\n")
    for r in range(len(read_first) - 1):
        L = int(read_offs[r + 1] - read_offs[r])
        if L == 0:
            continue
        rid, K = ids[rec], int(read_kmers[r])
        rec += 1
        cur = 0
        for i, c in enumerate(range(int(read_first[r]), int(read_first[r + 1]))):
            for j in range(te + 1):
                n = int(seg[c, j])
                s0, cur = cur, cur + n
                pos = i * te + j
                if n == 0 or j == te or pos >= K:
                    continue
                start, end = (L - (s0 + n), L - s0) if rna else (s0, s0 + n)
                S, Q = int(sums[c, j]), int(sumsq[c, j])
                mean = (float(S) / n + off) * rng / dig
                stdv = math.sqrt(float(max(n * Q - S * S, 0))) / n * rng / dig
                f = [rid, str(pos), seqs[r][pos:pos + k], str(start), str(end), "%.4f" % mean, "%.4f" % stdv]
                if dac is not None:
                    stored = dac[int(read_offs[r]) + start: int(read_offs[r]) + end]
                    f.append(",".join("%.3f" % ((float(x) + off) * rng / dig) for x in stored))
                lines.append("\t".join(f) + "\n")
        assert cur == L
    assert rec == len(ids)
    return "".join(lines).encode()


def parse_events(text: bytes, samples: bool):
    """-> [dict per row]; checks the header."""
    rows = text.decode().splitlines()
    assert rows[0].split("\t") == HEADER + (["samples"] if samples else [])
    out = []
    for line in rows[1:]:
        f = line.split("\t")
        assert len(f) == len(HEADER) + samples, line
        d = dict(read_name=f[0], position=int(f[1]), model_kmer=f[2], start_idx=int(f[3]), end_idx=int(f[4]), mean=f[5], stdv=f[6])
        if samples:
            d["samples"] = f[7].split(",")
        out.append(d)
    return out
