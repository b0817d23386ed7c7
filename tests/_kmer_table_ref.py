"""Restatements of `predict --kmer-table` in numpy / plain Python, shared by tests/test_kmer_table_cpu.py and
tests/test_gpu_kmer_table.py: `kmer_codes` is the table row of every k-mer slot, `ref_kmer_table` the definition of
s2s_kmer_table_accumulate as a reduction of s2s_event_stats' numbers, `py_table` the text of s2s_kmer_table_format
(include/s2s_hip.h states all three)."""
import math

import numpy as np

HEADER = ["kmer", "n_occ", "n_events", "n_samples", "level_mean", "level_stdv", "dwell_mean", "dwell_stdv"]
FIELDS = 6


def kmer_codes(flat: np.ndarray, chunk_start: np.ndarray, n_valid: np.ndarray, k: int, te: int) -> np.ndarray:
    """-> int64 [B, te]: the base-4 number of the k bytes at flat[chunk_start[b] + j ..] (A, C, G, T = 0..3, first letter most
    significant), 4^k for a k-mer with any other byte, -1 for a pad slot (j >= n_valid[b])."""
    lut = np.full(256, -1, np.int64)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    flat = np.concatenate([np.asarray(flat, np.uint8), np.zeros(te + k, np.uint8)])     # (pad slots may point past the end)
    idx = np.asarray(chunk_start, np.int64)[:, None, None] + np.arange(te)[None, :, None] + np.arange(k)[None, None, :]
    d = lut[flat[idx]]
    code = (np.maximum(d, 0) * (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))).sum(axis=2)
    code[(d < 0).any(axis=2)] = 4 ** k
    code[np.arange(te)[None, :] >= np.asarray(n_valid, np.int64)[:, None]] = -1
    return code


def ref_kmer_table(seg: np.ndarray, sums: np.ndarray, sumsq: np.ndarray, codes: np.ndarray, k: int) -> np.ndarray:
    """seg / sums / sumsq [B, te+1] (ref_event_stats or Engine.event_stats), codes [B, te] (kmer_codes) -> int64 [4^k + 1, 6]:
    occ, events, samples, samples_sq, sum, sumsq per row; the tail slot and the pad slots add nothing."""
    te = codes.shape[1]
    n = np.asarray(seg)[:, :te].astype(np.int64)
    S = np.asarray(sums)[:, :te].astype(np.int64)
    Q = np.asarray(sumsq)[:, :te].astype(np.int64)
    table = np.zeros((4 ** k + 1, FIELDS), np.int64)
    real = codes >= 0
    np.add.at(table[:, 0], codes[real], 1)
    ev = real & (n >= 1)
    for col, v in ((1, np.ones_like(n)), (2, n), (3, n * n), (4, S), (5, Q)):
        np.add.at(table[:, col], codes[ev], v[ev])
    return table


def kmer_name(code: int, k: int) -> str:
    return "N" * k if code == 4 ** k else "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def py_table(counts, k, digitisation, signal_range, offset, with_header=True) -> bytes:
    """The text of s2s_kmer_table_format from its column table, in Python integers: the products are exact, and float(int) is
    correctly rounded like the conversion of a 128-bit integer.  The calibration is the float32 the library is handed."""
    dig, rng, off = (float(np.float32(x)) for x in (digitisation, signal_range, offset))
    lines = ["\t".join(HEADER) + "\n"] if with_header else []
    for code in range(4 ** k + 1):
        occ, e, n, nn, S, Q = (int(x) for x in counts[code])
        if occ < 1:
            continue
        f = [kmer_name(code, k), str(occ), str(e), str(n)]
        if e == 0:
            f += ["nan"] * 4
        else:
            f += ["%.4f" % ((float(S) / float(n) + off) * rng / dig),
                  "%.4f" % (math.sqrt(float(max(n * Q - S * S, 0))) / float(n) * rng / dig),
                  "%.4f" % (float(n) / float(e)),
                  "%.4f" % (math.sqrt(float(max(e * nn - n * n, 0))) / float(e))]
        lines.append("\t".join(f) + "\n")
    return "".join(lines).encode()


def parse_table(text: bytes):
    """-> {kmer: dict(n_occ, n_events, n_samples, and the four statistics as printed)}; checks the header."""
    rows = text.decode().splitlines()
    assert rows[0].split("\t") == HEADER
    out = {}
    for line in rows[1:]:
        f = line.split("\t")
        assert len(f) == len(HEADER) and f[0] not in out, line
        out[f[0]] = dict(n_occ=int(f[1]), n_events=int(f[2]), n_samples=int(f[3]), level_mean=f[4], level_stdv=f[5], dwell_mean=f[6],
                         dwell_stdv=f[7])
    return out
