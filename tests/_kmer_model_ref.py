"""Restatements of `predict --kmer-model` in Python integers, shared by tests/test_kmer_model_cpu.py and
tests/test_gpu_kmer_model.py: `event_fixed` is the definition of s2s_event_fixed, `ref_kmer_model` that of s2s_kmer_model_accumulate
as a reduction of s2s_event_stats' numbers, `py_model` the text of s2s_kmer_model_format (include/s2s_hip.h states all three).  The
row of a k-mer is `kmer_codes` of tests/_kmer_table_ref.py."""
import math
import re

import numpy as np

from _kmer_table_ref import kmer_codes, kmer_name  # noqa: F401  (kmer_codes: re-exported for the tests)

COLUMNS = ["kmer", "level_mean", "level_stdv", "sd_mean", "sd_stdv", "n_events"]
FIELDS = 5


def event_fixed(n: int, S: int, Q: int):
    """-> (M, D): M = round-half-even(256 S / n), D = isqrt(floor((n Q - S^2) 2^16 / n^2)), in Python integers."""
    n, S, Q = int(n), int(S), int(Q)
    num = 256 * S
    q, r = divmod(num, n)                                      # floor division: 0 <= r < n
    if 2 * r > n or (2 * r == n and q % 2 == 1):
        q += 1
    V = n * Q - S * S
    assert V >= 0
    return q, math.isqrt((V << 16) // (n * n))


def ref_kmer_model(seg: np.ndarray, sums: np.ndarray, sumsq: np.ndarray, codes: np.ndarray, k: int) -> np.ndarray:
    """seg / sums / sumsq [B, te+1] (ref_event_stats or Engine.event_stats), codes [B, te] (kmer_codes) -> int64 [4^k + 1, 5]:
    events, sum_m, sum_m2, sum_d, sum_d2 per row; slots without samples, the tail slot and the pad slots add nothing."""
    return reduce_by_code(*fixed_of_slots(seg, sums, sumsq, codes.shape[1]), codes, k)


def fixed_of_slots(seg, sums, sumsq, te):
    """-> (has int64 [B, te]: 1 where the slot has samples, M, D int64 [B, te]: event_fixed of every such slot, 0 elsewhere)."""
    n = np.asarray(seg)[:, :te].astype(np.int64)
    S = np.asarray(sums)[:, :te].astype(np.int64)
    Q = np.asarray(sumsq)[:, :te].astype(np.int64)
    M, D = np.zeros_like(n), np.zeros_like(n)
    for b, j in zip(*np.nonzero(n >= 1)):
        M[b, j], D[b, j] = event_fixed(n[b, j], S[b, j], Q[b, j])
    return (n >= 1).astype(np.int64), M, D


def reduce_by_code(has, M, D, codes, k) -> np.ndarray:
    """The five sums per row (all far inside int64 for the tests' sizes: M^2, D^2 <= 2^46)."""
    table = np.zeros((4 ** k + 1, FIELDS), np.int64)
    ev = (codes >= 0) & (has > 0)
    for col, v in enumerate((has, M, M * M, D, D * D)):
        np.add.at(table[:, col], codes[ev], v[ev])
    return table


def py_model(counts, k, digitisation, signal_range, offset, with_header=True) -> bytes:
    """The text of s2s_kmer_model_format from its column table, in Python integers: the products are exact, and float(int) is
    correctly rounded like the conversion of a 128-bit integer.  The calibration is the float32 the library is handed."""
    dig, rng, off = (float(np.float32(x)) for x in (digitisation, signal_range, offset))
    lines = [f"#k\t{k}\n", "#alphabet\tnucleotide\n", "\t".join(COLUMNS) + "\n"] if with_header else []
    for code in range(4 ** k):                                 # (the extra row 4^k is never printed)
        e, A, A2, Bs, B2 = (int(x) for x in counts[code])
        if e < 1:
            continue
        den = 256.0 * e
        lines.append("\t".join([kmer_name(code, k),
                                "%.4f" % ((float(A) / den + off) * rng / dig),
                                "%.4f" % (math.sqrt(float(max(e * A2 - A * A, 0))) / den * rng / dig),
                                "%.4f" % (float(Bs) / den * rng / dig),
                                "%.4f" % (math.sqrt(float(max(e * B2 - Bs * Bs, 0))) / den * rng / dig),
                                str(e)]) + "\n")
    return "".join(lines).encode()


def parse_model(text: bytes):
    """-> (k, {kmer: dict(level_mean, level_stdv, sd_mean, sd_stdv as printed, n_events)}); checks the header."""
    rows = text.decode().splitlines()
    assert re.fullmatch(r"#k\t\d+", rows[0]) and rows[1] == "#alphabet\tnucleotide" and rows[2].split("\t") == COLUMNS
    out = {}
    for line in rows[3:]:
        f = line.split("\t")
        assert len(f) == len(COLUMNS) and f[0] not in out, line
        out[f[0]] = dict(level_mean=f[1], level_stdv=f[2], sd_mean=f[3], sd_stdv=f[4], n_events=int(f[5]))
    return int(rows[0].split("\t")[1]), out


def header_constants(header_text: str) -> dict:
    """The S2S_KMER_MODEL_* integers of include/s2s_hip.h: the cache geometry the GPU tests size their batches from."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define S2S_KMER_MODEL_(\w+)\s+(\d+)u?\b", header_text)}


def cache_slot(code: int, c: dict) -> int:
    """The first cache slot of a code on the hashed path (k > DIRECT_MAX_K), as the header states it."""
    return (((code * c["HASH_MUL"]) & 0xFFFFFFFF) * c["SLOTS"]) >> 32
