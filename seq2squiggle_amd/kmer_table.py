"""The k-mer table of a run (`predict --kmer-table OUT.tsv`): for every k-mer how often it occurred, how often it got stored samples,
the pooled mean and population deviation (ddof 0) of those samples in pA and the mean and deviation of its dwell (an event's stored
sample count) -- the form a published pore model (`kmer  level_mean  level_stdv ...`) and the k-mer level and dwell distributions of
a real run are compared in.  The six integer counters per k-mer are summed on the GPU (Engine.kmer_table_accumulate: integer
atomics, so the table does not depend on batching or sharding); only the finished table leaves the device, once per run, and the
library formats it (s2s_kmer_table_format; include/s2s_hip.h states the columns and the definitions).  The reference writes no such
file; the table is unvalidated against external tools -- DESIGN.md section 6."""
import os
from typing import Sequence

import numpy as np

FIELDS = 6          # occ, events, samples, samples_sq, sum, sumsq
MAX_K = 10


def _cal(digitisation, signal_range, offset):
    """The calibration as the float32 the library is handed."""
    return tuple(float(np.float32(x)) for x in (digitisation, signal_range, offset))


def format_table(counts: np.ndarray, k: int, digitisation: float, signal_range: float, offset: float,
                 with_header: bool = True) -> memoryview:
    """The text of a table (s2s_kmer_table_format): counts int64 [4^k + 1, 6], one row per k-mer that occurred, in code order, the
    row of k-mers with a letter outside ACGT last as k times N."""
    from ._lib import lib
    L = lib()
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be 1..{MAX_K}")
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if counts.shape != (4 ** k + 1, FIELDS):
        raise ValueError(f"counts must be int64 [{4 ** k + 1}, {FIELDS}]")
    cal = _cal(digitisation, signal_range, offset)
    cap = int(L.s2s_kmer_table_format_bound(counts.ctypes.data, k, *cal, int(bool(with_header))))
    if cap < 0:
        raise ValueError("digitisation and range must be non-zero numbers and no counter but sum negative")
    out = np.empty(max(cap, 1), np.uint8)
    got = L.s2s_kmer_table_format(counts.ctypes.data, k, *cal, int(bool(with_header)), out.ctypes.data, cap)
    if got < 0:
        raise RuntimeError(f"s2s_kmer_table_format failed ({got})")
    return memoryview(out)[:got]


def save_counts(path: str, counts: np.ndarray, k: int, digitisation: float, signal_range: float, offset: float) -> None:
    """The counters of one rank of a multi-process run: one .npz with the counts, k and the three calibration floats."""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if counts.shape != (4 ** int(k) + 1, FIELDS):
        raise ValueError(f"counts must be int64 [{4 ** int(k) + 1}, {FIELDS}]")
    with open(path, "wb") as f:                     # (a file object: np.savez appends no extension of its own)
        np.savez_compressed(f, counts=counts, k=np.int32(k), calibration=np.asarray(_cal(digitisation, signal_range, offset), np.float32))


def load_counts(path: str):
    """-> (counts int64 [4^k + 1, 6], k, (digitisation, range, offset))"""
    with np.load(path) as z:
        counts, k, cal = z["counts"].astype(np.int64), int(z["k"]), tuple(float(x) for x in z["calibration"])
    if counts.shape != (4 ** k + 1, FIELDS) or len(cal) != 3:
        raise ValueError(f"{path}: not the counts of a k-mer table")
    return counts, k, cal


def join_rank_files(paths: Sequence[str], out: str, keep: bool = False) -> int:
    """The counts of the ranks of a multi-process run -> one table: k and the calibration must agree; the counts are summed (integer
    sums: the result is the single-process table, whatever the sharding), formatted once and written to `out`; the rank files are
    removed unless keep.  -> bytes written."""
    total, k0, cal0 = None, None, None
    for p in paths:
        counts, k, cal = load_counts(p)
        if total is None:
            total, k0, cal0 = counts.copy(), k, cal
        elif k != k0 or cal != cal0:
            raise ValueError(f"{p}: k / calibration {k} / {cal} differ from {paths[0]}'s {k0} / {cal0}")
        else:
            total += counts
    if total is None:
        raise ValueError("no rank files to join")
    text = format_table(total, k0, *cal0)
    with open(out, "wb") as dst:
        dst.write(text)
    if not keep:
        for p in paths:
            if os.path.abspath(p) != os.path.abspath(out):
                os.remove(p)
    return len(text)


def rank_counts_path(path: str, rank: int) -> str:
    """OUT.tsv -> OUT.rank<r>.npz"""
    return f"{os.path.splitext(str(path))[0]}.rank{rank}.npz"
