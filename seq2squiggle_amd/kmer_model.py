"""The k-mer model of a run (`predict --kmer-model OUT.model`): for every k-mer that got events the mean and the deviation of its
EVENT MEANS (level_mean, level_stdv) and the mean and the deviation of its events' own sample deviations (sd_mean, sd_stdv), in pA,
and the number of events -- the `kmer level_mean level_stdv sd_mean sd_stdv` form of a nanopolish / f5c / uncalled4-style pore
model.  The k-mer table (kmer_table.py) pools samples; here every event counts once.  An event's mean and deviation are taken in
fixed point (2^-8 ADC counts: s2s_event_fixed), so the five integer counters per k-mer are summed on the GPU with integer adds
(Engine.kmer_model_accumulate) and do not depend on batching or sharding; only the finished table leaves the device, once per
run, and the library formats it (s2s_kmer_model_format; include/s2s_hip.h states the columns and the definitions).  The reference
writes no such file; the format is unvalidated against external tools -- DESIGN.md section 6."""
import os
from typing import Sequence

import numpy as np

FIELDS = 5          # events, sum_m, sum_m2, sum_d, sum_d2
MAX_K = 10


def _cal(digitisation, signal_range, offset):
    """The calibration as the float32 the library is handed."""
    return tuple(float(np.float32(x)) for x in (digitisation, signal_range, offset))


def format_model(counts: np.ndarray, k: int, digitisation: float, signal_range: float, offset: float,
                 with_header: bool = True) -> memoryview:
    """The text of a model (s2s_kmer_model_format): counts int64 [4^k + 1, 5], one row per ACGT k-mer with events, in code order; the
    row of k-mers with a letter outside ACGT is not printed."""
    from ._lib import lib
    L = lib()
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be 1..{MAX_K}")
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if counts.shape != (4 ** k + 1, FIELDS):
        raise ValueError(f"counts must be int64 [{4 ** k + 1}, {FIELDS}]")
    cal = _cal(digitisation, signal_range, offset)
    cap = int(L.s2s_kmer_model_format_bound(counts.ctypes.data, k, *cal, int(bool(with_header))))
    if cap < 0:
        raise ValueError("digitisation and range must be non-zero numbers and no counter but sum_m negative")
    out = np.empty(max(cap, 1), np.uint8)
    got = L.s2s_kmer_model_format(counts.ctypes.data, k, *cal, int(bool(with_header)), out.ctypes.data, cap)
    if got < 0:
        raise RuntimeError(f"s2s_kmer_model_format failed ({got})")
    return memoryview(out)[:got]


def missing_kmers(counts: np.ndarray, k: int) -> int:
    """How many of the 4^k ACGT k-mers have no row (no event)."""
    return int((np.asarray(counts)[:4 ** int(k), 0] < 1).sum())


def save_counts(path: str, counts: np.ndarray, k: int, digitisation: float, signal_range: float, offset: float) -> None:
    """The counters of one rank of a multi-process run: one .npz with the counts, k and the three calibration floats."""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if counts.shape != (4 ** int(k) + 1, FIELDS):
        raise ValueError(f"counts must be int64 [{4 ** int(k) + 1}, {FIELDS}]")
    with open(path, "wb") as f:                     # (a file object: np.savez appends no extension of its own)
        np.savez_compressed(f, counts=counts, k=np.int32(k), calibration=np.asarray(_cal(digitisation, signal_range, offset), np.float32))


def load_counts(path: str):
    """-> (counts int64 [4^k + 1, 5], k, (digitisation, range, offset))"""
    with np.load(path) as z:
        counts, k, cal = z["counts"].astype(np.int64), int(z["k"]), tuple(float(x) for x in z["calibration"])
    if counts.shape != (4 ** k + 1, FIELDS) or len(cal) != 3:
        raise ValueError(f"{path}: not the counts of a k-mer model")
    return counts, k, cal


def join_rank_files(paths: Sequence[str], out: str, keep: bool = False) -> int:
    """The counts of the ranks of a multi-process run -> one model: k and the calibration must agree; the counts are summed (integer
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
    text = format_model(total, k0, *cal0)
    with open(out, "wb") as dst:
        dst.write(text)
    log_missing(total, k0, out)
    if not keep:
        for p in paths:
            if os.path.abspath(p) != os.path.abspath(out):
                os.remove(p)
    return len(text)


def log_missing(counts: np.ndarray, k: int, out) -> None:
    import logging
    logging.getLogger("seq2squiggle").info("k-mer model %s: %d of the %d %d-mers have no row (no event in this run)", out,
                                           missing_kmers(counts, k), 4 ** int(k), int(k))


def rank_counts_path(path: str, rank: int) -> str:
    """OUT.model -> OUT.rank<r>.npz"""
    return f"{os.path.splitext(str(path))[0]}.rank{rank}.npz"
