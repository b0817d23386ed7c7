"""The k-mer model of a run (`predict --kmer-model OUT.model`): for every k-mer that got events the mean and the deviation of its
EVENT MEANS (level_mean, level_stdv) and the mean and the deviation of its events' own sample deviations (sd_mean, sd_stdv), in pA,
and the number of events -- the `kmer level_mean level_stdv sd_mean sd_stdv` form of a nanopolish / f5c / uncalled4-style pore
model.  The k-mer table (kmer_table.py) pools samples; here every event counts once.  An event's mean and deviation are taken in
fixed point (2^-8 ADC counts: s2s_event_fixed), so the five integer counters per k-mer are summed on the GPU with integer adds
(Engine.kmer_model_accumulate) and do not depend on batching or sharding; only the finished table leaves the device, once per
run, and the library formats it (s2s_kmer_model_format; include/s2s_hip.h states the columns and the definitions).  The reference
writes no such file; the format is unvalidated against external tools -- DESIGN.md section 6.

`resquiggle --kmer-model-out` and `eventalign --kmer-model-out` write the same file from ALIGNMENTS of stored records (ModelBuilder):
one round of re-estimation -- align with the model at hand, collect the event means per k-mer, write the next model.  There every
record has its own calibration, so the events are converted to 2^-8 pA before they are summed (s2s_kmer_model_events; include/s2s_hip.h
states the definition) and the table is formatted with the identity calibration."""
import math
import os
import time
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


# ------------------------------------------------------------------ the model of a run of resquiggle / eventalign
GAIN_ONE = 1 << 24      # gain: range / digitisation in units of 2^-24
CAL_LIMIT = 1 << 30     # gain 1 .. 2^30, |shift| <= 2^30
DROPPED = ("overlong", "out_of_range", "bad_code", "counted")


def gain_shift(cal):
    """(digitisation, offset, range) of a record -> (gain, shift) of s2s_kmer_model_events, formed in double: rint(range / digitisation
    * 2^24) and rint(offset * 256); (0, 0) for a calibration outside gain 1 .. 2^30, |shift| <= 2^30: the record contributes nothing."""
    digitisation, offset, signal_range = (float(x) for x in cal)
    if digitisation == 0 or not all(math.isfinite(x) for x in (digitisation, offset, signal_range)):
        return 0, 0
    g, s = float(np.rint(signal_range / digitisation * GAIN_ONE)), float(np.rint(offset * 256))
    if not 1 <= g <= CAL_LIMIT or abs(s) > CAL_LIMIT:
        return 0, 0
    return int(g), int(s)


class ModelBuilder:
    """`--kmer-model-out NEW.model` of `resquiggle` and `eventalign`: after a batch's last s2s_event_sums, `add` sums the batch's k-mer
    slots -- (ev_len, S, Q) where they lie -- into ONE table that lives as long as the command (s2s_kmer_model_events, or its host
    twin with --cpu); nothing returns to the host per batch.  `tables` gives the three arrays a batch uploads for it with its own: the
    row of every slot's k-mer (4^k for a k-mer with a letter outside ACGT; back to front where the slots are laid so: rna) and the
    records' gain and shift.  `close` brings the table down once and writes the file."""

    def __init__(self, k: int, rna: bool = False):
        self.k, self.rna = int(k), bool(rna)
        if not 1 <= self.k <= MAX_K:
            raise ValueError(f"k must be 1..{MAX_K}")
        self.rows = 4 ** self.k + 1
        self.buf = None                             # int64 [rows * 5 + 4]: the table, then `dropped`; numpy (--cpu) or torch
        self.left_out, self.seconds = 0, 0.0

    def tables(self, cal_list, clean_list):
        from .pore_align import kmer_codes
        codes = [np.where((c := kmer_codes(clean, self.k)) < 0, self.rows - 1, c).astype(np.int32) for clean in clean_list]
        if self.rna:
            codes = [c[::-1] for c in codes]
        gs = np.zeros((2, len(cal_list)), np.int64)
        for p, cal in enumerate(cal_list):
            gs[:, p] = gain_shift(cal)
            if gs[0, p] == 0:
                self.left_out += 1
                import logging
                logging.getLogger("seq2squiggle").warning(
                    "--kmer-model-out: a read is left out of the model: its calibration (digitisation %s, offset %s, range %s) is "
                    "outside gain 2^-24 .. 64 pA per count and |offset| <= 2^22", *cal)
        return [np.concatenate(codes + [np.zeros(0, np.int32)]), gs[0].copy(), gs[1].copy()]

    def _pointers(self, B):
        if self.buf is None:
            n = self.rows * FIELDS + len(DROPPED)
            self.buf = np.zeros(n, np.int64) if B.cpu else B.torch.zeros(n, dtype=B.torch.int64, device=B.where)
        base = self.buf.ctypes.data if isinstance(self.buf, np.ndarray) else self.buf.data_ptr()
        return base, base + 8 * self.rows * FIELDS

    def add(self, B, P: int, l_offs, ev_len, S, Q, codes, gain, shift, workgroups: int = 0) -> None:
        """l_offs ... shift: pointers on the batch's side."""
        from .signal_batch import device_only
        t0 = time.perf_counter()
        table, dropped = self._pointers(B)
        B.call("kmer_model_events", codes, ev_len, S, Q, l_offs, int(P), gain, shift, self.k, device_only(int(workgroups)), table, dropped)
        self.seconds += time.perf_counter() - t0

    def counts(self):
        """-> (table int64 [4^k + 1, 5], dropped int64 [4]) on the host: ONE copy down."""
        if self.buf is None:
            return np.zeros((self.rows, FIELDS), np.int64), np.zeros(len(DROPPED), np.int64)
        raw = self.buf if isinstance(self.buf, np.ndarray) else self.buf.cpu().numpy()
        return raw[:self.rows * FIELDS].reshape(self.rows, FIELDS).copy(), raw[self.rows * FIELDS:].copy()

    def close(self, out, min_events: int = 1) -> dict:
        """Write the model of the rows with at least min_events events to `out` -> the counters."""
        t0 = time.perf_counter()
        counts, dropped = self.counts()
        counts[counts[:, 0] < int(min_events)] = 0
        text = format_model(counts, self.k, 1.0, 1.0, 0.0)
        with open(os.fspath(out), "wb") as f:
            f.write(text)
        log_missing(counts, self.k, out)
        self.seconds += time.perf_counter() - t0
        return dict(out=str(out), min_events=int(min_events), **{name: int(v) for name, v in zip(DROPPED, dropped)},
                    rows=4 ** self.k - missing_kmers(counts, self.k), reads_left_out=self.left_out, seconds=self.seconds)
