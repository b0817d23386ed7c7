"""`segment SIGNALS -o OUT.events.tsv`: event detection -- every stored record cut into runs of constant level without its sequence, by
two windowed t-statistics (a short and a long window) whose peaks are the event boundaries.  Everything that decides an output byte is
an integer function stated in include/s2s_hip.h next to s2s_segment (tests/_segment_ref.py restates it); `--cpu` runs the host twin and
gives the same bytes, as does any batching.  Per batch of records (signal_batch.Batch): one host-to-device copy (offsets, slots,
samples), s2s_segment and s2s_event_sums on the same device buffers, one device-to-host copy; the rows are formatted by native host
threads (s2s_segment_format).  The defaults 3 / 6 / 1.4 / 9.0 are the figures commonly quoted for scrappie's R9.4 DNA detector; here they are
choices, not measurements, and this detector is not scrappie's (no peak-height state machine).  Unvalidated against scrappie / f5c /
uncalled4."""
import logging
import math
import os
import time
from typing import Sequence

import click
import numpy as np

from .signal_batch import MAX_SAMPLES, Batch, batches, calibration, host_threads, open_records, slots

logger = logging.getLogger("seq2squiggle")

MAX_WINDOW = 32                  # S2S_SEG_MAX_WINDOW
MAX_THRESHOLD = 1 << 40          # S2S_SEG_MAX_THRESHOLD
TOO_LONG = -2                    # S2S_DTW_COST_TOO_LONG in n_events
DEFAULT_WINDOW_SHORT = 3         # }
DEFAULT_WINDOW_LONG = 6          # } choices, not measurements
DEFAULT_THRESHOLD_SHORT = 1.4    # }
DEFAULT_THRESHOLD_LONG = 9.0     # }
DEFAULT_MAX_SAMPLES = 1 << 27    # samples per batch
COLUMNS = ("read_name", "event_index", "start_idx", "end_idx", "event_level_mean", "event_stdv")
SUMMARY_COLUMNS = ("read_name", "n_samples", "n_events")


def threshold_int(t: float) -> int:
    """The command line's t -> the integer threshold on 256 t^2: floor(256.0 * t * t) in double.  The one place."""
    t = float(t)
    if not math.isfinite(t):
        raise ValueError("a threshold must be finite")
    T = int(math.floor(256.0 * t * t))
    if not 1 <= T <= MAX_THRESHOLD:
        raise ValueError(f"a threshold t must give 1 <= floor(256 t^2) <= 2^40 (got {T})")
    return T


def _check_params(w_short: int, w_long: int, T_short: int, T_long: int):
    w_short, w_long, T_short, T_long = int(w_short), int(w_long), int(T_short), int(T_long)
    if not 1 <= w_short <= w_long <= MAX_WINDOW:
        raise ValueError(f"windows must satisfy 1 <= short <= long <= {MAX_WINDOW}")
    if not (1 <= T_short <= MAX_THRESHOLD and 1 <= T_long <= MAX_THRESHOLD):
        raise ValueError("integer thresholds must be 1..2^40")
    return w_short, w_long, T_short, T_long


def capacity(n, w_short: int) -> np.ndarray:
    """s2s_segment_capacity for an array of record lengths: max(1, n // w_short), 0 for n = 0."""
    n = np.asarray(n, np.int64)
    return np.where(n == 0, 0, np.maximum(1, n // int(w_short))).astype(np.int64)


def _run_batch(sig_list, w_short: int, w_long: int, T_short: int, T_long: int, cpu: bool, device: int = 0, threads: int = None,
               sums: bool = True):
    """One batch of records -> dict(n_events int32 [R], ev_offs int64 [R + 1], start / len int32 [slots], S / Q int64 [slots]): record
    r's events in the slots ev_offs[r] .. ev_offs[r] + n_events[r]."""
    from ._lib import lib
    R = len(sig_list)
    B = Batch(sig_list, lambda offs: (slots(capacity(np.diff(offs), w_short)),), cpu, device, threads)
    ev_offs = B.tables[0]
    KT = int(ev_offs[-1])
    res = B.alloc(S=(np.int64, KT), Q=(np.int64, KT), start=(np.int32, KT), len=(np.int32, KT), n_events=(np.int32, R))

    def scratch_bytes():
        need = int(lib().s2s_segment_scratch_bytes(B.total, R))
        if need < 0:
            raise ValueError("a batch holds more samples than s2s_segment takes")
        return need
    B.call("segment", B.samples, B.offs(), R, B.total, w_short, w_long, T_short, T_long, B.scratch(scratch_bytes), B.table(0),
           res.ptr("start"), res.ptr("len"), res.ptr("n_events"))
    if sums:
        B.call("event_sums", B.samples, B.offs(), res.ptr("start"), res.ptr("len"), B.table(0), R, res.ptr("S"), res.ptr("Q"))
    return dict(ev_offs=ev_offs, **res.fetch())


def segment(samples: Sequence[np.ndarray], window_short: int = DEFAULT_WINDOW_SHORT, window_long: int = DEFAULT_WINDOW_LONG,
            threshold_short: float = DEFAULT_THRESHOLD_SHORT, threshold_long: float = DEFAULT_THRESHOLD_LONG, cpu: bool = False,
            device: int = 0, T_short: int = None, T_long: int = None):
    """The events (include/s2s_hip.h, next to s2s_segment) of the int16 records samples[r] -> ([start int32 array per record], [length
    int32 array per record]): event k of record r holds the samples [start[k], start[k] + length[k]).  The thresholds are t values
    (threshold_int turns them into integers); T_short / T_long give the integer thresholds directly instead."""
    w_s, w_l, T_s, T_l = _check_params(window_short, window_long, threshold_int(threshold_short) if T_short is None else T_short,
                                       threshold_int(threshold_long) if T_long is None else T_long)
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    r = _run_batch(list(samples), w_s, w_l, T_s, T_l, cpu, device, sums=False)
    eo, n = r["ev_offs"], r["n_events"]
    return ([r["start"][eo[i]:eo[i] + n[i]].copy() for i in range(len(n))], [r["len"][eo[i]:eo[i] + n[i]].copy() for i in range(len(n))])


def _format(r, ids, cals, threads: int) -> bytes:
    """The rows of one batch (s2s_segment_format, no header)."""
    from ._lib import lib
    L = lib()
    R = len(ids)
    raw = [i.encode() for i in ids]
    id_offs = np.concatenate([[0], np.cumsum([len(b) for b in raw])]).astype(np.int64)
    idb = np.frombuffer(b"".join(raw) + b"\0", np.uint8)
    cal = np.ascontiguousarray(cals, np.float64).reshape(-1)
    n_ev = np.ascontiguousarray(r["n_events"], np.int32)
    bound = int(L.s2s_segment_format_bound(n_ev.ctypes.data, R, id_offs.ctypes.data, cal.ctypes.data, 0))
    if bound < 0:
        raise click.ClickException("segment: a record's digitisation, offset or range is not finite, or its digitisation or range is 0")
    out = np.empty(max(bound, 1), np.uint8)
    n = int(L.s2s_segment_format(r["start"].ctypes.data, r["len"].ctypes.data, r["S"].ctypes.data, r["Q"].ctypes.data,
                                 r["ev_offs"].ctypes.data, n_ev.ctypes.data, R, idb.ctypes.data, id_offs.ctypes.data, cal.ctypes.data, 0,
                                 threads, out.ctypes.data, bound))
    if n < 0:
        raise RuntimeError(f"s2s_segment_format failed ({n})")
    return out[:n].tobytes()


def segment_files(signals, out, window_short: int = DEFAULT_WINDOW_SHORT, window_long: int = DEFAULT_WINDOW_LONG,
                  threshold_short: float = DEFAULT_THRESHOLD_SHORT, threshold_long: float = DEFAULT_THRESHOLD_LONG, cpu: bool = False,
                  device: int = 0, summary_out=None, max_samples: int = DEFAULT_MAX_SAMPLES) -> dict:
    """Write OUT (COLUMNS; records in the order of SIGNALS, events in order; levels in pA by the record's own digitisation, offset and
    range, the formulas of compare --events-out) and return the counters: records, samples, events, refused records (more than 2^22
    samples: no rows, n_events 0 in the summary) and the mean samples per event.  A batch holds records until their samples pass
    max_samples (at least one record).  summary_out: one row per record (SUMMARY_COLUMNS)."""
    w_s, w_l, T_s, T_l = _check_params(window_short, window_long, threshold_int(threshold_short), threshold_int(threshold_long))
    if int(max_samples) < 1:
        raise ValueError("max_samples must be >= 1")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    threads = host_threads()
    cnt = dict(records=0, samples=0, events=0, refused=0, batches=0)
    tot = dict(solve_s=0.0, format_s=0.0)
    with open(out, "wb") as f, open(summary_out or os.devnull, "w") as fs:
        f.write(("\t".join(COLUMNS) + "\n").encode())
        fs.write("\t".join(SUMMARY_COLUMNS) + "\n")

        def flush(batch):
            t0 = time.perf_counter()
            live = [b for b in batch if b[1] is not None]
            n_ev = np.zeros(0, np.int32)
            t1 = t0
            if live:                                # (a batch may hold refused records only)
                r = _run_batch([b[1] for b in live], w_s, w_l, T_s, T_l, cpu, device, threads)
                t1 = time.perf_counter()
                f.write(_format(r, [b[0] for b in live], [b[2] for b in live], threads))
                n_ev = r["n_events"]
                cnt["batches"] += 1
            it = iter(n_ev)
            for rid, sig, _, n in batch:
                fs.write(f"{rid}\t{n}\t{0 if sig is None else int(next(it))}\n")
            cnt["events"] += int(n_ev.sum())
            tot["solve_s"] += t1 - t0
            tot["format_s"] += time.perf_counter() - t1

        def records():
            """(read id, samples or None for a refused record, calibration, stored length) of every record."""
            for rec in open_records(str(signals)):
                cnt["records"] += 1
                rid, sig = rec["read_id"], np.asarray(rec["signal"], np.int16)
                if len(sig) > MAX_SAMPLES:
                    cnt["refused"] += 1
                    logger.warning("segment: record %s refused: %d samples (limit %d)", rid, len(sig), MAX_SAMPLES)
                    yield rid, None, calibration(rec), len(sig)
                    continue
                cnt["samples"] += len(sig)
                yield rid, sig, calibration(rec), len(sig)

        for batch in batches(records(), lambda b: (0 if b[1] is None else b[3],), (max_samples,)):    # (a refused record costs nothing)
            flush(batch)
    s = dict(signals=str(signals), out=str(out), window_short=w_s, window_long=w_l, threshold_short=float(threshold_short),
             threshold_long=float(threshold_long), T_short=T_s, T_long=T_l, **cnt,
             mean_samples_per_event=(cnt["samples"] / cnt["events"]) if cnt["events"] else None,
             solve_seconds=tot["solve_s"], format_seconds=tot["format_s"])
    if summary_out is not None:
        s["summary_out"] = str(summary_out)
    logger.info("segment: %d record(s), %d sample(s): %d event(s), %d refused (too long); mean samples per event %s", cnt["records"],
                cnt["samples"], cnt["events"], cnt["refused"],
                "nan" if s["mean_samples_per_event"] is None else "%.3f" % s["mean_samples_per_event"])
    return s
