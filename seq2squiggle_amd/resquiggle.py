"""`resquiggle SEQS SIGNALS --kmer-model M -o OUT.events.tsv`: which samples of a stored record belong to which k-mer of its sequence
-- the signal aligned to the levels a pore model (`predict --kmer-model`, or a nanopolish-style table) expects for its k-mers, and
written as the event table `predict --events` writes.  Everything that decides an output byte is an integer function stated in
include/s2s_hip.h next to s2s_resquiggle (tests/_resquiggle_ref.py restates it): samples and levels are median / MAD normalised by the
entries `compare` uses, the alignment is the dynamic programme of csrc/s2s_resquiggle.h (one workgroup per read, then a walk back),
the per-event sums are s2s_event_sums; `--cpu` runs the host twins of the same entries and gives the same bytes, as does any batching.
Per batch of reads (signal_batch.Batch): one host-to-device copy (offsets, slot tables, samples, levels) and the mask of k-mers
without a level, the kernels, one device-to-host copy of all results.  The model, the sequences, the files and the rows are
pore_align's (align_files); this module holds the solver of a batch, what it counts per read and --intervals.  The reference
has no such command, and no f5c / uncalled4 was at hand: the output is unvalidated against them -- DESIGN.md section 6."""
from typing import Sequence

import click
import numpy as np

from .compare import EVENT_COLUMNS  # noqa: F401  (the columns of OUT, under this module's name too)
from .pore_align import (DEFAULT_MAX_SAMPLES, DEFAULT_TRACE_MEMORY, LEVEL_SCALE, MAX_SKIP_PENALTY, MAX_UNKNOWN_COST,  # noqa: F401
                         UNKNOWN, UNREACHED, Aligner, align_files, clean_sequence, format_rows, kmer_codes, level_ints, read_model,
                         read_sequences, split_levels)
from .signal_batch import MAX_SAMPLES, Batch, batches, check_band, device_only, max_band, sample_at, slots

DEFAULT_BAND = 512               # +-k-mers around the diagonal                       }
DEFAULT_SKIP_PENALTY = 128       # two MADs (64 units each) for a k-mer without sample } choices, not measurements
DEFAULT_UNKNOWN_COST = 64        # one MAD per sample on a k-mer without a level       }
SUMMARY_COLUMNS = ("read_id", "n_samples", "n_kmers", "status", "cost", "cost_per_sample", "events", "skipped", "med", "mad",
                   "level_med", "level_mad", "start", "end")


def read_intervals(path: str) -> dict:
    """A table of `compare --open-ends` -> {read_id: (b_start, b_end)}, the three columns taken by name."""
    out = {}
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        try:
            ci = [head.index(c) for c in ("read_id", "b_start", "b_end")]
        except ValueError:
            raise click.ClickException(f"{path}: an interval table needs the columns read_id, b_start and b_end")
        for no, line in enumerate(f, 2):
            v = line.rstrip("\n").split("\t")
            try:
                out.setdefault(v[ci[0]], (int(v[ci[1]]), int(v[ci[2]])))
            except (IndexError, ValueError):
                raise click.ClickException(f"{path}: line {no} is not a row of an interval table")
    return out


# ------------------------------------------------------------------ the solver
def _check_params(band: int, skip_penalty: int, unknown_cost: int):
    band, skip_penalty, unknown_cost = check_band(band), int(skip_penalty), int(unknown_cost)
    if not 0 <= skip_penalty <= MAX_SKIP_PENALTY:
        raise ValueError(f"skip_penalty must be 0..{MAX_SKIP_PENALTY}")
    if not 0 <= unknown_cost <= MAX_UNKNOWN_COST:
        raise ValueError(f"unknown_cost must be 0..{MAX_UNKNOWN_COST}")
    return band, skip_penalty, unknown_cost


def scratch_bytes(n: int, K: int, band: int) -> int:
    """Bytes of decision scratch s2s_resquiggle needs for n samples against K k-mers (0 for a read it does not solve)."""
    from ._lib import lib
    r = int(lib().s2s_resquiggle_scratch_bytes(int(n), int(K), int(band)))
    if r < 0:
        raise ValueError(f"band must be 1..{max_band()}")
    return r


def _run_batch(sig_list, lev_list, known_list, band: int, skip_penalty: int, unknown_cost: int, norm: bool, cpu: bool, device: int = 0,
               threads: int = None, sums: bool = True, chunks=None, model_out=None):
    """One batch of reads.  sig_list: the stored int16 samples; lev_list: int16 levels per k-mer (any value where known_list is False).
    norm: samples are normalised by their own median / MAD and the levels by the median / MAD of the read's KNOWN levels, both by
    s2s_signal_median_mad / s2s_signal_normalise at scale 64 (else both enter as they are); k-mers without a level get S2S_RSQ_UNKNOWN.
    -> dict(cost int64 [P], start / len int32 per read, S / Q int64 per read (raw samples), med / mad int32 [2 P]: samples, then levels).
    chunks: (preprocess.Chunker, the records' calibrations, the cleaned sequences) -- the training chunks are packed from the device
    buffers behind the sums; without it nothing else is uploaded or launched.  model_out: (kmer_model.ModelBuilder, the calibrations,
    the cleaned sequences) -- the k-mer slots are summed into the builder's table behind the sums, likewise."""
    P = len(sig_list)
    known_recs, full_recs, unknown = split_levels(lev_list, known_list)

    def tables(offs):
        """The pool is 3 P records: samples, known levels, all levels -> l_offs int64 [P + 1]: the reads' slots of k-mers (the offsets
        of the third part from its start); s_offs int64 [P + 1]: their slots of decision scratch (device only)."""
        lens = np.diff(offs)
        extra = chunks[0].tables(chunks[1], chunks[2]) if chunks is not None else []
        extra += model_out[0].tables(model_out[1], model_out[2]) if model_out is not None else []
        return [(offs[2 * P:] - offs[2 * P]).astype(np.int64), slots([scratch_bytes(lens[p], lens[2 * P + p], band) for p in range(P)])] + extra
    B = Batch(list(sig_list) + known_recs + full_recs, tables, cpu, device, threads)
    l_offs, s_offs = B.tables[:2]
    KT, l0 = int(l_offs[-1]), int(B.host_offs[2 * P])
    res = B.alloc(cost=(np.int64, P), S=(np.int64, KT), Q=(np.int64, KT), start=(np.int32, KT), len=(np.int32, KT),
                  med=(np.int32, 2 * P), mad=(np.int32, 2 * P))
    q = B.normalised(res.ptr("med"), res.ptr("mad"), norm, halves=P)
    q = B.marked(q, l0, unknown, UNKNOWN)               # the marker of a k-mer without a level
    B.call("resquiggle", q, B.offs(), sample_at(q, l0), B.table(0), P, band, skip_penalty, unknown_cost, res.ptr("cost"),
           B.scratch(s_offs[-1]), device_only(B.table(1)), res.ptr("start"), res.ptr("len"))
    if sums:
        B.call("event_sums", B.samples, B.offs(), res.ptr("start"), res.ptr("len"), B.table(0), P, res.ptr("S"), res.ptr("Q"))
    if chunks is not None:
        chunks[0].pack(B, P, B.table(0), np.diff(l_offs), res.ptr("start"), res.ptr("len"), res.ptr("S"), res.ptr("Q"), B.table(2), B.table(3))
    if model_out is not None:
        at = 2 if chunks is None else 4
        model_out[0].add(B, P, B.table(0), res.ptr("len"), res.ptr("S"), res.ptr("Q"), B.table(at), B.table(at + 1), B.table(at + 2))
    r = res.fetch()
    cut = lambda a: [a[l_offs[p]:l_offs[p + 1]] for p in range(P)]      # noqa: E731
    return dict(cost=r["cost"], start=cut(r["start"]), len=cut(r["len"]), S=cut(r["S"]), Q=cut(r["Q"]), med=r["med"], mad=r["mad"])


def resquiggle(samples: Sequence[np.ndarray], levels: Sequence[np.ndarray], band: int = DEFAULT_BAND,
               skip_penalty: int = DEFAULT_SKIP_PENALTY, unknown_cost: int = DEFAULT_UNKNOWN_COST, cpu: bool = False, device: int = 0,
               trace_memory: int = DEFAULT_TRACE_MEMORY):
    """The alignment (include/s2s_hip.h, next to s2s_resquiggle) of the int16 records samples[p] to the int16 levels[p] AS THEY ARE (no
    normalisation; -32768 marks a k-mer without a level) -> (cost int64 [P], [start int32 array per read], [len int32 array per
    read]): k-mer j owns samples [start[j], start[j] + len[j]); -1 / 0 for a skipped k-mer and for every k-mer of an unsolved read
    (cost -1: an empty member; -3: no path).  The reads run in batches whose decision scratch stays within trace_memory bytes; a
    single read beyond it is a ValueError."""
    if len(samples) != len(levels):
        raise ValueError("samples and levels must pair up")
    band, skip_penalty, unknown_cost = _check_params(band, skip_penalty, unknown_cost)
    if int(trace_memory) < 1:
        raise ValueError("trace_memory must be >= 1")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    if any(np.size(l) > MAX_SAMPLES for l in levels):
        raise ValueError(f"a read holds more than {MAX_SAMPLES} k-mers")
    need = [scratch_bytes(min(np.size(s), MAX_SAMPLES), np.size(l), band) for s, l in zip(samples, levels)]
    for p, nb in enumerate(need):
        if nb > trace_memory:
            raise ValueError(f"read {p}: the walk back needs {nb} bytes of decision scratch, more than trace_memory = {trace_memory}")
    cost, start, length = [np.zeros(0, np.int64)], [], []
    for run in batches(range(len(need)), lambda p: (need[p],), (trace_memory,)):
        lev = [np.asarray(l, np.int16).reshape(-1) for l in levels[run[0]:run[-1] + 1]]
        r = _run_batch(samples[run[0]:run[-1] + 1], lev, [l != UNKNOWN for l in lev], band, skip_penalty, unknown_cost, False, cpu, device,
                       sums=False)
        cost.append(r["cost"])
        start += r["start"]
        length += r["len"]
    return np.concatenate(cost), start, length


def event_sums(samples: Sequence[np.ndarray], start: Sequence[np.ndarray], length: Sequence[np.ndarray], cpu: bool = False, device: int = 0):
    """-> ([S int64 per read], [Q int64 per read]): sum and sum of squares of samples[p][start[j] : start[j] + length[j]) per k-mer
    (s2s_event_sums); 0, 0 for a skipped k-mer or an interval outside the record."""
    P = len(samples)
    st = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in start]
    ln = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in length]
    l_offs = slots([len(x) for x in st])
    ev = np.zeros((2, int(l_offs[-1])), np.int32)       # (as many lengths as starts, or a ValueError)
    ev[0], ev[1] = np.concatenate(st + [np.zeros(0, np.int32)]), np.concatenate(ln + [np.zeros(0, np.int32)])
    B = Batch(samples, (l_offs, ev[0], ev[1]), cpu, device)
    res = B.alloc(S=(np.int64, l_offs[-1]), Q=(np.int64, l_offs[-1]))
    B.call("event_sums", B.samples, B.offs(), B.table(1), B.table(2), B.table(0), P, res.ptr("S"), res.ptr("Q"))
    r = res.fetch()
    return [r["S"][l_offs[p]:l_offs[p + 1]] for p in range(P)], [r["Q"][l_offs[p]:l_offs[p + 1]] for p in range(P)]


# ------------------------------------------------------------------ files
def _account(r, p: int, n: int):
    """pore_align.Aligner.account: the read p of a _run_batch result, n samples long."""
    P = len(r["cost"])
    c, ln = int(r["cost"][p]), r["len"][p]
    mm = (int(r["med"][p]), int(r["mad"][p]), int(r["med"][P + p]), int(r["mad"][P + p]))
    if c < 0:
        return c, len(ln), mm, (0, 0)
    events = int((ln > 0).sum())
    skipped = len(ln) - events
    return c, len(ln), mm, (events, skipped), n, dict(events=events, skipped_kmers=skipped), (r["start"][p], ln, r["S"][p], r["Q"][p])


def _clip(intervals):
    """pore_align.Aligner.clip: every record that has a row in the interval table cut to its [b_start, b_end)."""
    iv = read_intervals(str(intervals)) if intervals is not None else {}

    def clip(rid, sig):
        if rid not in iv:
            return sig, 0, len(sig)
        b0, b1 = max(0, min(iv[rid][0], len(sig))), max(0, min(iv[rid][1], len(sig)))
        return sig[b0:max(b0, b1)], b0, max(b0, b1)
    return clip


def resquiggle_files(seqs, signals, model, out, band: int = DEFAULT_BAND, skip_penalty: int = DEFAULT_SKIP_PENALTY,
                     unknown_cost: int = DEFAULT_UNKNOWN_COST, rna: bool = False, intervals=None, with_samples: bool = False,
                     cpu: bool = False, device: int = 0, summary_out=None, max_samples: int = DEFAULT_MAX_SAMPLES,
                     trace_memory: int = DEFAULT_TRACE_MEMORY, chunks=None, model_out=None) -> dict:
    """pore_align.align_files with this module's solver -> the counters: reads solved, unreached (no path: more than two k-mers per
    sample, or the band too narrow), refused (or a walk back that needs more than trace_memory on its own), without a sequence,
    without a known level, events, skipped k-mers, and the mean cost per sample in MADs (sum of costs / sum of samples / 64 over the
    solved reads).  rna: `position` stays in read coordinates and start_idx falls as it rises.  intervals: restrict every record
    that has a row to [b_start, b_end) (read_intervals); rows come out in the record's own coordinates.  summary_out: one row per
    read (SUMMARY_COLUMNS).  model_out: (NEW.model, min_events) -- the pore model re-estimated from these alignments."""
    band, skip_penalty, unknown_cost = _check_params(band, skip_penalty, unknown_cost)
    return align_files(Aligner(
        name="resquiggle", columns=SUMMARY_COLUMNS, counters=("events", "skipped_kmers"),
        params=dict(band=band, skip_penalty=skip_penalty, unknown_cost=unknown_cost, rna=bool(rna)),
        need=lambda n, K: scratch_bytes(n, K, band),
        refusal=f"resquiggle: read %s refused: %d samples against %d k-mers at band {band} (limit %d each; %d bytes of decision scratch "
                "against --trace-memory %d)",
        solve=lambda sig, lev, known, ch, mo: _run_batch(sig, lev, known, band, skip_penalty, unknown_cost, True, cpu, device, chunks=ch,
                                                         model_out=mo),
        account=_account, mean_key="mean_cost_per_sample", log_tail="%d event(s), %d skipped k-mer(s); mean cost per sample %s MAD",
        clip=lambda: _clip(intervals)), seqs, signals, model, out, rna, with_samples, cpu, summary_out, max_samples, trace_memory, chunks,
        model_out)
