"""`eventalign SEQS SIGNALS --kmer-model M -o OUT.events.tsv`: which samples of an UNTRIMMED stored record belong to which k-mer of its
sequence, by the event-level route of nanopolish and f5c: the record is cut into events (`segment`), the event means are median / MAD
normalised, and the means are aligned to the levels a pore model expects inside a narrow band that follows the path, with free ends
that cost a trim penalty per event -- adapter and stall in front and trailing samples behind are trimmed, not aligned.  Everything
that decides an output byte is an integer function stated in include/s2s_hip.h next to s2s_event_means and s2s_eventalign
(tests/_eventalign_ref.py restates it); `--cpu` runs the host twins of the same entries and gives the same bytes, as does any
batching.  Per batch of reads: the samples with their slot tables go up in one copy and the levels in a second (signal_batch.Batch,
one each), then s2s_segment, s2s_event_sums, s2s_event_means, s2s_signal_median_mad and s2s_signal_normalise on the pool of means
and on the levels, s2s_eventalign, s2s_event_sums on the k-mer intervals -- every slot sized by s2s_segment_capacity, so nothing
returns to the host in between -- and one copy down.  The model, the sequences, the files and the rows are pore_align's
(align_files); this module holds the solver of a batch and what it counts per read.  The defaults 128 / 128 / 64 / 64 are choices,
not measurements.  The event means are normalised over the WHOLE record: junk at the ends of up to about a quarter of
the events still aligns, but when junk is more than half the events the junk is the median and the alignment is meaningless.  The
reference has no such command, and no f5c / nanopolish / uncalled4 was at hand: the output is unvalidated against them -- DESIGN.md
section 6."""
from typing import Sequence

import numpy as np

from .compare import EVENT_COLUMNS  # noqa: F401  (the columns of OUT, under this module's name too)
from .pore_align import (DEFAULT_MAX_SAMPLES, DEFAULT_TRACE_MEMORY, MAX_SKIP_PENALTY, MAX_UNKNOWN_COST, UNKNOWN, Aligner, align_files,
                         split_levels)
from .segment import (DEFAULT_THRESHOLD_LONG, DEFAULT_THRESHOLD_SHORT, DEFAULT_WINDOW_LONG, DEFAULT_WINDOW_SHORT, capacity,
                      threshold_int)
from .segment import _check_params as _check_segment
from .signal_batch import MAX_SAMPLES, SCALE, Batch, device_only, slots

MAX_WIDTH = 1024                 # S2S_EVA_MAX_WIDTH
MAX_TRIM_PENALTY = 1 << 20       # S2S_EVA_MAX_TRIM_PENALTY
DEFAULT_BAND_WIDTH = 128         # cells of a band                                          }
DEFAULT_SKIP_PENALTY = 128       # two MADs (64 units each) for a k-mer without an event    } choices, not measurements
DEFAULT_TRIM_PENALTY = 64        # one MAD per trimmed event                                }
DEFAULT_UNKNOWN_COST = 64        # one MAD per event on a k-mer without a level             }
SUMMARY_COLUMNS = ("read_id", "n_samples", "n_kmers", "status", "cost", "cost_per_event", "events", "aligned_events", "skipped",
                   "trim_head", "trim_tail", "med", "mad", "level_med", "level_mad")


def _check_params(band_width: int, skip_penalty: int, trim_penalty: int, unknown_cost: int):
    W, skip_penalty, trim_penalty, unknown_cost = int(band_width), int(skip_penalty), int(trim_penalty), int(unknown_cost)
    if not 64 <= W <= MAX_WIDTH or W % 64:
        raise ValueError(f"band_width must be a multiple of 64 in 64..{MAX_WIDTH}")
    if not 0 <= skip_penalty <= MAX_SKIP_PENALTY:
        raise ValueError(f"skip_penalty must be 0..{MAX_SKIP_PENALTY}")
    if not 0 <= trim_penalty <= MAX_TRIM_PENALTY:
        raise ValueError(f"trim_penalty must be 0..{MAX_TRIM_PENALTY}")
    if not 0 <= unknown_cost <= MAX_UNKNOWN_COST:
        raise ValueError(f"unknown_cost must be 0..{MAX_UNKNOWN_COST}")
    return W, skip_penalty, trim_penalty, unknown_cost


def scratch_bytes(E: int, K: int, band_width: int) -> int:
    """Bytes of decision scratch s2s_eventalign needs for E events against K k-mers (0 for a read it does not solve)."""
    from ._lib import lib
    r = int(lib().s2s_eventalign_scratch_bytes(int(E), int(K), int(band_width)))
    if r < 0:
        raise ValueError(f"band_width must be a multiple of 64 in 64..{MAX_WIDTH}")
    return r


def scratch_bound(n: int, K: int, band_width: int, w_short: int) -> int:
    """The decision scratch of a record of n samples before its events are known: that of s2s_segment_capacity events."""
    return scratch_bytes(int(capacity(n, w_short)), K, band_width)


def _levels(lev_list, known_list, cpu: bool, device: int, threads, norm: bool, lmed: int, lmad: int):
    """The levels' batch: 2 P records, the KNOWN levels of every read and then all of them (0 where unknown) -> (batch, pointer of the
    levels the solver takes, pointer of l_offs).  norm: median / MAD of the known levels into lmed / lmad (int32 pointers, P values
    each, behind P unused ones), all levels normalised by them; k-mers without a level get S2S_RSQ_UNKNOWN either way."""
    P = len(lev_list)
    known_recs, full_recs, unknown = split_levels(lev_list, known_list)
    BL = Batch(known_recs + full_recs, lambda offs: ((offs[P:] - offs[P]).astype(np.int64),), cpu, device, threads)
    l0 = int(BL.host_offs[P])
    if norm:
        BL.measure(lmed + 4 * P, lmad + 4 * P, P)       # the known levels' values where `normalised` looks for those of all levels
    q = BL.normalised(lmed, lmad, norm, given=True)
    q = BL.marked(q, l0, unknown, UNKNOWN)
    return BL, q + 2 * l0, BL.table(0)


def _run_batch(sig_list, lev_list, known_list, W: int, skip_penalty: int, trim_penalty: int, unknown_cost: int, seg, cpu: bool,
               device: int = 0, threads: int = None, chunks=None, model_out=None):
    """One batch of reads, the whole chain.  sig_list: the stored int16 samples; lev_list: int16 levels per k-mer (any value where
    known_list is False); seg: (w_short, w_long, T_short, T_long).  -> dict(cost int64 [P], first / end / n_events int32 [P], per read
    ev_start / ev_len / kmer (its events) and k_start / k_len / k_events / S / Q (its k-mers; S, Q over the raw samples), med / mad
    int32 [P] of the event means, lmed / lmad int32 [P] of the known levels).  chunks: (preprocess.Chunker, the records' calibrations,
    the cleaned sequences) -- the training chunks are packed from the device buffers behind the last sums; without it nothing else is
    uploaded or launched.  model_out: (kmer_model.ModelBuilder, the calibrations, the cleaned sequences) -- the k-mer slots are summed
    into the builder's table behind the last sums, likewise."""
    from ._lib import lib
    P = len(sig_list)
    w_s = seg[0]
    K = [int(np.size(l)) for l in lev_list]

    def tables(offs):
        cap = capacity(np.diff(offs), w_s)
        extra = chunks[0].tables(chunks[1], chunks[2]) if chunks is not None else []
        extra += model_out[0].tables(model_out[1], model_out[2]) if model_out is not None else []
        return [slots(cap), device_only(lambda: slots([scratch_bytes(c, k, W) for c, k in zip(cap, K)]))] + extra
    B = Batch(sig_list, tables, cpu, device, threads)
    ev_offs = B.tables[0]
    ET, KT = int(ev_offs[-1]), int(sum(K))
    res = B.alloc(cost=(np.int64, P), eS=(np.int64, ET), eQ=(np.int64, ET), m_offs=(np.int64, P + 1), S=(np.int64, KT), Q=(np.int64, KT),
                  ev_start=(np.int32, ET), ev_len=(np.int32, ET), n_events=(np.int32, P), kmer=(np.int32, ET), first=(np.int32, P),
                  end=(np.int32, P), k_start=(np.int32, KT), k_len=(np.int32, KT), k_events=(np.int32, KT), med=(np.int32, P),
                  mad=(np.int32, P), lmed=(np.int32, 2 * P), lmad=(np.int32, 2 * P), means=(np.int16, ET), mq=(np.int16, ET))
    BL, lq, l_offs = _levels(lev_list, known_list, cpu, device, threads, True, res.ptr("lmed"), res.ptr("lmad"))

    def segment_scratch():
        need = int(lib().s2s_segment_scratch_bytes(B.total, P))
        if need < 0:
            raise ValueError("a batch holds more samples than s2s_segment takes")
        return need
    B.call("segment", B.samples, B.offs(), P, B.total, *seg, B.scratch(segment_scratch), B.table(0), res.ptr("ev_start"),
           res.ptr("ev_len"), res.ptr("n_events"))
    B.call("event_sums", B.samples, B.offs(), res.ptr("ev_start"), res.ptr("ev_len"), B.table(0), P, res.ptr("eS"), res.ptr("eQ"))
    B.call("event_means", res.ptr("eS"), res.ptr("ev_len"), B.table(0), res.ptr("n_events"), P, ET, res.ptr("m_offs"), res.ptr("means"))
    B.call("signal_median_mad", res.ptr("means"), res.ptr("m_offs"), P, res.ptr("med"), res.ptr("mad"))
    B.call("signal_normalise", res.ptr("means"), res.ptr("m_offs"), P, res.ptr("med"), res.ptr("mad"), SCALE, res.ptr("mq"))
    B.call("eventalign", res.ptr("mq"), res.ptr("m_offs"), lq, l_offs, res.ptr("ev_start"), res.ptr("ev_len"), B.table(0), P, W,
           skip_penalty, trim_penalty, unknown_cost, res.ptr("cost"), B.scratch(lambda: B.tables[1][-1]), B.table(1), res.ptr("first"),
           res.ptr("end"), res.ptr("kmer"), res.ptr("k_start"), res.ptr("k_len"), res.ptr("k_events"))
    B.call("event_sums", B.samples, B.offs(), res.ptr("k_start"), res.ptr("k_len"), l_offs, P, res.ptr("S"), res.ptr("Q"))
    if chunks is not None:
        chunks[0].pack(B, P, l_offs, K, res.ptr("k_start"), res.ptr("k_len"), res.ptr("S"), res.ptr("Q"), B.table(2), B.table(3))
    if model_out is not None:
        at = 2 if chunks is None else 4
        model_out[0].add(B, P, l_offs, res.ptr("k_len"), res.ptr("S"), res.ptr("Q"), B.table(at), B.table(at + 1), B.table(at + 2))
    r = res.fetch()
    lo, mo, ne = BL.tables[0], r["m_offs"], r["n_events"]
    per_k = lambda a: [a[lo[p]:lo[p + 1]] for p in range(P)]                         # noqa: E731
    per_slot = lambda a: [a[ev_offs[p]:ev_offs[p] + max(int(ne[p]), 0)] for p in range(P)]      # noqa: E731
    return dict(cost=r["cost"], first=r["first"], end=r["end"], n_events=ne, ev_start=per_slot(r["ev_start"]), ev_len=per_slot(r["ev_len"]),
                kmer=[r["kmer"][mo[p]:mo[p + 1]] for p in range(P)], k_start=per_k(r["k_start"]), k_len=per_k(r["k_len"]),
                k_events=per_k(r["k_events"]), S=per_k(r["S"]), Q=per_k(r["Q"]), med=r["med"], mad=r["mad"], lmed=r["lmed"][P:],
                lmad=r["lmad"][P:])


def eventalign(means: Sequence[np.ndarray], levels: Sequence[np.ndarray], band_width: int = DEFAULT_BAND_WIDTH,
               skip_penalty: int = DEFAULT_SKIP_PENALTY, trim_penalty: int = DEFAULT_TRIM_PENALTY,
               unknown_cost: int = DEFAULT_UNKNOWN_COST, cpu: bool = False, device: int = 0, ev_start=None, ev_len=None):
    """The alignment (include/s2s_hip.h, next to s2s_eventalign) of the int16 event means means[p] to the int16 levels[p] AS THEY ARE
    (no normalisation; -32768 marks a k-mer without a level) -> dict(cost int64 [P], first / end int32 [P], per read kmer int32 [E]
    (-1: trimmed), k_start / k_len / k_events int32 [K]).  ev_start / ev_len: the events' samples per read (default: event e is
    sample e).  cost -1: an empty member; -3: no path."""
    if len(means) != len(levels):
        raise ValueError("means and levels must pair up")
    W, skip_penalty, trim_penalty, unknown_cost = _check_params(band_width, skip_penalty, trim_penalty, unknown_cost)
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    P = len(means)
    ms = [np.ascontiguousarray(x, np.int16).reshape(-1) for x in means]
    lv = [np.ascontiguousarray(x, np.int16).reshape(-1) for x in levels]
    if any(len(x) > MAX_SAMPLES for x in lv):
        raise ValueError(f"a read holds more than {MAX_SAMPLES} k-mers")
    E = [len(x) for x in ms]
    st = [np.arange(e, dtype=np.int32) if ev_start is None else np.ascontiguousarray(ev_start[p], np.int32) for p, e in enumerate(E)]
    ln = [np.ones(e, np.int32) if ev_len is None else np.ascontiguousarray(ev_len[p], np.int32) for p, e in enumerate(E)]
    if any(len(a) != e or len(b) != e for a, b, e in zip(st, ln, E)):
        raise ValueError("ev_start and ev_len must hold one value per event")
    m_offs = slots(E)
    ev = np.zeros((2, int(m_offs[-1])), np.int32)
    ev[0], ev[1] = np.concatenate(st + [np.zeros(0, np.int32)]), np.concatenate(ln + [np.zeros(0, np.int32)])
    B = Batch(ms, lambda offs: (ev[0], ev[1], device_only(lambda: slots([scratch_bytes(e, len(l), W) for e, l in zip(E, lv)]))), cpu, device)
    BL = Batch(lv, (), cpu, device)
    ET, KT = int(m_offs[-1]), BL.total
    res = B.alloc(cost=(np.int64, P), first=(np.int32, P), end=(np.int32, P), kmer=(np.int32, ET), k_start=(np.int32, KT),
                  k_len=(np.int32, KT), k_events=(np.int32, KT))
    B.call("eventalign", B.samples, B.offs(), BL.samples, BL.offs(), B.table(0), B.table(1), B.offs(), P, W, skip_penalty, trim_penalty,
           unknown_cost, res.ptr("cost"), B.scratch(lambda: B.tables[2][-1]), B.table(2), res.ptr("first"), res.ptr("end"), res.ptr("kmer"),
           res.ptr("k_start"), res.ptr("k_len"), res.ptr("k_events"))
    r = res.fetch()
    lo = BL.host_offs
    return dict(cost=r["cost"], first=r["first"], end=r["end"], kmer=[r["kmer"][m_offs[p]:m_offs[p + 1]] for p in range(P)],
                **{k: [r[k][lo[p]:lo[p + 1]] for p in range(P)] for k in ("k_start", "k_len", "k_events")})


def _account(r, p: int, n: int):
    """pore_align.Aligner.account: the read p of a _run_batch result, n samples long."""
    c, ke, E = int(r["cost"][p]), r["k_events"][p], max(int(r["n_events"][p]), 0)
    mm = (int(r["med"][p]), int(r["mad"][p]), int(r["lmed"][p]), int(r["lmad"][p]))
    if c < 0:
        return c, len(ke), mm, (E, 0, 0, 0, 0)
    first, end = int(r["first"][p]), int(r["end"][p])
    rows, aligned = int((ke > 0).sum()), end - first
    head = int(r["ev_start"][p][first])
    tail = n - int(r["ev_start"][p][end - 1] + r["ev_len"][p][end - 1])
    moves = dict(events=rows, aligned_events=aligned, skipped_kmers=len(ke) - rows, trimmed_head_samples=head, trimmed_tail_samples=tail)
    return (c, len(ke), mm, (E, aligned, len(ke) - rows, head, tail), aligned, moves,
            (r["k_start"][p], r["k_len"][p], r["S"][p], r["Q"][p]))


def eventalign_files(seqs, signals, model, out, band_width: int = DEFAULT_BAND_WIDTH, skip_penalty: int = DEFAULT_SKIP_PENALTY,
                     trim_penalty: int = DEFAULT_TRIM_PENALTY, unknown_cost: int = DEFAULT_UNKNOWN_COST, rna: bool = False,
                     window_short: int = DEFAULT_WINDOW_SHORT, window_long: int = DEFAULT_WINDOW_LONG,
                     threshold_short: float = DEFAULT_THRESHOLD_SHORT, threshold_long: float = DEFAULT_THRESHOLD_LONG,
                     with_samples: bool = False, cpu: bool = False, device: int = 0, summary_out=None,
                     max_samples: int = DEFAULT_MAX_SAMPLES, trace_memory: int = DEFAULT_TRACE_MEMORY, chunks=None,
                     model_out=None) -> dict:
    """pore_align.align_files with this module's solver (one row per unskipped k-mer) -> the counters: reads solved, unreached (no
    path inside the band), refused (or a walk back that may need more than trace_memory on its own: the bound of a read's decision
    scratch is that of s2s_segment_capacity events), without a sequence, without a known level, events (the rows: k-mers with
    events), aligned events, skipped k-mers, the samples trimmed at head and tail, and the mean cost per aligned event in MADs.
    summary_out: one row per read (SUMMARY_COLUMNS).  model_out: (NEW.model, min_events) -- the pore model re-estimated from these
    alignments."""
    W, skip_penalty, trim_penalty, unknown_cost = _check_params(band_width, skip_penalty, trim_penalty, unknown_cost)
    seg = _check_segment(window_short, window_long, threshold_int(threshold_short), threshold_int(threshold_long))
    return align_files(Aligner(
        name="eventalign", columns=SUMMARY_COLUMNS,
        counters=("events", "aligned_events", "skipped_kmers", "trimmed_head_samples", "trimmed_tail_samples"),
        params=dict(band_width=W, skip_penalty=skip_penalty, trim_penalty=trim_penalty, unknown_cost=unknown_cost, rna=bool(rna),
                    window_short=seg[0], window_long=seg[1], threshold_short=float(threshold_short), threshold_long=float(threshold_long)),
        need=lambda n, K: scratch_bound(n, K, W, seg[0]),
        refusal=f"eventalign: read %s refused: %d samples against %d k-mers at band width {W} (limit %d each; up to %d bytes of decision "
                "scratch against --trace-memory %d)",
        solve=lambda sig, lev, known, ch, mo: _run_batch(sig, lev, known, W, skip_penalty, trim_penalty, unknown_cost, seg, cpu, device,
                                                         chunks=ch, model_out=mo),
        account=_account, mean_key="mean_cost_per_event",
        log_tail="%d event row(s) of %d aligned event(s), %d skipped k-mer(s); %d / %d sample(s) trimmed at head / tail; mean cost per "
                 "aligned event %s MAD"), seqs, signals, model, out, rna, with_samples, cpu, summary_out, max_samples, trace_memory, chunks,
        model_out)
