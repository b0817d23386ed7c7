"""`resquiggle SEQS SIGNALS --kmer-model M -o OUT.events.tsv`: which samples of a stored record belong to which k-mer of its sequence
-- the signal aligned to the levels a pore model (`predict --kmer-model`, or a nanopolish-style table) expects for its k-mers, and
written as the event table `predict --events` writes.  Everything that decides an output byte is an integer function stated in
include/s2s_hip.h next to s2s_resquiggle (tests/_resquiggle_ref.py restates it): samples and levels are median / MAD normalised by the
entries `compare` uses, the alignment is the dynamic programme of csrc/s2s_resquiggle.h (one workgroup per read, then a walk back),
the per-event sums are s2s_event_sums; `--cpu` runs the host twins of the same entries and gives the same bytes, as does any batching.
Per batch of reads (signal_batch.Batch): one host-to-device copy (offsets, slot tables, samples, levels) and the mask of k-mers
without a level, the kernels, one device-to-host copy of all results; the rows are formatted on the host in Python.  The reference
has no such command, and no f5c / uncalled4 was at hand: the output is unvalidated against them -- DESIGN.md section 6."""
import logging
import os
import time
from typing import Sequence

import click
import numpy as np

from .compare import EVENT_COLUMNS
from .signal_batch import (MAX_SAMPLES, SCALE, Batch, batches, calibration, check_band, device_only, event_level, max_band,
                           open_records, sample_at, slots)

logger = logging.getLogger("seq2squiggle")

UNKNOWN = -32768                 # S2S_RSQ_UNKNOWN: a k-mer without a level
UNREACHED = -3                   # S2S_RSQ_UNREACHED
DEFAULT_BAND = 512               # +-k-mers around the diagonal                       }
DEFAULT_SKIP_PENALTY = 128       # two MADs (64 units each) for a k-mer without sample } choices, not measurements
DEFAULT_UNKNOWN_COST = 64        # one MAD per sample on a k-mer without a level       }
MAX_SKIP_PENALTY = 1 << 20
MAX_UNKNOWN_COST = 65535
DEFAULT_MAX_SAMPLES = 1 << 27    # samples per batch
DEFAULT_TRACE_MEMORY = 8 << 30   # bytes of decision scratch per batch
LEVEL_SCALE = 64                 # levels enter as integers of 1/64 pA
SUMMARY_COLUMNS = ("read_id", "n_samples", "n_kmers", "status", "cost", "cost_per_sample", "events", "skipped", "med", "mad",
                   "level_med", "level_mad", "start", "end")
_CODE = np.full(256, -1, np.int64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


# ------------------------------------------------------------------ model and sequences
def read_model(path: str):
    """A pore model -> (k, levels float64 [4^k], NaN where the file has no row).  Reads what s2s_kmer_model_format writes (`#k`,
    `#alphabet`, the column line, rows) and any nanopolish-style table: lines that start with `#` are skipped, the first other line
    names the columns, `kmer` and `level_mean` are taken by name."""
    rows, cols, k = {}, None, None
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line or line.startswith("#"):
                continue
            v = line.split("\t") if "\t" in line else line.split()
            if cols is None:
                if "kmer" not in v or "level_mean" not in v:
                    raise click.ClickException(f"{path}: line {no}: a model needs the columns kmer and level_mean (found {v})")
                cols = (v.index("kmer"), v.index("level_mean"))
                continue
            try:
                kmer, level = v[cols[0]].upper().replace("U", "T"), float(v[cols[1]])
            except (IndexError, ValueError):
                raise click.ClickException(f"{path}: line {no} is not a row of a model")
            if k is None:
                k = len(kmer)
            if len(kmer) != k or not 1 <= k <= 10 or any(c not in "ACGT" for c in kmer):
                raise click.ClickException(f"{path}: line {no}: k-mer {kmer!r} (k-mers must be ACGT and of one length 1..10)")
            rows[kmer] = level
    if not rows:
        raise click.ClickException(f"{path}: no k-mer rows")
    levels = np.full(4 ** k, np.nan)
    for kmer, level in rows.items():
        levels[int(kmer_codes(kmer, k)[0])] = level
    return k, levels


def clean_sequence(seq: str) -> str:
    """The project's cleaning of a sequence (utils.process_genome): upper case, everything but ACGT -> N."""
    from .utils import process_genome
    return process_genome(seq)[0]


def kmer_codes(clean: str, k: int) -> np.ndarray:
    """-> int64 [len - k + 1]: the base-4 code of the k-mer at every base (A, C, G, T = 0..3, the first letter most significant: the
    row order of a model), -1 for a k-mer with a letter outside ACGT."""
    b = _CODE[np.frombuffer(clean.encode("latin-1"), np.uint8)]
    K = len(b) - k + 1
    if K < 1:
        return np.zeros(0, np.int64)
    code, bad = np.zeros(K, np.int64), np.zeros(K, bool)
    for t in range(k):
        code = code * 4 + np.maximum(b[t:t + K], 0)
        bad |= b[t:t + K] < 0
    code[bad] = -1
    return code


def level_ints(levels: np.ndarray):
    """The level table in pA -> (int16 [4^k]: round-half-even of 64 x pA, clamped to +-32767; bool [4^k]: has a level)."""
    known = np.isfinite(levels)
    x = np.clip(np.rint(np.where(known, levels, 0.0) * LEVEL_SCALE), -32767, 32767)
    return x.astype(np.int16), known


def read_sequences(path: str) -> dict:
    """FASTA / FASTQ -> {record name: cleaned sequence}; the first record of a name counts."""
    from .utils import read_fasta
    out = {}
    for seq, name in read_fasta(str(path)):
        out.setdefault(name, clean_sequence(seq))
    return out


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
               threads: int = None, sums: bool = True, chunks=None):
    """One batch of reads.  sig_list: the stored int16 samples; lev_list: int16 levels per k-mer (any value where known_list is False).
    norm: samples are normalised by their own median / MAD and the levels by the median / MAD of the read's KNOWN levels, both by
    s2s_signal_median_mad / s2s_signal_normalise at scale 64 (else both enter as they are); k-mers without a level get S2S_RSQ_UNKNOWN.
    -> dict(cost int64 [P], start / len int32 per read, S / Q int64 per read (raw samples), med / mad int32 [2 P]: samples, then levels).
    chunks: (preprocess.Chunker, the records' calibrations, the cleaned sequences) -- the training chunks are packed from the device
    buffers behind the sums; without it nothing else is uploaded or launched."""
    P = len(sig_list)
    known_recs = [np.asarray(l, np.int16)[np.asarray(kn, bool)] for l, kn in zip(lev_list, known_list)]
    full_recs = [np.where(np.asarray(kn, bool), np.asarray(l, np.int16), np.int16(0)).astype(np.int16) for l, kn in zip(lev_list, known_list)]
    unknown = ~np.concatenate([np.asarray(kn, bool).reshape(-1) for kn in known_list] + [np.zeros(0, bool)])

    def tables(offs):
        """The pool is 3 P records: samples, known levels, all levels -> l_offs int64 [P + 1]: the reads' slots of k-mers (the offsets
        of the third part from its start); s_offs int64 [P + 1]: their slots of decision scratch (device only)."""
        lens = np.diff(offs)
        extra = chunks[0].tables(chunks[1], chunks[2]) if chunks is not None else []
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
def format_rows(rid: str, clean: str, k: int, start, length, S, Q, signal: np.ndarray, cal, rna: bool, shift: int, with_samples: bool) -> str:
    """The rows of one solved read, by position: one per k-mer with samples.  start / length / S / Q are in the order the solver saw the
    levels (back to front for RNA); `shift` is added to start_idx / end_idx (the record's own coordinates with --intervals).  Level and
    deviation by signal_batch.event_level (include/s2s_hip.h, s2s_events_format), in double."""
    digitisation, offset, signal_range = cal
    K = len(start)
    order = range(K - 1, -1, -1) if rna else range(K)
    out = []
    for j in order:
        n = int(length[j])
        if n <= 0:
            continue
        pos = K - 1 - j if rna else j
        s, Sj, Qj = int(start[j]), int(S[j]), int(Q[j])
        mean, stdv = event_level(Sj, Qj, n, cal)
        row = f"{rid}\t{pos}\t{clean[pos:pos + k]}\t{s + shift}\t{s + n + shift}\t{'%.4f' % mean}\t{'%.4f' % stdv}"
        if with_samples:
            row += "\t" + ",".join("%.3f" % ((float(x) + offset) * signal_range / digitisation) for x in signal[s:s + n])
        out.append(row + "\n")
    return "".join(out)


def resquiggle_files(seqs, signals, model, out, band: int = DEFAULT_BAND, skip_penalty: int = DEFAULT_SKIP_PENALTY,
                     unknown_cost: int = DEFAULT_UNKNOWN_COST, rna: bool = False, intervals=None, with_samples: bool = False,
                     cpu: bool = False, device: int = 0, summary_out=None, max_samples: int = DEFAULT_MAX_SAMPLES,
                     trace_memory: int = DEFAULT_TRACE_MEMORY, chunks=None) -> dict:
    """Write OUT (EVENT_COLUMNS, plus `samples` with with_samples; records in the order of SIGNALS, rows by position) and return the
    counters: reads solved, unreached (no path: more than two k-mers per sample, or the band too narrow), refused (more than 2^22
    samples or k-mers, or a walk back that needs more than trace_memory on its own -- by read id, before the batch computes),
    without a sequence (no record of that name in SEQS, or fewer than k letters), without a known level, events, skipped k-mers, and
    the mean cost per sample in MADs (sum of costs / sum of samples / 64 over the solved reads).  A batch holds reads until their
    samples pass max_samples or their decision scratch passes trace_memory (at least one read).  rna: the stored signal is reversed,
    so the levels are read back to front; `position` stays in read coordinates and start_idx falls as it rises.  intervals: restrict
    every record that has a row to [b_start, b_end) (read_intervals); rows come out in the record's own coordinates.
    summary_out: one row per read (SUMMARY_COLUMNS).  chunks: (OUTDIR, seq_kmer, max_dna_len, max_signal_len) -- also write the
    training chunks of the solved reads there (preprocess.Chunker), from the device buffers; their counters come back under "chunks"."""
    band, skip_penalty, unknown_cost = _check_params(band, skip_penalty, unknown_cost)
    if int(max_samples) < 1 or int(trace_memory) < 1:
        raise ValueError("max_samples and trace_memory must be >= 1")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    k, levels = read_model(str(model))
    chunker = None
    if chunks is not None:
        from .preprocess import Chunker
        if int(chunks[1]) != k:
            raise click.ClickException(f"--seq-kmer {int(chunks[1])} is not the model's k = {k}")
        chunker = Chunker(chunks[0], k, chunks[2], chunks[3], rna)
    table, has = level_ints(levels)
    sequences = read_sequences(str(seqs))
    iv = read_intervals(str(intervals)) if intervals is not None else None
    cnt = dict(records=0, solved=0, unreached=0, refused=0, no_sequence=0, no_known_level=0, events=0, skipped_kmers=0)
    tot = dict(cost=0, samples=0, solve_s=0.0, format_s=0.0)
    with open(out, "w") as f, open(summary_out or os.devnull, "w") as fs:
        f.write("\t".join(EVENT_COLUMNS + (("samples",) if with_samples else ())) + "\n")
        fs.write("\t".join(SUMMARY_COLUMNS) + "\n")

        notes, written = {}, [0]                    # the summary rows come out in record order, whatever order they are known in

        def note(no, rid, n, K, status, b0, b1, cost="nan", per="nan", events=0, skipped=0, mm=("nan",) * 4):
            notes[no] = f"{rid}\t{n}\t{K}\t{status}\t{cost}\t{per}\t{events}\t{skipped}\t{mm[0]}\t{mm[1]}\t{mm[2]}\t{mm[3]}\t{b0}\t{b1}\n"
            while written[0] in notes:
                fs.write(notes.pop(written[0]))
                written[0] += 1

        def flush(batch):
            t0 = time.perf_counter()
            r = _run_batch([b[2] for b in batch], [b[3] for b in batch], [b[4] for b in batch], band, skip_penalty, unknown_cost, True,
                           cpu, device, chunks=None if chunker is None else (chunker, [b[5] for b in batch], [b[1] for b in batch]))
            t1 = time.perf_counter()
            P = len(batch)
            for p, (rid, clean, sig, _, _, cal, b0, b1, no, _) in enumerate(batch):
                c, ln = int(r["cost"][p]), r["len"][p]
                mm = (int(r["med"][p]), int(r["mad"][p]), int(r["med"][P + p]), int(r["mad"][P + p]))
                if c < 0:
                    cnt["unreached"] += 1
                    note(no, rid, len(sig), len(ln), "unreached", b0, b1, mm=mm)
                    continue
                events = int((ln > 0).sum())
                cnt["solved"] += 1
                cnt["events"] += events
                cnt["skipped_kmers"] += len(ln) - events
                tot["cost"] += c
                tot["samples"] += len(sig)
                f.write(format_rows(rid, clean, k, r["start"][p], ln, r["S"][p], r["Q"][p], sig, cal, rna, b0, with_samples))
                note(no, rid, len(sig), len(ln), "solved", b0, b1, c, "%.6f" % (c / len(sig) / SCALE), events, len(ln) - events, mm)
            tot["solve_s"] += t1 - t0
            tot["format_s"] += time.perf_counter() - t1

        def reads():
            """The records that go to the solver, as flush takes them; the others are counted and noted here."""
            for rec in open_records(str(signals)):
                no = cnt["records"]
                cnt["records"] += 1
                rid, sig = rec["read_id"], np.asarray(rec["signal"], np.int16)
                cal = calibration(rec)
                b0, b1 = 0, len(sig)
                if iv is not None and rid in iv:
                    b0, b1 = max(0, min(iv[rid][0], len(sig))), max(0, min(iv[rid][1], len(sig)))
                    b1 = max(b0, b1)
                    sig = sig[b0:b1]
                clean = sequences.get(rid)
                codes = kmer_codes(clean, k) if clean is not None else np.zeros(0, np.int64)
                if not len(codes):
                    cnt["no_sequence"] += 1
                    note(no, rid, len(sig), 0, "no_sequence", b0, b1)
                    continue
                known = (codes >= 0) & has[np.maximum(codes, 0)]
                lev = table[np.maximum(codes, 0)]
                if rna:
                    known, lev = known[::-1], lev[::-1]
                if not known.any():
                    cnt["no_known_level"] += 1
                    note(no, rid, len(sig), len(codes), "no_known_level", b0, b1)
                    continue
                need = 0 if len(sig) > MAX_SAMPLES or len(codes) > MAX_SAMPLES else scratch_bytes(len(sig), len(codes), band)
                if len(sig) > MAX_SAMPLES or len(codes) > MAX_SAMPLES or need > trace_memory:
                    cnt["refused"] += 1
                    logger.warning("resquiggle: read %s refused: %d samples against %d k-mers at band %d (limit %d each; %d bytes of decision "
                                   "scratch against --trace-memory %d)", rid, len(sig), len(codes), band, MAX_SAMPLES, need, trace_memory)
                    note(no, rid, len(sig), len(codes), "refused", b0, b1)
                    continue
                yield rid, clean, sig, lev, known, cal, b0, b1, no, need

        for batch in batches(reads(), lambda b: (len(b[2]), b[9]), (max_samples, trace_memory)):
            flush(batch)
    s = dict(seqs=str(seqs), signals=str(signals), model=str(model), out=str(out), k=k, band=band, skip_penalty=skip_penalty,
             unknown_cost=unknown_cost, rna=bool(rna), **cnt,
             mean_cost_per_sample=(tot["cost"] / tot["samples"] / SCALE) if tot["samples"] else None,
             solve_seconds=tot["solve_s"], format_seconds=tot["format_s"])
    if summary_out is not None:
        s["summary_out"] = str(summary_out)
    if chunker is not None:
        s["chunks"] = chunker.close("resquiggle")
    logger.info("resquiggle: %d record(s): %d solved, %d unreached, %d refused, %d without a sequence, %d without a known level; %d "
                "event(s), %d skipped k-mer(s); mean cost per sample %s MAD", cnt["records"], cnt["solved"], cnt["unreached"],
                cnt["refused"], cnt["no_sequence"], cnt["no_known_level"], cnt["events"], cnt["skipped_kmers"],
                "nan" if s["mean_cost_per_sample"] is None else "%.4f" % s["mean_cost_per_sample"])
    return s
