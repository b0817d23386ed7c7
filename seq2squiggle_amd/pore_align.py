"""Reads against a pore model: what `resquiggle` and `eventalign` share above signal_batch.  The model and sequence helpers (a pore
model is the file `predict --kmer-model` writes, or a nanopolish-style table; levels enter the solvers as integers of 1/64 pA), the
split of a batch's levels into the records the solvers normalise, the rows of the event table, and `align_files`, the one file
driver: it reads the model and the sequences, filters the records of SIGNALS, batches those that go to a solver, and writes OUT,
the per-read summary and the training chunks.  A command is an `Aligner`: plain values and functions, no subclass."""
import logging
import os
import time
from dataclasses import dataclass
from typing import Callable, Optional

import click
import numpy as np

from .compare import EVENT_COLUMNS
from .signal_batch import MAX_SAMPLES, SCALE, batches, calibration, event_level, open_records

logger = logging.getLogger("seq2squiggle")

UNKNOWN = -32768                 # S2S_RSQ_UNKNOWN: a k-mer without a level
UNREACHED = -3                   # S2S_RSQ_UNREACHED
MAX_SKIP_PENALTY = 1 << 20
MAX_UNKNOWN_COST = 65535
DEFAULT_MAX_SAMPLES = 1 << 27    # samples per batch
DEFAULT_TRACE_MEMORY = 8 << 30   # bytes of decision scratch per batch
LEVEL_SCALE = 64                 # levels enter as integers of 1/64 pA
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


def split_levels(lev_list, known_list):
    """The int16 levels of a batch's reads (any value where known_list is False) -> (the records of the KNOWN levels, the records of
    all levels with 0 where unknown, the pooled mask of the k-mers without a level): the solvers take median / MAD over the first and
    normalise the second by them."""
    kn = [np.asarray(k, bool).reshape(-1) for k in known_list]
    lev = [np.asarray(l, np.int16).reshape(-1) for l in lev_list]
    return ([l[k] for l, k in zip(lev, kn)], [np.where(k, l, np.int16(0)).astype(np.int16) for l, k in zip(lev, kn)],
            ~np.concatenate(kn + [np.zeros(0, bool)]))


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


@dataclass
class Aligner:
    """What one command gives `align_files`."""
    name: str                   # in the log lines, and the chunker's label
    columns: tuple              # of the summary file: read_id, n_samples, n_kmers, status, cost, the cost per unit, the command's own,
                                # med, mad, level_med, level_mad and, with `clip`, start, end
    counters: tuple             # its counters, behind the six every command has
    params: dict                # its keys of the summary dict, between k and the counters
    need: Callable              # (samples, k-mers) -> bytes of decision scratch the read may take, before it runs
    refusal: str                # the warning of a refused read: rid, samples, k-mers, the limit of both, `need`, trace_memory
    solve: Callable             # (samples, levels, known flags per read; the chunks tuple of _run_batch or None; its model_out tuple
                                # or None) -> its result dict
    account: Callable           # (result, p, samples of read p) -> (cost, k-mers, (med, mad, level_med, level_mad), its summary
                                # fields, and for a cost >= 0: the units the cost is spread over, {counter: increment}, the
                                # (start, length, S, Q) of format_rows)
    mean_key: str               # of the summary dict: sum of costs / sum of units / 64 over the solved reads, None without any
    log_tail: str               # of the closing log line: the command's counters in their order, then the mean
    clip: Optional[Callable] = None     # () -> (rid, samples) -> (samples, start, end): restrict a record before its sequence is looked
                                        # up; called once, behind the sequences.  Rows are shifted by start


def align_files(cmd: Aligner, seqs, signals, model, out, rna: bool, with_samples: bool, cpu: bool, summary_out, max_samples: int,
                trace_memory: int, chunks, model_out=None) -> dict:
    """Write OUT (EVENT_COLUMNS, plus `samples` with with_samples; records in the order of SIGNALS, rows by position), one summary row
    per read (cmd.columns, in record order) and, with chunks = (OUTDIR, seq_kmer, max_dna_len, max_signal_len), the training chunks of
    the solved reads (preprocess.Chunker, from the device buffers) and, with model_out = (NEW.model, min_events), the pore model
    re-estimated from the run's own alignments (kmer_model.ModelBuilder, from the same buffers); -> the summary dict.  A record goes to
    the solver unless it has no sequence (no record of that name in SEQS, or fewer than k letters), no k-mer with a level, or is
    refused: more than 2^22 samples or k-mers, or cmd.need beyond trace_memory on its own -- by read id, before the batch computes.  A
    batch holds reads until their samples pass max_samples or their needs pass trace_memory (at least one read).  rna: the levels are
    read back to front."""
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
    builder = None
    if model_out is not None:
        from .kmer_model import ModelBuilder
        builder = ModelBuilder(k, rna)
    table, has = level_ints(levels)
    sequences = read_sequences(str(seqs))
    clip = cmd.clip() if cmd.clip is not None else None
    own = ("0",) * (len(cmd.columns) - (10 if clip is None else 12))
    cnt = dict.fromkeys(("records", "solved", "unreached", "refused", "no_sequence", "no_known_level") + cmd.counters, 0)
    tot = dict(cost=0, units=0, solve_s=0.0, format_s=0.0)
    with open(out, "w") as f, open(summary_out or os.devnull, "w") as fs:
        f.write("\t".join(EVENT_COLUMNS + (("samples",) if with_samples else ())) + "\n")
        fs.write("\t".join(cmd.columns) + "\n")

        notes, written = {}, [0]                    # the summary rows come out in record order, whatever order they are known in

        def note(no, rid, n, K, status, span, cost="nan", per="nan", fields=own, mm=("nan",) * 4):
            notes[no] = "\t".join(map(str, (rid, n, K, status, cost, per, *fields, *mm, *span))) + "\n"
            while written[0] in notes:
                fs.write(notes.pop(written[0]))
                written[0] += 1

        def flush(batch):
            t0 = time.perf_counter()
            r = cmd.solve([b[2] for b in batch], [b[3] for b in batch], [b[4] for b in batch],
                          None if chunker is None else (chunker, [b[5] for b in batch], [b[1] for b in batch]),
                          None if builder is None else (builder, [b[5] for b in batch], [b[1] for b in batch]))
            t1 = time.perf_counter()
            for p, (rid, clean, sig, _, _, cal, span, no, _) in enumerate(batch):
                c, K, mm, fields, *solved = cmd.account(r, p, len(sig))
                if c < 0:
                    cnt["unreached"] += 1
                    note(no, rid, len(sig), K, "unreached", span, fields=fields, mm=mm)
                    continue
                units, moves, spans = solved
                cnt["solved"] += 1
                for key, by in moves.items():
                    cnt[key] += by
                tot["cost"] += c
                tot["units"] += units
                f.write(format_rows(rid, clean, k, *spans, sig, cal, rna, span[0] if span else 0, with_samples))
                note(no, rid, len(sig), K, "solved", span, c, "%.6f" % (c / units / SCALE), fields, mm)
            tot["solve_s"] += t1 - t0
            tot["format_s"] += time.perf_counter() - t1

        def reads():
            """The records that go to the solver, as flush takes them; the others are counted and noted here."""
            for rec in open_records(str(signals)):
                no = cnt["records"]
                cnt["records"] += 1
                rid, sig = rec["read_id"], np.asarray(rec["signal"], np.int16)
                cal = calibration(rec)
                span = ()
                if clip is not None:
                    sig, *span = clip(rid, sig)
                clean = sequences.get(rid)
                codes = kmer_codes(clean, k) if clean is not None else np.zeros(0, np.int64)
                if not len(codes):
                    cnt["no_sequence"] += 1
                    note(no, rid, len(sig), 0, "no_sequence", span)
                    continue
                known = (codes >= 0) & has[np.maximum(codes, 0)]
                lev = table[np.maximum(codes, 0)]
                if rna:
                    known, lev = known[::-1], lev[::-1]
                if not known.any():
                    cnt["no_known_level"] += 1
                    note(no, rid, len(sig), len(codes), "no_known_level", span)
                    continue
                long = len(sig) > MAX_SAMPLES or len(codes) > MAX_SAMPLES
                need = 0 if long else cmd.need(len(sig), len(codes))
                if long or need > trace_memory:
                    cnt["refused"] += 1
                    logger.warning(cmd.refusal, rid, len(sig), len(codes), MAX_SAMPLES, need, trace_memory)
                    note(no, rid, len(sig), len(codes), "refused", span)
                    continue
                yield rid, clean, sig, lev, known, cal, span, no, need

        for batch in batches(reads(), lambda b: (len(b[2]), b[8]), (max_samples, trace_memory)):
            flush(batch)
    mean = (tot["cost"] / tot["units"] / SCALE) if tot["units"] else None
    s = dict(seqs=str(seqs), signals=str(signals), model=str(model), out=str(out), k=k, **cmd.params, **cnt, **{cmd.mean_key: mean},
             solve_seconds=tot["solve_s"], format_seconds=tot["format_s"])
    if summary_out is not None:
        s["summary_out"] = str(summary_out)
    if chunker is not None:
        s["chunks"] = chunker.close(cmd.name)
    if builder is not None:
        s["kmer_model"] = builder.close(model_out[0], model_out[1])
    logger.info("%s: %d record(s): %d solved, %d unreached, %d refused, %d without a sequence, %d without a known level; " + cmd.log_tail,
                cmd.name, *cnt.values(), "nan" if mean is None else "%.4f" % mean)
    return s
