"""`resquiggle SEQS SIGNALS --kmer-model M -o OUT.events.tsv`: which samples of a stored record belong to which k-mer of its sequence
-- the signal aligned to the levels a pore model (`predict --kmer-model`, or a nanopolish-style table) expects for its k-mers, and
written as the event table `predict --events` writes.  Everything that decides an output byte is an integer function stated in
include/s2s_hip.h next to s2s_resquiggle (tests/_resquiggle_ref.py restates it): samples and levels are median / MAD normalised by the
entries `compare` uses, the alignment is the dynamic programme of csrc/s2s_resquiggle.h (one workgroup per read, then a walk back),
the per-event sums are s2s_event_sums; `--cpu` runs the host twins of the same entries and gives the same bytes, as does any batching.
Per batch of reads: one host-to-device copy (offsets, samples, levels), the kernels, two device-to-host copies (int64 and int32
results); the rows are formatted on the host in Python.  The reference has no such command, and no f5c / uncalled4 was at hand: the
output is unvalidated against them -- DESIGN.md section 6."""
import logging
import math
import os
import time
from typing import Sequence

import click
import numpy as np

from . import compare as C

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
EVENT_COLUMNS = C.EVENT_COLUMNS
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
    band, skip_penalty, unknown_cost = C._check_band(band), int(skip_penalty), int(unknown_cost)
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
        raise ValueError(f"band must be 1..{C.max_band()}")
    return r


def _slots(need) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(need)]).astype(np.int64)


def _run_batch(sig_list, lev_list, known_list, band: int, skip_penalty: int, unknown_cost: int, norm: bool, cpu: bool, device: int = 0,
               threads: int = None, sums: bool = True):
    """One batch of reads.  sig_list: the stored int16 samples; lev_list: int16 levels per k-mer (any value where known_list is False).
    norm: samples are normalised by their own median / MAD and the levels by the median / MAD of the read's KNOWN levels, both by
    s2s_signal_median_mad / s2s_signal_normalise at scale 64 (else both enter as they are); k-mers without a level get S2S_RSQ_UNKNOWN.
    -> dict(cost int64 [P], start / len int32 per read, S / Q int64 per read (raw samples), med / mad int32 [2 P]: samples, then levels)."""
    from ._lib import lib
    L = lib()
    P = len(sig_list)
    known_recs = [np.asarray(l, np.int16)[np.asarray(kn, bool)] for l, kn in zip(lev_list, known_list)]
    full_recs = [np.where(np.asarray(kn, bool), np.asarray(l, np.int16), np.int16(0)).astype(np.int16) for l, kn in zip(lev_list, known_list)]
    flat, offs = C._pack(list(sig_list) + known_recs + full_recs)
    lens = np.diff(offs)
    n, K = lens[:P], lens[2 * P:]
    l_offs = (offs[2 * P:] - offs[2 * P]).astype(np.int64)
    KT, l0 = int(l_offs[-1]), int(offs[2 * P])
    unknown = ~np.concatenate([np.asarray(kn, bool).reshape(-1) for kn in known_list] + [np.zeros(0, bool)])
    need = np.array([scratch_bytes(n[p], K[p], band) for p in range(P)], np.int64)
    s_offs = _slots(need)
    out64 = np.zeros(P + 2 * max(KT, 1), np.int64)                  # cost, S, Q
    out32 = np.zeros(2 * max(KT, 1) + 4 * P, np.int32)              # start, len, med [2 P], mad [2 P]
    kt = max(KT, 1)
    if cpu:
        threads = threads or C._host_threads()
        med, mad = out32[2 * kt:2 * kt + 2 * P], out32[2 * kt + 2 * P:]
        q = flat
        if norm:
            C._check(L.s2s_signal_median_mad_host(flat.ctypes.data, offs.ctypes.data, 2 * P, med.ctypes.data, mad.ctypes.data, threads),
                     "s2s_signal_median_mad_host")
            q = np.zeros(len(flat), np.int16)
            C._check(L.s2s_signal_normalise_host(flat.ctypes.data, offs.ctypes.data, P, med.ctypes.data, mad.ctypes.data, C.SCALE,
                                                 q.ctypes.data, threads), "s2s_signal_normalise_host")
            C._check(L.s2s_signal_normalise_host(flat.ctypes.data, offs.ctypes.data + 16 * P, P, med.ctypes.data + 4 * P,
                                                 mad.ctypes.data + 4 * P, C.SCALE, q.ctypes.data, threads), "s2s_signal_normalise_host")
        else:
            q = flat.copy()
        q[l0:][unknown] = UNKNOWN
        C._check(L.s2s_resquiggle_host(q.ctypes.data, offs.ctypes.data, q.ctypes.data + 2 * l0, l_offs.ctypes.data, P, band, skip_penalty,
                                       unknown_cost, out64.ctypes.data, out32.ctypes.data, out32.ctypes.data + 4 * kt, threads),
                 "s2s_resquiggle_host")
        if sums:
            C._check(L.s2s_event_sums_host(flat.ctypes.data, offs.ctypes.data, out32.ctypes.data, out32.ctypes.data + 4 * kt,
                                           l_offs.ctypes.data, P, out64.ctypes.data + 8 * P, out64.ctypes.data + 8 * (P + kt), threads),
                     "s2s_event_sums_host")
    else:
        extra = np.concatenate([l_offs, s_offs]).astype(np.int64).view(np.uint8)
        dev = C._Device(flat, offs, device, extra=extra)
        torch, where = dev.torch, f"cuda:{dev.device}"
        d64 = torch.zeros(len(out64), dtype=torch.int64, device=where)
        d32 = torch.zeros(len(out32), dtype=torch.int32, device=where)
        p64, p32 = d64.data_ptr(), d32.data_ptr()
        med_p, mad_p = p32 + 8 * kt, p32 + 8 * kt + 8 * P
        if norm:
            C._check(L.s2s_signal_median_mad(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, 2 * P, med_p, mad_p), "s2s_signal_median_mad")
            q = torch.zeros(max(dev.total, 1), dtype=torch.int16, device=where)
            C._check(L.s2s_signal_normalise(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, P, med_p, mad_p, C.SCALE, q.data_ptr()),
                     "s2s_signal_normalise")
            C._check(L.s2s_signal_normalise(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr + 16 * P, P, med_p + 4 * P, mad_p + 4 * P,
                                            C.SCALE, q.data_ptr()), "s2s_signal_normalise")
        else:
            q = dev.up[dev.samples_ptr - dev.offs_ptr:].view(torch.int16).clone() if dev.total else torch.zeros(1, dtype=torch.int16, device=where)
        if KT:                                          # the marker of a k-mer without a level (a fill, no arithmetic)
            q[l0:l0 + KT].masked_fill_(torch.from_numpy(unknown).to(where), UNKNOWN)
        scratch = torch.empty(max(int(s_offs[-1]), 16), dtype=torch.uint8, device=where)
        q_ptr = q.data_ptr()
        C._check(L.s2s_resquiggle(dev.device, dev.stream, q_ptr, dev.offs_ptr, q_ptr + 2 * l0, dev.extra_ptr, P, band, skip_penalty,
                                  unknown_cost, p64, scratch.data_ptr(), dev.extra_ptr + 8 * (P + 1), p32, p32 + 4 * kt), "s2s_resquiggle")
        if sums:
            C._check(L.s2s_event_sums(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, p32, p32 + 4 * kt, dev.extra_ptr, P,
                                      p64 + 8 * P, p64 + 8 * (P + kt)), "s2s_event_sums")
        out64, out32 = d64.cpu().numpy(), d32.cpu().numpy()
    cut = lambda a: [a[l_offs[p]:l_offs[p + 1]] for p in range(P)]      # noqa: E731
    return dict(cost=out64[:P], start=cut(out32[:kt]), len=cut(out32[kt:2 * kt]), S=cut(out64[P:P + kt]), Q=cut(out64[P + kt:]),
                med=out32[2 * kt:2 * kt + 2 * P], mad=out32[2 * kt + 2 * P:2 * kt + 4 * P])


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
    if any(np.size(l) > C.MAX_SAMPLES for l in levels):
        raise ValueError(f"a read holds more than {C.MAX_SAMPLES} k-mers")
    need = [scratch_bytes(min(np.size(s), C.MAX_SAMPLES), np.size(l), band) for s, l in zip(samples, levels)]
    for p, nb in enumerate(need):
        if nb > trace_memory:
            raise ValueError(f"read {p}: the walk back needs {nb} bytes of decision scratch, more than trace_memory = {trace_memory}")
    cost, start, length, s0, held = [np.zeros(0, np.int64)], [], [], 0, 0
    for p in range(len(need) + 1):
        if p == len(need) or (p > s0 and held + need[p] > trace_memory):
            if p > s0:
                lev = [np.asarray(l, np.int16).reshape(-1) for l in levels[s0:p]]
                r = _run_batch(samples[s0:p], lev, [l != UNKNOWN for l in lev], band, skip_penalty, unknown_cost, False, cpu, device, sums=False)
                cost.append(r["cost"])
                start += r["start"]
                length += r["len"]
            s0, held = p, 0
        if p < len(need):
            held += need[p]
    return np.concatenate(cost), start, length


def event_sums(samples: Sequence[np.ndarray], start: Sequence[np.ndarray], length: Sequence[np.ndarray], cpu: bool = False, device: int = 0):
    """-> ([S int64 per read], [Q int64 per read]): sum and sum of squares of samples[p][start[j] : start[j] + length[j]) per k-mer
    (s2s_event_sums); 0, 0 for a skipped k-mer or an interval outside the record."""
    from ._lib import lib
    L = lib()
    P = len(samples)
    flat, offs = C._pack(samples)
    st = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in start]
    ln = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in length]
    l_offs = _slots([len(x) for x in st])
    kt = max(int(l_offs[-1]), 1)
    ev = np.zeros(2 * kt, np.int32)
    ev[:l_offs[-1]] = np.concatenate(st + [np.zeros(0, np.int32)])
    ev[kt:kt + l_offs[-1]] = np.concatenate(ln + [np.zeros(0, np.int32)])
    out = np.zeros(2 * kt, np.int64)
    if cpu:
        C._check(L.s2s_event_sums_host(flat.ctypes.data, offs.ctypes.data, ev.ctypes.data, ev.ctypes.data + 4 * kt, l_offs.ctypes.data, P,
                                       out.ctypes.data, out.ctypes.data + 8 * kt, C._host_threads()), "s2s_event_sums_host")
    else:
        import torch
        dev = C._Device(flat, offs, device, extra=np.concatenate([l_offs, ev.view(np.int64)]).view(np.uint8))
        d = torch.zeros(2 * kt, dtype=torch.int64, device=f"cuda:{dev.device}")
        ev_p = dev.extra_ptr + 8 * (P + 1)
        C._check(L.s2s_event_sums(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, ev_p, ev_p + 4 * kt, dev.extra_ptr, P, d.data_ptr(),
                                  d.data_ptr() + 8 * kt), "s2s_event_sums")
        out = d.cpu().numpy()
    return [out[l_offs[p]:l_offs[p + 1]] for p in range(P)], [out[kt + l_offs[p]:kt + l_offs[p + 1]] for p in range(P)]


# ------------------------------------------------------------------ files
def format_rows(rid: str, clean: str, k: int, start, length, S, Q, signal: np.ndarray, cal, rna: bool, shift: int, with_samples: bool) -> str:
    """The rows of one solved read, by position: one per k-mer with samples.  start / length / S / Q are in the order the solver saw the
    levels (back to front for RNA); `shift` is added to start_idx / end_idx (the record's own coordinates with --intervals).  Level and
    deviation by the formulas of compare.transfer_events (include/s2s_hip.h, s2s_events_format), in double."""
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
        mean = (float(Sj) / n + offset) * signal_range / digitisation
        stdv = math.sqrt(float(max(n * Qj - Sj * Sj, 0))) / n * signal_range / digitisation
        row = f"{rid}\t{pos}\t{clean[pos:pos + k]}\t{s + shift}\t{s + n + shift}\t{'%.4f' % mean}\t{'%.4f' % stdv}"
        if with_samples:
            row += "\t" + ",".join("%.3f" % ((float(x) + offset) * signal_range / digitisation) for x in signal[s:s + n])
        out.append(row + "\n")
    return "".join(out)


def resquiggle_files(seqs, signals, model, out, band: int = DEFAULT_BAND, skip_penalty: int = DEFAULT_SKIP_PENALTY,
                     unknown_cost: int = DEFAULT_UNKNOWN_COST, rna: bool = False, intervals=None, with_samples: bool = False,
                     cpu: bool = False, device: int = 0, summary_out=None, max_samples: int = DEFAULT_MAX_SAMPLES,
                     trace_memory: int = DEFAULT_TRACE_MEMORY) -> dict:
    """Write OUT (EVENT_COLUMNS, plus `samples` with with_samples; records in the order of SIGNALS, rows by position) and return the
    counters: reads solved, unreached (no path: more than two k-mers per sample, or the band too narrow), refused (more than 2^22
    samples or k-mers, or a walk back that needs more than trace_memory on its own -- by read id, before the batch computes),
    without a sequence (no record of that name in SEQS, or fewer than k letters), without a known level, events, skipped k-mers, and
    the mean cost per sample in MADs (sum of costs / sum of samples / 64 over the solved reads).  A batch holds reads until their
    samples pass max_samples or their decision scratch passes trace_memory (at least one read).  rna: the stored signal is reversed,
    so the levels are read back to front; `position` stays in read coordinates and start_idx falls as it rises.  intervals: restrict
    every record that has a row to [b_start, b_end) (read_intervals); rows come out in the record's own coordinates.
    summary_out: one row per read (SUMMARY_COLUMNS)."""
    band, skip_penalty, unknown_cost = _check_params(band, skip_penalty, unknown_cost)
    if int(max_samples) < 1 or int(trace_memory) < 1:
        raise ValueError("max_samples and trace_memory must be >= 1")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    k, levels = read_model(str(model))
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
                           cpu, device)
            t1 = time.perf_counter()
            P = len(batch)
            for p, (rid, clean, sig, _, _, cal, b0, b1, no) in enumerate(batch):
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
                note(no, rid, len(sig), len(ln), "solved", b0, b1, c, "%.6f" % (c / len(sig) / C.SCALE), events, len(ln) - events, mm)
            tot["solve_s"] += t1 - t0
            tot["format_s"] += time.perf_counter() - t1

        batch, held, held_scratch = [], 0, 0
        for rec in C._open_records(str(signals)):
            no = cnt["records"]
            cnt["records"] += 1
            rid, sig = rec["read_id"], np.asarray(rec["signal"], np.int16)
            cal = (float(rec["digitisation"]), float(rec["offset"]), float(rec["range"]))
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
            need = 0 if len(sig) > C.MAX_SAMPLES or len(codes) > C.MAX_SAMPLES else scratch_bytes(len(sig), len(codes), band)
            if len(sig) > C.MAX_SAMPLES or len(codes) > C.MAX_SAMPLES or need > trace_memory:
                cnt["refused"] += 1
                logger.warning("resquiggle: read %s refused: %d samples against %d k-mers at band %d (limit %d each; %d bytes of decision "
                               "scratch against --trace-memory %d)", rid, len(sig), len(codes), band, C.MAX_SAMPLES, need, trace_memory)
                note(no, rid, len(sig), len(codes), "refused", b0, b1)
                continue
            if batch and (held + len(sig) > max_samples or held_scratch + need > trace_memory):
                flush(batch)
                batch, held, held_scratch = [], 0, 0
            batch.append((rid, clean, sig, lev, known, cal, b0, b1, no))
            held += len(sig)
            held_scratch += need
        if batch:
            flush(batch)
    s = dict(seqs=str(seqs), signals=str(signals), model=str(model), out=str(out), k=k, band=band, skip_penalty=skip_penalty,
             unknown_cost=unknown_cost, rna=bool(rna), **cnt,
             mean_cost_per_sample=(tot["cost"] / tot["samples"] / C.SCALE) if tot["samples"] else None,
             solve_seconds=tot["solve_s"], format_seconds=tot["format_s"])
    if summary_out is not None:
        s["summary_out"] = str(summary_out)
    logger.info("resquiggle: %d record(s): %d solved, %d unreached, %d refused, %d without a sequence, %d without a known level; %d "
                "event(s), %d skipped k-mer(s); mean cost per sample %s MAD", cnt["records"], cnt["solved"], cnt["unreached"],
                cnt["refused"], cnt["no_sequence"], cnt["no_known_level"], cnt["events"], cnt["skipped_kmers"],
                "nan" if s["mean_cost_per_sample"] is None else "%.4f" % s["mean_cost_per_sample"])
    return s
