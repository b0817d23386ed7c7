"""`preprocess EVENTS.tsv OUTDIR`, and `--chunks OUTDIR` of `resquiggle` and `eventalign`: the training chunks the reference's
`preprocess` makes from an event table -- `chunks-NNNN.npy`, `chunks_lengths-`, `targets-`, `targets_lengths-`, `stdevs-`, the
directory `evaluate` reads.  The definition is stated in include/s2s_hip.h next to s2s_chunk_pack (tests/_preprocess_ref.py restates
it); it follows the reference's process_df -> get_chunks -> pad_lengths -> typical_indices per read, with the deviations the README
lists (no permutation, always per read, stdevs [N, te] float32, targets_lengths the true sum, no all-pad chunk for a read without
rows).  Everything that decides an output byte is one call of s2s_chunk_pack (or, with `--cpu`, of its host twin, which gives the
same bytes) per batch on buffers that already lie on the batch's side (signal_batch.Batch): behind `resquiggle` / `eventalign` the
alignment never leaves the device between the solver and the chunks.  Only the kept prefix of each output comes down."""
import logging
import os
import time
from typing import Optional, Sequence

import click
import numpy as np

from .signal_batch import Batch, batches

logger = logging.getLogger("seq2squiggle")

RAW, PA = 0, 1                   # S2S_CHUNK_RAW / S2S_CHUNK_PA
MAX_K, MAX_TE, MAX_TS = 10, 64, 1024
MAX_SLOTS = 1 << 22              # per read
KINDS = ("chunks", "chunks_lengths", "targets", "targets_lengths", "stdevs")
DEFAULT_CHUNKS_PER_FILE = 100_000   # a choice: 265 MB of targets and chunks per file set at 16 / 250 / 9
DEFAULT_MAX_SAMPLES = 1 << 27    # samples per batch
TABLE_COLUMNS = ("read_name", "position", "model_kmer", "start_idx", "end_idx", "event_stdv", "samples")
COUNTERS = ("reads", "rows", "all_n_rows", "pad_rows", "chunks_formed", "chunks_kept", "chunks_too_long")


def check_geometry(k: int, te: int, ts: int):
    k, te, ts = int(k), int(te), int(ts)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"seq_kmer must be 1..{MAX_K}")
    if not 1 <= te <= MAX_TE:
        raise ValueError(f"max_dna_len must be 1..{MAX_TE}")
    if not 1 <= ts <= MAX_TS:
        raise ValueError(f"max_signal_len must be 1..{MAX_TS}")
    return k, te, ts


def capacity(slot_counts, te: int) -> int:
    """The chunks a batch can form at most: the sum over the reads of floor(slots / te) + 1."""
    return int(sum(int(n) // int(te) + 1 for n in slot_counts))


def scratch_bytes(slots: int, P: int, cap: int) -> int:
    from ._lib import lib
    r = int(lib().s2s_chunk_scratch_bytes(int(slots), int(P), int(cap)))
    if r < 0:
        raise ValueError("slots, reads or chunk capacity beyond the limits of s2s_chunk_pack")
    return r


def sliding_kmers(clean: str, k: int) -> np.ndarray:
    """-> uint8 [len - k + 1, k]: the letters of the k-mer at every base of a cleaned sequence."""
    b = np.frombuffer(clean.encode("latin-1"), np.uint8)
    if len(b) < k:
        return np.zeros((0, k), np.uint8)
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(b, k))


def pack_batch(B: Batch, source: int, pool, s_offs, total: int, l_offs, slots: int, ev_start, ev_len, S, Q, cal, stdv, kmers, P: int,
               k: int, te: int, ts: int, reverse: bool, backwards: bool, cap: int) -> dict:
    """One call of s2s_chunk_pack / s2s_chunk_pack_host on pointers of the batch's side -> {kind: array of the kept chunks}, n_rows
    int32 [P], counters int64 [3] (formed, kept, all-N rows).  The count comes down first, then the kept prefix of each output; the
    unused capacity is neither zeroed nor copied."""
    P, cap, slots = int(P), int(cap), int(slots)
    small = B.alloc(n_rows=(np.int32, P), counters=(np.int64, 3))
    big = B.alloc_raw(chunks=(np.uint16, cap * te * k * 5), chunks_lengths=(np.int64, cap * te), targets=(np.float32, cap * ts),
                      targets_lengths=(np.int64, cap), stdevs=(np.float32, cap * te))
    B.call("chunk_pack", pool, s_offs, int(total), int(source), l_offs, slots, ev_start, ev_len, S, Q, cal, stdv, kmers, P, k, te, ts,
           int(bool(reverse)), int(bool(backwards)), cap, B.scratch(lambda: scratch_bytes(slots, P, cap)), big.ptr("chunks"),
           big.ptr("chunks_lengths"), big.ptr("targets"), big.ptr("targets_lengths"), big.ptr("stdevs"), small.ptr("n_rows"),
           small.ptr("counters"))
    r = small.fetch()
    formed, kept = int(r["counters"][0]), int(r["counters"][1])
    if formed > cap:
        raise RuntimeError(f"s2s_chunk_pack formed {formed} chunks, more than the capacity {cap}")
    return {"chunks": big.prefix("chunks", kept * te * k * 5).view(np.float16).reshape(kept, te, k, 5),
            "chunks_lengths": big.prefix("chunks_lengths", kept * te).reshape(kept, te),
            "targets": big.prefix("targets", kept * ts).reshape(kept, ts),
            "targets_lengths": big.prefix("targets_lengths", kept).reshape(kept),
            "stdevs": big.prefix("stdevs", kept * te).reshape(kept, te),
            "n_rows": r["n_rows"].copy(), "counters": r["counters"].copy()}


def pack(l_offs, ev_start, ev_len, kmers, k: int, te: int, ts: int, records: Optional[Sequence[np.ndarray]] = None, S=None, Q=None,
         cal=None, pool=None, s_offs=None, stdv=None, reverse: bool = False, backwards: bool = False, cpu: bool = False, device: int = 0,
         cap: Optional[int] = None, threads: Optional[int] = None) -> dict:
    """The chunks of host arrays, one batch.  Raw source: `records` (stored int16, one per read) with S, Q and cal float64 [P, 3]
    (digitisation, offset, range).  pa source: `pool` float32 with s_offs int64 [P + 1] and stdv float32 per slot.  Slots of read p:
    [l_offs[p], l_offs[p + 1]) of ev_start / ev_len / kmers (uint8 [slots, k]).  cap: the chunk capacity (default: what always
    suffices)."""
    k, te, ts = check_geometry(k, te, ts)
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    l_offs = np.ascontiguousarray(l_offs, np.int64)
    P, slots = len(l_offs) - 1, int(l_offs[-1])
    cap = capacity(np.diff(l_offs), te) if cap is None else int(cap)
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)          # noqa: E731
    letters = np.ascontiguousarray(kmers, np.uint8).reshape(-1)
    if records is not None:
        B = Batch(records, (l_offs, i32(ev_start), i32(ev_len), np.ascontiguousarray(S, np.int64), np.ascontiguousarray(Q, np.int64),
                            np.ascontiguousarray(cal, np.float64), letters), cpu, device, threads)
        return pack_batch(B, RAW, B.samples, B.offs(), B.total, B.table(0), slots, B.table(1), B.table(2), B.table(3), B.table(4),
                          B.table(5), None, B.table(6), P, k, te, ts, reverse, backwards, cap)
    pool = np.ascontiguousarray(pool, np.float32).reshape(-1)
    B = Batch([], (np.ascontiguousarray(s_offs, np.int64), l_offs, i32(ev_start), i32(ev_len), np.ascontiguousarray(stdv, np.float32),
                   pool, letters), cpu, device, threads)
    return pack_batch(B, PA, B.table(5), B.table(0), len(pool), B.table(1), slots, B.table(2), B.table(3), None, None, None, B.table(4),
                      B.table(6), P, k, te, ts, reverse, backwards, cap)


class ChunkWriter:
    """Buffers kept chunks and writes a numbered file set (<kind>-NNNN.npy, the five KINDS) every `chunks_per_file` chunks, the
    remainder at close; a run without a chunk writes one empty set, so that OUTDIR is a dataset.  The bytes on disk depend on the
    chunks and their order alone, not on how they were batched.  After `max_chunks` chunks the writer is `full` and takes no more."""

    def __init__(self, outdir: str, k: int, te: int, ts: int, chunks_per_file: int = DEFAULT_CHUNKS_PER_FILE,
                 max_chunks: Optional[int] = None):
        self.k, self.te, self.ts = check_geometry(k, te, ts)
        if int(chunks_per_file) < 1:
            raise ValueError("chunks_per_file must be >= 1")
        if max_chunks is not None and int(max_chunks) < 0:
            raise ValueError("max_chunks must be >= 0")
        self.outdir, self.per_file = str(outdir), int(chunks_per_file)
        self.max_chunks = None if max_chunks is None else int(max_chunks)
        self.held = {kind: [] for kind in KINDS}
        self.n_held = self.taken = self.files = 0
        self.seconds = 0.0
        os.makedirs(self.outdir, exist_ok=True)

    @property
    def full(self) -> bool:
        return self.max_chunks is not None and self.taken >= self.max_chunks

    def add(self, arrays: dict) -> int:
        """Take the chunks of one batch (the arrays of pack_batch) up to max_chunks -> how many were taken."""
        n = len(arrays["targets_lengths"])
        if self.max_chunks is not None:
            n = min(n, self.max_chunks - self.taken)
        if n > 0:
            for kind in KINDS:
                self.held[kind].append(arrays[kind][:n])
            self.n_held += n
            self.taken += n
        while self.n_held >= self.per_file:
            self._write(self.per_file)
        return max(n, 0)

    def _write(self, n: int) -> None:
        t0 = time.perf_counter()
        for kind in KINDS:
            a = np.concatenate(self.held[kind]) if self.held[kind] else self._empty(kind)
            np.save(os.path.join(self.outdir, f"{kind}-{self.files:04d}.npy"), np.ascontiguousarray(a[:n]))
            self.held[kind] = [a[n:]] if len(a) > n else []
        self.n_held -= n
        self.files += 1
        self.seconds += time.perf_counter() - t0

    def _empty(self, kind: str) -> np.ndarray:
        return {"chunks": np.zeros((0, self.te, self.k, 5), np.float16), "chunks_lengths": np.zeros((0, self.te), np.int64),
                "targets": np.zeros((0, self.ts), np.float32), "targets_lengths": np.zeros(0, np.int64),
                "stdevs": np.zeros((0, self.te), np.float32)}[kind]

    def close(self) -> int:
        """Write what is held -> the number of file sets written in all."""
        if self.n_held or not self.files:
            self._write(self.n_held)
        return self.files


def new_counters() -> dict:
    return dict.fromkeys(COUNTERS, 0)


def tally(cnt: dict, r: dict, te: int) -> None:
    """Add one batch's n_rows / counters (pack_batch) to the running counters."""
    n = r["n_rows"].astype(np.int64)
    cnt["reads"] += len(n)
    cnt["rows"] += int(n.sum())
    cnt["all_n_rows"] += int(r["counters"][2])
    cnt["pad_rows"] += int((te - n[n > 0] % te).sum())
    cnt["chunks_formed"] += int(r["counters"][0])
    cnt["chunks_kept"] += int(r["counters"][1])
    cnt["chunks_too_long"] += int(r["counters"][0] - r["counters"][1])


def log_counters(command: str, cnt: dict, files: int, written: int, outdir) -> None:
    logger.info("%s: %d read(s): %d row(s), %d all-N row(s) dropped, %d pad row(s); %d chunk(s) formed, %d kept, %d dropped as too long; "
                "%d chunk(s) in %d file set(s) -> %s", command, cnt["reads"], cnt["rows"], cnt["all_n_rows"], cnt["pad_rows"],
                cnt["chunks_formed"], cnt["chunks_kept"], cnt["chunks_too_long"], written, files, outdir)


class Chunker:
    """`--chunks OUTDIR` of `resquiggle` and `eventalign`: after a batch's last s2s_event_sums, `pack` cuts the chunks from the
    alignment where it lies -- (ev_start, ev_len, S, Q) per k-mer slot next to the raw samples, the raw source -- and hands the kept
    ones to a ChunkWriter.  `tables` gives the two arrays a batch uploads for it with its own: the records' calibrations and the
    letters of every slot, a sliding window of the cleaned sequence (back to front where the slots are laid so: rna)."""

    def __init__(self, outdir, k: int, te: int, ts: int, rna: bool = False, chunks_per_file: int = DEFAULT_CHUNKS_PER_FILE,
                 max_chunks: Optional[int] = None):
        self.writer = ChunkWriter(outdir, k, te, ts, chunks_per_file, max_chunks)
        self.k, self.te, self.ts, self.rna = self.writer.k, self.writer.te, self.writer.ts, bool(rna)
        self.cnt, self.pack_s = new_counters(), 0.0

    def tables(self, cal_list, clean_list):
        cal = np.array([tuple(c) for c in cal_list], np.float64).reshape(-1)
        letters = [sliding_kmers(c, self.k)[::-1] if self.rna else sliding_kmers(c, self.k) for c in clean_list]
        return [cal, np.concatenate(letters + [np.zeros((0, self.k), np.uint8)]).reshape(-1)]

    def pack(self, B: Batch, P: int, l_offs, slot_counts, ev_start, ev_len, S, Q, cal, kmers) -> None:
        """l_offs ... kmers: pointers on the batch's side; slot_counts: the reads' slots, on the host."""
        t0 = time.perf_counter()
        r = pack_batch(B, RAW, B.samples, B.offs(), B.total, l_offs, int(np.sum(slot_counts)), ev_start, ev_len, S, Q, cal, None, kmers, P,
                       self.k, self.te, self.ts, self.rna, self.rna, capacity(slot_counts, self.te))
        tally(self.cnt, r, self.te)
        self.writer.add(r)
        self.pack_s += time.perf_counter() - t0

    def close(self, command: str) -> dict:
        files = self.writer.close()
        log_counters(command + " --chunks", self.cnt, files, self.writer.taken, self.writer.outdir)
        return dict(outdir=self.writer.outdir, seq_kmer=self.k, max_dna_len=self.te, max_signal_len=self.ts, **self.cnt,
                    chunks_written=self.writer.taken, files=files, pack_seconds=self.pack_s, write_seconds=self.writer.seconds)


# ------------------------------------------------------------------ the table
def read_table(events_tsv: str, k: int):
    """The event table `predict --events --events-samples`, `resquiggle --samples` and `eventalign --samples` write -> the reads in
    order of first appearance, each (name, position int64 [n], letters uint8 [n, k], length int64 [n], stdv float32 [n], [float32
    samples per row]), rows sorted by position (stable).  Columns are taken by name."""
    path = str(events_tsv)
    reads = {}
    with open(path) as f:
        head = f.readline().rstrip("\r\n").split("\t")
        if "samples" not in head:
            raise click.ClickException(f"{path}: line 1: the table has no `samples` column; write it with `predict --events "
                                       "--events-samples`, `resquiggle --samples` or `eventalign --samples`")
        missing = [c for c in TABLE_COLUMNS if c not in head]
        if missing:
            raise click.ClickException(f"{path}: line 1: an event table needs the columns {', '.join(TABLE_COLUMNS)} (missing: "
                                       f"{', '.join(missing)})")
        ci = [head.index(c) for c in TABLE_COLUMNS]
        for no, line in enumerate(f, 2):
            v = line.rstrip("\r\n").split("\t")
            if v == [""]:
                continue
            try:
                name, kmer = v[ci[0]], v[ci[2]]
                pos, a, b = int(v[ci[1]]), int(v[ci[3]]), int(v[ci[4]])
                dev = np.float32(float(v[ci[5]]))
                text = v[ci[6]]
                x = np.array(text.split(","), np.float64).astype(np.float32) if text else np.zeros(0, np.float32)
            except (IndexError, ValueError):
                raise click.ClickException(f"{path}: line {no} is not a row of an event table with samples")
            if len(kmer) != k:
                raise click.ClickException(f"{path}: line {no}: model_kmer {kmer!r} has {len(kmer)} letters, seq_kmer is {k}")
            if len(x) != b - a:
                raise click.ClickException(f"{path}: line {no}: {len(x)} sample(s) for a row of length end_idx - start_idx = {b - a}")
            reads.setdefault(name, []).append((pos, kmer, b - a, dev, x))
    out = []
    for name, rows in reads.items():
        order = np.argsort(np.array([r[0] for r in rows], np.int64), kind="stable")
        rows = [rows[i] for i in order]
        letters = np.frombuffer("".join(r[1] for r in rows).encode("latin-1"), np.uint8).reshape(len(rows), k)
        out.append((name, np.array([r[0] for r in rows], np.int64), letters, np.array([r[2] for r in rows], np.int64),
                    np.array([r[3] for r in rows], np.float32), [r[4] for r in rows]))
    return out


def preprocess_table(events_tsv, outdir, k: int, te: int, ts: int, rna: bool = False, chunks_per_file: int = DEFAULT_CHUNKS_PER_FILE,
                     max_chunks: Optional[int] = None, max_samples: int = DEFAULT_MAX_SAMPLES, cpu: bool = False, device: int = 0) -> dict:
    """EVENTS.tsv -> the file sets under OUTDIR and the counters.  The table feeds the pa source: every sample text is parsed as a
    double and rounded to fp32, event_stdv likewise.  rna: every row's samples are read back to front.  A batch holds reads until
    their samples pass max_samples (at least one read)."""
    k, te, ts = check_geometry(k, te, ts)
    if int(max_samples) < 1:
        raise ValueError("max_samples must be >= 1")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    t0 = time.perf_counter()
    reads = read_table(events_tsv, k)
    for name, _, _, length, _, _ in reads:
        if len(length) > MAX_SLOTS:
            raise click.ClickException(f"{events_tsv}: read {name} has more than {MAX_SLOTS} rows")
    parse_s = time.perf_counter() - t0
    writer = ChunkWriter(outdir, k, te, ts, chunks_per_file, max_chunks)
    cnt, pack_s = new_counters(), 0.0
    for batch in batches(reads, lambda r: (int(r[3].sum()),), (int(max_samples),)):
        if writer.full:
            break
        t1 = time.perf_counter()
        length = np.concatenate([r[3] for r in batch])
        l_offs = np.concatenate([[0], np.cumsum([len(r[3]) for r in batch])]).astype(np.int64)
        s_offs = np.concatenate([[0], np.cumsum([int(r[3].sum()) for r in batch])]).astype(np.int64)
        ev_start = np.concatenate([np.cumsum(r[3]) - r[3] for r in batch])
        pool = np.concatenate([x for r in batch for x in r[5]] + [np.zeros(0, np.float32)])
        r = pack(l_offs, ev_start, length, np.concatenate([b[2] for b in batch]), k, te, ts, pool=pool, s_offs=s_offs,
                 stdv=np.concatenate([b[4] for b in batch]), reverse=rna, cpu=cpu, device=device)
        pack_s += time.perf_counter() - t1
        tally(cnt, r, te)
        writer.add(r)
    files = writer.close()
    s = dict(events=str(events_tsv), outdir=str(outdir), seq_kmer=k, max_dna_len=te, max_signal_len=ts, rna=bool(rna), **cnt,
             chunks_written=writer.taken, files=files, parse_seconds=parse_s, pack_seconds=pack_s, write_seconds=writer.seconds)
    log_counters("preprocess", cnt, files, writer.taken, outdir)
    return s
