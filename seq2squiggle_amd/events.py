"""The per-k-mer event table of simulated reads (`predict --events OUT.tsv`): for every k-mer that owns stored samples its range in
the record's signal and the mean and population deviation (ddof 0) of those samples in pA, optionally the samples themselves.  The
counts and integer sums come from the GPU (Engine.event_stats), the text from the library's worker threads (s2s_events_format;
include/s2s_hip.h states the columns); the reference writes no such file.  The columns carry the names the reference's `preprocess`
reads from an eventalign table (read_name, position, model_kmer, start_idx, end_idx, event_stdv, samples) and are unvalidated against
the tools that write such tables (f5c eventalign, uncalled4 align) -- DESIGN.md section 6."""
import os
from typing import Sequence

import numpy as np


def format_events(seg: np.ndarray, sums: np.ndarray, sumsq: np.ndarray, t_enc: int, read_first: np.ndarray, read_kmers: np.ndarray,
                  read_offsets: np.ndarray, read_ids: Sequence[str], letters: np.ndarray, letter_offsets: np.ndarray, k: int,
                  digitisation: float, signal_range: float, offset: float, rna: bool, dac: np.ndarray = None,
                  with_header: bool = False, threads: int = None) -> memoryview:
    """Event rows of one batch of reads (s2s_events_format).  seg uint16 / sums int32 / sumsq int64 [B, t_enc+1] (Engine.event_stats),
    read_first int32 [R+1], read_kmers [R], read_offsets int64 [R+1] (export_reads), read_ids: the id of every RECORD (the reads with at
    least one sample, in order), letters uint8 + letter_offsets int64 [R+1]: the cleaned letters of every read (pack_reads' flat
    blob and where each read starts in it), dac: the packed int16 samples (export_reads) for the `samples` column, or None."""
    from ._lib import lib
    from .signal_io import cpu_share
    L = lib()
    seg = np.ascontiguousarray(seg, dtype=np.uint16)
    sums = np.ascontiguousarray(sums, dtype=np.int32)
    sumsq = np.ascontiguousarray(sumsq, dtype=np.int64)
    read_first = np.ascontiguousarray(read_first, dtype=np.int32)
    read_kmers = np.ascontiguousarray(read_kmers, dtype=np.int64)
    read_offsets = np.ascontiguousarray(read_offsets, dtype=np.int64)
    letters = np.ascontiguousarray(letters, dtype=np.uint8)
    letter_offsets = np.ascontiguousarray(letter_offsets, dtype=np.int64)
    R = read_first.shape[0] - 1
    B = int(read_first[-1]) if R >= 0 else 0
    n = B * (t_enc + 1)
    if (R < 0 or read_kmers.shape[0] != R or read_offsets.shape[0] != R + 1 or letter_offsets.shape[0] != R + 1
            or seg.size != n or sums.size != n or sumsq.size != n):
        raise ValueError("seg / sums / sumsq [B, t_enc+1], read_first [R+1], read_kmers [R], read_offsets [R+1] and letter_offsets "
                         "[R+1] do not fit together")
    if R and (letter_offsets[0] < 0 or letter_offsets[-1] > letters.size or (np.diff(letter_offsets) < 0).any()):
        raise ValueError("letter_offsets do not lie inside letters")
    n_samples = int(read_offsets[-1] - read_offsets[0]) if R else 0
    if dac is not None:
        dac = np.ascontiguousarray(dac, dtype=np.int16)
        if R and (read_offsets[0] < 0 or dac.size < int(read_offsets[-1])):
            raise ValueError("dac is shorter than read_offsets say")
    ids = [i.encode() for i in read_ids]
    id_offs = np.zeros(len(ids) + 1, np.int64)
    np.cumsum([len(i) for i in ids], out=id_offs[1:])
    blob = np.frombuffer(b"".join(ids) + b"\0", dtype=np.uint8)
    cal = (float(digitisation), float(signal_range), float(offset))
    cap = int(L.s2s_events_format_bound(B, int(t_enc), max((len(i) for i in ids), default=0), int(k), *cal,
                                        n_samples if dac is not None else 0, int(bool(with_header))))
    if cap < 0:
        raise ValueError("digitisation and range must be non-zero numbers, k and t_enc at least 1")
    out = np.empty(max(cap, 1), np.uint8)
    got = L.s2s_events_format(seg.ctypes.data, sums.ctypes.data, sumsq.ctypes.data, int(t_enc), read_first.ctypes.data,
                              read_kmers.ctypes.data, read_offsets.ctypes.data, R, blob.ctypes.data, id_offs.ctypes.data, len(ids),
                              letters.ctypes.data, letter_offsets.ctypes.data, int(k), *cal,
                              dac.ctypes.data if dac is not None else None, int(bool(rna)), int(bool(with_header)),
                              int(threads or cpu_share()), out.ctypes.data, cap)
    if got < 0:
        raise RuntimeError(f"s2s_events_format failed ({got}): the counts, offsets, letters and record ids do not describe the same reads")
    return memoryview(out)[:got]


def join_rank_files(paths: Sequence[str], out: str, keep: bool = False) -> int:
    """The event tables of the ranks of a multi-process run -> one file: the rank files in the order given (the ranks own contiguous
    shares of the reads), the header line of the first one only; the rank files are removed unless keep.  -> bytes written."""
    import shutil
    n = 0
    with open(out, "wb") as dst:
        for i, p in enumerate(paths):
            with open(p, "rb") as src:
                if i:
                    src.readline()                  # every rank file starts with the header
                start = src.tell()
                shutil.copyfileobj(src, dst, 1 << 22)
                n += src.tell() - start
    if not keep:
        for p in paths:
            if os.path.abspath(p) != os.path.abspath(out):
                os.remove(p)
    return n
