"""The ground-truth base-to-signal alignment of simulated reads (`predict --alignment OUT.paf`): one PAF line per record of the
signal file, giving the stored samples of every k-mer.  The counts come from the GPU (Engine.align_chunks), the text from the
library's worker threads (s2s_paf_format, include/s2s_hip.h states the columns and the `ss:Z:` tokens); the reference writes no such
file.  The layout follows the published description of the signal-alignment PAF of squigulator / squigualiser and is NOT validated
against either tool."""
import os
from typing import Sequence

import numpy as np


def format_alignment(seg: np.ndarray, t_enc: int, read_first: np.ndarray, read_kmers: np.ndarray, read_offsets: np.ndarray,
                     read_ids: Sequence[str], rna: bool, threads: int = None) -> memoryview:
    """PAF text of one batch of reads (s2s_paf_format).  seg uint16 [B, t_enc+1] (Engine.align_chunks), read_first int32 [R+1],
    read_kmers [R] (real k-mers per read), read_offsets int64 [R+1] (export_reads), read_ids: the id of every RECORD -- the reads with
    at least one sample, in order."""
    from ._lib import lib
    from .signal_io import cpu_share
    L = lib()
    seg = np.ascontiguousarray(seg, dtype=np.uint16)
    read_first = np.ascontiguousarray(read_first, dtype=np.int32)
    read_kmers = np.ascontiguousarray(read_kmers, dtype=np.int64)
    read_offsets = np.ascontiguousarray(read_offsets, dtype=np.int64)
    R = read_first.shape[0] - 1
    B = int(read_first[-1]) if R >= 0 else 0
    if R < 0 or read_kmers.shape[0] != R or read_offsets.shape[0] != R + 1 or seg.size != B * (t_enc + 1):
        raise ValueError("seg [B, t_enc+1], read_first [R+1], read_kmers [R] and read_offsets [R+1] do not fit together")
    ids = [i.encode() for i in read_ids]
    id_offs = np.zeros(len(ids) + 1, np.int64)
    np.cumsum([len(i) for i in ids], out=id_offs[1:])
    blob = np.frombuffer(b"".join(ids) + b"\0", dtype=np.uint8)
    cap = int(L.s2s_paf_format_bound(B, int(t_enc), R, int(id_offs[-1])))
    out = np.empty(max(cap, 1), np.uint8)
    got = L.s2s_paf_format(seg.ctypes.data, int(t_enc), read_first.ctypes.data, read_kmers.ctypes.data, read_offsets.ctypes.data, R,
                           blob.ctypes.data, id_offs.ctypes.data, len(ids), int(bool(rna)), int(threads or cpu_share()),
                           out.ctypes.data, cap)
    if got < 0:
        raise RuntimeError(f"s2s_paf_format failed ({got}): the counts, offsets and record ids do not describe the same reads")
    return memoryview(out)[:got]


def join_rank_files(paths: Sequence[str], out: str, keep: bool = False) -> int:
    """The alignment files of the ranks of a multi-process run -> one file: plain bytes in the order given (the ranks own contiguous
    shares of the reads, so this is the single-process file); the rank files are removed unless keep.  -> bytes written."""
    import shutil
    n = 0
    with open(out, "wb") as dst:
        for p in paths:
            with open(p, "rb") as src:
                shutil.copyfileobj(src, dst, 1 << 22)
                n += src.tell()
    if not keep:
        for p in paths:
            if os.path.abspath(p) != os.path.abspath(out):
                os.remove(p)
    return n
