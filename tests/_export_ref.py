"""The definition of s2s_export_reads (include/s2s_hip.h) in numpy, for tests/test_gpu_export.py: the per-read zero-strip, the
packed pA, and the int16 of tests/_events_ref.py::ref_dac, reversed per read for RNA."""
import numpy as np

from _events_ref import ref_dac


def ref_export(sig, read_first, dig, rng, off, rna):
    """sig float32 [B, ts] (no NaN: ref_dac does not define them), read_first [R+1] with read_first[0] == 0, read_first[R] == B,
    non-decreasing -> (offsets int64 [R+1], pa float32 [total], dac int16 [total]).
    A sample is kept where sig != 0 (-0.0 is dropped, a subnormal is kept), chunk after chunk in row order.  pa is NEVER reversed;
    dac is reversed inside every read when rna (only out_dac is, by the header)."""
    sig = np.asarray(sig, np.float32)
    B = sig.shape[0]
    rf = np.asarray(read_first, np.int64)
    assert not np.isnan(sig).any() and rf[0] == 0 and rf[-1] == B and (np.diff(rf) >= 0).all()
    keep = sig != 0
    chunk_offs = np.concatenate([[0], np.cumsum(keep.sum(axis=1, dtype=np.int64))]).astype(np.int64)
    offsets = chunk_offs[rf]
    pa = sig[keep]                                            # (boolean indexing walks the array in row order)
    dac = ref_dac(pa, dig, rng, off).astype(np.int16)
    assert pa.dtype == np.float32 and pa.size == offsets[-1]
    if rna:
        for r in range(len(rf) - 1):
            dac[offsets[r]:offsets[r + 1]] = dac[offsets[r]:offsets[r + 1]][::-1].copy()
    return offsets, pa, dac
