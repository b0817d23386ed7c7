"""`compare` on the GPU: s2s_median_mad_kernel, s2s_normalise_kernel and s2s_dtw_kernel (csrc/s2s_dtw.h) against the host entries and
against the restatement of their definitions (tests/_dtw_ref.py), for equality: record sizes around the 256-thread sweep, the
degenerate records of the rank selection, the normalisation at its clamp and half-way points; the DTW at the strip boundaries of a
64-lane sweep, with sloped bands, through a small ring for thousands of diagonals, at the largest band, past 2^32, in batches; then
the command itself, whose bytes must not depend on the batching nor on --cpu.  tests/test_compare_cpu.py holds the host entries to
the restatement on the same inputs, so the few large shapes are compared with the host entry and the row-wise restatement."""
import numpy as np
import pytest

from seq2squiggle_amd import compare as CMP
from _dtw_ref import ref_dtw, ref_dtw_rows, ref_median_mad, ref_normalise
from test_compare_cpu import (DTW_SHAPES, MAX_BAND, dtw_pair, median_records, mixed_batch, mixed_pairs, normalise_cases, squiggles,
                              write_file)

pytestmark = pytest.mark.gpu


def pairs_of(med, mad):
    return [(int(a), int(b)) for a, b in zip(med, mad)]


def test_median_mad_equals_host_and_restatement():
    for recs in (median_records(), mixed_batch()):
        med, mad = CMP.median_mad(recs)
        hmed, hmad = CMP.median_mad(recs, cpu=True)
        assert med.dtype == np.int32 and np.array_equal(med, hmed) and np.array_equal(mad, hmad)
        assert pairs_of(med, mad) == [ref_median_mad(r) for r in recs]
    # one record at a time gives what the batch gives
    recs = mixed_batch()[:12]
    med, mad = CMP.median_mad(recs)
    assert pairs_of(med, mad) == [pairs_of(*CMP.median_mad([r]))[0] for r in recs]
    assert CMP.median_mad([])[0].shape == (0,)


def test_normalise_equals_host_and_restatement():
    recs = median_records() + mixed_batch()[:40]
    med, mad = CMP.median_mad(recs)
    got, host = CMP.normalise(recs), CMP.normalise(recs, cpu=True)
    for r, q, h, m, d in zip(recs, got, host, med, mad):
        assert q.dtype == np.int16 and np.array_equal(q, h) and np.array_equal(q, ref_normalise(r, m, d))
    for x, m, d in normalise_cases():
        (q,) = CMP.normalise([x], med=[m], mad=[d])
        assert np.array_equal(q, ref_normalise(x, m, d)), (m, d)


def test_dtw_shapes_in_one_launch_and_alone():
    """Every listed (n, m, R): the pair alone, and all pairs of one R in one launch."""
    by_band = {}
    for n, m, R in DTW_SHAPES:
        by_band.setdefault(R, []).append(dtw_pair(n, m))
    for R, pairs in sorted(by_band.items()):
        al, bl = [p[0] for p in pairs], [p[1] for p in pairs]
        want = [ref_dtw(a, b, R) for a, b in pairs]
        got = CMP.dtw_banded(al, bl, R)
        assert got.dtype == np.int64 and got.tolist() == want, R
        assert CMP.dtw_banded(al, bl, R, cpu=True).tolist() == want
        assert [int(CMP.dtw_banded([a], [b], R)[0]) for a, b in pairs] == want
        assert CMP.dtw_banded(bl, al, R).tolist() == want                                  # symmetric
        # constant signals: cost 0, ties everywhere
        assert CMP.dtw_banded([np.full(len(a), -5, np.int16) for a in al], [np.full(len(b), -5, np.int16) for b in bl], R).tolist() == [0] * len(al)


def test_dtw_at_the_largest_band():
    a, b = dtw_pair(3000, 3000)
    want = ref_dtw_rows(a, b, MAX_BAND)
    assert int(CMP.dtw_banded([a], [b], MAX_BAND)[0]) == want == int(CMP.dtw_banded([a], [b], MAX_BAND, cpu=True)[0])
    # and a sloped band at it
    a, b = dtw_pair(2500, 700)
    assert int(CMP.dtw_banded([a], [b], MAX_BAND)[0]) == ref_dtw_rows(a, b, MAX_BAND)


def test_dtw_passes_2_to_the_32():
    a, b = np.full(70000, -32767, np.int16), np.full(70000, 32767, np.int16)
    got = int(CMP.dtw_banded([a], [b], 1)[0])
    assert got == 70000 * 65534 and got > 1 << 32
    assert got == int(CMP.dtw_banded([a], [b], 1, cpu=True)[0])


def test_dtw_batches():
    al, bl = mixed_pairs()
    want = CMP.dtw_banded(al, bl, 5, cpu=True).tolist()
    assert want[:40] == [ref_dtw(a, b, 5) for a, b in zip(al[:40], bl[:40])]
    assert sum(w == -1 for w in want) == 5 and min(want) == -1
    for P in (1, 2, 257):
        assert CMP.dtw_banded(al[:P], bl[:P], 5).tolist() == want[:P]
    two = np.concatenate([CMP.dtw_banded(al[:100], bl[:100], 5), CMP.dtw_banded(al[100:], bl[100:], 5)])
    assert two.tolist() == want
    assert CMP.dtw_banded([], [], 5).shape == (0,)


def test_compare_files_bytes_do_not_depend_on_batching_or_cpu(tmp_path):
    al, bl = mixed_pairs()
    rng = np.random.default_rng(4)
    keep = [i for i in range(len(al)) if len(al[i]) and len(bl[i])]              # (the writer skips empty records)
    sa = [np.concatenate([s, al[i]])[:len(al[i]) + 20] for i, s in zip(keep, squiggles(6, [20] * len(keep)))]
    sb = [bl[i] for i in keep]
    ids = [f"read{i}" for i in keep]
    order = rng.permutation(len(ids))
    a = write_file(tmp_path / "a.blow5", ids, sa)
    b = write_file(tmp_path / "b.blow5", [ids[k] for k in order], [sb[k] for k in order], signal_compression="svb-zd")
    outs = {}
    for tag, kw in (("one", {}), ("split", dict(max_samples=1500)), ("tiny", dict(max_samples=1)), ("cpu", dict(cpu=True))):
        s = CMP.compare_files(a, b, str(tmp_path / f"{tag}.tsv"), band=16, **kw)
        assert (s["pairs"], s["unpaired_a"], s["unpaired_b"]) == (len(ids), 0, 0)
        outs[tag] = open(tmp_path / f"{tag}.tsv", "rb").read()
    assert outs["one"] == outs["split"] == outs["tiny"] == outs["cpu"]
    rows = outs["one"].decode().splitlines()
    assert len(rows) == len(ids) + 1
    for k in (0, 1, len(ids) - 1):
        x, y = sa[k], sb[k]
        (mx, dx), (my, dy) = ref_median_mad(x), ref_median_mad(y)
        c = ref_dtw(ref_normalise(x, mx, dx), ref_normalise(y, my, dy), 16)
        assert rows[k + 1] == f"{ids[k]}\t{len(x)}\t{len(y)}\t{mx}\t{dx}\t{my}\t{dy}\t16\t{c}\t" + "%.6f" % (c / (len(x) + len(y)) / 64)
    none = CMP.compare_files(a, b, str(tmp_path / "none.tsv"), band=16, normalise="none", max_samples=1500)
    none_cpu = CMP.compare_files(a, b, str(tmp_path / "none_cpu.tsv"), band=16, normalise="none", cpu=True)
    assert open(tmp_path / "none.tsv", "rb").read() == open(tmp_path / "none_cpu.tsv", "rb").read()
    assert none["mean_dtw_per_sample"] == none_cpu["mean_dtw_per_sample"]
