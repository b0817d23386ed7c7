"""s2s_chunk_pack on the device against its host twin, bit for bit (floats included): the cases of tests/test_preprocess_cpu.py, and
the sizes at which the kernels of csrc/s2s_chunk.h take another trip -- more reads than one block of the scan, more chunks than 64
trips of it, one read far longer than all others (the pooled split), a full wave of rows, and a chunk whose first row alone passes
ts.  All tiny: each takes well under a second of device time."""
import numpy as np
import pytest

import _preprocess_cases as C
import _preprocess_ref as R

pytestmark = pytest.mark.gpu


def both(case, source, te, ts, **kw):
    host = C.run(case, source, te, ts, cpu=True, **kw)
    dev = C.run(case, source, te, ts, cpu=False, **kw)
    C.same(host, dev, (source, te, ts, kw))
    return host


@pytest.mark.parametrize("te,ts,k", C.GEOMETRIES)
def test_device_equals_host_on_the_standard_batch(te, ts, k):
    case = C.standard(te, ts, k)
    for source in (R.RAW, R.PA):
        for reverse in (False, True):
            for backwards in (False, True):
                both(case, source, te, ts, reverse=reverse, backwards=backwards)


@pytest.mark.parametrize("te,ts,k", C.GEOMETRIES)
def test_device_equals_host_on_the_edge_cases(te, ts, k):
    for name, case in C.edges(te, ts, k).items():
        for source in (R.RAW, R.PA):
            r = both(case, source, te, ts, reverse=(source == R.PA))
            if name in ("keeps_nothing", "no_rows"):
                assert r["counters"][1] == 0 and r["targets"].shape == (0, ts)


def test_more_reads_than_one_scan_block():
    rng = np.random.default_rng(3)
    case = C.make(rng, 6, [rng.integers(1, 9, rng.integers(1, 4)) for _ in range(3000)], letters=b"ACGTN")
    r = both(case, R.RAW, 5, 37)
    assert r["counters"][0] == 3000 and 0 < r["counters"][1] <= 3000
    both(case, R.PA, 5, 37, backwards=True)


@pytest.mark.parametrize("P,te,ts,k", C.MANY_READS)
def test_second_and_third_step_of_the_scans_over_reads_and_capacity(P, te, ts, k):
    """s2s_chunk_pack launches the in-place instance of s2s_scan_kernel (csrc/s2s_prims.h) over the reads' chunk counts (P entries)
    and over the chunk capacity.  The cases below already take both scans deep into later steps (3,000 reads; 70,010 chunks); what is
    new here is the border itself: 1,025 and 2,049 reads of one or two rows leave ONE entry for the second and for the third step
    of 1,024, and at te = 1, where every read forms at least two chunks, the capacity scan passes 2,048 and 4,096 entries.  Both sample sources; every
    output and the three counters against the host twin, byte for byte.  The scan over the tiles takes a second step only past
    1,024 tiles, two million slots: it is the same instance that tests/test_gpu_segment_scan.py drives past 2,048 tiles through
    s2s_segment, so it is left out here."""
    case = C.many_reads(P, te, ts, k)
    for source in (R.RAW, R.PA):
        r = both(case, source, te, ts, reverse=(source == R.PA))
        assert len(r["n_rows"]) == P and r["counters"][0] > (2 * P if te == 1 else P) - 1 and r["counters"][1] > 0


def test_more_chunks_than_64_trips_of_the_scan():
    rng = np.random.default_rng(4)
    case = C.make(rng, 1, [rng.integers(1, 3, 7000) for _ in range(10)], gaps=False)
    r = both(case, R.RAW, 1, 1)
    assert r["counters"][0] == 70010 and 10 < r["counters"][1] < 70010           # rows of 2 samples are dropped, the pad chunks kept


def test_one_long_read_beside_short_ones():
    rng = np.random.default_rng(5)
    lens = [rng.integers(1, 30, rng.integers(1, 40)) for _ in range(50)]
    lens.insert(17, rng.integers(8, 24, 200000))
    case = C.make(rng, 9, lens, letters=b"ACGTN", gaps=False)
    r = both(case, R.RAW, 16, 250)
    assert r["n_rows"][17] > 190000 and r["counters"][1] > 1000
    both(case, R.PA, 16, 250, reverse=True, backwards=True)


def test_a_full_wave_of_rows():
    rng = np.random.default_rng(6)
    case = C.make(rng, 10, [[16] * 64, [16] * 128, [16] * 63 + [17]])
    r = both(case, R.RAW, 64, 1024, reverse=True)
    # every read ends with a chunk of 64 pads; the read with a row of 17 samples keeps that chunk alone
    assert list(r["targets_lengths"]) == [1024, 64, 1024, 1024, 64, 64]


def test_first_row_alone_exceeds_ts():
    rng = np.random.default_rng(7)
    case = C.make(rng, 9, [[251] + [1] * 15 + [3] * 16, [5000] + [1] * 40])
    r = both(case, R.RAW, 16, 250)
    assert r["counters"][0] == 6 and r["counters"][1] == 4


# ------------------------------------------------------------------ the reference's own chunk cutting (tests/golden/preprocess_*.npz)
@pytest.mark.parametrize("te,ts,k", C.GEOMETRIES)
def test_device_equals_the_reference_goldens(te, ts, k, tmp_path):
    """The `preprocess` command on the golden's table text and `pack` on its arrays, on the device, against what the reference's own
    functions gave (tests/test_preprocess_golden_cpu.py holds the host to the same files): every byte, after the documented mappings.
    The read listed with falling positions goes in alone, its slots in the table's order, with backwards=True."""
    g = C.golden(te, ts, k)
    case = C.golden_case(g)
    falling = str(g["falling_read"])
    listed, rows = C.golden_case(g, only=falling, as_listed=True), C.golden_rows_of(g, falling)
    for rna in (False, True):
        got, s = C.command(g, tmp_path / ("rna" if rna else "dna"), rna, cpu=False)
        assert C.same_as_golden(g, rna, got, what=("command", rna)) == len(g["kept"]) > 0
        assert (s["chunks_formed"], s["chunks_kept"], s["all_n_rows"]) == (len(g["t_lengths"]), len(g["kept"]), 3)
        got = C.run(case, R.PA, te, ts, reverse=rna, cpu=False)
        C.same_as_golden(g, rna, got, what=("pack", rna))
        assert got["counters"].tolist() == [len(g["t_lengths"]), len(g["kept"]), 3]
        got = C.run(listed, R.PA, te, ts, reverse=rna, backwards=True, cpu=False)
        assert C.same_as_golden(g, rna, got, rows=rows, what=("pack backwards", rna)) == len(rows) >= 2
