"""`resquiggle` without a GPU: the host twins (s2s_resquiggle_host, s2s_event_sums_host) against the Python restatement of the
definition (tests/_resquiggle_ref.py) and the invariants of a solved read, their refusals, the model reader on a file the project
writes, and the command with --cpu on hand-written files: a planted read comes back as exactly its planted table."""
import json
import math

import numpy as np
import pytest
from click.testing import CliRunner

import _resquiggle_ref as REF
from _dtw_ref import ref_median_mad, ref_normalise
from _events_ref import parse_events
from seq2squiggle_amd import _lib, cli, kmer_model
from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import signal_batch as SB
from seq2squiggle_amd import resquiggle as RSQ
from test_compare_cpu import write_file


def host(reads, band, skip=REF.SKIP, unk=REF.UNK, threads=1):
    """s2s_resquiggle_host on raw pointers, outputs preset to 77 -> (rc, cost, [start], [len])."""
    L = _lib.lib()
    q = [np.ascontiguousarray(r[0], np.int16) for r in reads]
    l = [np.ascontiguousarray(r[1], np.int16) for r in reads]
    qf, lf = np.concatenate(q + [np.zeros(1, np.int16)]), np.concatenate(l + [np.zeros(1, np.int16)])
    qo = np.concatenate([[0], np.cumsum([len(x) for x in q])]).astype(np.int64)
    lo = np.concatenate([[0], np.cumsum([len(x) for x in l])]).astype(np.int64)
    cost = np.full(len(reads), 77, np.int64)
    st, ln = np.full(int(lo[-1]) + 1, 77, np.int32), np.full(int(lo[-1]) + 1, 77, np.int32)
    rc = L.s2s_resquiggle_host(qf.ctypes.data, qo.ctypes.data, lf.ctypes.data, lo.ctypes.data, len(reads), band, skip, unk,
                               cost.ctypes.data, st.ctypes.data, ln.ctypes.data, threads)
    assert st[-1] == 77 and ln[-1] == 77
    return rc, cost, [st[lo[p]:lo[p + 1]] for p in range(len(reads))], [ln[lo[p]:lo[p + 1]] for p in range(len(reads))]


@pytest.mark.parametrize("kind", REF.KINDS)
@pytest.mark.parametrize("n,K,R", REF.SMALL)
def test_host_twin_equals_the_restatement(n, K, R, kind):
    q, l, plant = REF.case(n, K, R, kind)
    cost, start, length = REF.solve(q, l, R, REF.SKIP, REF.UNK)
    rc, c, st, ln = host([(q, l)], R)
    assert rc == 0 and int(c[0]) == cost
    assert st[0].tolist() == start and ln[0].tolist() == length
    if (n, K, R) in ((1, 2, 1), (3, 7, 4)):
        assert cost == REF.UNREACHED and set(start) == {-1} and set(length) == {0}
    else:
        REF.check_invariants(q, l, R, REF.SKIP, REF.UNK, cost, st[0], ln[0])
    if plant is not None:
        assert cost == 0 and (st[0] == plant[0]).all() and (ln[0] == plant[1]).all()
    if (n, K, R) == (2, 3, 2):
        assert ln[0].tolist() == [1, 0, 1]              # the skip is forced
    if (n, K, R) == (200, 260, 16):
        assert (ln[0] == 0).sum() >= 60                 # more k-mers than samples: at least K - n skips


def test_planted_shapes_are_planted():
    assert sum(REF.case(n, K, R, "planted")[2] is not None for n, K, R in REF.SMALL) >= 11


@pytest.mark.parametrize("n,K,R", REF.LARGE)
def test_host_twin_large_shapes_keep_the_invariants(n, K, R):
    for kind in ("noisy", "planted"):
        q, l, plant = REF.case(n, K, R, kind)
        rc, c, st, ln = host([(q, l)], R)
        assert rc == 0
        REF.check_invariants(q, l, R, REF.SKIP, REF.UNK, int(c[0]), st[0], ln[0])
        if plant is not None:
            assert int(c[0]) == 0 and (st[0] == plant[0]).all() and (ln[0] == plant[1]).all()


def test_host_twin_cost_passes_2_32():
    n, K, R = REF.EXTREME
    rc, c, st, ln = host([(np.full(n, 32767, np.int16), np.full(K, -32767, np.int16))], R)
    assert rc == 0 and int(c[0]) == 65534 * n > 1 << 32
    assert int(ln[0].sum()) == n


def test_host_twin_batch_threads_and_parameters():
    reads = [REF.case(n, K, 8, kind)[:2] for (n, K, kind) in ((300, 290, "noisy"), (0, 5, "noisy"), (40, 0, "noisy"), (120, 50, "unknown"),
                                                              (3, 7, "noisy"), (90, 100, "zeros"))]
    rc, c, st, ln = host(reads, 8, threads=3)
    assert rc == 0 and c[1] == REF.EMPTY and c[2] == REF.EMPTY and c[4] == REF.UNREACHED
    assert set(st[1].tolist()) == {-1} and set(ln[1].tolist()) == {0}
    for p in (0, 3, 5):
        cost, start, length = REF.solve(*reads[p], 8, REF.SKIP, REF.UNK)
        assert (int(c[p]), st[p].tolist(), ln[p].tolist()) == (cost, start, length)
    for skip, unk in ((0, 0), (1, 65535), (1 << 20, 3)):      # the limits of the two parameters
        rc, c, st, ln = host(reads[3:4], 8, skip, unk)
        assert rc == 0 and (int(c[0]), st[0].tolist(), ln[0].tolist()) == REF.solve(*reads[3], 8, skip, unk)


def test_refusals():
    L = _lib.lib()
    q, l = REF.case(50, 20, 4, "noisy")[:2]
    for band, skip, unk in ((0, 1, 1), (1025, 1, 1), (4, -1, 1), (4, (1 << 20) + 1, 1), (4, 1, -1), (4, 1, 65536)):
        rc, c, st, ln = host([(q, l)], band, skip, unk)
        assert rc == -1 and c[0] == 77 and set(st[0].tolist()) == {77}
    assert L.s2s_resquiggle_scratch_bytes(100, 50, 0) == -1 and L.s2s_resquiggle_scratch_bytes(100, 50, 1025) == -1
    # the formula and its bound: n * ceil((2 band + 1) / 64) * 16 <= n * (ceil((2 band + 1) / 64) + 1) * 16
    for n, K, band in ((100, 50, 1), (100, 50, 31), (100, 50, 32), (50000, 5000, 512), (7, 14, 1024)):
        got = L.s2s_resquiggle_scratch_bytes(n, K, band)
        assert got == n * -(-(2 * band + 1) // 64) * 16 <= n * (-(-(2 * band + 1) // 64) + 1) * 16
    assert L.s2s_resquiggle_scratch_bytes(50000, 5000, 512) == 13_600_000
    for n, K in ((0, 5), (5, 0), (3, 7), ((1 << 22) + 1, 5)):
        assert L.s2s_resquiggle_scratch_bytes(n, K, 8) == 0
    # a member longer than the limit: the host twin sees the lengths
    big = np.zeros((1 << 22) + 1, np.int16)
    assert host([(big, l)], 4)[0] == -1
    with pytest.raises(ValueError):
        RSQ.resquiggle([q], [l], band=0, cpu=True)
    with pytest.raises(ValueError):
        RSQ.resquiggle([q], [l], band=4, cpu=True, trace_memory=16)
    with pytest.raises(ValueError):
        RSQ.resquiggle([q], [l, l], band=4, cpu=True)


def test_python_entry_and_event_sums():
    shapes = ((300, 40, 3), (200, 260, 16), (65, 9, 1), (3, 7, 4))
    reads = [REF.case(n, K, 16, "noisy")[:2] for n, K, _ in shapes]
    cost, start, length = RSQ.resquiggle([r[0] for r in reads], [r[1] for r in reads], 16, REF.SKIP, REF.UNK, cpu=True,
                                         trace_memory=300 * 16 + 16)         # a budget that splits the batch
    for p, (q, l) in enumerate(reads):
        assert (int(cost[p]), start[p].tolist(), length[p].tolist()) == REF.solve(q, l, 16, REF.SKIP, REF.UNK)
    raw = [np.random.default_rng(p).integers(-32768, 32768, len(r[0])).astype(np.int16) for p, r in enumerate(reads)]
    start[0] = start[0].copy()
    length[0] = length[0].copy()
    start[0][3], length[0][3] = 290, 30_000                 # an interval outside the record counts as empty
    S, Q = RSQ.event_sums(raw, start, length, cpu=True)
    for p, x in enumerate(raw):
        x = x.astype(np.int64)
        for j, (s, n) in enumerate(zip(start[p], length[p])):
            ok = s >= 0 and n > 0 and s + n <= len(x)
            assert S[p][j] == (x[s:s + n].sum() if ok else 0) and Q[p][j] == ((x[s:s + n] ** 2).sum() if ok else 0)


# ------------------------------------------------------------------ every dealing of chunks to waves, both band edges
def test_bands_by_chunks_cover_every_dealing_of_chunks_to_waves():
    """The restatement of s2s_rsq_chunks / s2s_rsq_waves (the header's comment, no C): the 65 listed bands produce every (chunks, chunks
    per wave, waves) that the bands 1 .. 1024 produce, the 16-wave workgroups at one and at two chunks per wave among them."""
    R = REF.BANDS_BY_CHUNKS
    assert R == sorted(set(R)) and len(R) == 65 and R[:4] == [1, 31, 32, 63] and R[-3:] == [992, 1023, 1024]
    deal = lambda band: (REF.chunks(band), REF.per_wave(band), REF.waves(band))      # noqa: E731
    every = {deal(band) for band in range(1, 1025)}
    assert {deal(band) for band in R} == every and len(every) == 33
    assert {(16, 1, 16), (32, 2, 16), (33, 3, 11), (17, 2, 9), (4, 1, 4)} <= every
    assert sorted({d[0] for d in every}) == list(range(1, 34))                       # every chunk count 1 .. 33
    assert [band for band in range(1, 1025) if deal(band)[2] == 16] == list(range(480, 512)) + list(range(960, 1024))
    for c in range(1, 33):                           # the largest band of a count has the tightest ring: 64 c == 2 R + 2
        assert 64 * REF.chunks(32 * c - 1) == 2 * (32 * c - 1) + 2 and REF.chunks(32 * c) == c + 1
    L = _lib.lib()                                   # what the library states of the layout: 16 bytes per chunk and sample
    assert [L.s2s_resquiggle_scratch_bytes(10, 5, band) for band in R] == [10 * 16 * REF.chunks(band) for band in R]


@pytest.mark.parametrize("R", REF.BANDS_BY_CHUNKS)
def test_host_twin_at_the_bands_of_every_chunk_count(R):
    """The shapes of REF.band_shapes in their kinds: the invariants of a solved read at every band, the planted path exactly, `unreached`
    at K = 2 n, and the full-matrix restatement up to three chunks (measured: up to 2 s for a band of three chunks, and more for
    each band beyond)."""
    for n, K, kind in REF.band_shapes(R):
        q, l, plant = REF.case(n, K, R, kind)
        rc, c, st, ln = host([(q, l)], R)
        if K == 2 * n:                               # 2 n columns in n rows: no path, whatever the band
            assert rc == 0 and int(c[0]) == REF.UNREACHED and set(st[0].tolist()) == {-1} and set(ln[0].tolist()) == {0}
            assert REF.chunks(R) > 3 or REF.solve(q, l, R, REF.SKIP, REF.UNK)[0] == REF.UNREACHED
            continue
        assert rc == 0 and int(c[0]) >= 0
        REF.check_invariants(q, l, R, REF.SKIP, REF.UNK, int(c[0]), st[0], ln[0])
        if kind == "planted":
            assert plant is not None and int(c[0]) == 0 and (st[0] == plant[0]).all() and (ln[0] == plant[1]).all()
        if K > n:
            assert (ln[0] == 0).sum() >= K - n       # K = 2 n - 1: all but one column in two is skipped
        if kind == "zeros":
            assert K == 2 * n - 1 and int(c[0]) == (n - 1) * REF.SKIP      # every row but the first skips, and nothing else costs
        if REF.chunks(R) <= 3:
            assert (int(c[0]), st[0].tolist(), ln[0].tolist()) == REF.solve(q, l, R, REF.SKIP, REF.UNK)


@pytest.mark.parametrize("n,K,R", REF.PRESSED)
def test_pressed_path_runs_along_both_edges_of_the_band(n, K, R):
    q, l = REF.pressed(n, K, R)
    rc, c, st, ln = host([(q, l)], R)
    assert rc == 0 and int(c[0]) >= 0
    REF.check_invariants(q, l, R, REF.SKIP, REF.UNK, int(c[0]), st[0], ln[0])
    assert REF.edge_contact(n, K, R, st[0], ln[0]) == (True, True)      # a condition of the case: a shape without it is not listed
    if (n, K, R) in REF.PRESSED_SMALL:
        assert (int(c[0]), st[0].tolist(), ln[0].tolist()) == REF.solve(q, l, R, REF.SKIP, REF.UNK)


def test_pressed_needs_a_band_narrower_than_a_third_of_the_kmers():
    """Where K < 3 R or so the band holds the lag of a third of the samples and no edge is touched: why PRESSED has K >= 4 R."""
    for n, K, R in ((129, 64, 31), (1000, 200, 96), (3000, 2900, 1024)):
        rc, c, st, ln = host([REF.pressed(n, K, R)], R)
        assert rc == 0 and REF.edge_contact(n, K, R, st[0], ln[0]) == (False, False)
    assert all(K >= 4 * R for _, K, R in REF.PRESSED)


def event_sum_case():
    """-> (records, start, length, want): reads of 127, 128, 129, 1,025 and 0 k-mers and one of 131 whose samples are all -32768 -- past
    one stride of 128 k-mers of s2s_event_sums_kernel, with odd offsets of the samples and of the k-mers.  The lengths cycle through
    1, 15, 16, 17, 31, 32, 33 and 4,097 (one stride of a quarter wave, one less, one more, two, many); some intervals at indices >= 128
    are skipped k-mers or lie outside their record.  want: (S, Q) per k-mer in numpy int64, (0, 0) for what counts as empty."""
    rng = np.random.default_rng(12)
    cycle = np.array([1, 15, 16, 17, 31, 32, 33, 4097], np.int32)
    recs, start, length = [], [], []
    for p, K in enumerate((127, 128, 129, 1025, 0)):
        ln = cycle[(np.arange(K) + p) % 8]
        st = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int32) if K else np.zeros(0, np.int32)
        n = int(ln.sum()) + 1 + p
        recs.append(rng.integers(-32768, 32768, n).astype(np.int16))
        st, ln = st.copy(), ln.copy()
        if K > 128:
            st[128], ln[128] = -1, 0                # a skipped k-mer in the second trip
        if K > 200:
            st[130], ln[130] = n - 5, 6             # one sample past the record's end
            st[200], ln[200] = -3, 4                # begins in front of it
            st[640], ln[640] = 7, 0
            st[1024], ln[1024] = n - 4097, 4097     # the record's last samples, exactly
        start.append(st)
        length.append(ln)
    assert (np.cumsum([len(x) for x in recs]) % 2 == 1).sum() >= 2      # reads that begin at an odd offset of the pool
    recs.append(np.full(40_001, -32768, np.int16))   # |S| = 30,000 * 2^15, Q = 30,000 * 2^30 > 2^44
    start.append(np.concatenate([np.arange(129) * 50, [6450, 36_450]]).astype(np.int32))
    length.append(np.concatenate([np.full(129, 50), [30_000, 3_551]]).astype(np.int32))
    want = []
    for x, st, ln in zip(recs, start, length):
        x = x.astype(np.int64)
        ok = (st >= 0) & (ln > 0) & (st.astype(np.int64) + ln <= len(x))
        want.append([(int(x[s:s + n].sum()), int((x[s:s + n] ** 2).sum())) if o else (0, 0) for s, n, o in zip(st.tolist(), ln.tolist(), ok)])
    assert want[5][129] == (-32768 * 30_000, 30_000 << 30) and want[3][130] == (0, 0) and want[3][1024] != (0, 0)
    return recs, start, length, want


def test_event_sums_host_past_128_kmers_against_numpy():
    recs, start, length, want = event_sum_case()
    S, Q = RSQ.event_sums(recs, start, length, cpu=True)
    assert [list(zip(s.tolist(), q.tolist())) for s, q in zip(S, Q)] == want


# ------------------------------------------------------------------ the model reader
K3 = 3


def model_counts(adc_levels):
    """counts [4^k + 1, 5] of a model whose k-mer c has one event of mean adc_levels[c] ADC counts (NaN: no event)."""
    counts = np.zeros((4 ** K3 + 1, kmer_model.FIELDS), np.int64)
    for c, a in enumerate(adc_levels):
        if not math.isnan(a):
            counts[c] = (1, 256 * int(a), (256 * int(a)) ** 2, 0, 0)
    return counts


def test_model_reader(tmp_path):
    rng = np.random.default_rng(5)
    adc = rng.permutation(64).astype(float) * 17 + 200
    adc[[5, 40]] = np.nan
    text = bytes(kmer_model.format_model(model_counts(adc), K3, 8192.0, 1536.0, 10.0))
    assert text.startswith(b"#k\t3\n#alphabet\tnucleotide\nkmer\tlevel_mean")
    (tmp_path / "m.model").write_bytes(text)
    k, levels = RSQ.read_model(str(tmp_path / "m.model"))
    assert k == 3 and levels.shape == (64,) and np.isnan(levels[[5, 40]]).all()
    want = (adc + 10.0) * 1536.0 / 8192.0
    ok = ~np.isnan(adc)
    assert np.abs(levels[ok] - want[ok]).max() <= 0.5e-4    # the file prints %.4f
    # a plain nanopolish-style table, columns in another order, no comment lines
    (tmp_path / "n.model").write_text("level_stdv\tkmer\tlevel_mean\n1.0\tAC\t80.5\n2.0\tTT\t101.25\n")
    k, levels = RSQ.read_model(str(tmp_path / "n.model"))
    assert k == 2 and levels[1] == 80.5 and levels[15] == 101.25 and np.isnan(levels).sum() == 14
    ints, known = RSQ.level_ints(np.array([80.5, np.nan, 1e9, 0.0078125, 0.0234375]))
    assert ints.tolist() == [5152, 0, 32767, 0, 2] and known.tolist() == [True, False, True, True, True]      # halves go to even
    assert RSQ.kmer_codes("ACGTNAC", 2).tolist() == [1, 6, 11, -1, -1, 1]
    (tmp_path / "bad.model").write_text("kmer\tmean\nAC\t1\n")
    with pytest.raises(Exception):
        RSQ.read_model(str(tmp_path / "bad.model"))


# ------------------------------------------------------------------ the command
def planted_read(rng, n_bases, adc):
    """-> (sequence, stored int16 samples, start [K], len [K]): every k-mer's samples are its ADC level, dwell drawn from 3..15.  The
    sequence is grown base by base so that neighbouring k-mers lie at least 300 ADC counts (over one MAD of such a read) apart: the
    samples are normalised by their own, dwell-weighted median / MAD and the levels by theirs, which differ by up to a fifth, and a
    boundary must not move for that."""
    while True:
        seq = "".join(rng.choice(list("ACGT"), K3))
        while len(seq) < n_bases:
            last = adc[RSQ.kmer_codes(seq[-K3:], K3)[0]]
            nxt = [c for c in "ACGT" if abs(adc[RSQ.kmer_codes(seq[-K3 + 1:] + c, K3)[0]] - last) >= 300]     # (NaN compares False)
            if not nxt:
                break
            seq += str(rng.choice(nxt))
        if len(seq) == n_bases and not np.isnan(adc[RSQ.kmer_codes(seq, K3)]).any():
            break
    codes = RSQ.kmer_codes(seq, K3)
    dwell = rng.integers(3, 16, len(codes))
    start = np.concatenate([[0], np.cumsum(dwell)[:-1]])
    return seq, np.repeat(adc[codes], dwell).astype(np.int16), start, dwell


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("resquiggle")
    rng = np.random.default_rng(11)
    adc = rng.permutation(64).astype(float) * 23 + 150            # 64 distinct levels, 23 ADC counts apart
    adc[7] = np.nan
    reads = {f"r{i}": planted_read(rng, nb, adc) for i, nb in enumerate((40, 75, 33, 60))}
    ids = list(reads) + ["orphan"]
    sigs = [reads[i][1] for i in reads] + [np.arange(50, dtype=np.int16)]
    blow5 = write_file(d / "s.blow5", ids, sigs, record_compression="zlib")
    slow5 = write_file(d / "s.slow5", ids, sigs)
    rec = next(iter(SB.open_records(blow5)))
    cal = (float(rec["digitisation"]), float(rec["offset"]), float(rec["range"]))
    (d / "m.model").write_bytes(bytes(kmer_model.format_model(model_counts(adc), K3, cal[0], cal[2], cal[1])))
    (d / "r.fasta").write_text("".join(f">{i} comment\n{reads[i][0][:30]}\n{reads[i][0][30:]}\n" for i in reads))
    (d / "r.fastq").write_text("".join(f"@{i}\n{reads[i][0]}\n+\n{'I' * len(reads[i][0])}\n" for i in reads))
    return d, blow5, slow5, reads, cal, adc


def run(*args):
    r = CliRunner().invoke(cli.main, ["resquiggle", *[str(a) for a in args]], catch_exceptions=False)
    return r


def planted_rows(reads, cal, samples=False, rna=False, shift=None):
    dig, off, rng_ = cal
    out = []
    for rid, (seq, sig, start, dwell) in reads.items():
        K = len(start)
        for j in range(K):
            pos, jj = j, (K - 1 - j if rna else j)           # jj: the event in stored-signal order
            s = int(start[jj]) + (shift or {}).get(rid, 0)
            x = float(sig[start[jj]])
            row = f"{rid}\t{pos}\t{seq[pos:pos + K3]}\t{s}\t{s + int(dwell[jj])}\t{'%.4f' % ((x + off) * rng_ / dig)}\t0.0000"
            if samples:
                row += "\t" + ",".join(["%.3f" % ((x + off) * rng_ / dig)] * int(dwell[jj]))
            out.append(row)
    return out


def test_command_cpu_planted_rows_exactly(files):
    d, blow5, slow5, reads, cal, adc = files
    r = run(d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "a.tsv", "--cpu", "--json", "--summary", d / "a.sum.tsv")
    assert r.exit_code == 0, r.output
    s = json.loads(r.output.strip().splitlines()[-1])
    text = (d / "a.tsv").read_text().splitlines()
    assert text[0].split("\t") == list(RSQ.EVENT_COLUMNS)
    assert text[1:] == planted_rows(reads, cal)
    n_events = sum(len(v[2]) for v in reads.values())
    assert (s["records"], s["solved"], s["no_sequence"], s["unreached"], s["refused"], s["no_known_level"]) == (5, 4, 1, 0, 0, 0)
    assert s["events"] == n_events and s["skipped_kmers"] == 0 and s["k"] == 3
    assert 0 <= s["mean_cost_per_sample"] < 0.3     # what the two normalisations differ by: up to a fifth (planted_read) of levels within 1.5 MAD
    rows = parse_events((d / "a.tsv").read_bytes(), False)                       # the reader of predict --events
    assert len(rows) == n_events
    table = CMP.read_events(str(d / "a.tsv"))                                   # ... and of compare --events-a
    assert list(table) == list(reads) and [len(v) for v in table.values()] == [len(v[2]) for v in reads.values()]
    summary = [l.split("\t") for l in (d / "a.sum.tsv").read_text().splitlines()]
    assert summary[0] == list(RSQ.SUMMARY_COLUMNS) and [l[3] for l in summary[1:]] == ["solved"] * 4 + ["no_sequence"]
    # SLOW5, FASTQ, --samples, a batch per read: the same rows
    r = run(d / "r.fastq", slow5, "--kmer-model", d / "m.model", "-o", d / "b.tsv", "--cpu", "--samples", "--max-samples", 1)
    assert r.exit_code == 0, r.output
    text_b = (d / "b.tsv").read_text().splitlines()
    assert text_b[0].split("\t") == list(RSQ.EVENT_COLUMNS) + ["samples"] and text_b[1:] == planted_rows(reads, cal, samples=True)
    assert len(parse_events((d / "b.tsv").read_bytes(), True)) == n_events


def test_command_cpu_equals_the_restatement_on_noisy_reads(files):
    """Noise on the samples and a k-mer without a level: the rows are those of the Python restatement on the restated normalisation."""
    d, blow5, slow5, reads, cal, adc = files
    rng = np.random.default_rng(3)
    seqs = {f"n{i}": "".join(rng.choice(list("ACGT"), nb)) for i, nb in enumerate((50, 33))}
    seqs["n1"] = seqs["n1"][:10] + "NAC" + seqs["n1"][13:]
    full = np.where(np.isnan(adc), 0, adc)
    sigs = {}
    for rid, seq in seqs.items():
        codes = np.maximum(RSQ.kmer_codes(seq, K3), 0)
        sigs[rid] = np.repeat(full[codes], rng.integers(1, 12, len(codes))).astype(np.int16)
        sigs[rid] = (sigs[rid] + rng.integers(-30, 31, len(sigs[rid]))).astype(np.int16)
    path = write_file(d / "n.blow5", list(seqs), list(sigs.values()))
    (d / "n.fasta").write_text("".join(f">{i}\n{s}\n" for i, s in seqs.items()))
    r = run(d / "n.fasta", path, "--kmer-model", d / "m.model", "-o", d / "n.tsv", "--cpu", "--band", 9, "--skip-penalty", 70,
            "--unknown-cost", 50)
    assert r.exit_code == 0, r.output
    k, levels = RSQ.read_model(str(d / "m.model"))
    table, has = RSQ.level_ints(levels)
    dig, off, rng_ = cal
    want, unknown_seen = [], False
    for rid, seq in seqs.items():
        codes = RSQ.kmer_codes(RSQ.clean_sequence(seq), K3)
        known = (codes >= 0) & has[np.maximum(codes, 0)]
        unknown_seen |= not known.all()
        lev = table[np.maximum(codes, 0)]
        q = ref_normalise(sigs[rid], *ref_median_mad(sigs[rid]))
        l = np.where(known, ref_normalise(lev, *ref_median_mad(lev[known])), REF.UNKNOWN)
        cost, start, length = REF.solve(q, l, 9, 70, 50)
        assert cost >= 0
        x = sigs[rid].astype(np.int64)
        for j, (s, n) in enumerate(zip(start, length)):
            if n:
                S, Q = int(x[s:s + n].sum()), int((x[s:s + n] ** 2).sum())
                want.append(f"{rid}\t{j}\t{seq[j:j + K3]}\t{s}\t{s + n}\t{'%.4f' % ((S / n + off) * rng_ / dig)}\t"
                            f"{'%.4f' % (math.sqrt(max(n * Q - S * S, 0)) / n * rng_ / dig)}")
    assert unknown_seen and (d / "n.tsv").read_text().splitlines()[1:] == want


def test_command_cpu_rna_and_intervals(files):
    d, blow5, slow5, reads, cal, adc = files
    # --rna: the stored signal is the forward signal reversed
    ids = list(reads)
    rev = write_file(d / "rev.blow5", ids, [reads[i][1][::-1].copy() for i in ids])
    r = run(d / "r.fasta", rev, "--kmer-model", d / "m.model", "-o", d / "rna.tsv", "--cpu", "--rna")
    assert r.exit_code == 0, r.output
    mirrored = {i: (seq, sig[::-1], (len(sig) - start - dwell)[::-1], dwell[::-1]) for i, (seq, sig, start, dwell) in reads.items()}
    got = (d / "rna.tsv").read_text().splitlines()[1:]
    assert got == planted_rows(mirrored, cal, rna=True)
    first = [l.split("\t") for l in got if l.startswith("r0\t")]
    assert [int(l[1]) for l in first] == list(range(len(first))) and all(int(a[3]) > int(b[3]) for a, b in zip(first, first[1:]))
    # --intervals: records that carry samples in front and behind; rows in the record's own coordinates
    pad = {"r0": (13, 5), "r1": (0, 40), "r3": (21, 0)}
    sigs = [np.concatenate([np.full(pad.get(i, (0, 0))[0], 900, np.int16), reads[i][1], np.full(pad.get(i, (0, 0))[1], -900, np.int16)])
            for i in ids]
    padded = write_file(d / "pad.slow5", ids, sigs)
    (d / "iv.tsv").write_text("read_id\tn_a\tb_end\tb_start\n" +
                              "".join(f"{i}\t0\t{p[0] + len(reads[i][1])}\t{p[0]}\n" for i, p in pad.items()))
    r = run(d / "r.fasta", padded, "--kmer-model", d / "m.model", "-o", d / "iv.out.tsv", "--cpu", "--intervals", d / "iv.tsv")
    assert r.exit_code == 0, r.output
    assert (d / "iv.out.tsv").read_text().splitlines()[1:] == planted_rows(reads, cal, shift={i: p[0] for i, p in pad.items()})


def test_command_refusals(files):
    d, blow5, slow5, reads, cal, adc = files
    for extra in (("--band", 0), ("--band", 1025), ("--skip-penalty", -1), ("--unknown-cost", 65536), ("--max-samples", 0),
                  ("--trace-memory", 0)):
        r = CliRunner().invoke(cli.main, ["resquiggle", str(d / "r.fasta"), blow5, "--kmer-model", str(d / "m.model"), "-o",
                                          str(d / "x.tsv"), "--cpu", *[str(e) for e in extra]])
        assert r.exit_code != 0 and extra[0] in r.output, (extra, r.output)
    r = CliRunner().invoke(cli.main, ["resquiggle", str(d / "r.fasta"), str(d / "x.pod5"), "--kmer-model", str(d / "m.model"), "-o",
                                      str(d / "x.tsv"), "--cpu"])
    assert r.exit_code != 0 and "POD5" in r.output
    # a read whose walk back needs more than --trace-memory is refused by its id; the others are solved
    need = sorted(RSQ.scratch_bytes(len(v[1]), len(v[2]), 31) for v in reads.values())
    assert need[-1] == 16 * len(reads["r1"][1]) > need[-2]
    r = run(d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "t.tsv", "--cpu", "--json", "--band", 31, "--trace-memory", need[-2])
    s = json.loads(r.output.strip().splitlines()[-1])
    assert r.exit_code == 0 and s["refused"] == 1 and s["solved"] == 3
    assert not any(l.startswith("r1\t") for l in (d / "t.tsv").read_text().splitlines())
