"""`compare` without a GPU: the host entries (s2s_signal_median_mad_host, s2s_signal_normalise_host, s2s_dtw_banded_host) against the
restatement of their definitions (tests/_dtw_ref.py) on the shapes the GPU test uses, the properties of the band (symmetry,
monotone in R, reachable at R = 1, unbanded beyond max(n, m)), the error codes, and `compare --cpu` end to end on files written
with BLOW5Writer.  Every comparison is between integers or bytes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import signal_io
from seq2squiggle_amd import utils as U
from _dtw_ref import INF, SCALE, ref_dtw, ref_dtw_full, ref_dtw_rows, ref_median_mad, ref_normalise
from conftest import ROOT

MAX_BAND = CMP.max_band()
LIMIT = 1 << 22


def rnd(rng, n, lo=-32768, hi=32768):
    return rng.integers(lo, hi, n).astype(np.int16)


def median_records():
    """The records of the median / MAD and normalise checks (also tests/test_gpu_compare.py)."""
    rng = np.random.default_rng(11)
    recs = [rnd(rng, n) for n in (0, 1, 2, 3, 255, 256, 257, 65537)]
    recs += [np.full(n, v, np.int16) for n, v in ((1, -32768), (2, 32767), (300, 417), (257, 0))]            # all equal: MAD 0, divisor 1
    recs += [rng.choice(np.array([-32768, 32767], np.int16), n) for n in (2, 3, 256, 1001)]                   # |x - med| = 65,535
    recs += [np.array([-32768, 32767], np.int16), np.array([32767, -32768, -32768], np.int16)]
    recs += [rnd(rng, n, 0x1200, 0x1300) for n in (5, 256, 1000)]                                             # one high byte: the second pass decides
    recs += [rnd(rng, n, -0x0100, 0) for n in (7, 513)]                                                       # high byte 0x7f of x + 32768
    recs += [rnd(rng, n, -32768, -1) for n in (4, 255, 2000)]                                                 # negative only
    recs += [rnd(rng, n, -600, 900) for n in (64, 1000, 4097)]                                                # signal-like
    return recs


def mixed_batch(seed=5, count=257):
    """`count` records of mixed lengths with empty ones first, in the middle and last."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 400, count)
    lens[[0, 1, count // 2, count - 1]] = 0
    lens[7] = 3000
    return [rnd(rng, int(n), -2000, 2000) for n in lens]


def normalise_cases():
    """(record, med, mad): at the clamp, at exact half-way quotients and with negative numerators."""
    x = np.arange(-32768, 32768, 1, dtype=np.int64).astype(np.int16)
    cases = [(x, 0, 1), (x, -32768, 1), (x, 32767, 1), (x, 0, 0), (x, 5, 64), (x, -7, 128), (x, 100, 65535), (x, -32768, 65535),
             (x, 32767, 65535), (x, 12, 3), (x, -12, 7), (x, 0, 256), (x, 1, 2)]
    # 64 (x - med) / d is an integer + 1/2 exactly when 128 (x - med) is an odd multiple of d: d = 256 with x - med = +-2, +-6, ...;
    # d = 128 with x - med = +-1, +-3, ...
    cases.append((np.array([-7, -6, -5, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7], np.int16), 0, 256))
    cases.append((np.array([-3, -1, 1, 3, 101, 99], np.int16), 100, 128))
    return cases


DTW_SHAPES = ([(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 2, 1)] +
              [(n, n, R) for n in (63, 64, 65, 127, 129) for R in (1, 31, 32, 33, 200)] +
              [(n, m, R) for n, m in ((300, 97), (97, 300)) for R in (1, 2, 7)] +
              [(1000, 1000, 3)])


def dtw_pair(n, m, seed=None, lo=-2000, hi=2000):
    rng = np.random.default_rng(1000 * n + m if seed is None else seed)
    return rnd(rng, n, lo, hi), rnd(rng, m, lo, hi)


def mixed_pairs(count=257, seed=9):
    """Pairs of mixed lengths (1 .. 200), some with an empty member (cost -1)."""
    rng = np.random.default_rng(seed)
    na, nb = rng.integers(1, 200, count), rng.integers(1, 200, count)
    na[[0, 100, count - 1]] = 0
    nb[[1, 100, 156]] = 0
    return [rnd(rng, int(n), -3000, 3000) for n in na], [rnd(rng, int(n), -3000, 3000) for n in nb]


def host_dtw(a, b, R):
    return int(CMP.dtw_banded([a], [b], R, cpu=True)[0])


# ------------------------------------------------------------------ host entries against the restatement
def test_host_median_mad_equals_the_restatement():
    for recs in (median_records(), mixed_batch()):
        med, mad = CMP.median_mad(recs, cpu=True)
        assert med.dtype == np.int32 and mad.dtype == np.int32
        want = [ref_median_mad(r) for r in recs]
        assert [(int(a), int(b)) for a, b in zip(med, mad)] == want
    assert ref_median_mad(np.array([-32768, 32767], np.int16)) == (-32768, 0)
    assert ref_median_mad(np.array([32767, -32768, -32768], np.int16)) == (-32768, 0)
    assert ref_median_mad(np.array([-32768, 32767, 32767, -32768, 32767], np.int16)) == (32767, 0)
    assert ref_median_mad(np.array([-32768, 32767, 32767, -32768], np.int16)) == (-32768, 0)
    assert max(m for _, m in (ref_median_mad(r) for r in median_records())) <= 65535


def test_two_valued_records_put_65535_among_the_keys():
    """A record of -32768 and 32767 only: |x - med| = 65,535 is a key of the second selection (it does not fit int16) -- the MAD
    itself stays 0, since the median is the majority value and the rank (n - 1) // 2 lies inside the majority."""
    recs = [np.array([32767] * 3 + [-32768] * 2, np.int16), np.array([-32768] * 3 + [32767] * 3, np.int16),
            np.array([-32768, 32767], np.int16), np.array([32767, -32768, 0], np.int16)]
    med, mad = CMP.median_mad(recs, cpu=True)
    assert [(int(a), int(b)) for a, b in zip(med, mad)] == [ref_median_mad(r) for r in recs] == [(32767, 0), (-32768, 0), (-32768, 0), (0, 32767)]
    assert all(65535 in np.abs(r.astype(np.int64) - int(m)) for r, m in zip(recs[:3], med[:3]))


def test_host_normalise_equals_the_restatement():
    recs = median_records()
    med, mad = CMP.median_mad(recs, cpu=True)
    got = CMP.normalise(recs, cpu=True)
    for r, q, m, d in zip(recs, got, med, mad):
        assert q.dtype == np.int16 and np.array_equal(q, ref_normalise(r, m, d))
    for x, m, d in normalise_cases():
        (q,) = CMP.normalise([x], med=[m], mad=[d], cpu=True)
        want = ref_normalise(x, m, d)
        assert np.array_equal(q, want), (m, d)
    # spot values: round half up, floor for negatives, the clamp
    q = ref_normalise(np.array([1, -1, 3, -3, 2, -2, 6, -6, 0], np.int16), 0, 256)       # x / 4: 0.5 -> 1, -0.5 -> 0, 1.5 -> 2, -1.5 -> -1
    assert q.tolist() == [0, 0, 1, -1, 1, 0, 2, -1, 0]
    assert ref_normalise(np.array([32767, -32768], np.int16), 0, 1).tolist() == [32767, -32767]
    assert SCALE == CMP.SCALE == 64


@pytest.mark.parametrize("n,m,R", DTW_SHAPES)
def test_host_dtw_equals_the_restatement(n, m, R):
    a, b = dtw_pair(n, m)
    want = ref_dtw(a, b, R)
    assert 0 <= want < INF
    assert host_dtw(a, b, R) == want
    assert ref_dtw_rows(a, b, R) == want
    # constant signals: cost 0, ties everywhere
    assert host_dtw(np.full(n, 7, np.int16), np.full(m, 7, np.int16), R) == 0 == ref_dtw(np.full(n, 7, np.int16), np.full(m, 7, np.int16), R)


def test_host_dtw_large_shapes():
    a, b = dtw_pair(3000, 3000)
    assert host_dtw(a, b, MAX_BAND) == ref_dtw_rows(a, b, MAX_BAND)
    a, b = np.full(70000, -32767, np.int16), np.full(70000, 32767, np.int16)
    want = 70000 * 65534
    assert want > 1 << 32
    assert host_dtw(a, b, 1) == want == ref_dtw_rows(a, b, 1)


def test_host_dtw_batches():
    al, bl = mixed_pairs()
    want = [ref_dtw(a, b, 5) for a, b in zip(al, bl)]
    assert sorted(set(w for w in want if w < 0)) == [-1] and sum(w < 0 for w in want) == 5
    for P in (1, 2, 257):
        assert CMP.dtw_banded(al[:P], bl[:P], 5, cpu=True).tolist() == want[:P]
    two = np.concatenate([CMP.dtw_banded(al[:100], bl[:100], 5, cpu=True), CMP.dtw_banded(al[100:], bl[100:], 5, cpu=True)])
    assert two.tolist() == want


# ------------------------------------------------------------------ properties of the definition
def test_band_properties():
    rng = np.random.default_rng(3)
    for n, m in ((1, 1), (1, 5), (5, 1), (2, 2), (300, 97), (97, 300), (1000, 3)):
        a, b = rnd(rng, n, -500, 500), rnd(rng, m, -500, 500)
        r1 = ref_dtw(a, b, 1)
        assert 0 <= r1 < INF and host_dtw(a, b, 1) == r1                      # reachable at R = 1
    for n, m in ((1, 1), (3, 17), (17, 3), (40, 40), (60, 25), (25, 61)):
        a, b = rnd(rng, n, -500, 500), rnd(rng, m, -500, 500)
        full = ref_dtw_full(a, b)
        for R in (max(n, m), max(n, m) + 3):
            assert ref_dtw(a, b, R) == full
        prev = None
        for R in (1, 2, 3, 5, 8, 13, 21, 34, 61):
            c = ref_dtw(a, b, R)
            assert c == ref_dtw(b, a, R) == host_dtw(a, b, R) == host_dtw(b, a, R)      # symmetric
            assert prev is None or c <= prev                                              # a wider band never costs more
            assert c >= full
            prev = c


# ------------------------------------------------------------------ error codes
def test_error_codes():
    L = _lib.lib()
    a = np.zeros(8, np.int16)
    offs = np.array([0, 4, 8], np.int64)
    cost = np.zeros(2, np.int64)
    med, mad = np.zeros(2, np.int32), np.zeros(2, np.int32)
    out = np.zeros(8, np.int16)
    p = lambda x: x.ctypes.data                                                            # noqa: E731

    def dtw(P, band, ao=offs, bo=offs):
        return L.s2s_dtw_banded_host(p(a), p(ao), p(a), p(bo), P, band, p(cost), 2)
    assert dtw(2, 1) == 0 and dtw(2, MAX_BAND) == 0 and dtw(0, 1) == 0
    assert dtw(2, 0) == -1 and dtw(2, MAX_BAND + 1) == -1 and dtw(2, -5) == -1
    assert dtw(-1, 1) == -1
    long_offs = np.array([0, LIMIT + 1, LIMIT + 2], np.int64)                              # (refused before a sample is read)
    assert dtw(2, 1, ao=long_offs) == -1 and dtw(2, 1, bo=long_offs) == -1
    assert dtw(2, 1, ao=np.array([0, 4, 2], np.int64)) == -1                                # offsets that decrease
    assert L.s2s_dtw_banded_host(p(a), p(offs), p(a), p(offs), 2, 1, p(cost), 0) == -1      # no threads
    assert L.s2s_signal_median_mad_host(p(a), p(offs), 2, p(med), p(mad), 2) == 0
    assert L.s2s_signal_median_mad_host(p(a), p(offs), -1, p(med), p(mad), 2) == -1
    assert L.s2s_signal_median_mad_host(p(a), p(long_offs), 2, p(med), p(mad), 2) == -1
    assert L.s2s_signal_normalise_host(p(a), p(offs), 2, p(med), p(mad), 64, p(out), 2) == 0
    for scale in (0, -1, 8193):
        assert L.s2s_signal_normalise_host(p(a), p(offs), 2, p(med), p(mad), scale, p(out), 2) == -1
    assert L.s2s_signal_normalise_host(p(a), p(offs), -1, p(med), p(mad), 64, p(out), 2) == -1
    # the device entries refuse the same arguments without a device: nothing is launched, no HIP call is made
    vp = C.c_void_p
    assert L.s2s_dtw_banded(0, None, vp(8), vp(8), vp(8), vp(8), 1, 0, vp(8)) == -1
    assert L.s2s_dtw_banded(0, None, vp(8), vp(8), vp(8), vp(8), 1, MAX_BAND + 1, vp(8)) == -1
    assert L.s2s_dtw_banded(0, None, vp(8), vp(8), vp(8), vp(8), -1, 1, vp(8)) == -1
    assert L.s2s_signal_median_mad(0, None, vp(8), vp(8), -1, vp(8), vp(8)) == -1
    assert L.s2s_signal_normalise(0, None, vp(8), vp(8), 1, vp(8), vp(8), 0, vp(8)) == -1
    assert b"band" in L.s2s_last_error(None) or b"scale" in L.s2s_last_error(None)
    assert MAX_BAND >= 1024
    hdr = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()
    assert f"#define S2S_DTW_MAX_BAND {MAX_BAND}\n" in hdr and "#define S2S_DTW_SCALE 64\n" in hdr
    with pytest.raises(ValueError):
        CMP.dtw_banded([a], [a], 0, cpu=True)
    with pytest.raises(ValueError):
        CMP.dtw_banded([a], [a], MAX_BAND + 1, cpu=True)


# ------------------------------------------------------------------ the command
def write_file(path, ids, sigs, **kw):
    w = signal_io.BLOW5Writer(str(path), U.get_profile("dna-r10-prom"), True, "dna-r10-prom", True, **kw)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in sigs])])
    w.save_dac(ids, np.concatenate(sigs).astype(np.int16), offs)
    return str(path)


def squiggles(seed, lens):
    rng = np.random.default_rng(seed)
    return [(400 + np.repeat(rng.integers(-150, 150, n // 8 + 1), 8)[:n] + rng.integers(-12, 13, n)).astype(np.int16) for n in lens]


def run_cli(*args):
    return subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "compare", *args], cwd=ROOT, capture_output=True, text=True)


def expected_rows(pairs, band, norm=True):
    rows = ["\t".join(CMP.COLUMNS)]
    for rid, a, b in pairs:
        (ma, da), (mb, db) = ref_median_mad(a), ref_median_mad(b)
        qa, qb = (ref_normalise(a, ma, da), ref_normalise(b, mb, db)) if norm else (a, b)
        c = ref_dtw(qa, qb, band)
        per = "%.6f" % (c / (len(a) + len(b)) / 64)
        rows.append(f"{rid}\t{len(a)}\t{len(b)}\t{ma}\t{da}\t{mb}\t{db}\t{band}\t{c}\t{per}")
    return "\n".join(rows) + "\n"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("compare")
    sa = squiggles(1, (120, 333, 64, 500))
    sb = squiggles(2, (140, 300, 90, 410))
    ids_a, ids_b = ["r0", "r1", "onlyA", "r3"], ["r3", "onlyB", "r1", "r0"]
    a = write_file(d / "a.blow5", ids_a, sa, record_compression="zlib")
    b = write_file(d / "b.blow5", ids_b, sb, record_compression="none", signal_compression="svb-zd")
    s = write_file(d / "s.slow5", ids_b, sb)
    return d, a, b, s, dict(zip(ids_a, sa)), dict(zip(ids_b, sb)), ids_a, ids_b


def test_compare_cpu_end_to_end(files):
    d, a, b, s, A, B, ids_a, ids_b = files
    by_id = [(i, A[i], B[i]) for i in ids_a if i in B]
    assert [p[0] for p in by_id] == ["r0", "r1", "r3"]
    for other in (b, s):
        out = str(d / "o.tsv")
        r = run_cli(a, other, "-o", out, "--band", "40", "--cpu", "--json")
        assert r.returncode == 0, r.stderr
        assert open(out).read() == expected_rows(by_id, 40)
        js = json.loads(r.stdout.strip().splitlines()[-1])
        assert (js["pairs"], js["unpaired_a"], js["unpaired_b"], js["records_a"], js["records_b"]) == (3, 1, 1, 4, 4)
        per = [float(l.split("\t")[-1]) for l in open(out).read().splitlines()[1:]]
        assert abs(js["mean_dtw_per_sample"] - np.mean(per)) < 1e-6 and abs(js["median_dtw_per_sample"] - np.median(per)) < 1e-6
    # by order, unnormalised, the log line instead of JSON; a sample budget that splits the pairs changes nothing
    out = str(d / "o2.tsv")
    r = run_cli(a, s, "-o", out, "--band", "25", "--cpu", "--by-order", "--normalise", "none", "--max-samples", "300")
    assert r.returncode == 0, r.stderr
    assert "4 pairs" in r.stdout and "unpaired: 0 of 4" in r.stdout
    assert open(out).read() == expected_rows([(ia, A[ia], B[ib]) for ia, ib in zip(ids_a, ids_b)], 25, norm=False)
    # by order with files of different lengths
    short = write_file(d / "short.blow5", ids_b[:2], [B[i] for i in ids_b[:2]])
    s_ = CMP.compare_files(a, short, str(d / "o3.tsv"), band=25, by_order=True, cpu=True)
    assert (s_["pairs"], s_["unpaired_a"], s_["unpaired_b"]) == (2, 2, 0)
    assert open(d / "o3.tsv").read() == expected_rows([(ids_a[k], A[ids_a[k]], B[ids_b[k]]) for k in range(2)], 25)


def test_compare_refuses_what_it_cannot_read(files):
    d, a, b, s, *_ = files
    r = run_cli(a, str(d / "x.pod5"), "-o", str(d / "e.tsv"), "--cpu")
    assert r.returncode == 2 and "POD5" in r.stderr and "x.pod5" in r.stderr and not os.path.exists(d / "e.tsv")
    r = run_cli(a, str(d / "x.fast5"), "-o", str(d / "e.tsv"), "--cpu")
    assert r.returncode == 2 and "x.fast5" in r.stderr
    data = open(a, "rb").read()
    cut = d / "cut.blow5"
    cut.write_bytes(data[:len(data) - 40])
    r = run_cli(a, str(cut), "-o", str(d / "e.tsv"), "--cpu")
    assert r.returncode == 1 and "cut.blow5" in r.stderr and "truncated" in r.stderr and "Traceback" not in r.stderr
    assert not os.path.exists(d / "e.tsv")
    alien = d / "alien.blow5"
    alien.write_bytes(b"not a signal file at all" * 10)
    r = run_cli(str(alien), a, "-o", str(d / "e.tsv"), "--cpu")
    assert r.returncode == 1 and "alien.blow5" in r.stderr and "Traceback" not in r.stderr
    # a record damaged in the middle (the end marker is there): still an error that names the file
    bad = bytearray(data)
    pos = len(data) // 2
    bad[pos:pos + 64] = b"\xff" * 64
    broken = d / "broken.blow5"
    broken.write_bytes(bytes(bad))
    r = run_cli(str(broken), a, "-o", str(d / "e2.tsv"), "--cpu")
    assert r.returncode == 1 and "broken.blow5" in r.stderr and "Traceback" not in r.stderr
    r = run_cli(a, str(d / "missing.blow5"), "-o", str(d / "e.tsv"), "--cpu")
    assert r.returncode == 1 and "missing.blow5" in r.stderr
    r = run_cli(a, b, "-o", str(d / "e.tsv"), "--cpu", "--band", "0")
    assert r.returncode == 2 and "--band" in r.stderr
