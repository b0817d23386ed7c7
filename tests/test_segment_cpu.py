"""`segment` on the host: s2s_segment_host (the definition the kernels must equal) against its restatement in plain Python integers
(tests/_segment_ref.py), bit for bit; the consequences the header states, on every case; the formatter and the command with --cpu."""
import ctypes
import json
import math

import numpy as np
import pytest
from click.testing import CliRunner

import _segment_ref as REF
from seq2squiggle_amd import _lib, cli
from seq2squiggle_amd import segment as SEG
from test_compare_cpu import squiggles, write_file

WINDOWS = ((1, 1), (3, 6), (7, 14), (32, 32), (1, 32))
T_DEFAULT = (501, 20736)                             # floor(256 * 1.4^2), 256 * 9^2
PRESET = 77


def host(records, w_s, w_l, T_s, T_l, threads=1, caps=None):
    """s2s_segment_host on raw pointers, outputs preset to 77 -> (rc, n_events, [starts], [lengths], raw start slots, ev_offs)."""
    L = _lib.lib()
    recs = [np.ascontiguousarray(r, np.int16) for r in records]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    flat = np.concatenate(recs + [np.zeros(1, np.int16)])
    caps = [REF.capacity(len(r), w_s) for r in recs] if caps is None else caps
    eo = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    st, ln = np.full(int(eo[-1]) + 1, PRESET, np.int32), np.full(int(eo[-1]) + 1, PRESET, np.int32)
    ne = np.full(len(recs) + 1, PRESET, np.int32)
    rc = L.s2s_segment_host(flat.ctypes.data, offs.ctypes.data, len(recs), int(offs[-1]), w_s, w_l, T_s, T_l, eo.ctypes.data,
                            st.ctypes.data, ln.ctypes.data, ne.ctypes.data, threads)
    assert st[-1] == PRESET and ln[-1] == PRESET and ne[-1] == PRESET
    cut = lambda a: [a[eo[r]:eo[r] + max(int(ne[r]), 0)].tolist() for r in range(len(recs))]      # noqa: E731
    return rc, ne[:-1].tolist(), cut(st), cut(ln), st, eo


def agree(records, w_s, w_l, T_s, T_l):
    rc, ne, st, ln, _, _ = host(records, w_s, w_l, T_s, T_l)
    assert rc == 0
    for r, x in enumerate(records):
        es, el = REF.events(x, w_s, w_l, T_s, T_l)
        assert (ne[r], st[r], ln[r]) == (len(es), es, el), (r, len(x), w_s, w_l, T_s, T_l)
        REF.check_consequences(len(x), st[r], ln[r], w_s)
    return st, ln


def noisy(seed, n):
    return squiggles(seed, [n])[0]


@pytest.mark.parametrize("w", WINDOWS)
def test_host_equals_the_restatement_on_edge_lengths_and_noise(w):
    w_s, w_l = w
    lens = sorted({0, 1, 2 * w_s - 1, 2 * w_s, 2 * w_l - 1, 2 * w_l, 2 * w_l + 1})
    records = [noisy(10 + n, n) for n in lens] + [noisy(3, 2500), np.random.default_rng(4).integers(-32768, 32768, 1500).astype(np.int16)]
    for T_s, T_l in (T_DEFAULT, (1, 1), (1 << 40, 1 << 40), (6000, 300)):
        st, _ = agree(records, w_s, w_l, T_s, T_l)
    assert st[0] == [] and len(st[1]) == 1             # n = 0: no event; n = 1: one
    st, _ = agree(records, w_s, w_l, *T_DEFAULT)
    assert len(st[-2]) > 1


def test_constant_record_is_one_event_and_extremes_stay_inside_the_stated_bounds():
    st, ln = agree([np.full(1000, 123, np.int16)], 3, 6, 1, 1)
    assert st == [[0]] and ln == [[1000]]
    alt = np.tile(np.array([-32768, 32767], np.int16), 200)
    blocks = np.repeat(np.tile(np.array([-32768, 32767], np.int16), 6), 32)
    odd = np.concatenate([alt[:101], np.full(64, 32767, np.int16), np.full(64, -32768, np.int16)])
    for rec in (alt, blocks, odd):                    # REF.scores asserts 256 w d^2 < 2^56 and V < 2^42 on every position
        agree([rec], 32, 32, 1, 1)
        agree([rec], 1, 32, 501, 1 << 40)
    sc = REF.scores(blocks, 32)
    assert max(sc) == 256 * 32 * (32 * 65535) ** 2 > 1 << 54          # the largest score there is
    x = [int(v) for v in alt[:64]]
    assert 32 * 2 * sum(v * v for v in x[:32]) - 2 * sum(x[:32]) ** 2 > 1 << 40       # V next to its bound


def test_ties_inside_a_neighbourhood_go_to_the_leftmost():
    # a sawtooth's scores repeat with its period: period 2 ties inside the short window's neighbourhood, period 4 inside the long one's
    w_s, w_l = 3, 6
    for period, w in ((2, w_s), (4, w_l)):
        x = ((np.arange(400) % period) * 1000).astype(np.int16)
        agree([x], w_s, w_l, 1, 1)
        sc = REF.scores(x, w)
        pk = REF.peaks(sc, w, 1)
        assert pk
        tied = [p for p in pk if any(sc[q] == sc[p] for q in range(p + 1, min(len(sc) - 1, p + w) + 1))]
        assert tied, "the case must contain ties"
        for p in tied:                               # ... and the later position of a tie is no peak
            assert not any(q in pk for q in range(p + 1, p + w + 1))


def test_long_peak_dropped_at_distance_w_short_and_kept_one_further():
    w_s, w_l, T = 3, 6, 1
    found = {}
    for seed in range(400):
        x = noisy(1000 + seed, 120)
        short, long_ = REF.peaks(REF.scores(x, w_s), w_s, T), REF.peaks(REF.scores(x, w_l), w_l, T)
        for p in long_:
            dist = min([abs(p - q) for q in short] + [10 ** 6])
            if dist in (w_s, w_s + 1) and dist not in found:
                found[dist] = (x, p)
        if len(found) == 2:
            break
    assert sorted(found) == [w_s, w_s + 1]
    x, p = found[w_s]
    st, _ = agree([x], w_s, w_l, T, T)
    assert p not in st[0] and p in REF.peaks(REF.scores(x, w_l), w_l, T)
    x, p = found[w_s + 1]
    st, _ = agree([x], w_s, w_l, T, T)
    assert p in st[0] and p not in REF.peaks(REF.scores(x, w_s), w_s, T)


def planted(seed, levels=300):
    """Piecewise constant, noise free: steps of 1..200 units, dwells of 12..40 samples -> (samples, the planted boundaries)."""
    rng = np.random.default_rng(seed)
    level, parts, cuts, at = 0, [], [], 0
    for _ in range(levels):
        step = int(rng.integers(1, 201)) * (1 if rng.integers(0, 2) else -1)
        level += -step if abs(level + step) > 10000 else step
        dwell = int(rng.integers(12, 41))
        parts.append(np.full(dwell, level, np.int16))
        at += dwell
        cuts.append(at)
    return np.concatenate(parts), cuts[:-1]


def test_noise_free_planted_boundaries_come_back_exactly():
    recs = [planted(s) for s in range(5)]
    rc, ne, st, ln, _, _ = host([r[0] for r in recs], 3, 6, *T_DEFAULT, threads=4)
    assert rc == 0
    for (x, cuts), s, l in zip(recs, st, ln):
        assert s == [0] + cuts and min(l) >= 12
        REF.check_consequences(len(x), s, l, 3)
    assert REF.events(recs[0][0], 3, 6, *T_DEFAULT)[0] == [0] + recs[0][1]


def test_refusals_and_argument_errors():
    L = _lib.lib()
    recs = [noisy(1, 300), noisy(2, 400), noisy(3, 350)]
    rc, ne, st, ln, _, _ = host(recs, 3, 6, *T_DEFAULT)
    assert rc == 0 and min(ne) >= 3
    caps = [REF.capacity(300, 3), ne[1] - 1, REF.capacity(350, 3)]                   # one slot one event too small
    rc2, ne2, st2, ln2, raw, eo = host(recs, 3, 6, *T_DEFAULT, caps=caps)
    assert rc2 == -1 and ne2 == [ne[0], -ne[1], ne[2]] and (st2[0], ln2[0], st2[2], ln2[2]) == (st[0], ln[0], st[2], ln[2])
    assert (raw[eo[1]:eo[2]] == PRESET).all()          # nothing was written to the slot
    for bad in ((0, 1, 1, 1), (4, 3, 1, 1), (1, 33, 1, 1), (3, 6, 0, 1), (3, 6, 1, 0), (3, 6, (1 << 40) + 1, 1), (3, 6, 1, (1 << 40) + 1)):
        assert host(recs, *bad, caps=[100] * 3)[0] == -1
    assert host(recs, 3, 6, 1, 1, threads=0)[0] == -1
    x, eo3 = np.zeros(8, np.int16), np.zeros(3, np.int64)
    out = np.zeros(8, np.int32)
    for offs in ([0, (1 << 22) + 1, (1 << 22) + 1], [0, 5, 3], [-1, 2, 4]):         # too long, decreasing, negative: before any read
        o = np.array(offs, np.int64)
        assert L.s2s_segment_host(x.ctypes.data, o.ctypes.data, 2, max(offs), 3, 6, 1, 1, eo3.ctypes.data, out.ctypes.data, out.ctypes.data,
                                  out.ctypes.data, 1) == -1
    assert [L.s2s_segment_capacity(n, 3) for n in (0, 1, 2, 3, 5, 6, 100)] == [REF.capacity(n, 3) for n in (0, 1, 2, 3, 5, 6, 100)]
    assert L.s2s_segment_capacity(-1, 3) == -1 and L.s2s_segment_capacity(5, 0) == -1 and L.s2s_segment_capacity(5, 33) == -1
    assert L.s2s_segment_scratch_bytes(0, 0) == 8 and L.s2s_segment_scratch_bytes(2049, 1) == 2 * 384 + 3 * 8
    assert L.s2s_segment_scratch_bytes(-1, 0) == -1 and L.s2s_segment_scratch_bytes(1, -1) == -1
    with pytest.raises(ValueError):
        SEG.threshold_int(0.01)
    assert SEG.threshold_int(1.4) == 501 == REF.threshold_int(1.4) and SEG.threshold_int(9.0) == 20736


def test_one_and_sixteen_threads_agree():
    recs = [noisy(20 + i, 200 + 137 * i) for i in range(40)] + [np.zeros(0, np.int16)]
    a, b = host(recs, 3, 6, *T_DEFAULT, threads=1), host(recs, 3, 6, *T_DEFAULT, threads=16)
    assert a[0] == b[0] == 0 and a[1:4] == b[1:4]
    st, ln = SEG.segment(recs, cpu=True)
    assert [s.tolist() for s in st] == a[2] and [l.tolist() for l in ln] == a[3]


# ------------------------------------------------------------------ pools of more than 1,024 tiles (the step of the device's scan)
TILE, SCAN_STEP = 2048, 1024


def three_step_pool():
    """2,051 tiles, boundaries in every tile of the long record: three steps of the scan, every wave's count and the carry non-zero."""
    return [noisy(1, 1 << 22), noisy(2, 5000)]


def tiled_pool(total, seed=60):
    """`total` pooled samples: noisy records of 3,001 samples and one that makes up the remainder; every record but the first begins
    off a tile border (3,001 is odd, 2,048 a power of two: k * 3,001 is no multiple of 2,048 for 0 < k < 2,048)."""
    m = total // 3001
    recs = squiggles(seed, [3001] * m + [total - 3001 * m])
    assert m < TILE and sum(len(r) for r in recs) == total
    return recs


def silent_pool(variant):
    """Noisy records up to tile 1,000, one record of 100 * 2,048 + 5 samples across the tiles 1,000 .. 1,100, noisy records to past tile
    1,100.  `one`: the record is constant -- one event, no flag in the tiles around 1,024.  `cut`: the constant record cut in two at the
    pooled offset 1,024 * 2,048 exactly.  `step`: constant but for one step of 3,000 in tile 1,030 -- the search for the next flag crosses
    thirty empty tiles and the border of the scan's step.  -> (records, the index of the (first) silent record)."""
    m = -(-1000 * TILE // 3001)
    front, back = squiggles(61, [3001] * m), squiggles(62, [3001] * 20)
    at, n = 3001 * m, 100 * TILE + 5
    assert at // TILE == 1000 and (at + n - 1) // TILE == 1100 and at % TILE
    flat = np.full(n, -7, np.int16)
    if variant == "cut":
        mid = [flat[:SCAN_STEP * TILE - at], flat[SCAN_STEP * TILE - at:]]
    elif variant == "step":
        flat[1030 * TILE + 77 - at:] = 2993
        mid = [flat]
    else:
        mid = [flat]
    return front + mid + back, m


def test_three_scan_steps_host_reference_has_boundaries_in_every_tile():
    recs = three_step_pool()
    assert -(-sum(len(r) for r in recs) // TILE) == 2051
    a, b = host(recs, 3, 6, *T_DEFAULT, threads=1), host(recs, 3, 6, *T_DEFAULT, threads=16)
    assert a[0] == b[0] == 0 and a[1:4] == b[1:4]
    per_tile = np.bincount(np.asarray(a[2][0][1:]) // TILE, minlength=2048)           # (without the record's start)
    assert len(per_tile) == 2048 and per_tile.min() >= 1      # what makes the case meaningful (measured: 261 .. 299 a tile)
    for r, x in enumerate(recs):
        REF.check_consequences(len(x), a[2][r], a[3][r], 3)
    es, el = REF.events(recs[1], 3, 6, *T_DEFAULT)
    assert (a[2][1], a[3][1]) == (es, el)


@pytest.mark.parametrize("variant", ("one", "cut", "step"))
def test_silent_stretch_across_tile_1024_keeps_the_consequences(variant):
    recs, k = silent_pool(variant)
    rc, ne, st, ln, _, _ = host(recs, 3, 6, *T_DEFAULT, threads=16)
    assert rc == 0 and -(-sum(len(r) for r in recs) // TILE) > 1100
    for r, x in enumerate(recs):
        REF.check_consequences(len(x), st[r], ln[r], 3)
    if variant == "one":
        assert (st[k], ln[k]) == ([0], [100 * TILE + 5])
    elif variant == "cut":
        assert (st[k], ln[k], st[k + 1]) == ([0], [len(recs[k])], [0]) and ln[k + 1] == [len(recs[k + 1])]
        assert sum(len(r) for r in recs[:k + 1]) == SCAN_STEP * TILE and len(recs[k]) + len(recs[k + 1]) == 100 * TILE + 5
    else:
        at = 1030 * TILE + 77 - 3001 * k
        assert st[k] == [0, at] and ln[k] == [at, 100 * TILE + 5 - at]
    for r in (0, k - 1, k + 1 if variant != "cut" else k + 2, len(recs) - 1):       # the restatement on the neighbours
        assert (st[r], ln[r]) == REF.events(recs[r], 3, 6, *T_DEFAULT)


def test_formatter_rounds_a_huge_event_once_and_refuses_what_it_must():
    L = _lib.lib()
    n = 300000
    S, Q = -n // 2, n * (1 << 30) - 7                  # n Q passes 2^63: the difference is formed exactly
    cal = np.array([8192.0, 13.0, 1437.976], np.float64)
    st, ln = np.array([0], np.int32), np.array([n], np.int32)
    s64, q64, eo, ne = np.array([S], np.int64), np.array([Q], np.int64), np.array([0, 1], np.int64), np.array([1], np.int32)
    ids, id_offs = np.frombuffer(b"read_a", np.uint8), np.array([0, 6], np.int64)
    bound = L.s2s_segment_format_bound(ne.ctypes.data, 1, id_offs.ctypes.data, cal.ctypes.data, 1)
    out = np.zeros(bound + 8, np.uint8)
    args = (st.ctypes.data, ln.ctypes.data, s64.ctypes.data, q64.ctypes.data, eo.ctypes.data, ne.ctypes.data, 1, ids.ctypes.data,
            id_offs.ctypes.data, cal.ctypes.data, 1, 2, out.ctypes.data)
    got = L.s2s_segment_format(*args, bound)
    mean = (float(S) / n + 13.0) * 1437.976 / 8192.0
    stdv = math.sqrt(float(max(n * Q - S * S, 0))) / n * 1437.976 / 8192.0
    want = "\t".join(REF.COLUMNS) + f"\nread_a\t0\t0\t{n}\t{'%.4f' % mean}\t{'%.4f' % stdv}\n"
    assert got == len(want) and out[:got].tobytes().decode() == want and not out[got:].any()
    assert L.s2s_segment_format(*args, bound - 1) == -1
    for bad in ([0.0, 1.0, 2.0], [1.0, float("nan"), 2.0], [1.0, 1.0, 0.0], [float("inf"), 1.0, 1.0]):
        c = np.array(bad, np.float64)
        assert L.s2s_segment_format_bound(ne.ctypes.data, 1, id_offs.ctypes.data, c.ctypes.data, 1) == -1
    ln[0] = 0
    assert L.s2s_segment_format(*args, bound) == -1    # an event without samples


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("segment_cpu")
    sigs = [noisy(40 + i, n) for i, n in enumerate((900, 3, 1500, 5, 700, 1200))]          # (the writers keep no empty record)
    ids = [f"read_{i}" for i in range(len(sigs))]
    paths = [write_file(d / "s.blow5", ids, sigs), write_file(d / "s.slow5", ids, sigs)]
    return d, ids, sigs, paths


def run(*args):
    return CliRunner().invoke(cli.main, ["segment", *[str(a) for a in args]], catch_exceptions=False)


def test_cli_cpu_writes_the_restatements_bytes_whatever_the_batching(files):
    from seq2squiggle_amd import signal_batch as SB
    d, ids, sigs, paths = files
    for path in paths:
        recs = list(SB.open_records(path))
        assert [r["read_id"] for r in recs] == ids
        records = [(r["read_id"], np.asarray(r["signal"], np.int16), (float(r["digitisation"]), float(r["offset"]), float(r["range"])))
                   for r in recs]
        want, want_summary = REF.table(records, 3, 6, *T_DEFAULT)
        r = run(path, "-o", d / "a.tsv", "--cpu", "--json", "--summary", d / "a.sum")
        s = json.loads(r.output.strip().splitlines()[-1])
        assert r.exit_code == 0 and (d / "a.tsv").read_text() == want and (d / "a.sum").read_text() == want_summary
        assert want.count("\n") - 1 == s["events"] > 100 and s["records"] == 6 and s["refused"] == 0 and s["batches"] == 1
        assert s["samples"] == sum(len(x) for x in sigs) and s["mean_samples_per_event"] == s["samples"] / s["events"]
        r = run(path, "-o", d / "b.tsv", "--cpu", "--json", "--summary", d / "b.sum", "--max-samples", 2400)
        s3 = json.loads(r.output.strip().splitlines()[-1])
        assert r.exit_code == 0 and s3["batches"] == 3 and (d / "b.tsv").read_text() == want and (d / "b.sum").read_text() == want_summary
        r = run(path, "-o", d / "c.tsv", "--cpu", "--window-short", 2, "--window-long", 9, "--threshold-short", 2.5, "--threshold-long", 4.0)
        assert r.exit_code == 0 and (d / "c.tsv").read_text() == REF.table(records, 2, 9, REF.threshold_int(2.5), REF.threshold_int(4.0))[0]


def test_cli_refuses_pod5_and_bad_parameters(files):
    d, _, _, paths = files
    r = CliRunner().invoke(cli.main, ["segment", str(d / "x.pod5"), "-o", str(d / "x.tsv"), "--cpu"])
    assert r.exit_code != 0 and "reading POD5 is not supported" in r.output
    for extra in (("--window-short", 0), ("--window-long", 2), ("--window-long", 33), ("--threshold-short", 0.0), ("--max-samples", 0)):
        r = CliRunner().invoke(cli.main, ["segment", paths[0], "-o", str(d / "x.tsv"), "--cpu", *[str(e) for e in extra]])
        assert r.exit_code != 0 and extra[0] in r.output, (extra, r.output)


def test_every_new_symbol_resolves_with_the_stated_signature():
    L = _lib.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    stated = {
        "s2s_segment_capacity": (i64, [i64, i32]),
        "s2s_segment_scratch_bytes": (i64, [i64, i32]),
        "s2s_segment": (i32, [i32, vp, vp, vp, i32, i64, i32, i32, i64, i64, vp, vp, vp, vp, vp]),
        "s2s_segment_host": (i32, [vp, vp, i32, i64, i32, i32, i64, i64, vp, vp, vp, vp, i32]),
        "s2s_segment_format_bound": (i64, [vp, i32, vp, vp, i32]),
        "s2s_segment_format": (i64, [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, i64]),
    }
    for name, (res, args) in stated.items():
        assert name in _lib.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_refused_record_behind_a_lone_record_beyond_max_samples(tmp_path, monkeypatch):
    """The budget loop's corner: a record beyond --max-samples on its own, then a refused one, then two that share a batch.  The refused
    record costs nothing and ends no batch with a sample in it: rows and counters are those of one batch for everything -- but for
    `batches`, 2: the lone record's, then the rest."""
    monkeypatch.setattr(SEG, "MAX_SAMPLES", 1000)                   # (a refused record never reaches the solver, whose limit stays)
    sigs = [noisy(50, 900), noisy(51, 1001), noisy(52, 300), noisy(53, 300)]
    ids = [f"read_{i}" for i in range(len(sigs))]
    path = write_file(tmp_path / "s.blow5", ids, sigs)
    got = {}
    for max_samples in (1 << 27, 700):
        d = tmp_path / str(max_samples)
        d.mkdir()
        got[max_samples] = (SEG.segment_files(path, d / "o.tsv", cpu=True, summary_out=d / "s.tsv", max_samples=max_samples),
                            (d / "o.tsv").read_bytes(), (d / "s.tsv").read_text())
    (one, rows1, sum1), (split, rows2, sum2) = got[1 << 27], got[700]
    assert rows1 == rows2 and sum1 == sum2 and b"read_1\t" not in rows1 and b"read_0\t" in rows1 and b"read_3\t" in rows1
    assert sum1.splitlines()[2] == "read_1\t1001\t0"
    assert (one["batches"], split["batches"]) == (1, 2)
    for key in ("records", "samples", "events", "refused", "mean_samples_per_event"):
        assert one[key] == split[key], key
    assert one["records"] == 4 and one["refused"] == 1 and one["samples"] == 1500
