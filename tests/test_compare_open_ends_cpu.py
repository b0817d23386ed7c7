"""`compare --open-ends` without a GPU: the host entry s2s_sdtw_host against the restatement of the definition (tests/_sdtw_ref.py)
on small shapes, forward and reversed, on squiggle-like, three-level (ties decide S) and extreme inputs; the known answers of the
definition; planted queries; the coordinate rule of reverse; sub-range addressing; thread counts; the error codes; and the command
end to end on files whose B is A between junk, where every number is known in advance.  Every check is an equality."""
import ctypes as C
import json

import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd import compare as CMP
from _sdtw_ref import ref_sdtw
from test_compare_cpu import run_cli, write_file
from test_compare_path_cpu import event_table

MAX_QUERY = 2048
SHAPES = [(1, 1), (1, 50), (2, 1), (40, 20), (63, 257), (64, 256), (65, 513), (255, 300)]
KINDS = ("squiggle", "three", "extreme")

_REF = {}


def make(kind, L, H, seed=None):
    """(q, t) of a kind: squiggle-like levels with noise, values in {-1, 0, 1}, or +-32767 only."""
    rng = np.random.default_rng((1000 * L + H) * 3 + KINDS.index(kind) if seed is None else seed)
    if kind == "squiggle":
        one = lambda n: (400 + np.repeat(rng.integers(-150, 150, n // 8 + 1), 8)[:n] + rng.integers(-12, 13, n)).astype(np.int16)  # noqa: E731
    elif kind == "three":
        one = lambda n: rng.integers(-1, 2, n).astype(np.int16)                                                                   # noqa: E731
    else:
        one = lambda n: rng.choice(np.array([-32767, 32767], np.int16), n)                                                        # noqa: E731
    return one(L), one(H)


def ref_of(kind, L, H, rev):
    """(cost, start, end) of make(kind, L, H) by the restatement, computed once (tests/test_gpu_compare_open_ends.py shares it)."""
    key = (kind, L, H, bool(rev))
    if key not in _REF:
        _REF[key] = ref_sdtw(*make(kind, L, H), reverse=rev)
    return _REF[key]


def host(q, t, rev=False):
    c, s, e = CMP.sdtw([q], [t], reverse=rev, cpu=True)
    assert c.dtype == s.dtype == e.dtype == np.int64
    return int(c[0]), int(s[0]), int(e[0])


def raw_host(q, t, qb, ql, tb, tl, rev, threads=2):
    """s2s_sdtw_host as it is: pools and tables -> (rc, cost, start, end)."""
    L = _lib.lib()
    P = len(qb)
    q, t = np.ascontiguousarray(q, np.int16), np.ascontiguousarray(t, np.int16)
    tabs = [np.ascontiguousarray(v, np.int64) for v in (qb, ql, tb, tl)]
    rv = np.ascontiguousarray(rev, np.uint8)
    out = [np.full(max(P, 1), 77, np.int64) for _ in range(3)]
    rc = L.s2s_sdtw_host(q.ctypes.data, tabs[0].ctypes.data, tabs[1].ctypes.data, t.ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data,
                         rv.ctypes.data, P, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, threads)
    return (rc, *[o[:P].tolist() for o in out])


@pytest.mark.parametrize("L,H", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_equals_the_restatement(kind, L, H):
    q, t = make(kind, L, H)
    for rev in (False, True):
        want = ref_of(kind, L, H, rev)
        assert host(q, t, rev) == want, rev
        cost, s, e = want
        assert 0 <= s < e <= H and 0 <= cost <= L * 65535


@pytest.mark.parametrize("kind", KINDS)
def test_host_equals_the_restatement_at_1025_by_300(kind):
    """The smallest query that gives some threads of s2s_sdtw_kernel two rows and the others one, against a target shorter than the
    workgroup is wide (the restatement takes 0.2 s per direction here); tests/test_gpu_compare_open_ends.py holds the kernel to this."""
    L, H = 1025, 300
    q, t = make(kind, L, H)
    for rev in (False, True):
        want = ref_of(kind, L, H, rev)
        assert host(q, t, rev) == want, rev
        cost, s, e = want
        assert 0 <= s < e <= H and 0 <= cost <= L * 65535


def test_known_answers():
    # all-zero inputs: the first column forward, the last one reversed
    for L, H in ((1, 1), (5, 9), (64, 300)):
        z = np.zeros
        assert host(z(L, np.int16), z(H, np.int16)) == (0, 0, 1) == ref_sdtw(z(L), z(H))
        assert host(z(L, np.int16), z(H, np.int16), True) == (0, H - 1, H) == ref_sdtw(z(L), z(H), True)
    # the largest query at opposite extremes: every cell costs 65,534, any path holds L of them at least
    q, t = np.full(MAX_QUERY, 32767, np.int16), np.full(MAX_QUERY, -32767, np.int16)
    assert host(q, t)[0] == MAX_QUERY * 65534 == host(q, t, True)[0]
    assert host(q, t) == (MAX_QUERY * 65534, 0, 1)                                      # ties: (i - 1, j) beats (i, j - 1); the smallest j
    assert CMP.max_query() == MAX_QUERY


@pytest.mark.parametrize("L,H,at", [(1, 1, 0), (64, 300, 100), (65, 257, 0), (63, 257, 257 - 63), (256, 513, 129)])
def test_planted_query_is_found_at_its_place(L, H, at):
    t = np.random.default_rng(L + H).permutation(H).astype(np.int16)                    # distinct values: one placement costs 0
    q = t[at:at + L].copy()
    for rev in (False, True):
        assert host(q, t, rev) == (0, at, at + L) == ref_sdtw(q, t, rev)


def test_reverse_is_forward_on_reversed_copies():
    for kind in KINDS:
        for L, H in ((40, 20), (63, 257), (255, 300)):
            q, t = make(kind, L, H)
            c, s, e = host(q[::-1].copy(), t[::-1].copy(), False)
            assert host(q, t, True) == (c, H - e, H - s)


def test_sub_ranges_overlap_and_share_a_pool():
    rng = np.random.default_rng(4)
    pool = (400 + np.repeat(rng.integers(-150, 150, 200), 8)[:1500] + rng.integers(-12, 13, 1500)).astype(np.int16)
    # record A = pool[100:400], record B = pool[600:1500]; head and tail anchors of the pair, then two overlapping problems
    qb, ql = [100, 400 - 64, 130, 120], [64, 64, 50, 70]
    tb, tl = [600, 1500 - 500, 650, 640], [500, 500, 300, 333]
    rev = [0, 1, 0, 1]
    rc, cost, start, end = raw_host(pool, pool, qb, ql, tb, tl, rev)
    assert rc == 0
    for p in range(4):
        want = ref_sdtw(pool[qb[p]:qb[p] + ql[p]], pool[tb[p]:tb[p] + tl[p]], bool(rev[p]))
        assert (cost[p], start[p], end[p]) == want, p
    for threads in (1, 3, 16):
        assert raw_host(pool, pool, qb, ql, tb, tl, rev, threads) == (rc, cost, start, end)
    # a query planted in itself: q and t are the same range
    own = np.random.default_rng(5).permutation(300).astype(np.int16)
    assert raw_host(own, own, [50], [100], [0], [300], [0])[1:] == ([0], [50], [150])


def test_thread_counts_and_batches():
    probs = [make(k, L, H) for k in KINDS for L, H in SHAPES[:6]]
    probs += [(np.zeros(0, np.int16), probs[0][1]), (probs[0][0], np.zeros(0, np.int16)), (np.zeros(0, np.int16), np.zeros(0, np.int16))]
    rev = [bool(i % 3 == 1) for i in range(len(probs))]
    got = CMP.sdtw([p[0] for p in probs], [p[1] for p in probs], reverse=rev, cpu=True)
    want = [ref_sdtw(q, t, r) for (q, t), r in zip(probs, rev)]
    assert list(zip(*(g.tolist() for g in got))) == want
    assert want[-3:] == [(-1, 0, 0)] * 3
    flat = np.concatenate([np.concatenate(p) for p in probs])
    lens = np.array([[len(p[0]), len(p[1])] for p in probs]).reshape(-1)
    offs = np.concatenate([[0], np.cumsum(lens)])
    runs = [raw_host(flat, flat, offs[0:-1:2], lens[0::2], offs[1::2], lens[1::2], rev, th) for th in (1, 3, 16)]
    assert runs[0] == runs[1] == runs[2] and runs[0][0] == 0
    assert list(zip(*runs[0][1:])) == want
    assert all(len(x) == 0 for x in CMP.sdtw([], [], cpu=True))


def test_error_codes():
    q = np.zeros(4096, np.int16)
    ok = raw_host(q, q, [0], [MAX_QUERY], [0], [100], [0])
    assert ok[0] == 0 and ok[1] == [0]
    untouched = (-1, [77], [77], [77])                                                   # S2S_ERR_ARG before anything is computed
    assert raw_host(q, q, [0], [MAX_QUERY + 1], [0], [100], [0]) == untouched
    assert raw_host(q, q, [0], [-1], [0], [100], [0]) == untouched
    assert raw_host(q, q, [0], [10], [0], [-1], [0]) == untouched
    assert raw_host(q, q, [-1], [10], [0], [10], [0]) == untouched
    assert raw_host(q, q, [0], [10], [-5], [10], [0]) == untouched
    assert raw_host(q, q, [0], [10], [0], [(1 << 22) + 1], [0]) == untouched
    assert raw_host(q, q, [0, 0], [10, MAX_QUERY + 1], [0, 0], [10, 10], [0, 0])[0] == -1   # one bad problem refuses the call
    assert raw_host(q, q, [0], [10], [0], [10], [0], threads=0)[0] == -1
    assert raw_host(q, q, [], [], [], [], [])[0] == 0                                    # P = 0
    L = _lib.lib()
    assert L.s2s_sdtw_host(None, None, None, None, None, None, None, 0, None, None, None, 1) == 0
    assert L.s2s_sdtw_host(None, None, None, None, None, None, None, -1, None, None, None, 1) == -1
    assert L.s2s_sdtw_host(None, None, None, None, None, None, None, 1, None, None, None, 1) == -1
    # empty members: no error, EMPTY
    assert raw_host(q, q, [0, 0, 5], [0, 10, 0], [0, 0, 7], [10, 0, 0], [0, 1, 1]) == (0, [-1] * 3, [0] * 3, [0] * 3)
    # the device entry refuses bad arguments without a device: nothing is launched, no HIP call is made
    vp = C.c_void_p
    assert L.s2s_sdtw(0, None, *[vp(16)] * 7, -1, vp(16), vp(16), vp(16)) == -1
    assert L.s2s_sdtw(0, None, *[vp(16)] * 6, None, 1, vp(16), vp(16), vp(16)) == -1
    assert L.s2s_sdtw(0, None, *[vp(16)] * 7, 1, vp(16), None, vp(16)) == -1
    assert b"s2s_sdtw" in L.s2s_last_error(None)
    assert L.s2s_sdtw(0, None, *[vp(16)] * 7, 0, vp(16), vp(16), vp(16)) == 0
    with pytest.raises(ValueError):
        CMP.sdtw([q[:5]], [q[:5], q[:5]], cpu=True)
    with pytest.raises(ValueError):
        CMP.sdtw([q[:MAX_QUERY + 1]], [q[:5]], cpu=True)
    with pytest.raises(ValueError):
        CMP.sdtw([q[:5]], [q[:5]], reverse=[True, False], cpu=True)


# ------------------------------------------------------------------ the command
PLANTED = (("r0", 300, 0, 0), ("r1", 2000, 1500, 800), ("r2", 1200, 37, 0), ("r3", 700, 0, 50), ("r4", 1, 3, 4))


def planted_records(planted=PLANTED, seed=21):
    """A: records of distinct values in 0 .. 5,999; B: junk + A's record + junk, the junk from -20,000 .. -10,001 -> (ids, A, B)."""
    rng = np.random.default_rng(seed)
    A = [rng.permutation(6000)[:n].astype(np.int16) for _, n, _, _ in planted]
    junk = lambda n: rng.integers(-20000, -10000, n).astype(np.int16)                                                              # noqa: E731
    B = [np.concatenate([junk(pre), a, junk(suf)]) for a, (_, _, pre, suf) in zip(A, planted)]
    return [p[0] for p in planted], A, B


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("open_ends")
    ids, A, B = planted_records()
    a = write_file(d / "a.blow5", ids + ["onlyA"], A + [A[0]])
    b = write_file(d / "b.blow5", ids[::-1], B[::-1], signal_compression="svb-zd")
    rows = event_table(d / "a.events.tsv", [(i, len(x)) for i, x in zip(ids, A)])
    return d, a, b, ids, A, B, rows


def run_open(d, a, b, tag, *extra):
    out = [str(d / f"{tag}{ext}") for ext in (".tsv", ".paths.tsv", ".events.tsv")]
    r = run_cli(a, b, "-o", out[0], "--normalise", "none", "--cpu", "--json", "--path", out[1], "--events-a", str(d / "a.events.tsv"),
                "--events-out", out[2], *extra)
    return r, out


def test_planted_files_end_to_end(files):
    d, a, b, ids, A, B, rows = files
    r, out = run_open(d, a, b, "o", "--open-ends")
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert (js["open_ends"], js["anchor"], js["anchor_window"], js["anchors_crossed"]) == (True, 1024, 16384, 0)
    assert js["pairs"] == len(ids) and js["mean_dtw_per_sample"] == 0.0
    table = [ln.split("\t") for ln in open(out[0]).read().splitlines()]
    assert tuple(table[0]) == CMP.COLUMNS + CMP.OPEN_COLUMNS
    paths = [ln.split("\t") for ln in open(out[1]).read().splitlines()]
    assert tuple(paths[0]) == CMP.PATH_COLUMNS + ("b_start", "b_end")
    for row, prow, (rid, n, pre, suf), x, y in zip(table[1:], paths[1:], PLANTED, A, B):
        # read_id n_a n_b med_a mad_a med_b mad_b band dtw dtw_per_sample b_start b_end head_cost tail_cost
        assert (row[0], int(row[1]), int(row[2])) == (rid, n, pre + n + suf)
        assert (int(row[10]), int(row[11]), row[12], row[13]) == (pre, pre + n, "0", "0")
        assert (row[8], row[9]) == ("0", "0.000000")
        assert (int(row[3]), int(row[4])) == (int(row[5]), int(row[6]))                # med / mad of the interval: A's own
        assert prow[:6] == [rid, str(n), str(pre + n + suf), row[7], "0", str(n - 1)]
        assert prow[6] == (f"{n - 1}M" if n > 1 else "*") and prow[7:] == [str(pre), str(pre + n)]
    # the carried events: A's, shifted by the prefix
    got = [ln.split("\t") for ln in open(out[2]).read().splitlines()[1:]]
    want = [(rid, pos, kmer, s + pre, e + pre) for rid, _, pre, _ in PLANTED for pos, kmer, s, e in rows.get(rid, [])]
    assert [(g[0], g[1], g[2], int(g[3]), int(g[4])) for g in got] == want and len(want) > 100
    assert js["events_written"] == len(want) and js["events_dropped"] == 0
    # the same pairs WITHOUT the option: the global band cannot follow the prefix -- the case the feature exists for
    r, plain = run_open(d, a, b, "plain")
    assert r.returncode == 0, r.stderr
    ptable = [ln.split("\t") for ln in open(plain[0]).read().splitlines()]
    assert tuple(ptable[0]) == CMP.COLUMNS and "open_ends" not in json.loads(r.stdout.strip().splitlines()[-1])
    for row, (rid, n, pre, suf) in zip(ptable[1:], PLANTED):
        assert len(row) == len(CMP.COLUMNS) and (int(row[8]) > 0) == (pre + suf > 0), rid
    assert open(plain[1]).read().splitlines()[0].split("\t") == list(CMP.PATH_COLUMNS)


def test_anchor_and_window_shorter_than_the_records(files):
    """Anchors of 64 samples in windows of 2,000: the windows are proper parts of r1's B (4,300 samples) and still hold the anchors."""
    d, a, b, ids, A, B, rows = files
    r, out = run_open(d, a, b, "w", "--open-ends", "--anchor", "64", "--anchor-window", "2000")
    assert r.returncode == 0, r.stderr
    table = [ln.split("\t") for ln in open(out[0]).read().splitlines()[1:]]
    assert [(int(t[10]), int(t[11]), t[8]) for t in table] == [(pre, pre + n, "0") for _, n, pre, _ in PLANTED]
    r0, ref = run_open(d, a, b, "o2", "--open-ends")
    assert open(out[1]).read() == open(ref[1]).read() and open(out[2]).read() == open(ref[2]).read()


def test_batching_does_not_change_a_byte(files):
    d, a, b, *_ = files
    r, one = run_open(d, a, b, "one", "--open-ends")
    one_pair = str(CMP.path_scratch_bytes(2000, 2000, 512))                             # the scratch of the longest trimmed pair
    for tag, extra in (("split", ["--max-samples", "1"]), ("mid", ["--max-samples", "5000"]), ("mem", ["--path-memory", one_pair])):
        r2, two = run_open(d, a, b, tag, "--open-ends", *extra)
        assert r2.returncode == 0, r2.stderr
        assert [open(p, "rb").read() for p in one] == [open(p, "rb").read() for p in two], tag
    for tag, extra in (("m1", []), ("m2", ["--max-samples", "1"])):                     # under mad as well
        assert run_cli(a, b, "-o", str(d / f"{tag}.tsv"), "--cpu", "--open-ends", *extra).returncode == 0
    assert open(d / "m1.tsv", "rb").read() == open(d / "m2.tsv", "rb").read()


def test_crossed_anchors_fall_back_and_are_counted(tmp_path):
    x = np.random.default_rng(2).permutation(6000)[:200].astype(np.int16)
    # B holds A's tail in front of A's head: the head anchor starts where the tail anchor ends
    b_rec = np.concatenate([x[150:], x[:50]])
    a = write_file(tmp_path / "a.blow5", ["x", "short"], [x, x])
    b = write_file(tmp_path / "b.blow5", ["x", "short"], [b_rec, x[:1]])
    s = CMP.compare_files(a, b, str(tmp_path / "o.tsv"), band=100, normalise="none", cpu=True, open_ends=True, anchor=50, anchor_window=100,
                          path_out=str(tmp_path / "o.paths.tsv"))
    assert s["anchors_crossed"] == 1 and s["pairs"] == 2
    rows = [ln.split("\t") for ln in open(tmp_path / "o.tsv").read().splitlines()[1:]]
    assert rows[0][10:] == ["0", "100", "0", "0"] and int(rows[0][8]) == int(CMP.dtw_banded([x], [b_rec], 100, cpu=True)[0]) > 0
    dist = np.abs(x.astype(np.int64) - int(x[0]))                                        # one sample of B: every anchor sample lies on it
    assert rows[1][10:] == ["0", "1", str(int(dist[:50].sum())), str(int(dist[150:].sum()))]
    prow = open(tmp_path / "o.paths.tsv").read().splitlines()[1].split("\t")
    assert prow[7:] == ["0", "100"] and int(prow[5]) >= 199


def test_an_empty_record_gets_no_anchors(tmp_path, monkeypatch):
    """The writers store no empty record, so the pairs are handed in directly."""
    x = np.arange(30, dtype=np.int16)
    empty = np.zeros(0, np.int16)
    pairs = [("ea", empty, x, (1.0, 0.0, 1.0)), ("eb", x, empty, (1.0, 0.0, 1.0)), ("ok", x[5:20], x, (1.0, 0.0, 1.0))]
    monkeypatch.setattr(CMP, "_pairs", lambda *a: (iter(pairs), dict(records_a=3, records_b=3, unpaired_a=0, unpaired_b=0)))
    s = CMP.compare_files("a.blow5", "b.blow5", str(tmp_path / "o.tsv"), band=10, normalise="none", cpu=True, open_ends=True,
                          path_out=str(tmp_path / "o.paths.tsv"))
    rows = [ln.split("\t") for ln in open(tmp_path / "o.tsv").read().splitlines()[1:]]
    assert rows[0][8:] == ["nan", "nan", "0", "30", "nan", "nan"] and rows[1][8:] == ["nan", "nan", "0", "0", "nan", "nan"]
    assert rows[2][8:] == ["0", "0.000000", "5", "20", "0", "0"] and s["anchors_crossed"] == 0


def test_path_memory_refuses_by_read_id_once_the_interval_is_known(files):
    d, a, b, ids, A, B, _ = files
    need = CMP.path_scratch_bytes(2000, 2000, 512)
    r, _ = run_open(d, a, b, "pm", "--open-ends", "--path-memory", str(need - 1))
    assert r.returncode == 1 and "read r1" in r.stderr and "--path-memory" in r.stderr and "Traceback" not in r.stderr
    r, out = run_open(d, a, b, "pm2", "--open-ends", "--path-memory", str(need))         # the untrimmed pair would need more
    assert r.returncode == 0 and CMP.path_scratch_bytes(2000, 4300, 512) > need


def test_usage_errors(files):
    d, a, b, *_ = files
    o = str(d / "u.tsv")
    for extra in (["--anchor", "64"], ["--anchor-window", "5000"]):
        r = run_cli(a, b, "-o", o, "--cpu", *extra)
        assert r.returncode == 2 and "--open-ends" in r.stderr
    for extra in (["--anchor", "0"], ["--anchor", str(MAX_QUERY + 1)], ["--anchor-window", "0"], ["--anchor-window", str((1 << 22) + 1)]):
        r = run_cli(a, b, "-o", o, "--cpu", "--open-ends", *extra)
        assert r.returncode == 2 and extra[0] in r.stderr, extra
    for kw in (dict(anchor=0), dict(anchor=MAX_QUERY + 1), dict(anchor_window=0)):
        with pytest.raises(ValueError):
            CMP.compare_files(a, b, o, cpu=True, open_ends=True, **kw)
