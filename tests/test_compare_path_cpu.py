"""`compare --path` without a GPU: the host entry s2s_dtw_path_host against the restatement of the path's definition
(tests/_dtw_path_ref.py) on the shapes of tests/test_compare_cpu.py plus widest diagonals around one wave's 64 cells and around the
256-thread step, with random and with constant signals (ties everywhere); the invariants of the definition; pairs without path;
the error codes; the boundary map; and `compare --cpu --path --events-a --events-out` end to end.  Every check is an equality."""
import ctypes as C
import json

import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd import compare as CMP
from _dtw_ref import INF, ref_dtw, ref_median_mad, ref_normalise
from _dtw_path_ref import (check_path, ref_boundary_map, ref_cells, ref_path, ref_path_string, ref_transfer_events)
from test_compare_cpu import DTW_SHAPES, MAX_BAND, dtw_pair, mixed_pairs, run_cli, squiggles, write_file

PATH_SHAPES = (DTW_SHAPES + [(200, 200, R) for R in (62, 63, 64, 65)] + [(700, 700, R) for R in (255, 256, 257)] + [(700, 650, 300)])

_REF = {}


def shape_pairs(n, m):
    """The two pairs of a shape: random signals, and constant ones."""
    return [dtw_pair(n, m), (np.full(n, 7, np.int16), np.full(m, 7, np.int16))]


def ref_of(n, m, R):
    """[(cost, ops)] of shape_pairs(n, m) by the restatement, computed once (tests/test_gpu_compare_path.py shares it)."""
    if (n, m, R) not in _REF:
        _REF[(n, m, R)] = [ref_path(a, b, R) for a, b in shape_pairs(n, m)]
    return _REF[(n, m, R)]


def host_path(a, b, R):
    cost, ops = CMP.dtw_path([a], [b], R, cpu=True)
    return int(cost[0]), ops[0]


@pytest.mark.parametrize("n,m,R", PATH_SHAPES)
def test_host_path_equals_the_restatement(n, m, R):
    for (a, b), (want_cost, want_ops) in zip(shape_pairs(n, m), ref_of(n, m, R)):
        assert want_cost == ref_dtw(a, b, R) < INF                                     # the corner is reached
        check_path(a, b, R, want_cost, want_ops)
        cost, ops = host_path(a, b, R)
        assert ops.dtype == np.uint8 and (cost, ops.tolist()) == (want_cost, want_ops)
        assert cost == int(CMP.dtw_banded([a], [b], R, cpu=True)[0])
        check_path(a, b, R, cost, ops)
    if n == m:                                                                          # constant signals of one length: the diagonal
        assert ops.tolist() == [0] * (n - 1)


def test_host_path_batches_and_pairs_without_path():
    al, bl = mixed_pairs()
    cost, ops = CMP.dtw_path(al, bl, 5, cpu=True)
    assert cost.dtype == np.int64 and cost.tolist() == CMP.dtw_banded(al, bl, 5, cpu=True).tolist()
    empty = [k for k in range(len(al)) if not len(al[k]) or not len(bl[k])]
    assert len(empty) == 5 and all(cost[k] == -1 and len(ops[k]) == 0 for k in empty)
    for k in range(40):
        assert (int(cost[k]), ops[k].tolist()) == ref_path(al[k], bl[k], 5), k
    for k in range(len(al)):
        if k not in empty:
            check_path(al[k], bl[k], 5, int(cost[k]), ops[k])
    # any batching gives the same: a scratch budget of one longest pair cuts the 30 into many batches
    one, one_ops = CMP.dtw_path(al[:30], bl[:30], 5, cpu=True, path_memory=CMP.path_scratch_bytes(199, 199, 5))
    assert one.tolist() == cost[:30].tolist() and all(np.array_equal(x, y) for x, y in zip(one_ops, ops))
    assert CMP.dtw_path([], [], 5, cpu=True)[1] == []
    # n = m = 1: a path of no steps
    c, o = CMP.dtw_path([np.array([3], np.int16)], [np.array([-4], np.int16)], 1, cpu=True)
    assert c.tolist() == [7] and o[0].tolist() == []


def test_scratch_bytes_and_budget():
    # per diagonal ceil((floor(2 R max(n, m) / (n + m)) + 1) / 64) pairs of 64-bit words, n + m - 1 diagonals
    assert CMP.path_scratch_bytes(200, 200, 62) == 399 * 1 * 16 and CMP.path_scratch_bytes(200, 200, 63) == 399 * 1 * 16
    assert CMP.path_scratch_bytes(200, 200, 64) == 399 * 2 * 16
    assert CMP.path_scratch_bytes(2500, 700, MAX_BAND) == 3199 * ((2 * MAX_BAND * 2500 // 3200 + 64) // 64) * 16
    assert CMP.path_scratch_bytes(0, 5, 3) == 0 == CMP.path_scratch_bytes(5, 0, 3) == CMP.path_scratch_bytes((1 << 22) + 1, 5, 3)
    assert CMP.path_scratch_bytes(1, 1, 1) == 16
    for n, m, R in PATH_SHAPES:                    # no diagonal holds more cells than its words have bits
        chunks = CMP.path_scratch_bytes(n, m, R) // 16 // (n + m - 1)
        widest = max(np.bincount([i + j for i in range(n) for j in range(max(0, -((R * max(n, m) - i * m) // n)),
                                                                         min(m - 1, (i * m + R * max(n, m)) // n) + 1)]))
        assert widest <= 2 * R * max(n, m) // (n + m) + 1 <= 64 * chunks < 2 * R * max(n, m) // (n + m) + 1 + 64, (n, m, R)
    with pytest.raises(ValueError):
        CMP.path_scratch_bytes(5, 5, 0)
    a, b = dtw_pair(300, 97)
    with pytest.raises(ValueError, match="pair 1"):
        CMP.dtw_path([a[:5], a], [b[:5], b], 7, cpu=True, path_memory=CMP.path_scratch_bytes(300, 97, 7) - 1)
    with pytest.raises(ValueError):
        CMP.dtw_path([a], [b], 7, cpu=True, path_memory=0)


def test_boundary_map():
    for n, m, R in ((1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 2, 1), (300, 97, 7), (97, 300, 2), (129, 129, 33)):
        for (a, b), (_, ops) in zip(shape_pairs(n, m), ref_of(n, m, R)):
            g = CMP.boundary_map(np.array(ops, np.uint8), n, m)
            assert g.dtype == np.int64 and g.tolist() == ref_boundary_map(ops, n, m)
            i, j = CMP.path_cells(np.array(ops, np.uint8))
            assert list(zip(i.tolist(), j.tolist())) == ref_cells(ops)
            # abutting intervals stay abutting and cover b; a shared sample of b belongs to the last sample of a on it
            assert sum(g[k + 1] - g[k] for k in range(n)) == m
            for k, op in enumerate(ops):
                if op == 1:                                                            # (i, j) -> (i + 1, j): i owns nothing of j
                    assert g[i[k] + 1] == j[k] and (i[k] == 0 or g[i[k]] <= j[k])
    assert CMP.boundary_map([0, 1, 1, 2, 0], 5, 4).tolist() == [0, 1, 1, 1, 3, 4]
    assert CMP.boundary_map([], 1, 1).tolist() == [0, 1]
    for bad in (([0, 0], 5, 3), ([], 2, 2), ([3], 2, 2), ([0], 0, 0)):
        with pytest.raises(ValueError):
            CMP.boundary_map(*bad)
    assert CMP.path_string(np.array([0] * 12 + [1] * 3 + [0] + [2] * 2, np.uint8)) == "12M3A1M2B" and CMP.path_string([]) == "*"


def test_error_codes():
    L = _lib.lib()
    a = np.zeros(8, np.int16)
    offs = np.array([0, 4, 8], np.int64)
    slots = np.array([0, 6, 12], np.int64)
    cost, steps, ops = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(12, np.uint8)
    p = lambda x: x.ctypes.data                                                            # noqa: E731

    def path(P, band, ao=offs, bo=offs, po=slots, threads=2):
        return L.s2s_dtw_path_host(p(a), p(ao), p(a), p(bo), P, band, p(cost), p(ops), p(po), p(steps), threads)
    assert path(2, 1) == 0 and steps.tolist() == [3, 3] and ops.tolist() == [0, 0, 0, 0, 0, 0] * 2 and path(2, MAX_BAND) == 0
    assert path(0, 1) == 0
    assert path(2, 0) == -1 and path(2, MAX_BAND + 1) == -1 and path(-1, 1) == -1 and path(2, 1, threads=0) == -1
    long_offs = np.array([0, (1 << 22) + 1, (1 << 22) + 2], np.int64)
    assert path(2, 1, ao=long_offs) == -1 and path(2, 1, bo=long_offs) == -1
    assert path(2, 1, ao=np.array([0, 4, 2], np.int64)) == -1
    assert path(2, 1, po=np.array([0, 5, 11], np.int64)) == -1                              # a slot shorter than n + m - 2
    assert path(2, 1, po=np.array([-6, 0, 6], np.int64)) == -1
    # a path shorter than its slot is right-aligned in it
    wide = np.full(20, 9, np.uint8)
    assert L.s2s_dtw_path_host(p(a), p(offs), p(a), p(offs), 2, 1, p(cost), p(wide), p(np.array([0, 8, 20], np.int64)), p(steps), 1) == 0
    assert wide.tolist() == [9] * 5 + [0] * 3 + [9] * 9 + [0] * 3 and steps.tolist() == [3, 3]
    # the device entries refuse bad arguments without a device: nothing is launched, no HIP call is made
    vp = C.c_void_p
    ok = [vp(16)] * 4
    assert L.s2s_dtw_path(0, None, *ok, 1, 0, vp(16), vp(16), vp(16), vp(16), vp(16), vp(16)) == -1
    assert L.s2s_dtw_path(0, None, *ok, 1, MAX_BAND + 1, vp(16), vp(16), vp(16), vp(16), vp(16), vp(16)) == -1
    assert L.s2s_dtw_path(0, None, *ok, -1, 1, vp(16), vp(16), vp(16), vp(16), vp(16), vp(16)) == -1
    assert L.s2s_dtw_path(0, None, *ok, 1, 1, vp(16), vp(24), vp(16), vp(16), vp(16), vp(16)) == -1       # scratch not 16-byte aligned
    assert L.s2s_dtw_path(0, None, *ok, 1, 1, vp(16), None, vp(16), vp(16), vp(16), vp(16)) == -1
    assert b"s2s_dtw_path" in L.s2s_last_error(None)
    assert L.s2s_dtw_path_scratch_bytes(5, 5, 0) == -1 and L.s2s_dtw_path_scratch_bytes(5, 5, MAX_BAND + 1) == -1
    with pytest.raises(ValueError):
        CMP.dtw_path([a], [a, a], 1, cpu=True)
    with pytest.raises(ValueError):
        CMP.dtw_path([a], [a], MAX_BAND + 1, cpu=True)


# ------------------------------------------------------------------ the command
def event_table(path, reads, samples=False):
    """A hand-made event table of file A: per read abutting events of 1 .. 12 samples from sample 3 on, one gap, an unknown read."""
    rng = np.random.default_rng(8)
    rows = {}
    with open(path, "w") as f:
        f.write("\t".join(CMP.EVENT_COLUMNS + (("samples",) if samples else ())) + "\n")
        for rid, n in reads:
            cur, pos = 3, 0
            while cur < n:
                e = min(n, cur + int(rng.integers(1, 13)))
                kmer = "".join(rng.choice(list("ACGT"), 9))
                if pos != 4:                                                            # (k-mer 4 owns no row: a gap)
                    rows.setdefault(rid, []).append((str(pos), kmer, cur, e))
                    f.write(f"{rid}\t{pos}\t{kmer}\t{cur}\t{e}\t1.0000\t2.0000" + ("\t1.000,2.000" if samples else "") + "\n")
                cur, pos = e, pos + 1
    return rows


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("compare_path")
    lens = (120, 333, 64, 500)
    sa = squiggles(1, lens)
    # B: A's levels, stretched and squeezed in places, with other noise -- the same molecule read again
    rng = np.random.default_rng(3)
    sb = []
    for s in sa:
        keep = np.repeat(np.arange(len(s)), rng.choice([0, 1, 1, 1, 2, 3], len(s)))
        sb.append((s[keep] + rng.integers(-9, 10, len(keep))).astype(np.int16))
    ids_a, ids_b = ["r0", "r1", "onlyA", "r3"], ["r3", "onlyB", "r1", "r0"]
    A = dict(zip(ids_a, sa))
    B = dict(zip(ids_b, [sb[3], sb[2], sb[1], sb[0]]))
    a = write_file(d / "a.blow5", ids_a, sa, record_compression="zlib")
    b = write_file(d / "b.blow5", ids_b, [B[i] for i in ids_b], record_compression="none", signal_compression="svb-zd")
    return d, a, b, A, B, ids_a


def b_calibration(b_path):
    from seq2squiggle_amd import signal_io
    it = signal_io.iter_blow5(b_path)
    next(it)
    return {r["read_id"]: (float(r["digitisation"]), float(r["offset"]), float(r["range"])) for r in it}


def expected_files(pairs, band, rows, cal):
    """The bytes of --path and --events-out from the restatement: (paths text, events text, dropped)."""
    paths, events, dropped = ["\t".join(CMP.PATH_COLUMNS) + "\n"], ["\t".join(CMP.EVENT_COLUMNS) + "\n"], 0
    for rid, a, b in pairs:
        qa, qb = ref_normalise(a, *ref_median_mad(a)), ref_normalise(b, *ref_median_mad(b))
        cost, ops = ref_path(qa, qb, band)
        paths.append(f"{rid}\t{len(a)}\t{len(b)}\t{band}\t{cost}\t{len(ops)}\t{ref_path_string(ops)}\n")
        lines, drop = ref_transfer_events(rid, rows.get(rid, []), ref_boundary_map(ops, len(a), len(b)), b, *cal[rid])
        events += lines
        dropped += drop
    return "".join(paths), "".join(events), dropped


@pytest.mark.parametrize("samples", (False, True))
def test_compare_cpu_path_and_events_end_to_end(files, samples):
    d, a, b, A, B, ids_a = files
    rows = event_table(d / "a.events.tsv", [(i, len(A[i])) for i in ids_a] + [("elsewhere", 30)], samples)
    pairs = [(i, A[i], B[i]) for i in ids_a if i in B]
    want_paths, want_events, want_dropped = expected_files(pairs, 40, rows, b_calibration(b))
    assert want_dropped > 0 and want_events.count("\n") > 50                            # squeezed stretches drop events, most survive
    out, paths, events = str(d / "o.tsv"), str(d / "o.paths.tsv"), str(d / "b.events.tsv")
    r = run_cli(a, b, "-o", out, "--band", "40", "--cpu", "--json", "--path", paths, "--events-a", str(d / "a.events.tsv"),
                "--events-out", events)
    assert r.returncode == 0, r.stderr
    assert open(paths).read() == want_paths
    assert open(events).read() == want_events
    js = json.loads(r.stdout.strip().splitlines()[-1])
    unpaired = len(rows["onlyA"]) + len(rows["elsewhere"])
    assert (js["events_written"], js["events_dropped"], js["events_unpaired"]) == (want_events.count("\n") - 1, want_dropped, unpaired)
    # the distance table is the one of a run without the new options, and a scratch budget that splits the pairs changes nothing
    plain = str(d / "plain.tsv")
    assert run_cli(a, b, "-o", plain, "--band", "40", "--cpu").returncode == 0
    assert open(out).read() == open(plain).read()
    need = max(CMP.path_scratch_bytes(len(x), len(y), 40) for _, x, y in pairs)
    r = run_cli(a, b, "-o", out, "--band", "40", "--cpu", "--path", str(d / "split.paths.tsv"), "--path-memory", str(need))
    assert r.returncode == 0 and open(d / "split.paths.tsv").read() == want_paths
    # levels: every row is the mean of B's stored samples in its interval with the record's offset
    f = open(events).read().splitlines()[1].split("\t")
    dig, off, rng = b_calibration(b)[f[0]]
    assert f[5] == "%.4f" % ((float(B[f[0]][int(f[3]):int(f[4])].astype(np.int64).sum()) / (int(f[4]) - int(f[3])) + off) * rng / dig)


def test_compare_path_refusals(files):
    d, a, b, A, B, _ = files
    need = max(CMP.path_scratch_bytes(len(A[i]), len(B[i]), 40) for i in ("r0", "r1", "r3"))
    r = run_cli(a, b, "-o", str(d / "e.tsv"), "--band", "40", "--cpu", "--path", str(d / "e.paths.tsv"), "--path-memory", str(need - 1))
    assert r.returncode == 1 and "read r3" in r.stderr and "--path-memory" in r.stderr and "Traceback" not in r.stderr
    assert not (d / "e.tsv").exists() and not (d / "e.paths.tsv").exists()
    r = run_cli(a, b, "-o", str(d / "e.tsv"), "--cpu", "--events-out", str(d / "e.events.tsv"))
    assert r.returncode == 2 and "--events-a" in r.stderr
    r = run_cli(a, b, "-o", str(d / "e.tsv"), "--cpu", "--path", str(d / "e.paths.tsv"), "--path-memory", "0")
    assert r.returncode == 2 and "--path-memory" in r.stderr
    (d / "alien.tsv").write_text("read_id\tx\n1\t2\n")
    r = run_cli(a, b, "-o", str(d / "e.tsv"), "--cpu", "--events-a", str(d / "alien.tsv"), "--events-out", str(d / "e.events.tsv"))
    assert r.returncode == 1 and "alien.tsv" in r.stderr and "Traceback" not in r.stderr
