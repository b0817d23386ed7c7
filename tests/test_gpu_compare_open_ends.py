"""`compare --open-ends` on the GPU: s2s_sdtw (s2s_sdtw_kernel, csrc/s2s_sdtw.h) against the host entry s2s_sdtw_host, and against
the restatement (tests/_sdtw_ref.py) where it is small: every shape alone and all of them in one launch with mixed reverse flags,
an empty member and a too long query among them; sub-ranges of one pool; and the command, whose files must not depend on --cpu or
on the batching.  tests/test_compare_open_ends_cpu.py holds the host entry to the restatement on the same inputs."""
import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd import compare as CMP
from test_compare_cpu import write_file
from test_compare_open_ends_cpu import KINDS, MAX_QUERY, PLANTED, SHAPES, make, planted_records, ref_of
from test_compare_path_cpu import event_table

pytestmark = pytest.mark.gpu

# held to the host twin only: one stride per thread and more, the largest query, a one-sample target, many window refills
LARGE = [(256, 256), (257, 1000), (1024, 3000), (2048, 2500), (2048, 1), (16, 70000)]
# between one and two rows per thread (1,024 threads): some threads own two rows (the unrolled pair loop) and the others one (the tail
# cell) -- a query of 1,025 and of 2,047 samples, the middle -- against targets of one sample, shorter than the workgroup is wide (r
# rotates), around a multiple of 256 and of several window refills
BETWEEN = [(1025, 300), (1025, 3000), (1536, 255), (1536, 257), (2047, 1), (2047, 1023), (2047, 2500)]


def triple(r):
    return list(zip(*(v.tolist() for v in r)))


def raw_device(pool, qb, ql, tb, tl, rev):
    """s2s_sdtw as it is on one pool: tables -> (rc, cost, start, end); the outputs are preset to 77."""
    import torch
    L = _lib.lib()
    P = len(qb)
    d_pool = torch.from_numpy(np.ascontiguousarray(pool, np.int16)).cuda()
    tab = torch.from_numpy(np.concatenate([qb, ql, tb, tl]).astype(np.int64)).cuda()
    d_rev = torch.from_numpy(np.ascontiguousarray(rev, np.uint8)).cuda()
    out = torch.full((3 * P,), 77, dtype=torch.int64, device="cuda")
    p, o = tab.data_ptr(), out.data_ptr()
    rc = L.s2s_sdtw(0, torch.cuda.current_stream().cuda_stream, d_pool.data_ptr(), p, p + 8 * P, d_pool.data_ptr(), p + 16 * P, p + 24 * P,
                    d_rev.data_ptr(), P, o, o + 8 * P, o + 16 * P)
    r = out.cpu().numpy()
    return rc, r[:P].tolist(), r[P:2 * P].tolist(), r[2 * P:].tolist()


@pytest.fixture(scope="module")
def problems():
    """[(q, t, reverse)]: every small shape and kind in both directions, the large shapes in one direction per kind."""
    probs = [(*make(k, L, H), rev) for k in KINDS for L, H in SHAPES for rev in (False, True)]
    probs += [(*make(k, L, H), bool((i + n) % 2)) for i, k in enumerate(KINDS) for n, (L, H) in enumerate(LARGE)]
    probs += [(*make(k, L, H), bool((i + n) % 2)) for i, k in enumerate(KINDS) for n, (L, H) in enumerate(BETWEEN)]
    host = CMP.sdtw([p[0] for p in probs], [p[1] for p in probs], reverse=[p[2] for p in probs], cpu=True)
    return probs, triple(host)


def test_all_shapes_in_one_launch(problems):
    probs, host = problems
    got = CMP.sdtw([p[0] for p in probs], [p[1] for p in probs], reverse=[p[2] for p in probs])
    assert all(g.dtype == np.int64 for g in got)
    assert triple(got) == host
    small = [ref_of(k, L, H, rev) for k in KINDS for L, H in SHAPES for rev in (False, True)]
    assert host[:len(small)] == small


def test_every_shape_alone(problems):
    probs, host = problems
    for (q, t, rev), want in zip(probs, host):
        assert triple(CMP.sdtw([q], [t], reverse=rev)) == [want], (len(q), len(t), rev)


def test_large_shapes_in_the_other_direction():
    for shapes in (LARGE, BETWEEN):
        for i, k in enumerate(KINDS):
            for n, (L, H) in enumerate(shapes):
                q, t = make(k, L, H)
                rev = not bool((i + n) % 2)
                assert triple(CMP.sdtw([q], [t], reverse=rev)) == triple(CMP.sdtw([q], [t], reverse=rev, cpu=True)), (k, L, H)


def test_a_query_of_1025_samples_against_the_restatement():
    """(1025, 300) in both directions against the restatement itself (tests/test_compare_open_ends_cpu.py holds the host entry to it)."""
    for k in KINDS:
        q, t = make(k, 1025, 300)
        for rev in (False, True):
            assert triple(CMP.sdtw([q], [t], reverse=rev)) == [ref_of(k, 1025, 300, rev)], (k, rev)


def test_known_answers():
    z = np.zeros(300, np.int16)
    assert triple(CMP.sdtw([z[:64], z[:64]], [z, z], reverse=[False, True])) == [(0, 0, 1), (0, 299, 300)]
    q, t = np.full(MAX_QUERY, 32767, np.int16), np.full(MAX_QUERY, -32767, np.int16)
    assert triple(CMP.sdtw([q, q], [t, t], reverse=[False, True])) == [(MAX_QUERY * 65534, 0, 1), (MAX_QUERY * 65534, MAX_QUERY - 1, MAX_QUERY)]
    for L, H, at in ((1, 1, 0), (64, 300, 100), (65, 257, 0), (63, 257, 257 - 63), (256, 513, 129)):
        t = np.random.default_rng(L + H).permutation(H).astype(np.int16)
        assert triple(CMP.sdtw([t[at:at + L]] * 2, [t, t], reverse=[False, True])) == [(0, at, at + L)] * 2


def test_refused_and_empty_members_leave_their_neighbours_alone():
    rng = np.random.default_rng(4)
    pool = (400 + np.repeat(rng.integers(-150, 150, 700), 8)[:5000] + rng.integers(-12, 13, 5000)).astype(np.int16)
    # head and tail of one record pair, overlapping ranges, an empty query, an empty target, a 2,049-sample query, negative begin / len
    qb = [100, 400 - 64, 130, 120, 10, 10, 0, -1, 10, 300]
    ql = [64, 64, 50, 70, 0, 20, MAX_QUERY + 1, 10, -3, 40]
    tb = [600, 1500 - 500, 650, 640, 700, 700, 2100, 700, 700, 3000]
    tl = [500, 500, 300, 333, 100, 0, 2500, 100, 100, 2000]
    rev = [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    rc, cost, start, end = raw_device(pool, qb, ql, tb, tl, rev)
    assert rc == 0
    good = [0, 1, 2, 3, 9]
    host = CMP.sdtw([pool[qb[p]:qb[p] + ql[p]] for p in good], [pool[tb[p]:tb[p] + tl[p]] for p in good], reverse=[bool(rev[p]) for p in good],
                    cpu=True)
    assert [(cost[p], start[p], end[p]) for p in good] == triple(host)
    assert [(cost[p], start[p], end[p]) for p in (4, 5)] == [(-1, 0, 0)] * 2                      # S2S_DTW_COST_EMPTY
    assert [(cost[p], start[p], end[p]) for p in (6, 7, 8)] == [(-2, 0, 0)] * 3                   # S2S_DTW_COST_TOO_LONG: no work
    assert all(len(x) == 0 for x in CMP.sdtw([], []))


def test_compare_files_bytes_do_not_depend_on_cpu_or_batching(tmp_path):
    ids, A, B = planted_records()
    a = write_file(tmp_path / "a.blow5", ids + ["onlyA"], A + [A[0]])
    b = write_file(tmp_path / "b.blow5", ids[::-1], B[::-1], signal_compression="svb-zd")
    event_table(tmp_path / "a.events.tsv", [(i, len(x)) for i, x in zip(ids, A)])
    for norm in ("mad", "none"):
        outs = {}
        for tag, kw in (("one", {}), ("split", dict(max_samples=3000)), ("cpu", dict(cpu=True))):
            s = CMP.compare_files(a, b, str(tmp_path / f"{tag}.tsv"), normalise=norm, path_out=str(tmp_path / f"{tag}.paths.tsv"),
                                  events_a=str(tmp_path / "a.events.tsv"), events_out=str(tmp_path / f"{tag}.events.tsv"), open_ends=True,
                                  anchor=256, anchor_window=2500, **kw)
            outs[tag] = tuple(open(tmp_path / f"{tag}{ext}", "rb").read() for ext in (".tsv", ".paths.tsv", ".events.tsv"))
            assert s["pairs"] == len(ids) and s["open_ends"] and s["events_written"] > 100
        assert outs["one"] == outs["split"] == outs["cpu"], norm
        if norm == "none":                                                              # the planted intervals, exactly
            rows = [ln.split("\t") for ln in outs["one"][0].decode().splitlines()[1:]]
            assert [(int(r[10]), int(r[11]), r[8]) for r in rows] == [(pre, pre + n, "0") for _, n, pre, _ in PLANTED]
