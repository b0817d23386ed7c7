"""`compare --path` on the GPU: s2s_dtw_path (s2s_dtw_kernel<true> and s2s_dtw_trace_kernel, csrc/s2s_dtw.h) against the host entry
s2s_dtw_path_host for ops, steps and cost, and its cost against s2s_dtw_banded: the shapes of tests/test_compare_path_cpu.py (widest
diagonals around one wave's 64 cells and around the 256-thread step, sloped bands, random and constant signals) in one launch and
each alone, batches with empty members, the largest band, thousands of diagonals through a small ring, a cost past 2^32, a scratch
budget of one pair per batch, and the command, whose files must not depend on --cpu.  tests/test_compare_path_cpu.py holds the
host entry to the restatement on the same inputs; the restatement's paths are compared here too where it has them."""
import numpy as np
import pytest

from seq2squiggle_amd import compare as CMP
from _dtw_path_ref import check_path
from test_compare_cpu import MAX_BAND, dtw_pair, mixed_pairs
from test_compare_path_cpu import PATH_SHAPES, event_table, ref_of, shape_pairs

pytestmark = pytest.mark.gpu


def same(got, want):
    """(cost, [ops]) of two runs: equal costs, equal ops (so equal steps)."""
    return got[0].tolist() == want[0].tolist() and len(got[1]) == len(want[1]) and all(np.array_equal(x, y) for x, y in zip(got[1], want[1]))


def test_path_shapes_in_one_launch_and_alone():
    """Every listed (n, m, R), random and constant signals: the pairs of one R in one launch, and each alone."""
    by_band = {}
    for n, m, R in PATH_SHAPES:
        by_band.setdefault(R, []).extend(shape_pairs(n, m))
    for R, pairs in sorted(by_band.items()):
        al, bl = [p[0] for p in pairs], [p[1] for p in pairs]
        host = CMP.dtw_path(al, bl, R, cpu=True)
        got = CMP.dtw_path(al, bl, R)
        assert got[0].dtype == np.int64 and all(o.dtype == np.uint8 for o in got[1])
        assert same(got, host), R
        assert got[0].tolist() == CMP.dtw_banded(al, bl, R).tolist()
        for a, b in zip(al, bl):
            assert same(CMP.dtw_path([a], [b], R), CMP.dtw_path([a], [b], R, cpu=True)), (len(a), len(b), R)


def test_path_batches_with_empty_members():
    al, bl = mixed_pairs()
    host = CMP.dtw_path(al, bl, 5, cpu=True)
    assert sum(c == -1 for c in host[0]) == 5 and sum(len(o) == 0 for o in host[1]) == 5
    for P in (1, 2, 257):
        assert same(CMP.dtw_path(al[:P], bl[:P], 5), (host[0][:P], host[1][:P]))
    assert CMP.dtw_path(al, bl, 5)[0].tolist() == CMP.dtw_banded(al, bl, 5).tolist()
    # a scratch budget that holds one pair at a time: the same as one batch
    assert same(CMP.dtw_path(al, bl, 5, path_memory=CMP.path_scratch_bytes(199, 199, 5)), host)
    assert same(CMP.dtw_path(al[:40], bl[:40], 5, path_memory=max(CMP.path_scratch_bytes(len(a), len(b), 5) for a, b in zip(al[:40], bl[:40]))),
                (host[0][:40], host[1][:40]))
    assert CMP.dtw_path([], [], 5)[1] == []


def test_path_at_the_largest_band():
    for n, m in ((3000, 3000), (2500, 700)):
        a, b = dtw_pair(n, m)
        host = CMP.dtw_path([a], [b], MAX_BAND, cpu=True)
        got = CMP.dtw_path([a], [b], MAX_BAND)
        assert same(got, host)
        assert int(got[0][0]) == int(CMP.dtw_banded([a], [b], MAX_BAND)[0])
        check_path(a, b, MAX_BAND, int(got[0][0]), got[1][0])


def test_path_through_many_window_refills():
    a, b = dtw_pair(1000, 1000)
    got = CMP.dtw_path([a], [b], 3)
    assert same(got, CMP.dtw_path([a], [b], 3, cpu=True))
    check_path(a, b, 3, int(got[0][0]), got[1][0])


def test_small_paths_equal_the_restatement():
    for n, m, R in ((1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 2, 1), (65, 65, 33), (97, 300, 2), (129, 129, 200)):
        pairs = shape_pairs(n, m)
        cost, ops = CMP.dtw_path([p[0] for p in pairs], [p[1] for p in pairs], R)
        assert [(int(c), o.tolist()) for c, o in zip(cost, ops)] == ref_of(n, m, R), (n, m, R)


def test_path_of_a_cost_past_2_to_the_32():
    a, b = np.full(70000, -32767, np.int16), np.full(70000, 32767, np.int16)
    cost, ops = CMP.dtw_path([a], [b], 1)
    assert int(cost[0]) == 70000 * 65534 > 1 << 32 and ops[0].tolist() == [0] * 69999
    assert same((cost, ops), CMP.dtw_path([a], [b], 1, cpu=True))


def test_compare_files_path_bytes_do_not_depend_on_batching_or_cpu(tmp_path):
    from test_compare_cpu import squiggles, write_file
    sa = squiggles(1, (120, 333, 64, 500, 1, 2000))
    rng = np.random.default_rng(3)
    sb = []
    for s in sa:
        keep = np.repeat(np.arange(len(s)), rng.choice([0, 1, 1, 1, 2, 3], len(s)))
        keep = keep if len(s) > 1 else np.zeros(1, np.int64)                            # (one sample against one: a path of no steps)
        sb.append((s[keep] + rng.integers(-9, 10, len(keep))).astype(np.int16))
    ids = [f"read{k}" for k in range(len(sa))]
    a = write_file(tmp_path / "a.blow5", ids + ["onlyA"], sa + [sa[0]])
    b = write_file(tmp_path / "b.blow5", ids[::-1], sb[::-1], signal_compression="svb-zd")
    event_table(tmp_path / "a.events.tsv", [(i, len(s)) for i, s in zip(ids, sa)] + [("onlyA", 120)])
    need = max(CMP.path_scratch_bytes(len(x), len(y), 48) for x, y in zip(sa, sb))
    outs = {}
    for tag, kw in (("one", {}), ("tiny", dict(path_memory=need)), ("split", dict(max_samples=1500)), ("cpu", dict(cpu=True))):
        s = CMP.compare_files(a, b, str(tmp_path / f"{tag}.tsv"), band=48, path_out=str(tmp_path / f"{tag}.paths.tsv"),
                              events_a=str(tmp_path / "a.events.tsv"), events_out=str(tmp_path / f"{tag}.events.tsv"), **kw)
        outs[tag] = tuple(open(tmp_path / f"{tag}{ext}", "rb").read() for ext in (".tsv", ".paths.tsv", ".events.tsv"))
        assert s["pairs"] == len(ids) and s["events_written"] > 100 and s["events_unpaired"] > 0
    assert outs["one"] == outs["tiny"] == outs["split"] == outs["cpu"]
    plain = CMP.compare_files(a, b, str(tmp_path / "plain.tsv"), band=48)
    assert open(tmp_path / "plain.tsv", "rb").read() == outs["one"][0] and "events_written" not in plain
    rows = outs["one"][1].decode().splitlines()
    assert len(rows) == len(ids) + 1 and rows[5].split("\t")[-2:] == ["0", "*"]          # the one-sample pair


def test_cli_path_files_equal_with_and_without_cpu(tmp_path):
    from test_compare_cpu import run_cli, squiggles, write_file
    sa, sb = squiggles(1, (300, 777)), squiggles(1, (330, 700))
    a = write_file(tmp_path / "a.blow5", ["x", "y"], sa)
    b = write_file(tmp_path / "b.blow5", ["x", "y"], sb)
    event_table(tmp_path / "a.events.tsv", [("x", 300), ("y", 777)])
    got = {}
    for tag, extra in (("gpu", []), ("cpu", ["--cpu"])):
        r = run_cli(a, b, "-o", str(tmp_path / f"{tag}.tsv"), "--band", "100", "--path", str(tmp_path / f"{tag}.paths.tsv"), "--events-a",
                    str(tmp_path / "a.events.tsv"), "--events-out", str(tmp_path / f"{tag}.events.tsv"), *extra)
        assert r.returncode == 0, r.stderr
        got[tag] = tuple(open(tmp_path / f"{tag}{ext}", "rb").read() for ext in (".tsv", ".paths.tsv", ".events.tsv"))
    assert got["gpu"] == got["cpu"] and got["gpu"][1].count(b"\n") == 3 and got["gpu"][2].count(b"\n") > 50
