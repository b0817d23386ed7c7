"""`preprocess` against the reference's OWN chunk cutting.  tests/golden/preprocess_<te>x<ts>x<k>.npz hold what the reference's
split_eventtable_in_chunks(partition_by=True) -> typical_indices -> filter_chunks -> save_chunks gave for a table
(tools/make_goldens.py preprocess: the reference's functions, unmodified, over a stand-in for its polars calls -- not over polars).
The `preprocess --cpu` command on the table's text, s2s_chunk_pack_host on its arrays and the numpy restatement must all equal it
after the documented mechanical mappings and nothing else (tests/_preprocess_cases.same_as_golden).  Only the npz is read.

What this does not prove: polars' own parsing of a table, its order of ties in a sort (positions are unique inside every read), and
what the reference does with a read whose rows are all N (an empty frame: there the stand-in, not polars, would decide)."""
import numpy as np
import pytest

import _preprocess_cases as C
import _preprocess_ref as R


@pytest.fixture(scope="module", params=C.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def gold(request):
    return C.golden(*request.param)


def test_the_golden_is_what_the_issue_asks_for(gold):
    te, ts, k = (int(v) for v in gold["geometry"])
    N, kept = len(gold["t_lengths"]), gold["kept"]
    assert N == gold["chunks_per_read"].sum() and 4 * len(kept) >= N and 4 * (N - len(kept)) >= N      # both kinds, a quarter at least
    assert ts in gold["t_lengths"] and ts + 1 in gold["t_lengths"] and gold["t_lengths"].min() > 0
    case = C.golden_case(gold)
    counts = np.diff(case["l_offs"]).tolist()
    all_n = (case["kmers"] == ord("N")).all(axis=1)
    rows = [int(n - all_n[a:a + n].sum()) for a, n in zip(case["l_offs"], counts)]
    assert {1, te, te + 1, 3 * te} <= set(rows) and (te == 1 or te - 1 in rows) and case["ev_len"].max() > ts and case["ev_len"].min() >= 1
    p = counts.index(te + 3)                        # the read with all-N rows at both ends and in the middle
    assert all_n[case["l_offs"][p]] and all_n[case["l_offs"][p + 1] - 1] and all_n[case["l_offs"][p] + 1:case["l_offs"][p + 1] - 1].sum() == 1
    assert k == 1 or ((case["kmers"] == ord("N")).any(axis=1) & ~all_n).sum() >= min(2, te)
    lines = [v.split("\t") for v in gold["table"].tobytes().decode().split("\n")[1:] if v]
    assert sum(a[0] != b[0] for a, b in zip(lines, lines[1:])) > len(gold["names"])          # the reads' lines are interleaved
    mine = [(int(v[1]), int(v[3])) for v in lines if v[0] == str(gold["falling_read"])]
    assert len(mine) == 2 * te + 1 and all(a[0] > b[0] and a[1] < b[1] for a, b in zip(mine, mine[1:]))


def test_the_deviations_the_readme_lists_as_the_reference_shows_them(gold):
    te, ts, k = (int(v) for v in gold["geometry"])
    n = len(gold["kept"])
    for pre in ("dna_", "rna_"):
        # stdevs: filter_chunks hands the already expanded array to a second ChunkDataSet -> [N, 1, 1, te] float64; ours: [N, te] float32
        assert gold[pre + "stdevs"].shape == (n, 1, 1, te) and gold[pre + "stdevs"].dtype == np.float64
        # targets_lengths: pad_lengths' int16; ours: int64 (the same values below 32,768)
        assert gold[pre + "targets_lengths"].dtype == np.int16 and gold[pre + "chunks_lengths"].dtype == np.int64
        assert gold[pre + "chunks_lengths"].shape == (n, te) and gold[pre + "targets"].shape == (n, ts)
        # the order: typical_indices' result, unpermuted, is rising -- table order of the reads, then chunk order
        assert np.array_equal(gold[pre + "targets_lengths"], gold["t_lengths"][gold["kept"]]) and (np.diff(gold["kept"]) > 0).all()
        assert np.array_equal(gold[pre + "chunks_lengths"].sum(axis=1), gold[pre + "targets_lengths"])
    assert np.array_equal(gold["kept"], np.flatnonzero(gold["t_lengths"] <= ts))
    # n = te rows give a whole chunk of pads (README: agreed with the reference): the read of te rows has two chunks, the last kept
    names = [str(x) for x in gold["names"]]
    rows = C.golden_rows_of(gold, "full")
    assert gold["chunks_per_read"][names.index("full")] == 2 and gold["dna_targets_lengths"][rows].tolist() == [ts, te]
    assert (gold["dna_chunks"][rows[1]] == np.array([1, 0, 0, 0, 0], np.float16)).all() and (gold["dna_targets"][rows[1]] == 0).all()


@pytest.mark.parametrize("rna", (False, True))
def test_command_cpu_equals_the_reference(gold, rna, tmp_path):
    got, s = C.command(gold, tmp_path, rna, cpu=True)
    assert C.same_as_golden(gold, rna, got, what=("command", rna)) == len(gold["kept"]) > 0
    assert s["chunks_formed"] == len(gold["t_lengths"]) and s["chunks_kept"] == s["chunks_written"] == len(gold["kept"])
    assert s["reads"] == len(gold["names"]) and s["all_n_rows"] == 3


@pytest.mark.parametrize("rna", (False, True))
def test_host_twin_and_restatement_equal_the_reference(gold, rna):
    te, ts, k = (int(v) for v in gold["geometry"])
    case = C.golden_case(gold)
    for name, got in (("restatement", C.ref(case, R.PA, te, ts, reverse=rna)), ("host twin", C.run(case, R.PA, te, ts, reverse=rna, cpu=True))):
        C.same_as_golden(gold, rna, got, what=(name, rna))
        assert got["counters"].tolist() == [len(gold["t_lengths"]), len(gold["kept"]), 3], name
    # the read listed with falling positions, its slots in the table's order (start_idx rising): `backwards` is the reference's sort
    falling = str(gold["falling_read"])
    rows = C.golden_rows_of(gold, falling)
    listed = C.golden_case(gold, only=falling, as_listed=True)
    assert len(rows) >= 2 and listed["ev_len"].tolist() == C.golden_case(gold, only=falling)["ev_len"].tolist()[::-1]
    for name, got in (("restatement", C.ref(listed, R.PA, te, ts, reverse=rna, backwards=True)),
                      ("host twin", C.run(listed, R.PA, te, ts, reverse=rna, backwards=True, cpu=True))):
        C.same_as_golden(gold, rna, got, rows=rows, what=(name, rna, "backwards"))
