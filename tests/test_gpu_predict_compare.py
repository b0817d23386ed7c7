"""The loop predict -> compare: `compare` fed what `predict` wrote, not hand-made records.  One simulated run (20 reads, -r 400,
seed 11: the `_run` of tests/test_gpu_events.py) is written three times -- BLOW5 with its event table, BLOW5 with the GPU-coded
svb-zd signal, SLOW5 -- and the first file is compared with each of them, with paths and with its `predict --events` table
carried over (--events-a / --events-out), on the GPU and with cpu=True.  The same samples on both sides leave nothing to chance:
distance 0, equal medians and MADs, the diagonal as the path, every event carried onto its own interval.  The level of a carried
event differs from predict's by a constant per record: `compare` forms it with the record's own offset, `predict --events` with
the profile's offset_mean (tests/test_gpu_events.py, test_rows_agree_with_the_paf_and_with_the_samples_read_back).  Everything is
an equality of integers or bytes except the two formatted floats, each within 1.01e-4: two roundings to %.4f."""
import numpy as np
import pytest

from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import signal_batch as SB
from seq2squiggle_amd import utils as U
from _events_ref import parse_events
from test_gpu_events import _run

pytestmark = pytest.mark.gpu

BOUND = 1.01e-4


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("predict_compare")
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("S2S_BLOW5_SIGNAL", "none")
        _run(d / "a.blow5", events=d / "a.events.tsv")
        _run(d / "a.slow5")
        mp.setenv("S2S_BLOW5_SIGNAL", "svb-zd")
        _run(d / "c.blow5")
    finally:
        mp.undo()
    return d


@pytest.mark.parametrize("other", ["a.blow5", "c.blow5", "a.slow5"])
def test_compare_of_a_predicted_file_with_itself(run, other):
    d = run
    a, b, tag = str(d / "a.blow5"), str(d / other), other.replace(".", "_")
    outs, sums = {}, {}
    for mode, cpu in (("gpu", False), ("cpu", True)):
        names = [str(d / f"{tag}.{mode}{ext}") for ext in (".tsv", ".paths.tsv", ".events.tsv")]
        sums[mode] = CMP.compare_files(a, b, names[0], path_out=names[1], events_a=str(d / "a.events.tsv"), events_out=names[2], cpu=cpu)
        outs[mode] = tuple(open(n, "rb").read() for n in names)
    assert outs["gpu"] == outs["cpu"]
    s = sums["gpu"]
    recs_a, recs_b = list(SB.open_records(a)), {r["read_id"]: r for r in SB.open_records(b)}
    assert s["pairs"] == len(recs_a) == len(recs_b) >= 10 and (s["unpaired_a"], s["unpaired_b"]) == (0, 0)
    assert s["events_dropped"] == 0 == s["events_unpaired"] and s["events_written"] > 100
    assert all(np.array_equal(r["signal"], recs_b[r["read_id"]]["signal"]) for r in recs_a)            # the same samples thrice
    # every pair: distance 0, equal median / MAD, the diagonal
    rows = [ln.split("\t") for ln in outs["gpu"][0].decode().splitlines()]
    paths = [ln.split("\t") for ln in outs["gpu"][1].decode().splitlines()]
    assert rows[0] == list(CMP.COLUMNS) and paths[0] == list(CMP.PATH_COLUMNS) and len(rows) == len(paths) == len(recs_a) + 1
    for r, p, rec in zip(rows[1:], paths[1:], recs_a):
        n = len(rec["signal"])
        assert r[:3] == [rec["read_id"], str(n), str(n)] and r[8:] == ["0", "0.000000"], r
        assert (r[3], r[4]) == (r[5], r[6]) and int(r[4]) > 0, r
        assert p == [rec["read_id"], str(n), str(n), str(CMP.DEFAULT_BAND), "0", str(n - 1), f"{n - 1}M"], p[:6]
    # the carried table: predict's own rows, the level shifted by the record's offset against the profile's
    mine = parse_events(open(d / "a.events.tsv", "rb").read(), False)
    got = parse_events(outs["gpu"][2], False)
    key = ("read_name", "position", "model_kmer", "start_idx", "end_idx")
    assert [tuple(r[k] for k in key) for r in got] == [tuple(r[k] for k in key) for r in mine] and len(got) == s["events_written"]
    prof_off = float(U.get_profile("dna-r10-prom")["offset_mean"])
    shift = {i: (float(r["offset"]) - prof_off) * float(r["range"]) / float(r["digitisation"]) for i, r in recs_b.items()}
    assert sum(abs(float(r["offset"]) - prof_off) > 0.5 for r in recs_b.values()) >= 1                  # the term is exercised
    assert max(abs(v) for v in shift.values()) > 100 * BOUND
    for g, m in zip(got, mine):
        assert abs(float(g["stdv"]) - float(m["stdv"])) <= BOUND, (g, m)
        assert abs(float(g["mean"]) - (float(m["mean"]) + shift[g["read_name"]])) <= BOUND, (g, m)
