"""`preprocess` on the host: s2s_chunk_pack_host against the numpy restatement of the definition (tests/_preprocess_ref.py), byte for
byte, at four geometries, the six row counts and the edge cases of tests/_preprocess_cases.py; then the commands with --cpu: the files
do not depend on batching or on --chunks-per-file, --max-chunks, the table reader's errors, `resquiggle --cpu --chunks` against
`resquiggle --cpu --samples` -> `preprocess --cpu` on planted reads, and evaluate.EvalData opens every directory written."""
import json
import os

import numpy as np
import pytest
from click.testing import CliRunner

import _preprocess_cases as CS
import _preprocess_ref as R
from seq2squiggle_amd import _lib, cli, evaluate
from seq2squiggle_amd import preprocess as PP
from test_resquiggle_cpu import K3, files  # noqa: F401  (the planted reads of `resquiggle`, their model and files)


# ------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("te,ts,k", CS.GEOMETRIES)
def test_host_twin_equals_the_restatement_on_the_standard_batch(te, ts, k):
    case = CS.standard(te, ts, k)
    assert [len(r) for r in np.split(case["ev_len"], case["l_offs"][1:-1])] == [0, 1, te - 1, te, te + 1, 3 * te]
    for source in (R.RAW, R.PA):
        for reverse in (False, True):
            for backwards in (False, True):
                want = CS.ref(case, source, te, ts, reverse, backwards)
                CS.same(want, CS.run(case, source, te, ts, reverse, backwards), (source, reverse, backwards))
    assert want["n_rows"].tolist() == [0, 1, te - 1, te, te + 1, 3 * te] and want["counters"][0] == sum(n // te + 1 for n in want["n_rows"] if n)
    # one thread and many give the same bytes
    CS.same(CS.run(case, R.RAW, te, ts, threads=1), CS.run(case, R.RAW, te, ts, threads=7))


@pytest.mark.parametrize("te,ts,k", CS.GEOMETRIES)
def test_host_twin_equals_the_restatement_on_the_edge_cases(te, ts, k):
    got = {}
    for name, case in CS.edges(te, ts, k).items():
        for source in (R.RAW, R.PA):
            want = CS.ref(case, source, te, ts, reverse=(source == R.PA))
            got[name] = CS.run(case, source, te, ts, reverse=(source == R.PA))
            CS.same(want, got[name], (name, source))
    r = got["exactly_ts_and_one_more"]              # three reads of te rows: ts samples, ts + 1, ts; each followed by a chunk of pads
    assert r["counters"].tolist() == [6, 5, 0] and r["targets_lengths"].tolist() == [ts, te, te, ts, te]
    r = got["row_longer_than_ts"]
    assert r["counters"][0] - r["counters"][1] == 1 and (r["targets_lengths"] <= ts).all()
    r = got["row_longer_than_int16"]                # the chunks with rows of 40,000 and 33,000 samples are dropped, none wraps into range
    assert r["counters"][0] - r["counters"][1] == 2
    assert (r["targets_lengths"] <= ts).all() and r["n_rows"].tolist() == [3, te + 1, min(te, 4)]
    assert got["skipped_slots"]["n_rows"].tolist() == [3 * te, 0, 1]
    assert got["interval_outside"]["n_rows"].tolist() == [3, 2 * te - 1]
    r = got["n_letters"]
    if k > 1:
        assert r["n_rows"].tolist() == [te + 1, 2] and r["counters"][2] == 2
        hot = r["chunks"][0]                        # rows 1.. of the read: the k-mer with one letter, then the one with one N
        assert (hot[1, 1:] == 0).all() and hot[1, 0, 1] == 0x3C00 and (hot[2, k - 1] == 0).all() and hot[2, :k - 1].sum() == (k - 1) * 0x3C00
    else:
        assert r["n_rows"].tolist() == [te + 1, 1] and r["counters"][2] == 3
    for name in ("keeps_nothing", "no_rows"):
        assert got[name]["counters"][1] == 0 and got[name]["targets"].shape == (0, ts) and got[name]["chunks"].shape == (0, te, k, 5)
    assert got["no_rows"]["counters"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("P,te,ts,k", CS.MANY_READS)
def test_host_twin_equals_the_restatement_on_many_short_reads(P, te, ts, k):
    """The inputs on which tests/test_gpu_preprocess.py takes the device's scans over reads and capacity past one and two steps: the
    host twin that the device is held to there is held to the numpy restatement here."""
    case = CS.many_reads(P, te, ts, k)
    assert len(case["l_offs"]) == P + 1 and set(np.diff(case["l_offs"]).tolist()) == {1, 2}
    for source in (R.RAW, R.PA):
        want = CS.ref(case, source, te, ts, reverse=(source == R.PA))
        CS.same(want, CS.run(case, source, te, ts, reverse=(source == R.PA)), (P, source))
    assert want["counters"][0] == sum(n // te + 1 for n in want["n_rows"] if n) >= (2 * P if te == 1 else P)


def test_pad_rows_and_true_lengths():
    rng = np.random.default_rng(2)
    case = CS.make(rng, 6, [[3, 4, 5, 6, 7], [2]], gaps=False)      # n = te: a whole chunk of pads follows
    r = CS.run(case, R.RAW, 5, 37)
    assert r["targets_lengths"].tolist() == [25, 5, 6] and r["chunks_lengths"].tolist() == [[3, 4, 5, 6, 7], [1] * 5, [2, 1, 1, 1, 1]]
    assert (r["chunks"][1] == np.array([0x3C00, 0, 0, 0, 0], np.uint16)).all() and (r["targets"][1] == 0).all()
    assert (r["stdevs"][1] == 0).all() and (r["stdevs"][2][1:] == 0).all() and r["stdevs"][0].min() > 0
    x = case["records"][0][:25].astype(np.float64)
    dig, off, rng_ = CS.CAL
    assert r["targets"][0][:25].tolist() == ((x + off) * rng_ / dig).astype(np.float32).tolist() and (r["targets"][0][25:] == 0).all()
    back = CS.run(case, R.RAW, 5, 37, reverse=True)
    assert back["targets"][0][:3].tolist() == r["targets"][0][:3][::-1].tolist()
    assert back["targets"][0][3:7].tolist() == r["targets"][0][3:7][::-1].tolist()
    flip = CS.run(case, R.RAW, 5, 37, backwards=True)
    assert flip["chunks_lengths"][0].tolist() == [7, 6, 5, 4, 3] and flip["targets"][0][:7].tolist() == r["targets"][0][18:25].tolist()


def test_refusals():
    L = _lib.lib()
    case = CS.make(np.random.default_rng(3), 6, [[3, 4], [2]])
    P, slots, total = 2, 3, len(case["flat"])
    out = dict(chunks=np.zeros(4 * 5 * 6 * 5, np.uint16), cl=np.zeros(4 * 5, np.int64), tg=np.zeros(4 * 37, np.float32),
               tl=np.zeros(4, np.int64), sd=np.zeros(4 * 5, np.float32), n=np.zeros(2, np.int32), cnt=np.zeros(3, np.int64))
    p = lambda a: a.ctypes.data                     # noqa: E731

    def call(source=0, k=6, te=5, ts=37, cap=4, threads=1, l_offs=case["l_offs"], s_offs=case["s_offs"], total=total, slots=slots,
             cal=case["cal"], P=P):
        keep = [np.ascontiguousarray(x) for x in (l_offs, s_offs, cal)]
        return L.s2s_chunk_pack_host(p(case["flat"]), p(keep[1]), total, source, p(keep[0]), slots, p(case["ev_start"]), p(case["ev_len"]),
                                     p(case["S"]), p(case["Q"]), p(keep[2]), None, p(case["kmers"]), P, k, te, ts, 0, 0, cap, p(out["chunks"]),
                                     p(out["cl"]), p(out["tg"]), p(out["tl"]), p(out["sd"]), p(out["n"]), p(out["cnt"]), threads)
    assert call() == 0 and out["cnt"].tolist() == [2, 2, 0]
    for bad in (dict(k=0), dict(k=11), dict(te=0), dict(te=65), dict(ts=0), dict(ts=1025), dict(source=2), dict(threads=0), dict(cap=1),
                dict(P=-1), dict(total=total - 1), dict(slots=slots + 1), dict(l_offs=np.array([0, 3, 2], np.int64)),
                dict(s_offs=case["s_offs"][::-1]), dict(cal=np.array([0.0, 1, 1, 1, 1, 1])), dict(cal=np.array([1.0, np.nan, 1, 1, 1, 1]))):
        assert call(**bad) == -1, bad
    assert call(source=1) == -1                     # the pa source without its deviations
    assert L.s2s_chunk_pack(0, None, None, None, 0, 0, None, 0, *[None] * 7, 0, 0, 5, 37, 0, 0, 0, *[None] * 8) == -1      # nothing is launched
    assert L.s2s_chunk_scratch_bytes(-1, 0, 0) == -1 and L.s2s_chunk_scratch_bytes(1 << 31, 1, 1) == -1
    assert L.s2s_chunk_scratch_bytes(0, (1 << 22) + 1, 1 << 23) == -1 and L.s2s_chunk_scratch_bytes(5000, 3, 400) > 5000 * 4
    with pytest.raises(ValueError):
        PP.check_geometry(9, 65, 250)
    assert PP.capacity([0, 15, 16, 17], 16) == 1 + 1 + 2 + 2


# ------------------------------------------------------------------ the writer and the table
def load_dir(d):
    return {kind: [np.load(f[kind]) for f in evaluate.discover(str(d))] for kind in evaluate.KINDS}


def whole(d):
    return {kind: np.concatenate(v) for kind, v in load_dir(d).items()}


def same_dirs(a, b):
    wa, wb = whole(a), whole(b)
    for kind in evaluate.KINDS:
        assert wa[kind].dtype == wb[kind].dtype and wa[kind].shape == wb[kind].shape and wa[kind].tobytes() == wb[kind].tobytes(), kind


def opens(d, k, te, ts):
    data = evaluate.EvalData(str(d), dict(seq_kmer=k, max_dna_len=te, max_signal_len=ts, scaling_max_value=165.0))
    return sum(len(np.load(f["targets_lengths"])) for f in data.files)


def table_text(reads, k, with_samples=True, rng=None):
    """An event table of given reads {name: [(position, kmer, start, [samples], stdv)]}, rows of different reads interleaved."""
    lines = ["read_name\tposition\tmodel_kmer\tstart_idx\tend_idx\tevent_level_mean\tevent_stdv" + ("\tsamples" if with_samples else "")]
    rows = [(name, r) for name, rs in reads.items() for r in rs]
    for name, (pos, kmer, start, x, dev) in rows:
        row = f"{name}\t{pos}\t{kmer}\t{start}\t{start + len(x)}\t{np.mean(x) if len(x) else 0:.4f}\t{dev:.4f}"
        lines.append(row + ("\t" + ",".join("%.3f" % v for v in x) if with_samples else ""))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("preprocess")
    rng = np.random.default_rng(21)
    reads = {}
    for i, n in enumerate((7, 0, 23, 5, 16, 1)):
        rows, at = [], 0
        for pos in range(n):
            x = rng.normal(90, 12, rng.integers(1, 13))
            kmer = "".join(rng.choice(list("ACGTN"), 4))
            rows.append((pos, kmer, at, x, float(rng.random())))
            at += len(x)
        reads[f"read{i}"] = [rows[j] for j in rng.permutation(n)]               # positions out of order inside a read
    (d / "e.tsv").write_text(table_text(reads, 4))
    return d, reads


def restated(reads, k, te, ts, rna=False):
    """The table's chunks by the restatement: reads in order of first appearance, rows by position, text -> double -> fp32."""
    names = [n for n, rs in reads.items() if rs]
    rows = {n: sorted(reads[n], key=lambda r: r[0]) for n in names}
    fl = lambda text: np.float32(float(text))       # noqa: E731
    pool = np.array([fl("%.3f" % v) for n in names for r in rows[n] for v in r[3]], np.float32)
    lens = [np.array([len(r[3]) for r in rows[n]], np.int64) for n in names]
    return R.pack(pool, np.concatenate([[0], np.cumsum([l.sum() for l in lens])]), R.PA,
                  np.concatenate([[0], np.cumsum([len(l) for l in lens])]), np.concatenate([np.cumsum(l) - l for l in lens]),
                  np.concatenate(lens), None, None, None, np.array([fl("%.4f" % r[4]) for n in names for r in rows[n]], np.float32),
                  np.frombuffer("".join(r[1] for n in names for r in rows[n]).encode(), np.uint8), k, te, ts, rna, False)


def run(*args):
    return CliRunner().invoke(cli.main, [str(a) for a in args], catch_exceptions=False)


def test_command_equals_the_restatement_whatever_the_batching(table):
    d, reads = table
    geometry = ("--seq-kmer", 4, "--max-dna-len", 5, "--max-signal-len", 37)
    r = run("preprocess", d / "e.tsv", d / "all", *geometry, "--cpu", "--json")
    assert r.exit_code == 0, r.output
    s = json.loads(r.output.strip().splitlines()[-1])
    want = restated(reads, 4, 5, 37)
    got = whole(d / "all")
    assert got["chunks"].dtype == np.float16 and got["chunks"].shape == (len(want["targets"]), 5, 4, 5)
    assert got["stdevs"].dtype == np.float32 and got["stdevs"].shape == (len(want["targets"]), 5)       # [N, te], not the reference's [N, 1, 1, te]
    assert got["targets_lengths"].dtype == np.int64 and got["chunks_lengths"].dtype == np.int64
    for kind in evaluate.KINDS:
        assert got[kind].view(want[kind].dtype).tobytes() == want[kind].tobytes(), kind
    n = want["n_rows"]
    assert (s["reads"], s["rows"], s["all_n_rows"]) == (5, int(n.sum()), int(want["counters"][2]))
    assert (s["chunks_formed"], s["chunks_kept"], s["chunks_too_long"]) == (want["counters"][0], want["counters"][1],
                                                                            want["counters"][0] - want["counters"][1])
    assert s["pad_rows"] == sum(5 - v % 5 for v in n if v) and s["files"] == 1 and s["chunks_written"] == want["counters"][1]
    assert 0 < s["chunks_too_long"] < s["chunks_formed"]
    assert opens(d / "all", 4, 5, 37) == want["counters"][1]
    # one record per batch; three values of --chunks-per-file, one of them 1
    r = run("preprocess", d / "e.tsv", d / "one", *geometry, "--cpu", "--max-samples", 1)
    assert r.exit_code == 0, r.output
    same_dirs(d / "all", d / "one")
    assert [len(os.listdir(d / x)) for x in ("all", "one")] == [5, 5]
    for per, where in ((1, "per1"), (3, "per3"), (1000, "per1000")):
        r = run("preprocess", d / "e.tsv", d / where, *geometry, "--cpu", "--chunks-per-file", per, "--max-samples", 40, "--json")
        assert r.exit_code == 0, r.output
        same_dirs(d / "all", d / where)
        files_ = load_dir(d / where)["targets_lengths"]
        N = int(want["counters"][1])
        assert [len(f) for f in files_] == [per] * (N // per) + ([N % per] if N % per else [])
        assert json.loads(r.output.strip().splitlines()[-1])["files"] == len(files_) and opens(d / where, 4, 5, 37) == N
    # --rna reads every row back to front
    r = run("preprocess", d / "e.tsv", d / "rna", *geometry, "--cpu", "--rna")
    assert r.exit_code == 0, r.output
    assert whole(d / "rna")["targets"].tobytes() == restated(reads, 4, 5, 37, rna=True)["targets"].tobytes()
    assert whole(d / "rna")["targets"].tobytes() != got["targets"].tobytes()


def test_command_max_chunks(table):
    d, reads = table
    geometry = ("--seq-kmer", 4, "--max-dna-len", 5, "--max-signal-len", 37)
    want = restated(reads, 4, 5, 37)
    for m, batch in ((4, 1 << 27), (4, 1), (0, 1 << 27)):
        where = d / f"max{m}_{batch}"
        r = run("preprocess", d / "e.tsv", where, *geometry, "--cpu", "--max-chunks", m, "--max-samples", batch, "--chunks-per-file", 3)
        assert r.exit_code == 0, r.output
        got = whole(where)
        for kind in evaluate.KINDS:
            assert got[kind].view(want[kind].dtype).tobytes() == want[kind][:m].tobytes(), (kind, m)
        assert opens(where, 4, 5, 37) == m


def test_table_reader_errors(table, tmp_path):
    d, reads = table
    (tmp_path / "no_samples.tsv").write_text(table_text(reads, 4, with_samples=False))
    r = run("preprocess", tmp_path / "no_samples.tsv", tmp_path / "o", "--seq-kmer", 4, "--cpu")
    assert r.exit_code != 0 and "line 1" in r.output and "samples" in r.output and "--events-samples" in r.output
    lines = table_text(reads, 4).splitlines()
    v = lines[7].split("\t")
    v[-1] += ",1.000"
    (tmp_path / "count.tsv").write_text("\n".join(lines[:7] + ["\t".join(v)] + lines[8:]) + "\n")
    r = run("preprocess", tmp_path / "count.tsv", tmp_path / "o", "--seq-kmer", 4, "--cpu")
    assert r.exit_code != 0 and "line 8" in r.output and "sample" in r.output
    v = lines[3].split("\t")
    (tmp_path / "text.tsv").write_text("\n".join(lines[:3] + ["\t".join(v[:-1] + ["x" + v[-1]])] + lines[4:]) + "\n")
    r = run("preprocess", tmp_path / "text.tsv", tmp_path / "o", "--seq-kmer", 4, "--cpu")
    assert r.exit_code != 0 and "line 4" in r.output
    r = run("preprocess", d / "e.tsv", tmp_path / "o", "--seq-kmer", 5, "--cpu")
    assert r.exit_code != 0 and "line 2" in r.output and "seq_kmer" in r.output
    r = run("preprocess", d / "e.tsv", tmp_path / "o", "--max-dna-len", 65, "--cpu")
    assert r.exit_code != 0 and "--max-dna-len" in r.output
    assert not (tmp_path / "o").exists() or not os.listdir(tmp_path / "o")


# ------------------------------------------------------------------ resquiggle --chunks against the text round trip
@pytest.mark.parametrize("rna", (False, True))
def test_resquiggle_chunks_against_samples_then_preprocess(files, rna):  # noqa: F811
    d, blow5, slow5, reads, cal, adc = files
    tag = "rna" if rna else "dna"
    geometry = ("--seq-kmer", K3, "--max-dna-len", 5, "--max-signal-len", 48)
    more = ("--rna",) if rna else ()
    r = run("resquiggle", d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / f"c_{tag}.tsv", "--cpu", "--samples", "--json",
            "--chunks", d / f"direct_{tag}", *geometry, *more)
    assert r.exit_code == 0, r.output
    s = json.loads(r.output.strip().splitlines()[-1])
    r = run("preprocess", d / f"c_{tag}.tsv", d / f"text_{tag}", *geometry, "--cpu", "--json", *more)
    assert r.exit_code == 0, r.output
    t = json.loads(r.output.strip().splitlines()[-1])
    a, b = whole(d / f"direct_{tag}"), whole(d / f"text_{tag}")
    assert s["chunks"]["reads"] == 4 and s["chunks"]["rows"] == s["events"] == t["rows"]        # (the table has no row for the orphan)
    assert 0 < s["chunks"]["chunks_kept"] < s["chunks"]["chunks_formed"] and s["chunks"]["chunks_kept"] == t["chunks_kept"] == len(a["targets"])
    for kind in ("chunks", "chunks_lengths", "targets_lengths"):
        assert a[kind].dtype == b[kind].dtype and a[kind].tobytes() == b[kind].tobytes(), kind
    va, vb = a["targets"].astype(np.float64), b["targets"].astype(np.float64)
    assert (np.abs(va - vb) <= 5.0e-4 + 2.0 ** -23 * np.abs(va)).all(), np.abs(va - vb).max()       # the table's %.3f and one fp32 rounding
    va, vb = a["stdevs"].astype(np.float64), b["stdevs"].astype(np.float64)
    assert (np.abs(va - vb) <= 5.0e-5 + 2.0 ** -23 * np.abs(va)).all(), np.abs(va - vb).max()       # its %.4f
    assert np.abs(a["targets"]).max() > 10 and opens(d / f"direct_{tag}", K3, 5, 48) == opens(d / f"text_{tag}", K3, 5, 48) == len(a["targets"])
    # without the option the table is the same bytes
    r = run("resquiggle", d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / f"p_{tag}.tsv", "--cpu", "--samples", *more)
    assert r.exit_code == 0 and (d / f"p_{tag}.tsv").read_bytes() == (d / f"c_{tag}.tsv").read_bytes()
    # a batch per read writes the same files
    r = run("resquiggle", d / "r.fasta", slow5, "--kmer-model", d / "m.model", "-o", d / f"q_{tag}.tsv", "--cpu", "--max-samples", 1,
            "--chunks", d / f"direct1_{tag}", *geometry, *more)
    assert r.exit_code == 0, r.output
    same_dirs(d / f"direct_{tag}", d / f"direct1_{tag}")
    r = run("resquiggle", d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "x.tsv", "--cpu", "--chunks", d / "x", "--seq-kmer", 4)
    assert r.exit_code != 0 and "--seq-kmer" in r.output


def test_eventalign_chunks_open(files):  # noqa: F811
    d, blow5, slow5, reads, cal, adc = files
    geometry = ("--seq-kmer", K3, "--max-dna-len", 5, "--max-signal-len", 48)
    r = run("eventalign", d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "ea.tsv", "--cpu", "--samples", "--json",
            "--chunks", d / "ea_direct", *geometry)
    assert r.exit_code == 0, r.output
    s = json.loads(r.output.strip().splitlines()[-1])
    r = run("preprocess", d / "ea.tsv", d / "ea_text", *geometry, "--cpu", "--json")
    assert r.exit_code == 0, r.output
    a, b = whole(d / "ea_direct"), whole(d / "ea_text")
    assert s["chunks"]["rows"] == s["events"] and len(a["targets"]) == s["chunks"]["chunks_kept"] > 0
    for kind in ("chunks", "chunks_lengths", "targets_lengths"):
        assert a[kind].tobytes() == b[kind].tobytes(), kind
    assert opens(d / "ea_direct", K3, 5, 48) == len(a["targets"])


def test_eventalign_chunks_seq_kmer_mismatch_is_a_usage_error(files):  # noqa: F811
    d, blow5, slow5, reads, cal, adc = files
    args = ("eventalign", d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "y.tsv", "--cpu", "--chunks", d / "y", "--seq-kmer", 4)
    r = CliRunner().invoke(cli.main, [str(a) for a in args])             # (exceptions caught: a NameError would show as r.exception)
    assert r.exit_code != 0 and "--seq-kmer" in r.output and "Traceback" not in r.output
    assert isinstance(r.exception, SystemExit), repr(r.exception)
