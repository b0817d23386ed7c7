"""Inputs of s2s_chunk_pack for the tests of `preprocess`: reads with given row lengths, both sample sources, and the edge cases
the issue lists.  A case is a dict of host arrays; `ref` runs the numpy restatement on it, `run` the package (host twin or device)."""
import os

import numpy as np

import _preprocess_ref as R

GEOMETRIES = ((1, 1, 1), (5, 37, 6), (16, 250, 9), (64, 1024, 10))      # (te, ts, k)
CAL = (8192.0, -243.0, 1437.976)
KEYS = ("chunks", "chunks_lengths", "targets", "targets_lengths", "stdevs", "n_rows", "counters")


def sums(case):
    """S, Q of every slot as s2s_event_sums leaves them (0, 0 for a skipped slot or an interval outside the record)."""
    S, Q = np.zeros(len(case["ev_start"]), np.int64), np.zeros(len(case["ev_start"]), np.int64)
    for p, rec in enumerate(case["records"]):
        for g in range(case["l_offs"][p], case["l_offs"][p + 1]):
            st, ln = int(case["ev_start"][g]), int(case["ev_len"][g])
            if st >= 0 and ln > 0 and st + ln <= len(rec):
                x = rec[st:st + ln].astype(np.int64)
                S[g], Q[g] = x.sum(), (x * x).sum()
    case["S"], case["Q"] = S, Q
    return case


def make(rng, k, lens_per_read, letters=b"ACGT", gaps=True, tail=3):
    """Reads whose slots have the given lengths (0: a skipped slot), laid left to right in their records with random gaps."""
    records, start, length, kmers = [], [], [], []
    for lens in lens_per_read:
        lens = np.asarray(lens, np.int64)
        gap = rng.integers(0, 3, len(lens)) if gaps else np.zeros(len(lens), np.int64)
        st = np.cumsum(lens + gap) - lens
        st[lens == 0] = -1
        records.append(rng.integers(-3000, 3000, int((lens + gap).sum()) + tail).astype(np.int16))
        start.append(st)
        length.append(lens)
        kmers.append(rng.choice(np.frombuffer(letters, np.uint8), (len(lens), k)))
    case = dict(records=records, l_offs=np.concatenate([[0], np.cumsum([len(x) for x in length])]).astype(np.int64),
                s_offs=np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.int64),
                ev_start=np.concatenate(start + [np.zeros(0, np.int64)]).astype(np.int32),
                ev_len=np.concatenate(length + [np.zeros(0, np.int64)]).astype(np.int32),
                kmers=np.concatenate(kmers + [np.zeros((0, k), np.uint8)]).astype(np.uint8), k=k,
                cal=np.tile(CAL, (len(records), 1)).reshape(-1))
    case["flat"] = np.concatenate(records + [np.zeros(0, np.int16)])
    case["pool"] = (case["flat"].astype(np.float64) / 7.0).astype(np.float32)
    case["stdv"] = rng.random(len(case["ev_start"])).astype(np.float32)
    return sums(case)


def row_lengths(rng, n, te, ts):
    """n row lengths around ts / te: some chunks pass ts, some do not."""
    return rng.integers(1, max(2, 2 * ts // te + 1), n)


def ref(case, source, te, ts, reverse=False, backwards=False, capacity=None):
    if source == R.RAW:
        return R.pack(case["flat"], case["s_offs"], R.RAW, case["l_offs"], case["ev_start"], case["ev_len"], case["S"], case["Q"],
                      case["cal"], None, case["kmers"], case["k"], te, ts, reverse, backwards, capacity)
    return R.pack(case["pool"], case["s_offs"], R.PA, case["l_offs"], case["ev_start"], case["ev_len"], None, None, None, case["stdv"],
                  case["kmers"], case["k"], te, ts, reverse, backwards, capacity)


def run(case, source, te, ts, reverse=False, backwards=False, cpu=True, **kw):
    from seq2squiggle_amd import preprocess as PP
    if source == R.RAW:
        out = PP.pack(case["l_offs"], case["ev_start"], case["ev_len"], case["kmers"], case["k"], te, ts, records=case["records"],
                      S=case["S"], Q=case["Q"], cal=case["cal"], reverse=reverse, backwards=backwards, cpu=cpu, **kw)
    else:
        out = PP.pack(case["l_offs"], case["ev_start"], case["ev_len"], case["kmers"], case["k"], te, ts, pool=case["pool"],
                      s_offs=case["s_offs"], stdv=case["stdv"], reverse=reverse, backwards=backwards, cpu=cpu, **kw)
    out["chunks"] = out["chunks"].view(np.uint16)
    return out


def same(a, b, what=""):
    for key in KEYS:
        x, y = a[key], b[key]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, key, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.reshape(-1).view(np.uint8 if x.dtype.kind == "f" else x.dtype) !=
                                 y.reshape(-1).view(np.uint8 if y.dtype.kind == "f" else y.dtype))
            raise AssertionError((what, key, "first difference at", int(bad[0]), "of", x.size))


# ------------------------------------------------------------------ the goldens of the reference's own chunk cutting
def golden(te, ts, k):
    """tests/golden/preprocess_<te>x<ts>x<k>.npz (tools/make_goldens.py preprocess): the reference's own functions on a table."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"preprocess_{te}x{ts}x{k}.npz")) as z:
        return {key: z[key] for key in z.files}


def golden_case(g, only=None, as_listed=False):
    """The table of a golden as the arrays of the pa source: the reads in order of first appearance (only: that read alone), the
    rows of a read by position (as_listed: in the order of the table's lines), a row's interval where its samples lie in the pool,
    every text parsed as a double and rounded to fp32.  A parser of its own: nothing of the package reads the table here."""
    k = int(g["geometry"][2])
    reads = {}
    for line in g["table"].tobytes().decode("ascii").split("\n")[1:]:
        if line:
            v = line.split("\t")
            assert int(v[4]) - int(v[3]) == len(v[7].split(",")) and len(v[2]) == k
            reads.setdefault(v[0], []).append((int(v[1]), v[2], np.float32(float(v[6])), [np.float32(float(x)) for x in v[7].split(",")]))
    assert list(reads) == [str(n) for n in g["names"]]
    kmers, lens, stdv, pool, counts = [], [], [], [], []
    for name, rows in reads.items():
        if only is not None and name != only:
            continue
        assert len({r[0] for r in rows}) == len(rows)                        # positions are unique: no tie for any sort to break
        rows = rows if as_listed else sorted(rows, key=lambda r: r[0])
        counts.append(len(rows))
        for _, kmer, dev, x in rows:
            kmers.append(kmer)
            lens.append(len(x))
            stdv.append(dev)
            pool.extend(x)
    lens = np.array(lens, np.int64)
    l_offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dict(k=k, l_offs=l_offs, s_offs=np.concatenate([[0], np.cumsum(lens)])[l_offs].astype(np.int64),
                ev_start=np.concatenate([np.cumsum(r) - r for r in np.split(lens, l_offs[1:-1])]).astype(np.int32), ev_len=lens.astype(np.int32),
                kmers=np.frombuffer("".join(kmers).encode("ascii"), np.uint8).reshape(-1, k).copy(), pool=np.array(pool, np.float32),
                stdv=np.array(stdv, np.float32))


def golden_rows_of(g, name):
    """The rows of the reference's filtered arrays that come from read `name`: its chunks among the unfiltered ones, then the filter."""
    i = [str(n) for n in g["names"]].index(name)
    first = int(g["chunks_per_read"][:i].sum())
    return np.flatnonzero((g["kept"] >= first) & (g["kept"] < first + int(g["chunks_per_read"][i])))


def same_as_golden(g, rna, got, rows=None, what=""):
    """got (the arrays of C.run, or the files of the command) against the reference's arrays, after the documented mechanical mappings
    and nothing else: chunks bit for bit as fp16; the two lengths as integers (the reference: int64 and int16); targets bit for bit;
    stdevs = the reference's float64 [N, 1, 1, te] squeezed and cast to float32."""
    te, ts, k = (int(v) for v in g["geometry"])
    want = {kind: g[("rna_" if rna else "dna_") + kind] for kind in ("chunks", "chunks_lengths", "targets", "targets_lengths", "stdevs")}
    if rows is not None:
        want = {kind: v[rows] for kind, v in want.items()}
    N = len(want["targets_lengths"])
    assert want["chunks"].dtype == np.float16 and want["chunks"].shape == (N, te, k, 5) and want["targets"].dtype == np.float32
    chunks = np.asarray(got["chunks"])
    assert chunks.dtype in (np.float16, np.uint16) and chunks.shape == (N, te, k, 5), (what, chunks.dtype, chunks.shape)
    assert chunks.view(np.uint16).tobytes() == want["chunks"].view(np.uint16).tobytes(), (what, "chunks")
    for kind in ("chunks_lengths", "targets_lengths"):
        assert got[kind].dtype.kind == "i" and want[kind].dtype.kind == "i" and got[kind].shape == want[kind].shape, (what, kind)
        assert np.array_equal(got[kind].astype(np.int64), want[kind].astype(np.int64)), (what, kind)
    assert got["targets"].dtype == np.float32 and got["targets"].shape == (N, ts) == want["targets"].shape, (what, "targets")
    assert got["targets"].tobytes() == want["targets"].tobytes(), (what, "targets")
    dev = want["stdevs"].reshape(N, te).astype(np.float32)
    assert got["stdevs"].dtype == np.float32 and got["stdevs"].shape == (N, te) and got["stdevs"].tobytes() == dev.tobytes(), (what, "stdevs")
    return N


def command(g, outdir, rna, cpu):
    """`preprocess TABLE OUTDIR` on the golden's table text -> (the arrays of the files written, the JSON summary)."""
    import json

    from click.testing import CliRunner

    from seq2squiggle_amd import cli, evaluate
    te, ts, k = (int(v) for v in g["geometry"])
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(str(outdir), "events.tsv")
    with open(path, "wb") as f:
        f.write(g["table"].tobytes())
    args = ["preprocess", path, os.path.join(str(outdir), "out"), "--seq-kmer", k, "--max-dna-len", te, "--max-signal-len", ts, "--json"]
    r = CliRunner().invoke(cli.main, [str(a) for a in args + (["--rna"] if rna else []) + (["--cpu"] if cpu else [])], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    files = evaluate.discover(os.path.join(str(outdir), "out"))
    return ({kind: np.concatenate([np.load(f[kind]) for f in files]) for kind in evaluate.KINDS}, json.loads(r.output.strip().splitlines()[-1]))


def standard(te, ts, k, seed=0):
    """The six row counts of the issue in one batch, N letters among the k-mers (none all N: every slot is a row)."""
    rng = np.random.default_rng([seed, te, ts, k])
    case = make(rng, k, [row_lengths(rng, n, te, ts) for n in (0, 1, te - 1, te, te + 1, 3 * te)], letters=b"ACGTN")
    case["kmers"][(case["kmers"] == ord("N")).all(axis=1), 0] = ord("A")
    return case


MANY_READS = tuple((P, te, ts, k) for P in (1025, 2049) for te, ts, k in GEOMETRIES[:2])


def many_reads(P, te, ts, k, seed=8):
    """P reads of one or two rows each: more reads than one and than two steps of the scan hold, and at te = 1, where every read forms
    two chunks or three, more than two and than four steps of chunks."""
    rng = np.random.default_rng([seed, P, te, ts, k])
    return make(rng, k, [row_lengths(rng, n, te, ts) for n in rng.integers(1, 3, P)])


def edges(te, ts, k, seed=1):
    """-> {name: case}: the specific cases of the issue at one geometry."""
    rng = np.random.default_rng([seed, te, ts, k])
    out = {}
    even = np.full(te, ts // te)
    even[:ts - even.sum()] += 1                     # te lengths that sum to ts (ts >= te at every geometry in use)
    over = even.copy()
    over[-1] += 1
    out["exactly_ts_and_one_more"] = make(rng, k, [even, over, even])
    out["row_longer_than_ts"] = make(rng, k, [[1, ts + 1, 1], [1] * te])
    out["row_longer_than_int16"] = make(rng, k, [[1, 40000, 1], [1] * (te + 1), [33000] * min(te, 4)])
    out["skipped_slots"] = make(rng, k, [[1, 0, 2, 0, 0, 1] * te, [0] * 5, [0, 1]])
    c = make(rng, k, [[2, 1, 2, 1, 1], [1] * (2 * te)], tail=0, gaps=False)
    c["ev_start"][1] = -1                           # before the record
    c["ev_start"][4] += 1                           # its last sample would lie behind the record's end
    c["ev_start"][5 + te] = 1 << 30
    out["interval_outside"] = sums(c)
    c = make(rng, k, [[1] * (te + 2), [2] * 3])
    c["kmers"][0] = ord("N")                        # all N: dropped
    c["kmers"][2] = ord("N")
    c["kmers"][2, 0] = ord("A")                     # k - 1 N: kept (at k = 1 no N is left)
    c["kmers"][3, k - 1] = ord("N")                 # one N: kept, that letter's one-hot row all zero (at k = 1 it is all N: dropped)
    c["kmers"][te + 3] = ord("N")
    out["n_letters"] = c
    # (at te = 1 a read with rows always keeps its chunk of pads: there only a batch without rows keeps nothing)
    out["keeps_nothing"] = make(rng, k, [[ts + 1] * 3, [ts] * (te + 1)] if te > 3 else [[0, 0, 0]])
    out["no_rows"] = make(rng, k, [[0, 0], []])
    return out
