"""`eventalign` on the host: the twins s2s_event_means_host and s2s_eventalign_host against the restatement of their definitions in
Python integers (tests/_eventalign_ref.py), the consequences include/s2s_hip.h holds a solved read to, planted reads with junk at
both ends through the whole chain segment -> sums -> means -> normalise -> align, and the command with --cpu."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

import _eventalign_ref as REF
from _events_ref import parse_events
from seq2squiggle_amd import _lib, cli, kmer_model
from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import eventalign as EA
from seq2squiggle_amd import resquiggle as RSQ
from seq2squiggle_amd import signal_batch as SB
from test_compare_cpu import write_file
from test_resquiggle_cpu import K3, model_counts

SKIP, TRIM, UNK = REF.SKIP_PENALTY, REF.TRIM_PENALTY, REF.UNKNOWN_COST
SEG = (3, 6, 501, 20736)                                # the defaults of `segment`: floor(256 t^2) of 1.4 and 9.0
ERR_ARG = -1


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def pooled(arrs, dtype):
    return np.concatenate([np.ascontiguousarray(a, dtype).reshape(-1) for a in arrs] + [np.zeros(0, dtype)])


def pack_reads(reads):
    """reads: [(m, l)] or [(m, l, ev_start, ev_len)] -> the pooled arrays the entries take (events default to one sample each)."""
    ms = [np.asarray(r[0], np.int16) for r in reads]
    ls = [np.asarray(r[1], np.int16) for r in reads]
    st = [np.asarray(r[2], np.int32) if len(r) > 2 else np.arange(len(r[0]), dtype=np.int32) for r in reads]
    ln = [np.asarray(r[3], np.int32) if len(r) > 2 else np.ones(len(r[0]), np.int32) for r in reads]
    m_offs, l_offs = offsets([len(x) for x in ms]), offsets([len(x) for x in ls])
    return dict(m=pooled(ms, np.int16), m_offs=m_offs, l=pooled(ls, np.int16), l_offs=l_offs, st=pooled(st, np.int32),
                ln=pooled(ln, np.int32), ev_offs=m_offs.copy())


def host(reads, W, skip=SKIP, trim=TRIM, unk=UNK, threads=1):
    """s2s_eventalign_host -> (rc, [dict like REF.solve's per read])."""
    P = len(reads)
    a = pack_reads(reads)
    ET, KT = int(a["m_offs"][-1]), int(a["l_offs"][-1])
    cost, first, end = np.full(P, 77, np.int64), np.full(P, 77, np.int32), np.full(P, 77, np.int32)
    kmer, ks, kl, ke = (np.full(n, 77, np.int32) for n in (ET, KT, KT, KT))
    p = lambda x: x.ctypes.data                         # noqa: E731
    rc = _lib.lib().s2s_eventalign_host(p(a["m"]), p(a["m_offs"]), p(a["l"]), p(a["l_offs"]), p(a["st"]), p(a["ln"]), p(a["ev_offs"]), P, W,
                                        skip, trim, unk, p(cost), p(first), p(end), p(kmer), p(ks), p(kl), p(ke), threads)
    mo, lo = a["m_offs"], a["l_offs"]
    return rc, [dict(cost=int(cost[i]), first=int(first[i]), end=int(end[i]), kmer=kmer[mo[i]:mo[i + 1]].tolist(),
                     k_start=ks[lo[i]:lo[i + 1]].tolist(), k_len=kl[lo[i]:lo[i + 1]].tolist(), k_events=ke[lo[i]:lo[i + 1]].tolist())
                for i in range(P)]


def ref(read, W, skip=SKIP, trim=TRIM, unk=UNK):
    return REF.solve(read[0], read[1], W, skip, trim, unk, *(read[2:4] if len(read) > 2 else ()))


def same(got, want):
    return all(got[k] == want[k] for k in ("cost", "first", "end", "kmer", "k_start", "k_len", "k_events"))


def check(reads, W, skip=SKIP, trim=TRIM, unk=UNK, threads=1):
    """The host twin equals the restatement on every read, and every solved read keeps the consequences -> the results."""
    rc, got = host(reads, W, skip, trim, unk, threads)
    assert rc == 0
    for i, (read, g) in enumerate(zip(reads, got)):
        want = ref(read, W, skip, trim, unk)
        assert same(g, want), (i, len(read[0]), len(read[1]), W, g["cost"], want["cost"])
        if g["cost"] >= 0:
            REF.check_consequences(read[0], read[1], skip, trim, unk, g, *(read[2:4] if len(read) > 2 else ()))
    return got


# ------------------------------------------------------------------ event means
def means_host(S, ev_len, ev_offs, n_events, capacity=None, threads=1):
    S, ev_len = np.ascontiguousarray(S, np.int64), np.ascontiguousarray(ev_len, np.int32)
    ev_offs, n_events = np.ascontiguousarray(ev_offs, np.int64), np.ascontiguousarray(n_events, np.int32)
    R = len(n_events)
    capacity = int(ev_offs[-1]) if capacity is None else capacity
    m_offs, means = np.full(R + 1, 77, np.int64), np.full(max(capacity, 1), 77, np.int16)
    rc = _lib.lib().s2s_event_means_host(S.ctypes.data, ev_len.ctypes.data, ev_offs.ctypes.data, n_events.ctypes.data, R, capacity,
                                         m_offs.ctypes.data, means.ctypes.data, threads)
    return rc, m_offs, means


MEAN_CASES = [(5, 2), (7, 2), (-5, 2), (-7, 2), (3, 2), (-3, 2), (1, 2), (-1, 2), (0, 3), (10, 4), (-10, 4), (14, 4), (-14, 4), (7, 3),
              (-7, 3), (32767, 1), (-32768, 1), (-32768 * 9, 9), (32767 * 1000, 1000), (123, 1), (-1, 3), (1, 3), (2, 3), (-2, 3)]


def test_round_half_even_of_the_restatement():
    got = [REF.round_half_even_div(S, n) for S, n in MEAN_CASES[:8]]
    assert got == [2, 4, -2, -4, 2, -2, 0, 0]           # 2.5, 3.5, -2.5, -3.5, 1.5, -1.5, 0.5, -0.5
    for S, n in MEAN_CASES:
        assert REF.round_half_even_div(S, n) == int(np.rint(S / n))


def test_event_means_host_ties_and_record_kinds():
    S, n = [c[0] for c in MEAN_CASES], [c[1] for c in MEAN_CASES]
    # records: all cases; 0 events; -3 (a slot that was too small); too long; one event of one sample; the cases again
    caps = [len(S), 4, 3, 2, 1, len(S)]
    n_events = [len(S), 0, -3, REF.TOO_LONG, 1, len(S)]
    ev_offs = offsets(caps)
    slots_S, slots_n = np.full(ev_offs[-1], 99, np.int64), np.full(ev_offs[-1], 5, np.int32)
    for r in (0, 5):
        slots_S[ev_offs[r]:ev_offs[r] + len(S)], slots_n[ev_offs[r]:ev_offs[r] + len(S)] = S, n
    slots_S[ev_offs[4]], slots_n[ev_offs[4]] = -17, 1
    rc, m_offs, means = means_host(slots_S, slots_n, ev_offs, n_events, threads=3)
    want_offs, want = REF.event_means(slots_S, slots_n, ev_offs, n_events)
    assert rc == 0 and m_offs.tolist() == want_offs == [0, len(S), len(S), len(S), len(S), len(S) + 1, 2 * len(S) + 1]
    assert means[:m_offs[-1]].tolist() == want and (means[m_offs[-1]:] == 77).all()
    assert means[len(S)] == -17 and want[:8] == [2, 4, -2, -4, 2, -2, 0, 0]
    # no records; a pool that is too small; a count beyond its slot counts as none
    rc, m_offs, _ = means_host([], [], [0], [])
    assert rc == 0 and m_offs.tolist() == [0]
    assert means_host(slots_S, slots_n, ev_offs, n_events, capacity=2 * len(S))[0] == ERR_ARG
    rc, m_offs, _ = means_host([4, 4], [2, 2], [0, 1, 2], [2, 1])
    assert rc == 0 and m_offs.tolist() == [0, 0, 1]


# ------------------------------------------------------------------ the alignment against the restatement
def zeros(E, K):
    return np.zeros(E, np.int16), np.zeros(K, np.int16)


EDGE_SHAPES = [(E, K) for E in range(4) for K in range(4)] + [(1, 1000), (1000, 1), (20, 25), (31, 33), (40, 90), (90, 40), (70, 70)]


@pytest.mark.parametrize("W", (64, 128, 192))
def test_host_twin_equals_the_restatement_on_edge_shapes(W):
    reads = [REF.random_case(E, K, kind, seed=W) for E, K in EDGE_SHAPES for kind in ("noisy", "zeros", "unknown", "extreme")]
    got = check(reads, W, threads=4)
    assert [g["cost"] for g, r in zip(got, reads) if 0 in (len(r[0]), len(r[1]))] == [REF.EMPTY] * 28
    assert all(g["cost"] >= 0 for g, r in zip(got, reads) if len(r[0]) in (1, 2, 3) and len(r[1]) in (1, 2, 3))


def test_all_zero_reads_follow_every_tie_rule():
    """Every cell cost ties: diag wins over stay over skip, the band's tie moves down, and what that gives is what the restatement says.
    For 100 events against 1,000 k-mers that is a solved read: the band runs down the event axis while its lower end is reached and its
    upper end is not, and right along the last event once the lower end has left the matrix -- 900 k-mers skipped, the optimum."""
    got = check([zeros(100, 1000), zeros(1000, 100), zeros(100, 100), zeros(5, 40)], 64, skip=0, trim=0)
    assert [g["cost"] for g in got] == [0, 0, 0, 0]
    for W in (64, 128):
        got = check([zeros(100, 1000), zeros(1000, 100), zeros(30, 31)], W)
        assert [g["cost"] for g in got] == [900 * SKIP, 0, SKIP] and got[0]["k_events"].count(0) == 900


@pytest.mark.parametrize("skip,trim,unk", [(0, 0, 0), (1 << 20, 1 << 20, 65535), (0, 1 << 20, 64), (1 << 20, 0, 0)])
def test_penalties_at_their_limits(skip, trim, unk):
    reads = [REF.random_case(E, K, kind, seed=5) for E, K in ((3, 3), (40, 30), (30, 40), (120, 90)) for kind in ("noisy", "unknown", "extreme")]
    check(reads, 64, skip, trim, unk)


def random_shapes():
    rng = np.random.default_rng(2024)
    dims = np.exp(rng.uniform(0, np.log(400), (200, 2))).astype(int)            # up to 400 x 400, small ones as likely as large ones
    dims[:6] = [(400, 400), (400, 37), (37, 400), (399, 257), (64, 64), (65, 129)]
    kinds = ("noisy", "noisy", "unknown", "zeros", "extreme")
    return [REF.random_case(int(E), int(K), kinds[i % 5], seed=i) for i, (E, K) in enumerate(dims)]


@pytest.mark.parametrize("W", (64, 128, 192))
def test_host_twin_equals_the_restatement_on_200_random_shapes(W):
    got = check(random_shapes(), W, threads=8)
    assert sum(g["cost"] >= 0 for g in got) >= 150


def test_events_with_their_own_samples_and_threads():
    rng = np.random.default_rng(9)
    reads = []
    for E, K in ((50, 30), (7, 9), (200, 150)):
        m, l = REF.random_case(E, K, "noisy", seed=1)
        ln = rng.integers(1, 30, E)
        reads.append((m, l, 100 + np.concatenate([[0], np.cumsum(ln)[:-1]]), ln))
    a = check(reads, 64, threads=1)
    assert check(reads, 64, threads=5) == a


def test_refusals():
    L = _lib.lib()
    read = REF.random_case(10, 8, "noisy")
    for W in (0, 32, 96, 1088, -64):
        assert host([read], W)[0] == ERR_ARG and L.s2s_eventalign_scratch_bytes(10, 8, W) == ERR_ARG
    for kw in (dict(skip=-1), dict(skip=(1 << 20) + 1), dict(trim=-1), dict(trim=(1 << 20) + 1), dict(unk=-1), dict(unk=65536)):
        assert host([read], 64, **kw)[0] == ERR_ARG
    assert host([read], 64, threads=0)[0] == ERR_ARG
    for E, K, W in ((10, 8, 64), (1, 1, 1024), (7000, 5000, 128), (1 << 22, 1 << 22, 1024)):
        assert L.s2s_eventalign_scratch_bytes(E, K, W) == REF.scratch_bytes(E, K, W) > 0
    assert L.s2s_eventalign_scratch_bytes(7000, 5000, 128) < 1 << 20            # under 1 MB for a read of 50,000 samples
    for E, K in ((0, 5), (5, 0), ((1 << 22) + 1, 5)):
        assert L.s2s_eventalign_scratch_bytes(E, K, 64) == 0


# ------------------------------------------------------------------ planted reads through the whole chain
def host_chain(records, levels, known, W, skip=SKIP, trim=TRIM, unk=UNK, seg=SEG, threads=4):
    """The host twins in the order of the command on raw arrays -> [dict like REF.chain's per read]."""
    L = _lib.lib()
    P = len(records)
    recs = [np.ascontiguousarray(r, np.int16) for r in records]
    x, offs = pooled(recs, np.int16), offsets([len(r) for r in recs])
    ev_offs = offsets([max(1, len(r) // seg[0]) if len(r) else 0 for r in recs])
    ET = int(ev_offs[-1])
    st, ln, ne = np.zeros(ET, np.int32), np.zeros(ET, np.int32), np.zeros(P, np.int32)
    S, Q, m_offs = np.zeros(ET, np.int64), np.zeros(ET, np.int64), np.zeros(P + 1, np.int64)
    means, mq, med, mad = np.zeros(ET, np.int16), np.zeros(ET, np.int16), np.zeros(P, np.int32), np.zeros(P, np.int32)
    p = lambda a: a.ctypes.data                         # noqa: E731
    assert L.s2s_segment_host(p(x), p(offs), P, int(offs[-1]), *seg, p(ev_offs), p(st), p(ln), p(ne), threads) == 0
    assert L.s2s_event_sums_host(p(x), p(offs), p(st), p(ln), p(ev_offs), P, p(S), p(Q), threads) == 0
    assert L.s2s_event_means_host(p(S), p(ln), p(ev_offs), p(ne), P, ET, p(m_offs), p(means), threads) == 0
    assert L.s2s_signal_median_mad_host(p(means), p(m_offs), P, p(med), p(mad), threads) == 0
    assert L.s2s_signal_normalise_host(p(means), p(m_offs), P, p(med), p(mad), 64, p(mq), threads) == 0
    lq = []
    for lev, kn in zip(levels, known):
        lev, kn = np.asarray(lev, np.int16), np.asarray(kn, bool)
        lmed, lmad = REF.median_mad(lev[kn])
        lq.append(np.where(kn, np.array(REF.normalise(lev, lmed, lmad), np.int64), REF.UNKNOWN).astype(np.int16))
    reads = [(mq[m_offs[i]:m_offs[i + 1]], lq[i], st[ev_offs[i]:ev_offs[i] + ne[i]], ln[ev_offs[i]:ev_offs[i] + ne[i]]) for i in range(P)]
    rc, got = host(reads, W, skip, trim, unk, threads)
    assert rc == 0
    for g, r in zip(got, reads):
        g.update(m=r[0].tolist(), lq=r[1].tolist(), ev_start=r[2].tolist(), ev_len=r[3].tolist())
    return got


@pytest.fixture(scope="module")
def planted():
    """The planted reads, and their full-matrix (W = 1024 covers every band whole) result by the restatement of the whole chain."""
    out = []
    for K, head, tail in REF.PLANTED:
        adc, lev, bounds = REF.planted_read(K, head, tail)
        ints, known = RSQ.level_ints(lev)
        out.append(dict(adc=adc, ints=ints, known=known, bounds=bounds, full=REF.chain(adc, ints, known, 1024)))
    return out


def test_planted_reads_come_back_with_exact_trims(planted):
    for rd in planted:
        full, bounds, n = rd["full"], rd["bounds"], len(rd["adc"])
        E, K = len(full["m"]), len(rd["ints"])
        assert E + K - 1 <= 1024                        # every cell of the matrix lies in its band at W = 1024
        assert full["cost"] >= 0
        REF.check_consequences(full["m"], full["lq"], SKIP, TRIM, UNK, full, full["ev_start"], full["ev_len"])
        ks, kl = np.array(full["k_start"]), np.array(full["k_len"])
        assert (kl > 0).all()
        # every sample of every k-mer lies in that k-mer's interval, and both trims are exact
        assert (ks <= bounds[:-1]).all() and (ks + kl >= bounds[1:]).all()
        assert ks[0] == bounds[0] and ks[-1] + kl[-1] == bounds[-1] == n - (n - bounds[-1])
        assert full["ev_start"][full["first"]] == bounds[0]
        for W in (64, 128):
            narrow = REF.chain(rd["adc"], rd["ints"], rd["known"], W)
            assert same(narrow, full), W


def test_host_chain_equals_the_restated_chain_on_planted_reads(planted):
    for W in (64, 128, 1024):
        got = host_chain([rd["adc"] for rd in planted], [rd["ints"] for rd in planted], [rd["known"] for rd in planted], W)
        for g, rd in zip(got, planted):
            want = rd["full"]                           # (the narrow bands give the same: the test above)
            assert g["ev_start"] == want["ev_start"] and g["ev_len"] == want["ev_len"] and g["m"] == want["m"] and g["lq"] == want["lq"]
            assert same(g, want), W


# ------------------------------------------------------------------ the command
def junked_read(rng, n_bases, adc, head, tail):
    """-> (sequence, stored int16 samples, k-mer bounds): every k-mer's samples are its ADC level with a dwell of 12..40, neighbours at
    least 200 ADC counts apart; junk runs far above every level in front and far below behind."""
    while True:
        seq = "".join(rng.choice(list("ACGT"), K3))
        while len(seq) < n_bases:
            last = adc[RSQ.kmer_codes(seq[-K3:], K3)[0]]
            nxt = [c for c in "ACGT" if abs(adc[RSQ.kmer_codes(seq[-K3 + 1:] + c, K3)[0]] - last) >= 200]     # (NaN compares False)
            if not nxt:
                break
            seq += str(rng.choice(nxt))
        if len(seq) == n_bases and not np.isnan(adc[RSQ.kmer_codes(seq, K3)]).any():
            break
    codes = RSQ.kmer_codes(seq, K3)
    dwell = rng.integers(12, 41, len(codes))

    def junk(n, centre):
        return np.repeat(centre + rng.integers(-40, 41, n // 12 + 1), rng.integers(12, 41, n // 12 + 1))[:n]
    sig = np.concatenate([junk(head, 2600), np.repeat(adc[codes], dwell), junk(tail, -700)]).astype(np.int16)
    return seq, sig, head + np.concatenate([[0], np.cumsum(dwell)])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("eventalign")
    rng = np.random.default_rng(21)
    adc = rng.permutation(64).astype(float) * 23 + 150            # 64 distinct levels, 23 ADC counts apart
    adc[7] = np.nan
    shapes = ((40, 0, 0), (75, 300, 120), (33, 90, 0), (60, 0, 200), (50, 150, 150))
    reads = {f"r{i}": junked_read(rng, nb, adc, h, t) for i, (nb, h, t) in enumerate(shapes)}
    ids = list(reads) + ["orphan", "dark"]
    sigs = [reads[i][1] for i in reads] + [np.arange(50, dtype=np.int16), np.repeat(rng.integers(100, 900, 20), 15).astype(np.int16)]
    blow5 = write_file(d / "s.blow5", ids, sigs, record_compression="zlib")
    slow5 = write_file(d / "s.slow5", ids, sigs)
    rec = next(iter(SB.open_records(blow5)))
    cal = (float(rec["digitisation"]), float(rec["offset"]), float(rec["range"]))
    (d / "m.model").write_bytes(bytes(kmer_model.format_model(model_counts(adc), K3, cal[0], cal[2], cal[1])))
    dark = "ACT" * 8                                    # ACT, CTA, TAC only: the fixture leaves none of them a level (below)
    (d / "r.fasta").write_text("".join(f">{i} comment\n{reads[i][0][:30]}\n{reads[i][0][30:]}\n" for i in reads) + f">dark\n{dark}\n")
    return d, blow5, slow5, reads, cal, adc, dark


def run(*args):
    return CliRunner().invoke(cli.main, ["eventalign", *[str(a) for a in args]], catch_exceptions=False)


def dark_model(d, adc, cal, dark):
    """A model without a level for any k-mer of `dark`."""
    a = adc.copy()
    a[np.unique(RSQ.kmer_codes(dark, K3))] = np.nan
    (d / "dark.model").write_bytes(bytes(kmer_model.format_model(model_counts(a), K3, cal[0], cal[2], cal[1])))
    return d / "dark.model", a


def test_command_cpu_rows_trims_and_batching(files):
    d, blow5, slow5, reads, cal, adc, dark = files
    r = run(d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "a.tsv", "--cpu", "--json", "--summary", d / "a.sum.tsv")
    assert r.exit_code == 0, r.output
    s = json.loads(r.output.strip().splitlines()[-1])
    assert (s["records"], s["solved"], s["no_sequence"], s["unreached"], s["refused"], s["no_known_level"]) == (7, 6, 1, 0, 0, 0)
    raw = (d / "a.tsv").read_bytes()
    text = raw.decode().splitlines()
    assert text[0].split("\t") == list(EA.EVENT_COLUMNS)
    rows = parse_events(raw, False)                                             # the reader of predict --events
    assert len(rows) == len(text) - 1 == s["events"]
    table = CMP.read_events(str(d / "a.tsv"))                                   # ... and of compare --events-a
    assert list(table) == list(reads) + ["dark"]
    # the planted reads: every k-mer's row holds exactly its samples; both trims are exact
    for rid, (seq, sig, bounds) in reads.items():
        mine = [l.split("\t") for l in text[1:] if l.startswith(rid + "\t")]
        assert [int(l[1]) for l in mine] == list(range(len(bounds) - 1)) and [l[2] for l in mine] == [seq[j:j + K3] for j in range(len(mine))]
        assert [int(l[3]) for l in mine] == bounds[:-1].tolist() and [int(l[4]) for l in mine] == bounds[1:].tolist(), rid
        assert all(l[6] == "0.0000" for l in mine)
    summary = [l.split("\t") for l in (d / "a.sum.tsv").read_text().splitlines()]
    assert summary[0] == list(EA.SUMMARY_COLUMNS) and [l[3] for l in summary[1:]] == ["solved"] * 5 + ["no_sequence", "solved"]
    heads, tails = [int(l[9]) for l in summary[1:6]], [int(l[10]) for l in summary[1:6]]
    assert heads == [b[2][0] for b in reads.values()] and tails == [len(b[1]) - b[2][-1] for b in reads.values()]
    assert s["trimmed_head_samples"] >= sum(heads) and s["trimmed_tail_samples"] >= sum(tails)
    # SLOW5 and any batching: the same bytes
    for i, extra in enumerate((("--max-samples", 1), ("--trace-memory", EA.scratch_bound(len(reads["r1"][1]), 73, 128, 3)),
                               ("--max-samples", 2500))):
        r = run(d / "r.fasta", slow5 if i else blow5, "--kmer-model", d / "m.model", "-o", d / f"b{i}.tsv", "--cpu", "--summary",
                d / f"b{i}.sum.tsv", *extra)
        assert r.exit_code == 0, r.output
        assert (d / f"b{i}.tsv").read_bytes() == raw and (d / f"b{i}.sum.tsv").read_bytes() == (d / "a.sum.tsv").read_bytes()
    r = run(d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "c.tsv", "--cpu", "--samples", "--band-width", 64)
    assert r.exit_code == 0, r.output
    with_samples = (d / "c.tsv").read_bytes()
    assert len(parse_events(with_samples, True)) == len(rows)
    assert [l.split("\t")[:7] for l in with_samples.decode().splitlines()[1:]] == [l.split("\t") for l in text[1:]]


def test_command_cpu_rna_unknown_levels_and_refusals(files):
    d, blow5, slow5, reads, cal, adc, dark = files
    ids = list(reads)
    rev = write_file(d / "rev.blow5", ids, [reads[i][1][::-1].copy() for i in ids])
    r = run(d / "r.fasta", rev, "--kmer-model", d / "m.model", "-o", d / "rna.tsv", "--cpu", "--rna")
    assert r.exit_code == 0, r.output
    got = [l.split("\t") for l in (d / "rna.tsv").read_text().splitlines()[1:]]
    for rid, (seq, sig, bounds) in reads.items():
        mine = [l for l in got if l[0] == rid]
        K, n = len(bounds) - 1, len(sig)
        assert [int(l[1]) for l in mine] == list(range(K)) and [l[2] for l in mine] == [seq[j:j + K3] for j in range(K)]
        assert [int(l[3]) for l in mine] == [n - int(bounds[j + 1]) for j in range(K)], rid       # start_idx falls as position rises
        assert [int(l[4]) for l in mine] == [n - int(bounds[j]) for j in range(K)]
    # a read without a known level
    model, _ = dark_model(d, adc, cal, dark)
    r = run(d / "r.fasta", blow5, "--kmer-model", model, "-o", d / "dk.tsv", "--cpu", "--json", "--summary", d / "dk.sum.tsv")
    assert r.exit_code == 0, r.output
    s = json.loads(r.output.strip().splitlines()[-1])
    assert s["no_known_level"] == 1 and s["no_sequence"] == 1 and s["solved"] + s["unreached"] == 5
    assert [l.split("\t")[3] for l in (d / "dk.sum.tsv").read_text().splitlines()[1:]][5:] == ["no_sequence", "no_known_level"]
    assert not any(l.startswith("dark\t") for l in (d / "dk.tsv").read_text().splitlines())
    # a read whose walk back may need more than --trace-memory is refused by its id; the others are solved
    need = sorted(EA.scratch_bound(len(v[1]), len(v[0]) - K3 + 1, 128, 3) for v in reads.values())
    r = run(d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / "t.tsv", "--cpu", "--json", "--trace-memory", need[-2])
    s = json.loads(r.output.strip().splitlines()[-1])
    assert r.exit_code == 0 and s["refused"] == 1 and s["solved"] == 5
    assert not any(l.startswith("r1\t") for l in (d / "t.tsv").read_text().splitlines())
    for extra in (("--band-width", 0), ("--band-width", 96), ("--band-width", 1088), ("--skip-penalty", -1), ("--trim-penalty", (1 << 20) + 1),
                  ("--unknown-cost", 65536), ("--max-samples", 0), ("--trace-memory", 0), ("--window-short", 0), ("--threshold-long", 0)):
        r = CliRunner().invoke(cli.main, ["eventalign", str(d / "r.fasta"), blow5, "--kmer-model", str(d / "m.model"), "-o",
                                          str(d / "x.tsv"), "--cpu", *[str(e) for e in extra]])
        assert r.exit_code != 0 and extra[0] in r.output, (extra, r.output)
    r = CliRunner().invoke(cli.main, ["eventalign", str(d / "r.fasta"), str(d / "x.pod5"), "--kmer-model", str(d / "m.model"), "-o",
                                      str(d / "x.tsv"), "--cpu"])
    assert r.exit_code != 0 and "POD5" in r.output


def test_python_entry_equals_the_restatement():
    reads = [REF.random_case(E, K, "noisy", seed=3) for E, K in ((60, 40), (0, 5), (25, 70), (5, 0))]
    r = EA.eventalign([x[0] for x in reads], [x[1] for x in reads], band_width=64, cpu=True)
    for i, read in enumerate(reads):
        want = ref(read, 64)
        got = dict(cost=int(r["cost"][i]), first=int(r["first"][i]), end=int(r["end"][i]),
                   **{k: r[k][i].tolist() for k in ("kmer", "k_start", "k_len", "k_events")})
        assert same(got, want), i
    with pytest.raises(ValueError):
        EA.eventalign([reads[0][0]], [reads[0][1]], band_width=96, cpu=True)
