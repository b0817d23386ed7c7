"""`predict --kmer-model` on the GPU: s2s_kmer_model_accumulate against its definition -- the numpy restatement of s2s_event_stats
(tests/_events_ref.py), every slot's fixed-point mean and deviation in Python integers and the reduction by k-mer code
(tests/_kmer_model_ref.py) -- over the chunk geometries and over k; the per-workgroup cache under contention, overfilled, with
codes that collide in its hash and across several flushes of one walk, the batches sized from the constants of include/s2s_hip.h;
sliced, at the accumulators' bounds; then the model of whole `predict` runs, in one process and sharded over three ranks.  Every
comparison is between integers or bytes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from seq2squiggle_amd import utils as U
from seq2squiggle_amd.kmer_model import join_rank_files, load_counts
from _events_ref import parse_events, ref_event_stats
from _kmer_model_ref import (cache_slot, event_fixed, fixed_of_slots, header_constants, kmer_codes, parse_model, py_model, reduce_by_code,
                             ref_kmer_model)
from conftest import GOLDEN, ROOT
from test_gpu_events import CAL, make_inputs, pa
from test_gpu_kmer_table import dev_, engine, make_letters

pytestmark = pytest.mark.gpu

CKPT = os.path.join(GOLDEN, "synthetic_k9.ckpt")
FASTA = os.path.join(GOLDEN, "example_test.fasta")
LAMBDA = os.path.join(GOLDEN, "example_lambda_genome.fasta")
K = header_constants(open(os.path.join(ROOT, "include", "s2s_hip.h")).read())      # the cache's geometry: SLOTS, PROBES, FLUSH_ROUNDS, ...
CAL2 = (2048.0, 281.345551, -127.5655735)                                          # a profile's own numbers


def accumulate(eng, sig, dur, flat, start, nv, table=None, cal=CAL, rows=slice(None)):
    """One call on the chunks `rows` -> the table (a fresh one unless given) as numpy after the call."""
    t = eng.kmer_model_new() if table is None else table
    s_d, d_d, f_d, c_d, n_d = dev_(eng, sig[rows], dur[rows], flat, start[rows], nv[rows])
    assert eng.kmer_model_accumulate(s_d, d_d, f_d, c_d, n_d, *cal, t) is t
    return t.cpu().numpy()


def expected(sig, dur, flat, start, nv, k, cal=CAL):
    te = dur.shape[1]
    return ref_kmer_model(*ref_event_stats(sig, dur, *cal), kmer_codes(flat, start, nv, k, te), k)


_BASE = {}


def tiled(te, ts, B, dense=False):
    """B chunks that repeat the 257 crafted chunks of make_inputs (dense: 64 chunks in which every k-mer owns ts // te non-zero
    samples, so that every real slot is an event) -> (sig, dur, has, M, D): the reference statistics of the base are computed once
    (ref_event_stats, event_fixed per slot) and repeated like the chunks."""
    key = (te, ts, dense)
    if key not in _BASE:
        if dense:
            rng = np.random.default_rng(te * ts)
            q = rng.integers(-3000, 3000, (64, ts))
            q[q == -10] = 7                                    # (q = -10 is 0.0 pA: stripped)
            sig, dur = pa(q).astype(np.float32), np.full((64, te), ts // te, np.int32)
        else:
            sig, dur, _ = make_inputs(te, ts)
        _BASE[key] = (sig, dur) + fixed_of_slots(*ref_event_stats(sig, dur, *CAL), te)
    sig, dur, has, M, D = _BASE[key]
    idx = np.arange(B) % sig.shape[0]
    return sig[idx], dur[idx], has[idx], M[idx], D[idx]


def walk_of_workgroups(B):
    """-> int [B]: (workgroup, round) of every chunk as the kernel walks them: four chunks per round, the grid capped."""
    groups = (B + 3) // 4
    grid = min(groups, K["MAX_WORKGROUPS"])
    g = np.arange(B) // 4
    return g % grid, g // grid


# every geometry; every k of the list at 16 / 250; k = 5 / 6: the last k that indexes the cache directly and the first that hashes
DEFINITION = [(16, 250, 9), (16, 250, 1), (16, 250, 5), (16, 250, 6), (16, 250, 10), (1, 1, 3), (5, 37, 9), (64, 1024, 10), (17, 1023, 6)]


@pytest.mark.parametrize("te,ts,k", DEFINITION)
def test_model_equals_its_definition(te, ts, k):
    assert K["DIRECT_MAX_K"] == 5 and K["FIELDS"] == 5
    eng = engine(te, ts, k)
    sig, dur, _ = make_inputs(te, ts)
    flat, start, nv = make_letters(257, te, k, seed=te + ts + k)
    codes = kmer_codes(flat, start, nv, k, te)
    stats = ref_event_stats(sig, dur, *CAL)
    want = ref_kmer_model(*stats, codes, k)
    n_events = int(((codes >= 0) & (stats[0][:, :te] >= 1)).sum())
    assert want[:, 0].sum() == n_events > 0 and n_events < nv.sum() and want[4 ** k, 0] > 0      # slots without samples add nothing
    assert (want[:, 1] < 0).any() and (want[:, 3] > 0).any() == (ts > te) and (want[:, 2] >= 0).all()      # (one sample per event: D = 0)
    table = eng.kmer_model_new()
    assert table.dtype == torch.int64 and tuple(table.shape) == (4 ** k + 1, 5) and not table.any()
    got = accumulate(eng, sig, dur, flat, start, nv, table)
    assert np.array_equal(got, want)
    # the numbers are event_stats' for the same inputs, by definition
    s_d, d_d = dev_(eng, sig, dur)
    st = eng.event_stats(s_d, d_d, *CAL)
    assert np.array_equal(got, ref_kmer_model(st["seg"].cpu().numpy(), st["sum"].cpu().numpy(), st["sumsq"].cpu().numpy(), codes, k))
    # another calibration
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv, cal=CAL2), expected(sig, dur, flat, start, nv, k, CAL2))


@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_partial_workgroups(B, k):
    """One, three and five chunks: a workgroup with idle waves, and a second one with a single chunk."""
    eng = engine(16, 250, k)
    sig, dur, _ = make_inputs(16, 250)
    flat, start, nv = make_letters(257, 16, k, seed=B)
    rows = slice(3, 3 + B)                                     # (the chunks from 3 on have n_valid = te)
    want = ref_kmer_model(*ref_event_stats(sig[rows], dur[rows], *CAL), kmer_codes(flat, start[rows], nv[rows], k, 16), k)
    assert want[:, 0].sum() > 0
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv, rows=rows), want)


@pytest.mark.parametrize("k", [3, 9])
def test_contention(k):
    """1,030 chunks whose letters are all A: every event of the launch lands in ONE cache slot of its workgroup and in row 0 of the
    table.  Then two alternating k-mers (ACAC.. / CACA..)."""
    eng = engine(16, 250, k)
    B, te = 1030, 16
    sig, dur, has, M, D = tiled(te, 250, B)
    rng = np.random.default_rng(k)
    nv = rng.integers(1, te + 1, B).astype(np.uint8)
    nv[::7] = te
    w = te + k - 1
    start = (np.arange(B) * w).astype(np.int64)
    flat = np.full(B * w + 1, ord("A"), np.uint8)
    want = reduce_by_code(has, M, D, kmer_codes(flat, start, nv, k, te), k)
    assert want[0, 0] > 1000 and not want[1:].any()
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv), want)
    flat = np.frombuffer(b"AC" * (B * w // 2 + 1), np.uint8)[:B * w + 1].copy()
    want = reduce_by_code(has, M, D, kmer_codes(flat, start, nv, k, te), k)
    assert (want[:, 0] > 0).sum() == 2 and want[:, 0].sum() > 1000
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv), want)


def test_more_codes_than_slots_between_two_flushes():
    """64 k-mers per chunk, every one an event with a code of its own (k = 10, random letters): a workgroup inserts 256 codes per
    round.  B makes every workgroup walk enough rounds WITHOUT a flush in between that it meets more distinct codes than the cache
    has slots: by the pigeonhole principle some of them find no place and add straight to the table."""
    te, ts, k = 64, 1024, 10
    rounds = K["SLOTS"] // (4 * te) + 1                         # (rounds * 4 * te > SLOTS)
    assert rounds <= K["FLUSH_ROUNDS"]                          # (else a flush would empty the cache in time)
    B = 4 * K["MAX_WORKGROUPS"] * rounds
    eng = engine(te, ts, k)
    sig, dur, has, M, D = tiled(te, ts, B, dense=True)
    assert has.all()
    flat, start, nv = make_letters(B, te, k, seed=3, n_rate=0.0)
    nv[:] = te
    codes = kmer_codes(flat, start, nv, k, te)
    wg, rnd = walk_of_workgroups(B)
    assert rnd.max() == rounds - 1
    for w_ in (0, K["MAX_WORKGROUPS"] // 2, K["MAX_WORKGROUPS"] - 1):
        assert len(np.unique(codes[wg == w_])) > K["SLOTS"]
    want = reduce_by_code(has, M, D, codes, k)
    assert want[:, 0].sum() == B * te
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv), want)


def test_codes_that_collide_beyond_the_probe_limit():
    """Three times PROBES codes (k = 9) with ONE home slot in the cache's hash, as the first k-mer of every chunk, dealt so that every
    workgroup meets all of them before its first flush: PROBES of them take the slots from the home slot on, the others find no
    place within the probe limit and add to the table directly.  The k-mers behind the first are random."""
    te, ts, k = 16, 250, 9
    P = K["PROBES"]
    home = {}
    for code in range(4 ** k):
        home.setdefault(cache_slot(code, K), []).append(code)
    slot = max(home, key=lambda s_: len(home[s_]))
    crafted = home[slot][:3 * P]
    assert len(crafted) == 3 * P and len({cache_slot(c, K) for c in crafted}) == 1
    rounds = 3 * P // 4
    assert 4 * rounds == 3 * P and rounds <= K["FLUSH_ROUNDS"]
    B = 4 * K["MAX_WORKGROUPS"] * rounds
    eng = engine(te, ts, k)
    sig, dur, has, M, D = tiled(te, ts, B, dense=True)
    flat, start, nv = make_letters(B, te, k, seed=4)
    wg, rnd = walk_of_workgroups(B)
    which = (np.arange(B) % 4 + 4 * rnd) % (3 * P)             # round r of a workgroup: the crafted codes 4r .. 4r + 3
    letters = np.frombuffer(b"ACGT", np.uint8)
    for b in range(B):
        c = crafted[which[b]]
        flat[start[b]: start[b] + k] = letters[[(c >> (2 * (k - 1 - i))) & 3 for i in range(k)]]
    codes = kmer_codes(flat, start, nv, k, te)
    assert all(set(codes[wg == w_][:, 0].tolist()) == set(crafted) for w_ in (0, 5, K["MAX_WORKGROUPS"] - 1))
    want = reduce_by_code(has, M, D, codes, k)
    assert all(want[c, 0] >= B // (3 * P) for c in crafted)
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv), want)


def test_a_walk_with_several_flushes():
    """Enough chunks that every workgroup flushes its cache twice in mid-walk and once at the end, the last interval a partial one
    and the last round of the walk short of workgroups."""
    te, ts, k = 5, 37, 9
    rounds = 2 * K["FLUSH_ROUNDS"] + 2
    B = 4 * K["MAX_WORKGROUPS"] * (rounds - 1) + 4 * 17 + 3
    eng = engine(te, ts, k)
    sig, dur, has, M, D = tiled(te, ts, B)
    flat, start, nv = make_letters(B, te, k, seed=6)
    wg, rnd = walk_of_workgroups(B)
    assert rnd.max() == rounds - 1 and (rnd[wg == 0] >= K["FLUSH_ROUNDS"]).sum() > 4 * K["FLUSH_ROUNDS"]
    want = reduce_by_code(has, M, D, kmer_codes(flat, start, nv, k, te), k)
    assert want[:, 0].sum() > B
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv), want)
    # the same walk on one row: all A
    w = te + k - 1
    start = (np.arange(B) * w).astype(np.int64)
    flat = np.full(B * w + 1, ord("A"), np.uint8)
    want = reduce_by_code(has, M, D, kmer_codes(flat, start, nv, k, te), k)
    assert want[0, 0] > B and not want[1:].any()
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv), want)


@pytest.mark.parametrize("k", [3, 9])
def test_additivity(k):
    eng = engine(16, 250, k)
    sig, dur, _ = make_inputs(16, 250)
    flat, start, nv = make_letters(257, 16, k, seed=5)
    whole = accumulate(eng, sig, dur, flat, start, nv)
    assert np.array_equal(whole, expected(sig, dur, flat, start, nv, k))
    slices = [slice(0, 5), slice(5, 6), slice(6, 257)]
    for order in (slices, slices[::-1]):
        t = eng.kmer_model_new()
        for sl in order:
            got = accumulate(eng, sig, dur, flat, start, nv, t, rows=sl)
        assert np.array_equal(got, whole)
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv, t, rows=slice(0, 0)), whole)     # B == 0 changes nothing
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv, t), 2 * whole)                   # a second call doubles it


@pytest.mark.parametrize("k", [1, 10])
def test_extremes(k):
    """64 / 1024: 64 chunks whose first k-mer owns all 1,024 samples -- at q = -32768 (M = -2^23, M^2 = 2^46, D = 0), then
    alternating -32768 / 32767 (D just under 2^23)."""
    eng = engine(64, 1024, k)
    B, te, ts = 64, 64, 1024
    dur = np.zeros((B, te), np.int32)
    dur[:, 0] = ts
    w = te + k - 1
    flat = np.frombuffer((b"G" * k + b"T" * (te - 1)) * B + b"_", np.uint8).copy()
    start = (np.arange(B) * w).astype(np.int64)
    nv = np.full(B, te, np.uint8)
    row = int("2" * k, 4)
    sig = np.full((B, ts), np.float32(pa(-32768)), np.float32)
    got = accumulate(eng, sig, dur, flat, start, nv)
    assert got[row].tolist() == [64, -64 * 2 ** 23, 64 * 2 ** 46, 0, 0] and got[:, 0].sum() == 64
    assert np.array_equal(got, expected(sig, dur, flat, start, nv, k))
    sig[:, 1::2] = np.float32(pa(32767))
    M, D = event_fixed(1024, -512, 512 * (32768 ** 2 + 32767 ** 2))
    assert M == -128 and 2 ** 23 - 256 <= D < 2 ** 23
    got = accumulate(eng, sig, dur, flat, start, nv)
    assert got[row].tolist() == [64, 64 * M, 64 * M * M, 64 * D, 64 * D * D] and got[:, 0].sum() == 64
    assert np.array_equal(got, expected(sig, dur, flat, start, nv, k))


def test_argument_checks():
    import ctypes as C
    from seq2squiggle_amd import _lib
    eng = engine(16, 250, 9)
    sig, dur, _ = make_inputs(16, 250)
    flat, start, nv = make_letters(257, 16, 9, seed=1)
    s_d, d_d, f_d, c_d, n_d = dev_(eng, sig[:2], dur[:2], flat, start[:2], nv[:2])
    table = eng.kmer_model_new()
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    ok = [p(s_d), p(d_d), p(f_d), p(c_d), p(n_d), 2, *CAL, p(table)]
    for i in (0, 1, 2, 3, 4, 9):                              # each pointer NULL in turn (9: the table)
        args = list(ok)
        args[i] = None
        assert L.s2s_kmer_model_accumulate(eng._h, None, *args) == -1
    for i, v in ((5, -1), (6, 0.0), (7, 0.0)):                # B < 0, digitisation 0, range 0
        args = list(ok)
        args[i] = v
        assert L.s2s_kmer_model_accumulate(eng._h, None, *args) == -1
    assert L.s2s_kmer_model_accumulate(None, None, *ok) == -1
    args = list(ok)
    args[5] = 0
    assert L.s2s_kmer_model_accumulate(eng._h, None, *args) == 0          # B == 0: a successful no-op
    torch.cuda.synchronize()
    assert not table.any()                                    # ... and none of them launched anything
    for bad in (lambda: eng.kmer_model_accumulate(s_d.double(), d_d, f_d, c_d, n_d, *CAL, table),
                lambda: eng.kmer_model_accumulate(s_d, d_d[:1], f_d, c_d, n_d, *CAL, table),
                lambda: eng.kmer_model_accumulate(s_d, d_d, f_d, c_d[:1], n_d, *CAL, table),
                lambda: eng.kmer_model_accumulate(s_d, d_d, f_d, c_d, n_d.int(), *CAL, table),
                lambda: eng.kmer_model_accumulate(s_d, d_d, f_d, c_d, n_d, 0.0, 1.0, 0.0, table),
                lambda: eng.kmer_model_accumulate(s_d, d_d, f_d, c_d, n_d, *CAL, table[:-1]),
                lambda: eng.kmer_model_accumulate(s_d, d_d, f_d, c_d, n_d, *CAL, eng.kmer_table_new()),      # six columns: the other table
                lambda: eng.kmer_model_accumulate(s_d, d_d, f_d, c_d, n_d, *CAL, table.cpu())):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------- predict end to end
SEED = 11
PROFILE = "dna-r10-prom"


def _run(out, events=None, samples=False, kmer_table=None, kmer_model=None):
    """`predict FASTA --read-input --preserve-read-ids -o out --seed 11 [--events ...] [--kmer-table ...] [--kmer-model ...]` in this
    process."""
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    U.set_seeds(SEED)
    opt = lambda x: None if x is None else str(x)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=FASTA, read_input=True, n=-1, r=400, c=-1, out=str(out),
                  profile=PROFILE, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                  distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None, digitisation=None,
                  range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None, min_noise=0.0,
                  min_duration=3, min_read_len=30, preserve_read_ids=True, seed=SEED, events=opt(events), events_samples=samples,
                  kmer_table=opt(kmer_table), kmer_model=opt(kmer_model))


def _masked(path):
    """The file's bytes with the header's wall-clock attribute blanked."""
    return re.sub(rb"@exp_start_time\t[^\n]*", b"@exp_start_time\t-", open(path, "rb").read())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmer_model_runs")
    _run(d / "plain.blow5")
    _run(d / "model.blow5", kmer_model=d / "model.model")
    _run(d / "table.blow5", kmer_table=d / "table.tsv")
    _run(d / "all.blow5", events=d / "all_ev.tsv", samples=True, kmer_table=d / "all.tsv", kmer_model=d / "all.model")
    return d


def test_the_model_is_the_reduction_of_the_runs_event_table(runs):
    """The stored int16 samples of every event, read back from the `samples` column of the same run's event table (pA to three
    decimals: far finer than one ADC count), give n / S / Q; event_fixed and the sums per model_kmer give the counters."""
    prof = U.get_profile(PROFILE)
    cal = tuple(float(np.float32(prof[x])) for x in ("digitisation", "range", "offset_mean"))
    events = parse_events(open(runs / "all_ev.tsv", "rb").read(), True)
    counts = [[0] * 5 for _ in range(4 ** 9 + 1)]
    lut = {c: i for i, c in enumerate("ACGT")}
    for r in events:
        raw = np.array([float(x) for x in r["samples"]]) * cal[0] / cal[1] - cal[2]
        q = np.rint(raw).astype(np.int64)
        assert len(q) == r["end_idx"] - r["start_idx"] >= 1 and np.abs(raw - q).max() < 0.05
        M, D = event_fixed(len(q), int(q.sum()), int((q * q).sum()))
        code = 4 ** 9 if set(r["model_kmer"]) - set("ACGT") else int("".join(str(lut[c]) for c in r["model_kmer"]), 4)
        row = counts[code]
        row[0] += 1; row[1] += M; row[2] += M * M; row[3] += D; row[4] += D * D
    counts = np.array(counts, np.int64)
    assert len(events) > 500 and counts[:, 0].sum() == len(events) and (counts[:, 3] > 0).any()
    text = open(runs / "all.model", "rb").read()
    assert text == py_model(counts, 9, *cal)
    k, rows = parse_model(text)
    assert k == 9 and len(rows) == int((counts[:4 ** 9, 0] > 0).sum()) and sum(r_["n_events"] for r_ in rows.values()) <= len(events)


def test_the_option_changes_no_other_file(runs, tmp_path):
    d = runs
    assert _masked(d / "plain.blow5") == _masked(d / "model.blow5") == _masked(d / "table.blow5") == _masked(d / "all.blow5")
    assert open(d / "model.model", "rb").read() == open(d / "all.model", "rb").read()
    assert open(d / "table.tsv", "rb").read() == open(d / "all.tsv", "rb").read()
    _run(tmp_path / "npz.blow5", kmer_model=tmp_path / "r.npz")  # a path ending in .npz receives the counts (a rank's file)
    counts, k, cal = load_counts(str(tmp_path / "r.npz"))
    prof = U.get_profile(PROFILE)
    assert k == 9 and cal == tuple(float(np.float32(prof[x])) for x in ("digitisation", "range", "offset_mean"))
    assert py_model(counts, 9, *cal) == open(d / "model.model", "rb").read()


ENV0 = {k_: v for k_, v in os.environ.items() if k_ not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "S2S_ONE_GPU")}
CLI = [sys.executable, "-m", "seq2squiggle_amd", "predict", LAMBDA, "-n", "30", "-r", "1500", "-m", CKPT, "--seed", "5"]


def test_three_ranks_sum_to_the_single_process_model(tmp_path):
    r = subprocess.run(["timeout", "-k", "10", "300", *CLI, "-o", str(tmp_path / "one.blow5"), "--kmer-model", str(tmp_path / "one.model")],
                       cwd=ROOT, capture_output=True, text=True, timeout=330, env=ENV0)
    assert r.returncode == 0, r.stderr[-3000:]
    want = open(tmp_path / "one.model", "rb").read()
    assert want.count(b"\n") > 1000 and re.search(r"of the 262144 9-mers have no row", r.stdout + r.stderr)
    r = subprocess.run(["timeout", "-k", "10", "600", *CLI, "-o", str(tmp_path / "a.blow5"), "--gpus", "3", "--kmer-model",
                        str(tmp_path / "a.model"), "--keep-shards"], cwd=ROOT, capture_output=True, text=True, timeout=630,
                       env=dict(ENV0, S2S_ONE_GPU="1"))
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert open(tmp_path / "a.model", "rb").read() == want
    shards = [str(tmp_path / f"a.rank{rank}.npz") for rank in range(3)]
    assert all(os.path.exists(p) for p in shards)
    join_rank_files(shards, str(tmp_path / "joined.model"))
    assert open(tmp_path / "joined.model", "rb").read() == want and not any(os.path.exists(p) for p in shards)
