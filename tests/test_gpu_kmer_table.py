"""`predict --kmer-table` on the GPU: s2s_kmer_table_accumulate against its definition -- the numpy restatement of s2s_event_stats
(tests/_events_ref.py) reduced by k-mer code (tests/_kmer_table_ref.py) -- over the chunk geometries and over k on both of the
kernel's paths (the LDS table up to k = 5, global adds from k = 6), under contention, sliced, at the accumulators' bounds; then
the table of whole `predict` runs, in one process and sharded over three ranks.  Every comparison is between integers or bytes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _lib
from seq2squiggle_amd import utils as U
from seq2squiggle_amd.chunker import n_chunks, pack_reads
from seq2squiggle_amd.kmer_table import join_rank_files, load_counts
import _envelope_models as EM
import _geometry_models as GM
from _events_ref import parse_events, ref_event_stats
from _kmer_table_ref import kmer_codes, parse_table, py_table, ref_kmer_table
from conftest import GOLDEN, ROOT, load_ckpt
from test_gpu_events import CAL, make_inputs, pa          # the crafted signal / dur of the event-statistics tests, and their calibration

pytestmark = pytest.mark.gpu

CKPT = os.path.join(GOLDEN, "synthetic_k9.ckpt")
FASTA = os.path.join(GOLDEN, "example_test.fasta")
LAMBDA = os.path.join(GOLDEN, "example_lambda_genome.fasta")
_ENGINES = {}


def engine(te, ts, k):
    """One engine per (geometry, k) and session.  (16, 250, 9) is the committed checkpoint on its split-f16 instance; the others are
    dmodel 16 handles (generic at 16 / 250, generic-geometry elsewhere): the kernel only reads the handle's geometry and k."""
    key = (te, ts, k)
    if key not in _ENGINES:
        if key == (16, 250, 9):
            sd, cfg = load_ckpt("k9")
            _ENGINES[key] = S.Engine(sd, cfg)
        else:
            tag = f"e{te}x{ts}k{k}"
            cases = {tag: dict(seed=100 + len(_ENGINES), seq_kmer=k, max_dna_len=te, max_signal_len=ts, dmodel=16, dff=8, encoder_heads=2,
                               decoder_heads=1, pre_layers=0, encoder_layers=1, decoder_layers=1)}
            _ENGINES[key] = S.Engine(GM.geometry_state_dict(tag, cases), GM.geometry_config(tag, cases=cases),
                                     mode="generic" if (te, ts) == (16, 250) else None)
    eng = _ENGINES[key]
    assert (eng.t_enc, eng.t_dec, eng.k) == key
    return eng


def make_letters(B, te, k, seed, alphabet="ACGT", n_rate=0.02):
    """-> (flat uint8, chunk_start int64 [B], n_valid uint8 [B]): every chunk its own te + k - 1 letters, the windows laid out in a
    shuffled order (chunk_start is no ramp), about 2 % N among the letters, n_valid random in 1..te with rows of exactly 1 and te."""
    rng = np.random.default_rng(seed)
    w = te + k - 1
    order = rng.permutation(B)
    flat = rng.choice(np.frombuffer(alphabet.encode(), np.uint8), B * w)
    flat[rng.random(B * w) < n_rate] = ord("N")
    n_valid = rng.integers(1, te + 1, B).astype(np.uint8)
    n_valid[:3] = 1
    n_valid[3:6] = te
    n_valid[-1] = te
    return np.concatenate([flat, np.frombuffer(b"_", np.uint8)]), (order * w).astype(np.int64), n_valid


def dev_(eng, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in arrays]


def accumulate(eng, sig, dur, flat, start, nv, table=None, cal=CAL, rows=slice(None)):
    """One call on the chunks `rows` -> the table (a fresh one unless given) as numpy after the call."""
    t = eng.kmer_table_new() if table is None else table
    s_d, d_d, f_d, c_d, n_d = dev_(eng, sig[rows], dur[rows], flat, start[rows], nv[rows])
    assert eng.kmer_table_accumulate(s_d, d_d, f_d, c_d, n_d, *cal, t) is t
    return t.cpu().numpy()


def expected(sig, dur, flat, start, nv, k, cal=CAL):
    te = dur.shape[1]
    return ref_kmer_table(*ref_event_stats(sig, dur, *cal), kmer_codes(flat, start, nv, k, te), k)


# every geometry on both paths; every k of the list at 16 / 250; k = 5 / 6: the last k of the LDS path and the first of the global one
DEFINITION = [(16, 250, 9), (16, 250, 1), (16, 250, 3), (16, 250, 5), (16, 250, 6), (16, 250, 10), (1, 1, 3), (1, 1, 6), (5, 37, 5),
              (5, 37, 9), (64, 1024, 1), (64, 1024, 10), (17, 1023, 3), (17, 1023, 6)]


@pytest.mark.parametrize("te,ts,k", DEFINITION)
def test_table_equals_its_definition(te, ts, k):
    eng = engine(te, ts, k)
    sig, dur, _ = make_inputs(te, ts)
    flat, start, nv = make_letters(257, te, k, seed=te + ts + k)
    codes = kmer_codes(flat, start, nv, k, te)
    assert (codes == 4 ** k).any() and (codes == -1).any() == (te > 1) and set(nv[:6].tolist()) == {1, te}
    want = expected(sig, dur, flat, start, nv, k)
    assert want[:, 0].sum() == nv.sum() and 0 < want[:, 1].sum() <= want[:, 0].sum() and want[4 ** k, 0] > 0
    assert (want[:, 1] < want[:, 0]).any()                    # k-mers that occurred without samples: occ alone
    table = eng.kmer_table_new()
    assert table.dtype == torch.int64 and tuple(table.shape) == (4 ** k + 1, 6) and not table.any()
    got = accumulate(eng, sig, dur, flat, start, nv, table)
    assert np.array_equal(got, want)
    # the numbers are event_stats' for the same inputs, by definition
    s_d, d_d = dev_(eng, sig, dur)
    st = eng.event_stats(s_d, d_d, *CAL)
    assert np.array_equal(got, ref_kmer_table(st["seg"].cpu().numpy(), st["sum"].cpu().numpy(), st["sumsq"].cpu().numpy(), codes, k))
    # another calibration (a profile's own numbers)
    cal2 = (2048.0, 281.345551, -127.5655735)
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv, cal=cal2), expected(sig, dur, flat, start, nv, k, cal2))


@pytest.mark.parametrize("k", [3, 9])
def test_contention(k):
    """1,030 chunks (258 workgroups on either path) whose letters are all A: every slot of the launch lands in row 0 (k = 3: of
    every workgroup's LDS table, k = 9: of the table in global memory).  Then two alternating k-mers (ACAC.. / CACA..)."""
    eng = engine(16, 250, k)
    B, te = 1030, 16
    sig, dur, _ = make_inputs(te, 250, B=B, seed=k)
    rng = np.random.default_rng(k)
    nv = rng.integers(1, te + 1, B).astype(np.uint8)
    nv[::7] = te
    w = te + k - 1
    start = (np.arange(B) * w).astype(np.int64)
    flat = np.full(B * w + 1, ord("A"), np.uint8)
    want = expected(sig, dur, flat, start, nv, k)
    assert want[0, 0] == nv.sum() and not want[1:].any() and want[0, 1] > 1000
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv), want)
    flat = np.frombuffer(b"AC" * (B * w // 2 + 1), np.uint8)[:B * w + 1].copy()
    want = expected(sig, dur, flat, start, nv, k)
    assert (want[:, 0] > 0).sum() == 2 and want[:, 0].sum() == nv.sum()
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
        t = eng.kmer_table_new()
        for sl in order:
            got = accumulate(eng, sig, dur, flat, start, nv, t, rows=sl)
        assert np.array_equal(got, whole)
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv, t, rows=slice(0, 0)), whole)     # B == 0 changes nothing
    assert np.array_equal(accumulate(eng, sig, dur, flat, start, nv, t), 2 * whole)                   # a second call doubles it


@pytest.mark.parametrize("k", [1, 10])
def test_extremes(k):
    """64 / 1024: 64 chunks whose first k-mer owns all 1,024 samples at q = -32768."""
    eng = engine(64, 1024, k)
    B, te, ts = 64, 64, 1024
    sig = np.full((B, ts), np.float32(pa(-32768)), np.float32)
    dur = np.zeros((B, te), np.int32)
    dur[:, 0] = ts
    w = te + k - 1
    flat = np.frombuffer((b"G" * k + b"T" * (te - 1)) * B + b"_", np.uint8).copy()
    start = (np.arange(B) * w).astype(np.int64)
    nv = np.full(B, te, np.uint8)
    got = accumulate(eng, sig, dur, flat, start, nv)
    row = int("2" * k, 4)
    assert got[row].tolist()[1:] == [64, 64 * 1024, 64 * 1024 * 1024, -2 ** 31, 2 ** 46]
    assert got[:, 4].sum() == -2 ** 31 and got[:, 5].sum() == 2 ** 46 and got[:, 1].sum() == 64 and got[:, 0].sum() == 64 * 64
    assert np.array_equal(got, expected(sig, dur, flat, start, nv, k))


def test_argument_checks():
    eng = engine(16, 250, 9)
    sig, dur, _ = make_inputs(16, 250)
    flat, start, nv = make_letters(257, 16, 9, seed=1)
    s_d, d_d, f_d, c_d, n_d = dev_(eng, sig[:2], dur[:2], flat, start[:2], nv[:2])
    table = eng.kmer_table_new()
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    ok = [p(s_d), p(d_d), p(f_d), p(c_d), p(n_d), 2, *CAL, p(table)]
    for i in (0, 1, 2, 3, 4, 9):                              # each pointer NULL in turn (9: the table)
        args = list(ok)
        args[i] = None
        assert L.s2s_kmer_table_accumulate(eng._h, None, *args) == -1
    for i, v in ((5, -1), (6, 0.0), (7, 0.0)):                # B < 0, digitisation 0, range 0
        args = list(ok)
        args[i] = v
        assert L.s2s_kmer_table_accumulate(eng._h, None, *args) == -1
    assert L.s2s_kmer_table_accumulate(None, None, *ok) == -1
    args = list(ok)
    args[5] = 0
    assert L.s2s_kmer_table_accumulate(eng._h, None, *args) == 0          # B == 0: a successful no-op
    torch.cuda.synchronize()
    assert not table.any()                                    # ... and none of them launched anything
    for bad in (lambda: eng.kmer_table_accumulate(s_d.double(), d_d, f_d, c_d, n_d, *CAL, table),
                lambda: eng.kmer_table_accumulate(s_d, d_d[:1], f_d, c_d, n_d, *CAL, table),
                lambda: eng.kmer_table_accumulate(s_d, d_d, f_d, c_d[:1], n_d, *CAL, table),
                lambda: eng.kmer_table_accumulate(s_d, d_d, f_d, c_d, n_d.int(), *CAL, table),
                lambda: eng.kmer_table_accumulate(s_d, d_d, f_d, c_d, n_d, 0.0, 1.0, 0.0, table),
                lambda: eng.kmer_table_accumulate(s_d, d_d, f_d, c_d, n_d, *CAL, table[:-1]),
                lambda: eng.kmer_table_accumulate(s_d, d_d, f_d, c_d, n_d, *CAL, table.int()),
                lambda: eng.kmer_table_accumulate(s_d, d_d, f_d, c_d, n_d, *CAL, table.cpu())):
        with pytest.raises(ValueError):
            bad()
    # k = 16 (the envelope's hd24 model): refused by the library, with the limit in the message
    big = S.Engine(GM.geometry_state_dict("hd24", EM.CASES), EM.envelope_config("hd24"))
    assert big.k == 16
    with pytest.raises(ValueError, match=r"1\.\.10"):
        big.kmer_table_new()
    z = torch.zeros(64, dtype=torch.uint8, device=big.device)
    rc = L.s2s_kmer_table_accumulate(big._h, None, p(z), p(z), p(z), p(z), p(z), 1, *CAL, p(z))
    assert rc == -1 and re.search(r"seq_kmer 1\.\.10\b", L.s2s_last_error(big._h).decode())
    torch.cuda.synchronize()
    assert not z.any()
    big.close()


# ---------------------------------------------------------------------------------------------------------- predict end to end
SEED = 11
PROFILE = "dna-r10-prom"


def _run(out, events=None, kmer_table=None):
    """`predict FASTA --read-input --preserve-read-ids -o out --seed 11 [--events ...] [--kmer-table ...]` in this process."""
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=FASTA, read_input=True, n=-1, r=400, c=-1, out=str(out),
                  profile=PROFILE, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                  distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None, digitisation=None,
                  range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None, min_noise=0.0,
                  min_duration=3, min_read_len=30, preserve_read_ids=True, seed=SEED,
                  events=None if events is None else str(events), kmer_table=None if kmer_table is None else str(kmer_table))


def _masked(path):
    """The file's bytes with the header's wall-clock attribute blanked."""
    return re.sub(rb"@exp_start_time\t[^\n]*", b"@exp_start_time\t-", open(path, "rb").read())


@pytest.fixture(scope="module")
def reconstruction():
    """The table of `predict` on the reads of example_test.fasta from first principles, once: Engine.predict_packed on all chunks at
    once (same seed, first_global_chunk 0), the numpy restatement of the slot statistics, the reduction by k-mer code."""
    eng = engine(16, 250, 9)
    reads = [(s, n) for s, n in U.read_fasta(FASTA) if n_chunks(len(s), 9) > 0]
    prof = U.get_profile(PROFILE)
    cal = (prof["digitisation"], prof["range"], prof["offset_mean"])
    params = S.PredictParams(dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0,
                             min_duration=3.0, seed=SEED)
    flat, start, nv, _ = pack_reads([s for s, _ in reads], 9)
    out = eng.predict_packed(*dev_(eng, flat, start, nv), params, first_global_chunk=0)
    sig, dur = out["signal"].cpu().numpy(), out["dur"].cpu().numpy()
    counts = ref_kmer_table(*ref_event_stats(sig, dur, *cal), kmer_codes(flat, start, nv, 9, 16), 9)
    assert counts[:, 0].sum() == sum(len(s) - 8 for s, _ in reads) and counts[:, 2].sum() > 1000
    return dict(reads=reads, counts=counts, cal=cal, text=py_table(counts, 9, *cal))


def test_run_streaming_writes_the_reconstructed_table(reconstruction, tmp_path):
    """8 chunks per super-batch: the reads spread over several launches that add into one table; nothing is formatted per batch."""
    from seq2squiggle_amd.inference import get_writer, run_streaming
    from seq2squiggle_amd.model import seq2squiggle
    prof = U.get_profile(PROFILE)
    for name, max_chunks in (("split", 8), ("whole", 32768)):
        U.set_seeds(SEED)
        writer, _ = get_writer(str(tmp_path / f"{name}.blow5"), prof, False, 1000000, PROFILE, True)
        model = seq2squiggle.load_from_checkpoint(checkpoint_path=CKPT, out_writer=writer, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0,
                                                  noise_sampling=True, duration_sampling=True, export_every_n_samples=1000000,
                                                  min_noise=0.0, min_duration=3, device=0, seed=SEED)
        trace = []
        run_streaming(model, reconstruction["reads"], writer, prof, PROFILE, max_chunks=max_chunks, trace=trace,
                      kmer_table=str(tmp_path / f"{name}.tsv"))
        assert sum(1 for ev, _ in trace if ev == "h2d+launch") >= (4 if name == "split" else 1)
        assert sum(1 for ev, _ in trace if ev == "kmer table") == 1 and not any(ev in ("events", "alignment") for ev, _ in trace)
        assert open(tmp_path / f"{name}.tsv", "rb").read() == reconstruction["text"]
    # no reads: a header-only file; a file object works as well as a path
    U.set_seeds(SEED)
    writer, _ = get_writer(str(tmp_path / "none.blow5"), prof, False, 1000000, PROFILE, True)
    with open(tmp_path / "none.tsv", "wb") as f:
        run_streaming(model, [], writer, prof, PROFILE, kmer_table=f)
    assert open(tmp_path / "none.tsv", "rb").read() == reconstruction["text"].split(b"\n")[0] + b"\n"


def test_the_option_changes_no_other_file(reconstruction, tmp_path):
    d = tmp_path
    _run(d / "plain.blow5")
    _run(d / "ev.blow5", events=d / "ev.tsv")
    _run(d / "tab.blow5", kmer_table=d / "tab.tsv")
    _run(d / "both.blow5", events=d / "both_ev.tsv", kmer_table=d / "both.tsv")
    assert _masked(d / "plain.blow5") == _masked(d / "ev.blow5") == _masked(d / "tab.blow5") == _masked(d / "both.blow5")
    assert open(d / "ev.tsv", "rb").read() == open(d / "both_ev.tsv", "rb").read()
    assert open(d / "tab.tsv", "rb").read() == open(d / "both.tsv", "rb").read() == reconstruction["text"]
    _run(d / "npz.blow5", kmer_table=d / "r.npz")               # a path ending in .npz receives the counts (a rank's file)
    counts, k, cal = load_counts(str(d / "r.npz"))
    assert np.array_equal(counts, reconstruction["counts"]) and k == 9
    assert cal == tuple(float(np.float32(x)) for x in reconstruction["cal"])


ENV0 = {k_: v for k_, v in os.environ.items() if k_ not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "S2S_ONE_GPU")}
CLI = [sys.executable, "-m", "seq2squiggle_amd", "predict", LAMBDA, "-n", "30", "-r", "1500", "-m", CKPT, "--seed", "5"]


@pytest.fixture(scope="module")
def cli_single(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmer_table_cli")
    r = subprocess.run(["timeout", "-k", "10", "300", *CLI, "-o", str(d / "one.blow5"), "--events", str(d / "one_ev.tsv"), "--kmer-table",
                        str(d / "one.tsv")], cwd=ROOT, capture_output=True, text=True, timeout=330, env=ENV0)
    assert r.returncode == 0, r.stderr[-3000:]
    return d


def test_cli_table_is_the_group_by_of_the_event_table(cli_single):
    table = parse_table(open(cli_single / "one.tsv", "rb").read())
    events = parse_events(open(cli_single / "one_ev.tsv", "rb").read(), False)
    groups = {}
    for r in events:
        name = r["model_kmer"] if set(r["model_kmer"]) <= set("ACGT") else "N" * 9
        g = groups.setdefault(name, [0, 0, 0.0])
        n = r["end_idx"] - r["start_idx"]
        g[0] += 1
        g[1] += n
        g[2] += n * float(r["mean"])
    assert len(events) > 1000 and set(groups) == {name for name, row in table.items() if row["n_events"] > 0}
    for name, (e, n, weighted) in groups.items():
        row = table[name]
        assert (row["n_events"], row["n_samples"]) == (e, n) and row["n_occ"] >= e
        # each side is rounded to "%.4f": 5e-5 + 5e-5, plus float slack
        assert abs(float(row["level_mean"]) - weighted / n) <= 1.01e-4, name
        assert row["dwell_mean"] == "%.4f" % (float(n) / float(e))
    assert all(row["level_mean"] == "nan" for row in table.values() if row["n_events"] == 0)


def test_three_ranks_sum_to_the_single_process_table(cli_single, tmp_path):
    want = open(cli_single / "one.tsv", "rb").read()
    run = lambda *a: subprocess.run(["timeout", "-k", "10", "600", *CLI, *a], cwd=ROOT, capture_output=True, text=True, timeout=630,
                                    env=dict(ENV0, S2S_ONE_GPU="1"))
    r = run("-o", str(tmp_path / "a.blow5"), "--gpus", "3", "--kmer-table", str(tmp_path / "a.tsv"))
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert open(tmp_path / "a.tsv", "rb").read() == want
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("a.")) == ["a.blow5", "a.tsv"]       # no .rankR.npz is left
    r = run("-o", str(tmp_path / "b.blow5"), "--gpus", "3", "--kmer-table", str(tmp_path / "b.tsv"), "--keep-shards")
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    shards = [str(tmp_path / f"b.rank{rank}.npz") for rank in range(3)]
    assert all(os.path.exists(p) for p in shards) and open(tmp_path / "b.tsv", "rb").read() == want
    join_rank_files(shards, str(tmp_path / "joined.tsv"), keep=True)
    assert open(tmp_path / "joined.tsv", "rb").read() == want
