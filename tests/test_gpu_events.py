"""`predict --events` on the GPU: s2s_event_stats against the numpy restatement of its definition (tests/_events_ref.py) over the
chunk geometries, and the event table of whole `predict` runs against a reconstruction from Engine.predict_packed + export_reads.
Every comparison is between integers or bytes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _lib, signal_io
from seq2squiggle_amd import utils as U
from seq2squiggle_amd.chunker import n_chunks, pack_reads
import _geometry_models as GM
from _alignment_ref import kmer_counts, parse_line
from _events_ref import parse_events, py_events, ref_dac, ref_event_stats
from conftest import GOLDEN, load_ckpt

pytestmark = pytest.mark.gpu

CKPT = os.path.join(GOLDEN, "synthetic_k9.ckpt")
FASTA = os.path.join(GOLDEN, "example_test.fasta")
CAL = (8192.0, 1024.0, 10.0)          # q = rint(8 v - 10): v = (q + 10) / 8 is exact in float32 for every q used below


def _c(seed, te, ts):
    return dict(seed=seed, seq_kmer=6, max_dna_len=te, max_signal_len=ts, dmodel=16, dff=8, encoder_heads=2, decoder_heads=1,
                pre_layers=0, encoder_layers=1, decoder_layers=1)


# dmodel 16 engines: the kernel only reads the handle's geometry
CASES = {"e16x250": _c(71, 16, 250), "e1x1": _c(72, 1, 1), "e5x37": _c(73, 5, 37), "e64x1024": _c(74, 64, 1024),
         "e17x1023": _c(75, 17, 1023)}
GEOMETRIES = ["tuned", "e16x250", "e1x1", "e5x37", "e64x1024", "e17x1023"]
_ENGINES = {}


def engine(tag):
    """One engine per geometry and session: "tuned" is the committed checkpoint on its split-f16 instance (16 / 250), "e16x250" a
    generic handle at the same geometry (both take the kernel's 250-row instance), the others run generic-geometry."""
    if tag not in _ENGINES:
        if tag == "tuned":
            sd, cfg = load_ckpt("k9")
            _ENGINES[tag] = S.Engine(sd, cfg)
        else:
            _ENGINES[tag] = S.Engine(GM.geometry_state_dict(tag, CASES), GM.geometry_config(tag, cases=CASES),
                                     mode="generic" if tag == "e16x250" else None)
    return _ENGINES[tag]


def pa(q):
    """The float32 pA whose stored int16 is q under CAL (before the wrap, for |q| beyond int16)."""
    return (np.asarray(q, np.float64) + 10.0) / 8.0


def make_inputs(te, ts, B=257, seed=0):
    """Crafted, not predicted: see the comments.  -> (signal float32 [B, ts], dur int32 [B, te])."""
    rng = np.random.default_rng(1000 * te + ts + seed)
    q = rng.integers(-3000, 3000, (B, ts))
    edge = rng.random((B, ts))
    q[edge < 0.02] = 32767
    q[(edge >= 0.02) & (edge < 0.04)] = -32767
    q[(edge >= 0.04) & (edge < 0.06)] = -32768
    q[(edge >= 0.06) & (edge < 0.08)] = 32768                 # beyond int16: wraps to -32768
    q[(edge >= 0.08) & (edge < 0.10)] = -40000                # ... wraps to 25536
    q[(edge >= 0.10) & (edge < 0.11)] = 70000
    sig = pa(q).astype(np.float32)
    half = edge >= 0.97                                       # exact halves: round to even
    sig[half] = ((rng.integers(-50, 50, (B, ts)) + 0.5 + 10.0) / 8.0).astype(np.float32)[half]
    sig[(edge >= 0.95) & (edge < 0.97)] = np.float32(3e38)    # the product overflows float32: clamps, then wraps
    kind = rng.random((B, ts))
    sig[kind < 0.25] = 0.0                                    # stripped by value, inside runs
    sig[(kind >= 0.25) & (kind < 0.30)] = -0.0                # ... minus zero is zero for the export
    sig[(kind >= 0.30) & (kind < 0.33)] = np.float32(1e-41)   # a subnormal is not: q = -10
    mean = max(1, ts // te)
    dur = rng.integers(0, 2 * mean + 2, (B, te)).astype(np.int64)
    dur[rng.random((B, te)) < 0.15] = 0                       # zero-dwell k-mers between others
    rows = []
    rows.append(np.zeros(te))                                 # everything is tail
    r = np.full(te, ts // te); r[-1] += ts - r.sum(); rows.append(r)              # a sum of exactly ts
    r = np.full(te, ts // te); r[-1] += ts - r.sum() + 3; rows.append(r)          # the last k-mer crosses ts: cropped
    r = np.full(te, 2); r[0] = ts + 5; rows.append(r)                             # cropped inside the first k-mer
    rows.append(np.full(te, 2 ** 31 - 1))                     # the sum saturates, it must not wrap
    r = np.full(te, mean); r[::2] = -7; rows.append(r)        # negative entries count as zero
    r = np.full(te, -(2 ** 31)); r[-1] = 3; rows.append(r)
    r = np.zeros(te); r[0] = 64; r[-1] = 64 if te > 1 else 0; rows.append(r)      # runs that end exactly on a multiple of 64
    r = np.zeros(te); r[0] = 60; r[-1] = 10 if te > 1 else 0; rows.append(r)      # a run that straddles a 64-sample pass
    r = np.zeros(te); r[0] = 1; r[-1] = 2 ** 31 - 1; rows.append(r)
    r = np.zeros(te); r[te // 2] = ts; rows.append(r)         # ONE run of the whole window ...
    for i, r in enumerate(rows):
        dur[i] = r
    sig[len(rows) - 1] = np.float32(pa(-32768))               # ... of q = -32768: the bounds of both accumulators at ts = 1024
    sig[len(rows)] = 0.0                                      # an all-zero chunk (random dwells)
    sig[len(rows) + 1] = np.float32(pa(32767))                # every sample at the top (random dwells)
    dur[200:200 + len(rows)] = dur[:len(rows)]                # ... the dwell rows again away from the front of the launch
    return sig, dur.astype(np.int32), len(rows) - 1


@pytest.mark.parametrize("tag", GEOMETRIES)
def test_event_stats_equals_its_definition(tag):
    eng = engine(tag)
    te, ts = eng.t_enc, eng.t_dec
    assert (te, ts) == ((16, 250) if tag == "tuned" else (CASES[tag]["max_dna_len"], CASES[tag]["max_signal_len"]))
    sig, dur, i_run = make_inputs(te, ts)
    q = ref_dac(sig, *CAL)
    assert {32767, -32767, -32768, 25536}.issubset(set(np.unique(q[sig != 0]).tolist())) or ts == 1
    seg, s, ss = ref_event_stats(sig, dur, *CAL)
    assert seg[i_run, te // 2] == ts and s[i_run, te // 2] == -32768 * ts and ss[i_run, te // 2] == ts * 2 ** 30
    sig_d, dur_d = torch.from_numpy(sig).to(eng.device), torch.from_numpy(dur).to(eng.device)
    full = eng.event_stats(sig_d, dur_d, *CAL)
    assert (full["seg"].dtype, full["sum"].dtype, full["sumsq"].dtype) == (torch.uint16, torch.int32, torch.int64)
    assert all(tuple(v.shape) == (257, te + 1) and v.data_ptr() % 16 == 0 for v in full.values())
    full = {k_: v.cpu().numpy() for k_, v in full.items()}
    assert np.array_equal(full["seg"], seg) and np.array_equal(full["sum"], s) and np.array_equal(full["sumsq"], ss)
    assert np.array_equal(full["seg"], eng.align_chunks(sig_d, dur_d).cpu().numpy())          # by definition the alignment's counts
    for B in (1, 3, 4, 5):                                    # less than, exactly and more than one workgroup of four chunks
        got = eng.event_stats(sig_d[:B].contiguous(), dur_d[:B].contiguous(), *CAL)
        assert all(np.array_equal(got[k_].cpu().numpy(), full[k_][:B]) for k_ in full), B
    for b in (203, 256):                                      # a chunk alone = the same chunk inside the 257
        got = eng.event_stats(sig_d[b:b + 1].contiguous(), dur_d[b:b + 1].contiguous(), *CAL)
        assert all(np.array_equal(got[k_].cpu().numpy()[0], full[k_][b]) for k_ in full), b
    # the sums are those of the int16 the export stores: one-chunk reads, slot after slot
    ex = eng.export_reads(sig_d, torch.arange(258, dtype=torch.int32, device=eng.device), *CAL, want_pa=False, want_dac=True)
    offs, dac = ex["offsets"].cpu().numpy(), ex["dac"].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.diff(offs), seg.sum(axis=1, dtype=np.int64))
    cuts = np.concatenate([[0], np.cumsum(seg.reshape(-1).astype(np.int64))])
    csum, csq = np.concatenate([[0], np.cumsum(dac[:offs[-1]])]), np.concatenate([[0], np.cumsum(dac[:offs[-1]] ** 2)])
    assert np.array_equal(np.diff(csum[cuts]), s.reshape(-1)) and np.array_equal(np.diff(csq[cuts]), ss.reshape(-1))
    # another calibration (a profile's own numbers), and out=: into a caller's buffer, nothing written behind the sections
    cal2 = (2048.0, 281.345551, -127.5655735)
    want = ref_event_stats(sig, dur, *cal2)
    size = eng.event_stats_layout(257, te)[3]
    buf = torch.full((size + 32,), 0xAB, dtype=torch.uint8, device=eng.device)
    got = eng.event_stats(sig_d, dur_d, *cal2, out=buf)
    assert got["seg"].data_ptr() == buf.data_ptr()
    assert all(np.array_equal(got[k_].cpu().numpy(), w) for k_, w in zip(("seg", "sum", "sumsq"), want))
    assert (buf[size:].cpu().numpy() == 0xAB).all()


def test_event_stats_argument_checks():
    eng = engine("tuned")
    sig = torch.zeros(2, 250, device=eng.device)
    dur = torch.zeros(2, 16, dtype=torch.int32, device=eng.device)
    assert all(tuple(v.shape) == (0, 17) for v in eng.event_stats(sig[:0], dur[:0], *CAL).values())
    small = torch.zeros(eng.event_stats_layout(2, 16)[3] - 1, dtype=torch.uint8, device=eng.device)
    for bad in (lambda: eng.event_stats(sig.double(), dur, *CAL), lambda: eng.event_stats(sig, dur.long(), *CAL),
                lambda: eng.event_stats(sig[:, :249].contiguous(), dur, *CAL), lambda: eng.event_stats(sig, dur[:1], *CAL),
                lambda: eng.event_stats(sig.cpu(), dur, *CAL), lambda: eng.event_stats(sig, dur, 0.0, 1.0, 0.0),
                lambda: eng.event_stats(sig, dur, 1.0, 0.0, 0.0), lambda: eng.event_stats(sig, dur, *CAL, out=small),
                lambda: eng.event_stats(sig, dur, *CAL, out=torch.zeros(600, dtype=torch.uint8, device=eng.device)[8:])):
        with pytest.raises(ValueError):
            bad()
    L = _lib.lib()
    out = torch.zeros(544, dtype=torch.uint8, device=eng.device)
    p = lambda t, at=0: C.c_void_p(t.data_ptr() + at)
    o = (p(out), p(out, 128), p(out, 272))
    assert L.s2s_event_stats(eng._h, None, p(sig), p(dur), 0, *CAL, *o) == 0           # B == 0: a successful no-op
    assert L.s2s_event_stats(eng._h, None, p(sig), p(dur), -1, *CAL, *o) == -1
    for args in ((None, p(dur), 2, *CAL, *o), (p(sig), None, 2, *CAL, *o), (p(sig), p(dur), 2, *CAL, None, o[1], o[2]),
                 (p(sig), p(dur), 2, *CAL, o[0], None, o[2]), (p(sig), p(dur), 2, *CAL, o[0], o[1], None),
                 (p(sig), p(dur), 2, 0.0, 1.0, 0.0, *o), (p(sig), p(dur), 2, 1.0, 0.0, 0.0, *o)):
        assert L.s2s_event_stats(eng._h, None, *args) == -1
    assert L.s2s_event_stats(None, None, p(sig), p(dur), 2, *CAL, *o) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()                     # ... and none of them launched anything


# ---------------------------------------------------------------------------------------------------------- predict end to end
SEED = 11


def _run(out, profile="dna-r10-prom", read_input=False, preserve=False, alignment=None, events=None, samples=False, dwell_mean=None):
    """`predict FASTA -n 20 -r 400 -o out --seed 11 [--events ...]` with the command's defaults, in this process."""
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=FASTA, read_input=read_input, n=-1 if read_input else 20, r=400,
                  c=-1, out=str(out), profile=profile, dwell_mean=dwell_mean, dwell_std=0.0, noise_std=2.0, noise_sampling=True,
                  duration_sampling=True, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None,
                  bps=None, digitisation=None, range_val=None, offset_mean=None, offset_std=None, median_before_mean=None,
                  median_before_std=None, min_noise=0.0, min_duration=3, min_read_len=30, preserve_read_ids=preserve, seed=SEED,
                  alignment=None if alignment is None else str(alignment), events=None if events is None else str(events),
                  events_samples=samples)


def _sampled_reads(profile="dna-r10-prom"):
    """The reads `predict -n 20 -r 400 --seed 11` samples, replayed."""
    from seq2squiggle_amd.cli import set_config
    U.set_seeds(SEED)
    cfg = U.update_config(profile, set_config(None))
    reads, _ = U.get_reads(FASTA, False, 20, 400, -1, cfg, "expon", SEED, profile, 30)
    return [(s, n) for s, n in reads if n_chunks(len(s), 9) > 0]


_RECON = {}


def _reconstruct(reads, profile, rna=False, dwell_mean=None):
    """What the table is made from, from first principles and once per (reads, profile): Engine.predict_packed on all chunks at once
    (same seed, first_global_chunk 0), export_reads for the offsets and the stored samples, the numpy restatement for the sums.
    -> a function (ids, samples, header) -> the expected text, and the export's offsets."""
    key = (profile, rna, dwell_mean, len(reads))
    if key not in _RECON:
        eng = engine("tuned")
        prof = U.get_profile(profile)
        cal = (prof["digitisation"], prof["range"], prof["offset_mean"])
        params = S.PredictParams(dwell_mean=dwell_mean if dwell_mean is not None else prof["sample_rate"] / prof["bps"], dwell_std=0.0,
                                 noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, min_duration=3.0, seed=SEED)
        flat, chunk_start, n_valid, read_first = pack_reads([s for s, _ in reads], 9)
        dev = eng.device
        out = eng.predict_packed(torch.from_numpy(flat).to(dev), torch.from_numpy(chunk_start).to(dev), torch.from_numpy(n_valid).to(dev),
                                 params, first_global_chunk=0)
        ex = eng.export_reads(out["signal"], torch.from_numpy(read_first).to(dev), *cal, rna=rna, want_pa=False, want_dac=True)
        offs, dac = ex["offsets"].cpu().numpy(), ex["dac"].cpu().numpy()
        seg, s, ss = ref_event_stats(out["signal"].cpu().numpy(), out["dur"].cpu().numpy(), *cal)
        assert np.array_equal(np.diff(offs), [seg[read_first[r]:read_first[r + 1]].sum() for r in range(len(reads))])
        kmers = [len(s_) - 9 + 1 for s_, _ in reads]
        seqs = [s_ for s_, _ in reads]
        _RECON[key] = (lambda ids, samples, header=True: py_events(seg, s, ss, 16, read_first, kmers, offs, ids, seqs, 9, *cal, rna,
                                                                   dac=dac if samples else None, with_header=header), offs, cal)
    return _RECON[key]


def _masked(path):
    """The file's bytes with the header's wall-clock attribute blanked."""
    return re.sub(rb"@exp_start_time\t[^\n]*", b"@exp_start_time\t-", open(path, "rb").read())


@pytest.fixture(scope="module")
def dna_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("events")
    _run(d / "plain.blow5")
    _run(d / "align.blow5", alignment=d / "align.paf")
    _run(d / "ev.blow5", events=d / "ev.tsv")
    _run(d / "both.blow5", alignment=d / "both.paf", events=d / "both.tsv", samples=True)
    reads = _sampled_reads()
    _, recs = signal_io.read_blow5(str(d / "both.blow5"))
    return dict(dir=d, reads=reads, recs=recs, ids=[r["read_id"] for r in recs])


def test_signal_file_and_paf_do_not_change_and_the_table_is_the_reconstruction(dna_runs):
    d = dna_runs["dir"]
    plain = _masked(d / "plain.blow5")
    assert plain == _masked(d / "ev.blow5") == _masked(d / "both.blow5") == _masked(d / "align.blow5")
    paf = open(d / "align.paf", "rb").read()
    assert paf == open(d / "both.paf", "rb").read() and paf.count(b"\n") == len(dna_runs["recs"]) >= 10
    expect, offs, _ = _reconstruct(dna_runs["reads"], "dna-r10-prom")
    assert np.diff(offs).tolist() == [r["len_raw_signal"] for r in dna_runs["recs"]]
    assert open(d / "ev.tsv", "rb").read() == expect(dna_runs["ids"], False)
    assert open(d / "both.tsv", "rb").read() == expect(dna_runs["ids"], True)


def test_rows_agree_with_the_paf_and_with_the_samples_read_back(dna_runs):
    """The calibration of the recomputation is the one the conversion ran with -- the record's digitisation and range and the
    profile's offset_mean, each as the float32 the library is handed: the reference's writer stores a per-record DRAW around
    offset_mean as the record's offset (offset_std), which shifts a reader's levels by a constant per record and leaves the
    deviation alone."""
    d = dna_runs["dir"]
    rows = parse_events(open(d / "both.tsv", "rb").read(), True)
    lines = [parse_line(x) for x in open(d / "both.paf").read().splitlines()]
    off = float(np.float32(U.get_profile("dna-r10-prom")["offset_mean"]))
    seen = 0
    for rec, line, (seq, _) in zip(dna_runs["recs"], lines, dna_runs["reads"]):
        mine = [r for r in rows if r["read_name"] == rec["read_id"]]
        seen += len(mine)
        assert [r["end_idx"] - r["start_idx"] for r in mine] == [n for n in kmer_counts(line) if n]      # the PAF's `N,` tokens in order
        assert [r["position"] for r in mine] == [i for i, n in enumerate(kmer_counts(line)) if n]
        dig, rng = float(np.float32(rec["digitisation"])), float(np.float32(rec["range"]))
        sig = np.asarray(rec["signal"]).astype(np.float64)
        for r in mine:
            assert r["model_kmer"] == seq[r["position"]: r["position"] + 9]
            x = sig[r["start_idx"]: r["end_idx"]]
            n, S_, Q_ = len(x), int(x.sum()), int((x * x).sum())
            assert r["mean"] == "%.4f" % ((S_ / n + off) * rng / dig)
            assert r["stdv"] == "%.4f" % (np.sqrt(float(max(n * Q_ - S_ * S_, 0))) / n * rng / dig)
            assert abs(float(r["stdv"]) - x.std() * abs(rng / dig)) < 1e-4 and abs(float(r["mean"]) - (x.mean() + off) * rng / dig) < 1e-4
            assert r["samples"] == ["%.3f" % ((v + off) * rng / dig) for v in x]
    assert seen == len(rows) > 100


def test_super_batches_that_split_the_reads_write_the_same_table(dna_runs, tmp_path):
    """run_streaming with 8 chunks per super-batch: the reads spread over several launches, one header, rows in record order."""
    from seq2squiggle_amd.inference import get_writer, run_streaming
    from seq2squiggle_amd.model import seq2squiggle
    prof = U.get_profile("dna-r10-prom")
    U.set_seeds(SEED)
    writer, _ = get_writer(str(tmp_path / "split.blow5"), prof, False, 1000000, "dna-r10-prom", False)
    model = seq2squiggle.load_from_checkpoint(checkpoint_path=CKPT, out_writer=writer, dwell_mean=prof["sample_rate"] / prof["bps"],
                                              dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                                              export_every_n_samples=1000000, min_noise=0.0, min_duration=3, device=0, seed=SEED)
    trace = []
    with open(tmp_path / "split.tsv", "wb") as f:                        # (a file object works as well as a path)
        run_streaming(model, dna_runs["reads"], writer, prof, "dna-r10-prom", max_chunks=8, trace=trace, events=f, events_samples=True)
    assert sum(1 for ev, _ in trace if ev == "h2d+launch") >= 4 and not any(ev == "alignment" for ev, _ in trace)
    assert open(tmp_path / "split.tsv", "rb").read() == open(dna_runs["dir"] / "both.tsv", "rb").read()


@pytest.mark.parametrize("profile", ["dna-r10-min", "rna-004-min"])
def test_coded_signal_writer_and_an_rna_profile(profile, tmp_path, monkeypatch):
    """BLOW5 with svb-zd signal compression takes the coded-signal path (the samples ride behind the blobs); rna-004-min accepts the
    committed k = 9 checkpoint and stores every read reversed, so start_idx falls as position rises."""
    rna = profile.startswith("rna")
    reads = [(s, n) for s, n in U.read_fasta(FASTA) if n_chunks(len(s), 9) > 0]
    ids = [n for _, n in reads]
    expect, _, _ = _reconstruct(reads, profile, rna=rna, dwell_mean=20.0)
    texts = {}
    for coded in (False, True):
        monkeypatch.setenv("S2S_BLOW5_SIGNAL", "svb-zd" if coded else "none")
        for samples in (False, True):
            out, tsv = tmp_path / f"{coded}{samples}.blow5", tmp_path / f"{coded}{samples}.tsv"
            _run(out, profile=profile, read_input=True, preserve=True, events=tsv, samples=samples, dwell_mean=20.0)
            texts[coded, samples] = open(tsv, "rb").read()
            assert texts[coded, samples] == expect(ids, samples), (coded, samples)
    rows = parse_events(texts[True, True], True)
    first = [r for r in rows if r["read_name"] == rows[0]["read_name"]]
    starts = [r["start_idx"] for r in first]
    assert len(first) > 5 and starts == sorted(starts, reverse=rna)
