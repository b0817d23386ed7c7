"""`predict --alignment` on the GPU: s2s_align_chunks against the numpy restatement of its definition (tests/_alignment_ref.py) over
the chunk geometries, and the PAF file of whole `predict` runs against a reconstruction from Engine.predict_packed.  Every
comparison is between integers or bytes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _lib, signal_io
from seq2squiggle_amd import utils as U
from seq2squiggle_amd.chunker import n_chunks, pack_reads
import _geometry_models as GM
from _alignment_ref import kmer_counts, parse_line, py_format, ref_align
from conftest import GOLDEN, ROOT, load_ckpt

pytestmark = pytest.mark.gpu

CKPT = os.path.join(GOLDEN, "synthetic_k9.ckpt")
FASTA = os.path.join(GOLDEN, "example_test.fasta")


def _c(seed, te, ts):
    return dict(seed=seed, seq_kmer=6, max_dna_len=te, max_signal_len=ts, dmodel=16, dff=8, encoder_heads=2, decoder_heads=1,
                pre_layers=0, encoder_layers=1, decoder_layers=1)


# dmodel 16 engines: the kernel only reads the handle's geometry
CASES = {"a16x250": _c(61, 16, 250), "a1x1": _c(62, 1, 1), "a5x37": _c(63, 5, 37), "a64x1024": _c(64, 64, 1024),
         "a17x1023": _c(65, 17, 1023)}
GEOMETRIES = ["tuned", "a16x250", "a1x1", "a5x37", "a64x1024", "a17x1023"]
_ENGINES = {}


def engine(tag):
    """One engine per geometry and session: "tuned" is the committed checkpoint on its split-f16 instance (16 / 250), "a16x250" a
    generic handle at the same geometry (both take the kernel's 250-row instance), the others run generic-geometry."""
    if tag not in _ENGINES:
        if tag == "tuned":
            sd, cfg = load_ckpt("k9")
            _ENGINES[tag] = S.Engine(sd, cfg)
        else:
            _ENGINES[tag] = S.Engine(GM.geometry_state_dict(tag, CASES), GM.geometry_config(tag, cases=CASES),
                                     mode="generic" if tag == "a16x250" else None)
    return _ENGINES[tag]


def make_inputs(te, ts, B=257, seed=0):
    rng = np.random.default_rng(1000 * te + ts + seed)
    sig = rng.standard_normal((B, ts)).astype(np.float32) * 50
    kind = rng.random((B, ts))
    sig[kind < 1 / 3] = 0.0                                   # a third stripped by value
    sig[(kind >= 1 / 3) & (kind < 0.38)] = -0.0               # ... minus zero is zero for the export
    sig[(kind >= 0.38) & (kind < 0.43)] = np.float32(1e-41)   # a subnormal is not
    sig[(kind >= 0.43) & (kind < 0.45)] = np.float32(-1e-44)
    assert (sig != 0).sum() < sig.size and np.signbit(sig[sig == 0]).any() and (np.abs(sig[sig != 0]) < 1e-38).any()
    mean = max(1, ts // te)
    dur = rng.integers(0, 2 * mean + 2, (B, te)).astype(np.int64)
    dur[rng.random((B, te)) < 0.15] = 0                       # zero-dwell k-mers between others
    rows = []
    rows.append(np.zeros(te))                                 # everything is tail
    r = np.full(te, ts // te); r[-1] += ts - r.sum(); rows.append(r)              # a sum of exactly ts
    r = np.full(te, ts // te); r[-1] += ts - r.sum() + 3; rows.append(r)          # the last k-mer crosses ts
    r = np.full(te, 2); r[0] = ts + 5; rows.append(r)                             # cropped inside the first k-mer
    rows.append(np.full(te, 32767))
    rows.append(np.full(te, 2 ** 31 - 1))                     # the sum saturates, it must not wrap
    r = np.full(te, mean); r[::2] = -7; rows.append(r)        # negative entries count as zero
    r = np.full(te, -(2 ** 31)); r[-1] = 3; rows.append(r)
    r = np.zeros(te); r[::3] = mean + 1; rows.append(r)       # zero-dwell k-mers between others
    r = np.zeros(te); r[-1] = 2 ** 31 - 1; r[0] = 1; rows.append(r)
    for i, r in enumerate(rows):
        dur[i] = r
    dur[200:200 + len(rows)] = dur[:len(rows)]                # ... and again away from the front of the launch
    return sig, dur.astype(np.int32)


@pytest.mark.parametrize("tag", GEOMETRIES)
def test_align_chunks_equals_its_definition(tag):
    eng = engine(tag)
    te, ts = eng.t_enc, eng.t_dec
    assert (te, ts) == ((16, 250) if tag == "tuned" else (CASES[tag]["max_dna_len"], CASES[tag]["max_signal_len"]))
    sig, dur = make_inputs(te, ts)
    ref = ref_align(sig, dur)
    assert np.array_equal(ref.sum(axis=1), (sig != 0).sum(axis=1))
    sig_d, dur_d = torch.from_numpy(sig).to(eng.device), torch.from_numpy(dur).to(eng.device)
    full = eng.align_chunks(sig_d, dur_d)
    assert full.dtype == torch.uint16 and tuple(full.shape) == (257, te + 1)
    full = full.cpu().numpy()
    assert np.array_equal(full, ref)
    for B in (1, 3, 4, 5):                                    # less than, exactly and more than one workgroup of four chunks
        got = eng.align_chunks(sig_d[:B].contiguous(), dur_d[:B].contiguous()).cpu().numpy()
        assert np.array_equal(got, ref[:B]), B
    for b in (203, 256):                                      # a chunk alone = the same chunk inside the 257
        got = eng.align_chunks(sig_d[b:b + 1].contiguous(), dur_d[b:b + 1].contiguous()).cpu().numpy()
        assert np.array_equal(got[0], full[b]), b
    # one-chunk reads: the export's offsets are the running sum of the rows
    offs = eng.export_reads(sig_d, torch.arange(258, dtype=torch.int32, device=eng.device), want_pa=False)["offsets"].cpu().numpy()
    assert np.array_equal(np.diff(offs), full.sum(axis=1, dtype=np.int64))
    # out=: into a caller's buffer, nothing written behind the rows
    buf = torch.from_numpy(np.full(257 * (te + 1) + 8, 0xABCD, np.uint16)).to(eng.device)
    view = eng.align_chunks(sig_d, dur_d, out=buf)
    assert view.data_ptr() == buf.data_ptr() and np.array_equal(view.cpu().numpy(), ref)
    assert (buf[257 * (te + 1):].cpu().numpy() == 0xABCD).all()


def test_align_chunks_argument_checks():
    eng = engine("tuned")
    sig = torch.zeros(2, 250, device=eng.device)
    dur = torch.zeros(2, 16, dtype=torch.int32, device=eng.device)
    assert tuple(eng.align_chunks(sig[:0], dur[:0]).shape) == (0, 17)
    for bad in (lambda: eng.align_chunks(sig.double(), dur), lambda: eng.align_chunks(sig, dur.long()),
                lambda: eng.align_chunks(sig[:, :249].contiguous(), dur), lambda: eng.align_chunks(sig, dur[:1]),
                lambda: eng.align_chunks(sig.cpu(), dur), lambda: eng.align_chunks(sig, dur, out=torch.zeros(34, dtype=torch.int16, device=eng.device)),
                lambda: eng.align_chunks(sig, dur, out=torch.from_numpy(np.zeros(33, np.uint16)).to(eng.device))):
        with pytest.raises(ValueError):
            bad()
    L = _lib.lib()
    out = torch.from_numpy(np.zeros(34, np.uint16)).to(eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.s2s_align_chunks(eng._h, None, p(sig), p(dur), 0, p(out)) == 0           # B == 0: a successful no-op
    assert L.s2s_align_chunks(eng._h, None, p(sig), p(dur), -1, p(out)) == -1
    for args in ((None, p(dur), 2, p(out)), (p(sig), None, 2, p(out)), (p(sig), p(dur), 2, None)):
        assert L.s2s_align_chunks(eng._h, None, *args) == -1
    assert L.s2s_align_chunks(None, None, p(sig), p(dur), 2, p(out)) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------------------- predict end to end
SEED = 11


def _run(out, profile="dna-r10-prom", read_input=False, preserve=False, alignment=None, dwell_mean=None, fasta=FASTA):
    """`predict FASTA -n 20 -r 400 -o out --seed 11 [--alignment ...]` with the command's defaults, in this process."""
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=fasta, read_input=read_input, n=-1 if read_input else 20, r=400,
                  c=-1, out=str(out), profile=profile, dwell_mean=dwell_mean, dwell_std=0.0, noise_std=2.0, noise_sampling=True,
                  duration_sampling=True, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None,
                  bps=None, digitisation=None, range_val=None, offset_mean=None, offset_std=None, median_before_mean=None,
                  median_before_std=None, min_noise=0.0, min_duration=3, min_read_len=30, preserve_read_ids=preserve, seed=SEED,
                  alignment=None if alignment is None else str(alignment))


def _sampled_reads(profile="dna-r10-prom"):
    """The reads `predict -n 20 -r 400 --seed 11` samples, replayed (the sequences: their names are fresh uuid4 draws every time;
    reads longer than their contig are skipped, so there are fewer than 20)."""
    from seq2squiggle_amd.cli import set_config
    U.set_seeds(SEED)
    cfg = U.update_config(profile, set_config(None))
    reads, _ = U.get_reads(FASTA, False, 20, 400, -1, cfg, "expon", SEED, profile, 30)
    return [(s, n) for s, n in reads if n_chunks(len(s), 9) > 0]


def _reconstruct(reads, ids, profile, rna=False, dwell_mean=None):
    """The PAF text from first principles: Engine.predict_packed on all chunks at once (same seed, first_global_chunk 0), the
    numpy restatement of s2s_align_chunks, the Python formatter."""
    eng = engine("tuned")
    prof = U.get_profile(profile)
    params = S.PredictParams(dwell_mean=dwell_mean if dwell_mean is not None else prof["sample_rate"] / prof["bps"], dwell_std=0.0,
                             noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, min_duration=3.0, seed=SEED)
    flat, chunk_start, n_valid, read_first = pack_reads([s for s, _ in reads], 9)
    dev = eng.device
    out = eng.predict_packed(torch.from_numpy(flat).to(dev), torch.from_numpy(chunk_start).to(dev), torch.from_numpy(n_valid).to(dev),
                             params, first_global_chunk=0)
    seg = ref_align(out["signal"].cpu().numpy(), out["dur"].cpu().numpy())
    per_chunk = np.concatenate([[0], np.cumsum(seg.sum(axis=1, dtype=np.int64))])
    offs = per_chunk[read_first]
    kmers = [len(s) - 9 + 1 for s, _ in reads]
    assert all(k == 16 * (read_first[i + 1] - read_first[i] - 1) + int(n_valid[read_first[i + 1] - 1]) for i, k in enumerate(kmers))
    return py_format(seg, 16, read_first, kmers, offs, ids, rna), offs


def _masked(path):
    """The file's bytes with the header's wall-clock attribute blanked."""
    return re.sub(rb"@exp_start_time\t[^\n]*", b"@exp_start_time\t-", open(path, "rb").read())


def _check_against_records(paf: bytes, blow5) -> list:
    _, recs = signal_io.read_blow5(str(blow5))
    lines = [parse_line(x) for x in paf.decode().splitlines()]
    assert len(lines) == len(recs) > 0
    assert [d["read_id"] for d in lines] == [r["read_id"] for r in recs]
    assert [d["n"] for d in lines] == [r["len_raw_signal"] for r in recs] == [len(r["signal"]) for r in recs]
    return lines


@pytest.fixture(scope="module")
def dna_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("align")
    _run(d / "plain.blow5")
    _run(d / "with.blow5", alignment=d / "with.paf")
    reads = _sampled_reads()
    _, recs = signal_io.read_blow5(str(d / "with.blow5"))
    expected, offs = _reconstruct(reads, [r["read_id"] for r in recs], "dna-r10-prom")
    return dict(dir=d, reads=reads, expected=expected, offs=offs)


def test_the_signal_file_does_not_change_and_every_line_is_the_reconstruction(dna_runs):
    d = dna_runs["dir"]
    assert _masked(d / "plain.blow5") == _masked(d / "with.blow5")
    paf = open(d / "with.paf", "rb").read()
    lines = _check_against_records(paf, d / "with.blow5")
    assert len(lines) == len(dna_runs["reads"]) >= 10 and [x["n"] for x in lines] == np.diff(dna_runs["offs"]).tolist()
    assert paf == dna_runs["expected"]
    assert all((x["kmer_start"], x["kmer_end"]) == (0, x["K"]) and x["K"] == len(s) - 8 for x, (s, _) in zip(lines, dna_runs["reads"]))
    assert any(k == "D" for x in lines for _, k in x["toks"]) or any(k == "I" for x in lines for _, k in x["toks"])


def test_the_command_line_writes_the_same_two_files(dna_runs, tmp_path):
    r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "predict", FASTA, "-n", "20", "-r", "400", "-o", str(tmp_path / "cli.blow5"),
                        "-m", CKPT, "--seed", str(SEED), "--alignment", str(tmp_path / "cli.paf")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _masked(tmp_path / "cli.blow5") == _masked(dna_runs["dir"] / "plain.blow5")
    assert open(tmp_path / "cli.paf", "rb").read() == dna_runs["expected"]


def test_super_batches_that_split_the_reads_write_the_same_lines(dna_runs, tmp_path):
    """run_streaming with 8 chunks per super-batch: the reads spread over several launches, lines stay in record order."""
    from seq2squiggle_amd.inference import get_writer, run_streaming
    from seq2squiggle_amd.model import seq2squiggle
    prof = U.get_profile("dna-r10-prom")
    U.set_seeds(SEED)
    writer, _ = get_writer(str(tmp_path / "split.blow5"), prof, False, 1000000, "dna-r10-prom", False)
    model = seq2squiggle.load_from_checkpoint(checkpoint_path=CKPT, out_writer=writer, dwell_mean=prof["sample_rate"] / prof["bps"],
                                              dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                                              export_every_n_samples=1000000, min_noise=0.0, min_duration=3, device=0, seed=SEED)
    trace = []
    with open(tmp_path / "split.paf", "wb") as f:                        # (a file object works as well as a path)
        n = run_streaming(model, dna_runs["reads"], writer, prof, "dna-r10-prom", max_chunks=8, trace=trace, alignment=f)
    assert n == sum(n_chunks(len(s), 9) for s, _ in dna_runs["reads"])
    assert sum(1 for ev, _ in trace if ev == "h2d+launch") >= 4
    paf = open(tmp_path / "split.paf", "rb").read()
    _check_against_records(paf, tmp_path / "split.blow5")
    assert paf == dna_runs["expected"]


def test_preserved_read_ids_are_the_ids_of_the_lines(dna_runs, tmp_path):
    _run(tmp_path / "ids.blow5", preserve=True, alignment=tmp_path / "ids.paf")
    paf = open(tmp_path / "ids.paf", "rb").read()
    lines = _check_against_records(paf, tmp_path / "ids.blow5")
    names = [x["read_id"] for x in lines]                      # the sampled reads' own names (uuid4), no longer 00000000-...-N
    assert len(set(names)) == len(names) == len(dna_runs["reads"]) and not any(n.startswith("00000000-") for n in names)
    expected, _ = _reconstruct(dna_runs["reads"], names, "dna-r10-prom")
    assert paf == expected


def test_an_rna_profile_walks_the_kmers_backwards(tmp_path):
    """rna-004-min accepts the committed k = 9 checkpoint.  The same reads, seed and dwell mean under a DNA and an RNA profile
    predict the same chunks; the RNA signal is stored reversed per read, so its lines are the DNA lines walked backwards."""
    runs = {}
    for profile in ("dna-r10-min", "rna-004-min"):
        out, paf = tmp_path / f"{profile}.blow5", tmp_path / f"{profile}.paf"
        _run(out, profile=profile, read_input=True, preserve=True, alignment=paf, dwell_mean=20.0)    # (one dwell mean: the profiles' own differ)
        runs[profile] = (_check_against_records(open(paf, "rb").read(), out), open(paf, "rb").read())
    (dna, _), (rna, rna_text) = runs["dna-r10-min"], runs["rna-004-min"]
    assert len(dna) == len(rna) > 0
    for a, b in zip(dna, rna):
        assert (a["read_id"], a["n"], a["K"], a["mapped"]) == (b["read_id"], b["n"], b["K"], b["mapped"])
        assert (a["kmer_start"], a["kmer_end"]) == (0, a["K"]) and (b["kmer_start"], b["kmer_end"]) == (b["K"], 0)
        assert kmer_counts(b) == kmer_counts(a)[::-1] and b["toks"] == a["toks"][::-1]
        assert (b["sig_start"], b["sig_end"]) == (a["n"] - a["sig_end"], a["n"] - a["sig_start"])
    reads = [(s, n) for s, n in U.read_fasta(FASTA) if n_chunks(len(s), 9) > 0]
    expected, _ = _reconstruct(reads, [n for _, n in reads], "rna-004-min", rna=True, dwell_mean=20.0)
    assert rna_text == expected
