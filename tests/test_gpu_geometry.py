"""The chunk-geometry instance (S2S_MODE_GENERIC_GEOMETRY) on the GPU.

Against the imported reference's vectors at other max_dna_len / max_signal_len (tests/golden/geometry_*.npz; the checkpoints are
rebuilt from tests/_geometry_models.py), against S2S_MODE_GENERIC at 16 / 250 bit for bit, through the sub-module operators, the
streaming and predict_step paths, the CLI into .blow5 / .pod5 and a two-rank sharded run.  Tolerances are
tests/test_gpu_generic.py's: dwell indices bit-exact, zero pattern exact, MAE < 1e-4 pA, max < 2e-3 pA."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import chunker, signal_io
from seq2squiggle_amd import utils as U
from oracle import s2s_oracle as O
from conftest import GOLDEN, ROOT, load_npz
from _bounds import MAE_TOL, MAX_TOL  # noqa: F401  (1e-4, 2e-3 pA; other test modules import them from here)
from _geometry_models import CASES, checkpoint_path
from _sized_models import checkpoint_path as sized_checkpoint_path

pytestmark = pytest.mark.gpu
STAGE_TOL = dict(emb=2e-6, enc=2e-5, sig=2e-6, rel=2e-6, y=2e-5)


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return base


MODES = [
    ("y_gamma_nsamp", dict(), True, True, False),
    ("y_gamma_nconst", dict(noise_sampling=False), True, True, False),
    ("y_ideal", dict(noise_std=0.0, noise_sampling=False, duration_sampling=False), False, False, False),
    ("y_normal_nsamp", dict(duration_sampling=False, dwell_std=4.0), False, True, True),
    ("y_ideal_dwell31", dict(noise_std=0.0, noise_sampling=False, duration_sampling=False, dwell_mean=4000 / 130), False, False, False),
]


@pytest.fixture(scope="module", params=list(CASES))
def gcase(request):
    tag = request.param
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    eng = S.Engine(sd, cfg)
    assert eng.mode == "generic-geometry" and (eng.t_enc, eng.t_dec) == (cfg["max_dna_len"], cfg["max_signal_len"])
    g = load_npz(f"geometry_{tag}.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    assert np.array_equal(nv, g["n_valid"])
    dev = eng.device
    yield dict(tag=tag, sd=sd, cfg=cfg, eng=eng, g=g, bases=torch.from_numpy(bases).to(dev), nv=torch.from_numpy(nv).to(dev), dev=dev)
    eng.close()


def dev_t(case, key):
    return torch.from_numpy(np.ascontiguousarray(case["g"][key]).astype(np.float32)).to(case["dev"])


def close(y, ref):
    assert y.shape == ref.shape
    assert np.array_equal(y == 0, ref == 0)
    d = np.abs(y - ref)
    assert d.mean() < MAE_TOL and d.max() < MAX_TOL, (d.mean(), d.max())


def test_stage_outputs(gcase):
    g, eng, t = gcase["g"], gcase["eng"], STAGE_TOL
    out = eng.predict_chunks(gcase["bases"], gcase["nv"], S.PredictParams(**P(noise_std=0.0)), inject_g=dev_t(gcase, "g"), debug=True)
    torch.cuda.synchronize()
    B, te, d = g["codes"].shape[0], eng.t_enc, eng.dmodel
    assert out["emb_out"].shape == (B, te, d) and out["y_scaled"].shape == (B, eng.t_dec)
    assert np.abs(out["emb_out"].cpu().numpy() - g["emb_out"]).max() < t["emb"]
    assert np.abs(out["enc_out"].cpu().numpy() - g["enc_out"]).max() < t["enc"]
    assert np.abs(out["sigma"].cpu().numpy() - g["sigma"]).max() < t["sig"]
    assert np.allclose(out["conc"].cpu().numpy(), g["conc"], rtol=t["rel"], atol=t["rel"])
    assert np.allclose(out["rate"].cpu().numpy(), g["rate"], rtol=t["rel"], atol=t["rel"])
    assert np.array_equal(out["dur"].cpu().numpy(), g["dur_gamma"])
    assert np.abs(out["y_scaled"].cpu().numpy() - g["y_scaled_gamma"]).max() < t["y"]


@pytest.mark.parametrize("key,over,use_g,use_z,use_zdw", MODES)
def test_predict_modes_vs_reference_goldens(gcase, key, over, use_g, use_z, use_zdw):
    g, eng = gcase["g"], gcase["eng"]
    out = eng.predict_chunks(gcase["bases"], gcase["nv"], S.PredictParams(**P(**over)),
                             inject_g=dev_t(gcase, "g") if use_g else None,
                             inject_z01=dev_t(gcase, "z01") if use_z else None,
                             inject_zdw=dev_t(gcase, "zdw") if use_zdw else None)
    close(out["signal"].cpu().numpy(), g[key])
    if use_g:
        assert np.array_equal(out["dur"].cpu().numpy(), g["dur_gamma"])
    if key == "y_normal_nsamp":
        assert np.array_equal(out["dur"].cpu().numpy(), g["dur_normal"])


def test_export_vs_reference(gcase):
    """s2s_export_reads on rows of max_signal_len samples: the reference's zero-stripped signal per read."""
    g, eng = gcase["g"], gcase["eng"]
    out = eng.predict_chunks(gcase["bases"], gcase["nv"], S.PredictParams(**P()), inject_g=dev_t(gcase, "g"),
                             inject_z01=dev_t(gcase, "z01"))
    names = [str(n) for n in g["names"]]
    order = [str(r) for r in g["export_reads"]]
    first = [names.index(r) for r in order] + [len(names)]
    ex = eng.export_reads(out["signal"], torch.tensor(first, dtype=torch.int32, device=gcase["dev"]), want_pa=True)
    offs = ex["offsets"].cpu().numpy()
    assert np.array_equal(offs, g["export_offsets"])
    pa = ex["pa"][: int(offs[-1])].cpu().numpy()
    d = np.abs(pa - g["export_pa"])
    assert d.mean() < MAE_TOL and d.max() < MAX_TOL


@pytest.mark.parametrize("source", ["k9", "d128"])
def test_default_geometry_equals_generic_bit_for_bit(source):
    """At 16 / 250 the geometry instance runs generic's kernels on generic's numbers: signal, dwell and every debug stage equal."""
    sd, cfg = S.load_checkpoint(os.path.join(GOLDEN, "synthetic_k9.ckpt") if source == "k9" else sized_checkpoint_path(source))
    rng = np.random.default_rng(3)
    reads = ["".join(rng.choice(list("ACGT"), int(n))) for n in rng.integers(9, 2000, size=40)]
    bases, nv, _ = S.encode_reads(reads, int(cfg["seq_kmer"]))
    bases, nv = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    outs = {}
    for mode in ("generic", "generic-geometry"):
        eng = S.Engine(sd, cfg, mode=mode)
        assert eng.mode == mode
        outs[mode] = (eng.predict_chunks(bases, nv, S.PredictParams(seed=42), first_global_chunk=77),
                      eng.predict_chunks(bases, nv, S.PredictParams(seed=5, dwell_std=3.0, duration_sampling=False), debug=True))
        torch.cuda.synchronize()
        eng.close()
    for a, b in zip(outs["generic"], outs["generic-geometry"]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


def _random_batch(k, te, B, seed):
    rng = np.random.default_rng(seed)
    reads = ["".join(rng.choice(list("ACGT"), int(n))) for n in rng.integers(k, 4000, size=max(1, B // 8))]
    bases, nv, _ = S.encode_reads(reads, k, te)
    while bases.shape[0] < B:
        bases, nv = np.concatenate([bases, bases]), np.concatenate([nv, nv])
    return torch.from_numpy(bases[:B].copy()).cuda(), torch.from_numpy(nv[:B].copy()).cuda()


def test_upper_edges_slices_determinism_packed_and_empty():
    """64 / 1024: a launch larger than one workspace slice equals the same chunks in two launches and itself, bit for bit; the packed
    entry point equals the plain one; B = 0 gives (0, 1024)."""
    sd, cfg = S.load_checkpoint(checkpoint_path("g64x1024"))
    eng = S.Engine(sd, cfg)
    k, te, ts, d, f = cfg["seq_kmer"], 64, 1024, cfg["dmodel"], cfg["dff"]
    slice_chunks = (512 << 20) // (4 * (te * d + te + ts * d + ts + max(te, ts) * max(3 * d, f)))
    n = slice_chunks + 13
    bases, nv = _random_batch(k, te, n, 3)
    p = S.PredictParams(seed=9)
    whole = eng.predict_chunks(bases, nv, p, first_global_chunk=100)
    again = eng.predict_chunks(bases, nv, p, first_global_chunk=100)
    m = n // 2
    a = eng.predict_chunks(bases[:m].contiguous(), nv[:m].contiguous(), p, first_global_chunk=100)
    b = eng.predict_chunks(bases[m:].contiguous(), nv[m:].contiguous(), p, first_global_chunk=100 + m)
    torch.cuda.synchronize()
    assert whole["signal"].shape == (n, ts) and whole["dur"].shape == (n, te)
    for key in ("signal", "dur"):
        assert torch.equal(whole[key], again[key])
        assert torch.equal(whole[key], torch.cat([a[key], b[key]]))
    assert (whole["signal"] > 0).any()
    assert eng.predict_chunks(bases[:0], nv[:0], p)["signal"].shape == (0, ts)
    reads = ["".join(np.random.default_rng(4).choice(list("ACGT"), L)) for L in (700, 64 + 8, 5000, 9, 1500)]
    rb, cs, pnv, _ = chunker.pack_reads(reads, k, te)
    ub, unv, _ = S.encode_reads(reads, k, te)
    packed = eng.predict_packed(torch.from_numpy(rb).cuda(), torch.from_numpy(cs).cuda(), torch.from_numpy(pnv).cuda(), p)
    plain = eng.predict_chunks(torch.from_numpy(ub).cuda(), torch.from_numpy(unv).cuda(), p)
    torch.cuda.synchronize()
    assert torch.equal(packed["signal"], plain["signal"]) and torch.equal(packed["dur"], plain["dur"])
    eng.close()


@pytest.mark.parametrize("tag", ["r16x500", "g5x37"])
def test_length_regulator_and_decoder_operators(tag):
    """modules.py's LengthRegulator and stand-alone Decoder at max_signal_len != 250 against the reference formulas (the oracle's
    restatement of LR at max_len = max_signal_len, Decoder.forward) and the reference's own stage vectors."""
    from seq2squiggle_amd.modules import Stages
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    eng = S.Engine(sd, cfg)
    dev, d, te, ts = eng.device, eng.dmodel, eng.t_enc, eng.t_dec
    gen = torch.Generator().manual_seed(11)
    B = 9
    emb = torch.rand(B, te, d, generator=gen) * 1.5
    x = torch.randn(B, te, d, generator=gen)
    sig = torch.rand(B, te, 1, generator=gen)
    g_inj = torch.rand(B, te, generator=gen) * 40
    st = Stages(eng, S.PredictParams(**P(noise_std=0.0)), inject_g=g_inj.to(dev))
    out, dur, _, noise_ext, _ = st.length_regulator(emb.to(dev), x.to(dev), sig.to(dev), max_length=ts)
    ref_dur = torch.round(torch.clamp(torch.clamp(g_inj, min=1.0), min=3.0))
    ref_out, ref_sx = O.length_regulate(x, sig[..., 0], ref_dur, max_len=ts)
    assert out.shape == (B, ts, d) and np.array_equal(dur.cpu().numpy(), ref_dur.numpy())
    assert torch.equal(out.cpu(), ref_out) and torch.equal(noise_ext[..., 0].cpu(), ref_sx)
    h = torch.randn(B, ts, d, generator=gen) * 0.7
    y = st.decoder(h.to(dev))[..., 0].cpu().numpy()
    ref_y = O.decoder(sd, cfg, h).numpy()
    assert not ((y == 0) != (ref_y == 0)).any() and np.abs(y - ref_y).max() < 6e-5
    # chained like predict_step, against the reference's stage vectors
    g = load_npz(f"geometry_{tag}.npz")
    codes = torch.from_numpy(g["codes"].astype(np.int64))
    onehot = torch.zeros(*codes.shape, 5)
    onehot[codes < 5] = torch.nn.functional.one_hot(codes[codes < 5], 5).float()
    st2 = Stages(eng, S.PredictParams(**P(noise_std=0.0)), inject_g=torch.from_numpy(g["g"]).to(dev))
    enc_out, emb_out = st2.encoder(onehot.reshape(codes.shape[0], te, -1).to(dev))
    lr, dur2, _, _, _ = st2.length_regulator(emb_out, enc_out, st2.noise_sampler(emb_out))
    assert np.array_equal(dur2.cpu().numpy(), g["dur_gamma"].astype(np.float32))
    assert np.abs(st2.decoder(lr)[..., 0].cpu().numpy() - g["y_scaled_gamma"]).max() < STAGE_TOL["y"]
    eng.close()


def _reads_fasta(path):
    rng = np.random.default_rng(1)
    with open(path, "w") as f:
        for i, n in enumerate([5, 9, 40, 333, 1200, 16 + 8, 2500]):
            f.write(f">r{i}\n{''.join(rng.choice(list('ACGT'), n))}\n")


@pytest.mark.parametrize("ext", [".blow5", ".pod5"])
def test_streaming_and_predict_step_paths_agree_with_predict_chunks(tmp_path, ext):
    """rna-004-min with the RNA-shaped 16 / 500 checkpoint, samplers on: the streaming path (GPU export, svb rows of 500-sample
    chunks) writes the predict_step path's file, and every read holds the samples predict_chunks + export_reads give."""
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    from seq2squiggle_amd import pod5_io
    fa = tmp_path / "reads.fa"
    _reads_fasta(fa)
    outs = []
    for streaming in (True, False):
        out = tmp_path / f"s{int(streaming)}{ext}"
        np.random.seed(0)
        inference_run(config=set_config(None), saved_weights=checkpoint_path("r16x500"), fasta=str(fa), read_input=True, n=-1,
                      r=1000, c=-1, out=str(out), profile="rna-004-min", dwell_mean=None, dwell_std=0.0, noise_std=2.0,
                      noise_sampling=True, duration_sampling=True, distr="expon", predict_batch_size=64, export_every_n_samples=100,
                      sample_rate=None, bps=None, digitisation=None, range_val=None, offset_mean=None, offset_std=None,
                      median_before_mean=None, median_before_std=None, min_noise=0.0, min_duration=3, min_read_len=30,
                      preserve_read_ids=True, seed=11, streaming=streaming)
        outs.append(pod5_io.read_pod5(str(out))["reads"] if ext == ".pod5" else signal_io.read_blow5(str(out))[1])
    a, b = outs
    assert len(a) == len(b) == 6
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["signal"], rb["signal"])
    # per-read sample counts: predict_chunks + export_reads over the same reads with the same seed and chunk keys
    sd, cfg = S.load_checkpoint(checkpoint_path("r16x500"))
    eng = S.Engine(sd, cfg)
    seqs = [s for s, _ in U.read_fasta(str(fa))][1:]
    bases, nv, first = S.encode_reads(seqs, 9, 16)
    prof = U.get_profile("rna-004-min")
    pp = S.PredictParams(dwell_mean=prof["sample_rate"] / prof["bps"], noise_std=2.0, min_noise=0.0, min_duration=3, seed=11)
    out = eng.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), pp)
    ex = eng.export_reads(out["signal"], torch.from_numpy(first).cuda(), want_pa=True)
    counts = np.diff(ex["offsets"].cpu().numpy())
    assert [len(r["signal"]) for r in a] == list(counts)
    eng.close()


def test_cli_rna_checkpoint_and_two_rank_shards(tmp_path):
    """`predict -m <16 / 500 checkpoint> --profile rna-004-min` picks the geometry instance and says so; two ranks (one after the
    other, on GPU 0) carry exactly the single-process run's samples."""
    fa = tmp_path / "reads.fa"
    _reads_fasta(fa)
    base = [sys.executable, "-m", "seq2squiggle_amd", "predict", str(fa), "--read-input", "-m", checkpoint_path("r16x500"),
            "--profile", "rna-004-min", "--seed", "9", "--preserve-read-ids"]
    env0 = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "S2S_ONE_GPU")}
    r = subprocess.run(["timeout", "-k", "10", "600"] + base + ["-o", str(tmp_path / "one.blow5")], cwd=ROOT, capture_output=True,
                       text=True, timeout=660, env=env0)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (r.stdout + r.stderr).count("predict instance: generic-geometry") == 1
    _, one = signal_io.read_blow5(str(tmp_path / "one.blow5"))
    assert len(one) == 6
    parts = []
    for rank in range(2):
        env = dict(env0, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
        r = subprocess.run(["timeout", "-k", "10", "600"] + base + ["-o", str(tmp_path / "out.blow5")], cwd=ROOT, capture_output=True,
                           text=True, timeout=660, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        parts += signal_io.read_blow5(str(tmp_path / f"out.rank{rank}.blow5"))[1]
    assert len(parts) == len(one)
    for a, b in zip(parts, one):
        assert a["read_id"] == b["read_id"] and np.array_equal(a["signal"], b["signal"])
    r = subprocess.run(["timeout", "-k", "10", "600"] + base + ["-o", str(tmp_path / "x.pod5")], cwd=ROOT, capture_output=True,
                       text=True, timeout=660, env=env0)
    assert r.returncode == 0, r.stderr[-2000:]
    from seq2squiggle_amd import pod5_io
    p5 = pod5_io.read_pod5(str(tmp_path / "x.pod5"))["reads"]
    assert [len(x["signal"]) for x in p5] == [len(x["signal"]) for x in one]
