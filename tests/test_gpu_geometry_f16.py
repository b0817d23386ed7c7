"""The reduced-precision chunk-geometry instance (S2S_MODE_GENERIC_GEOMETRY_F16, compute mode "generic-geometry-f16") on the GPU.

Its bar is the reference's own GPU arithmetic, as for S2S_MODE_GENERIC_F16 (tests/test_gpu_generic_f16.py): the imported reference's
predict_step under fp16 autocast on the geometry cases' chunks with the same injected variates (tests/golden/geometry_mixed16.npz,
tools/make_geometry_mixed16_goldens.py).  Against the fp32 golden the mode must be at least as close as that reference, in MAE and
max, with its own dwell indices bit-exact (the encoder side is S2S_MODE_GENERIC_GEOMETRY's fp32 code: its stage outputs are
bit-equal to a "generic-geometry" engine's).  At 16 / 250 it computes S2S_MODE_GENERIC_F16's numbers bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import chunker, signal_io
from conftest import GOLDEN, ROOT, load_npz
from _geometry_models import CASES, checkpoint_path
from _sized_models import checkpoint_path as sized_checkpoint_path

pytestmark = pytest.mark.gpu
MODE = "generic-geometry-f16"
STAGES = ("emb_out", "enc_out", "sigma", "conc", "rate", "g", "dur")


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return base


def ref16_bar(tag, g):
    """The reference 16-mixed's MAE / max against the fp32 golden where its dwell indices agree with fp32's, re-derived from the
    committed vectors."""
    m16 = load_npz("geometry_mixed16.npz")
    r16, dur16 = m16[f"y_gamma_nsamp_16mixed_{tag}"], m16[f"dur_gamma_16mixed_{tag}"]
    agree = (dur16 == g["dur_gamma"]).all(1)
    d = np.abs(r16 - g["y_gamma_nsamp"])[agree]
    assert abs(d.mean() - float(m16[f"mae_vs_fp32_where_dwell_equal_{tag}"])) < 1e-6
    return d.mean(), d.max()


def _run(sd, cfg, mode, fn):
    eng = S.Engine(sd, cfg, mode=mode)
    assert eng.mode == mode
    out = fn(eng)
    torch.cuda.synchronize()
    eng.close()
    return out


@pytest.mark.parametrize("tag", list(CASES))
def test_against_fp32_and_reference_16_mixed(tag):
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    g = load_npz(f"geometry_{tag}.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    b, n = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    kw = dict(inject_g=torch.from_numpy(g["g"]).cuda(),
              inject_z01=torch.from_numpy(np.ascontiguousarray(g["z01"]).astype(np.float32)).cuda())
    out = {m: _run(sd, cfg, m, lambda e: e.predict_chunks(b, n, S.PredictParams(**P()), debug=True, **kw))
           for m in ("generic-geometry", MODE)}
    a = out[MODE]
    for key in STAGES:                                           # the encoder side is the geometry instance's own code
        assert torch.equal(a[key], out["generic-geometry"][key]), key
    assert np.array_equal(a["dur"].cpu().numpy(), g["dur_gamma"])
    y, t = a["signal"].cpu().numpy(), g["y_gamma_nsamp"]
    assert y.shape == (g["codes"].shape[0], cfg["max_signal_len"])
    same = (y == 0) == (t == 0)
    assert same.mean() > 0.999
    d = np.abs(y - t)[same]
    ref_mae, ref_max = ref16_bar(tag, g)
    print(f"GENERIC_GEOMETRY_F16 {tag}: mode MAE {d.mean():.4f} max {d.max():.3f} | reference 16-mixed MAE {ref_mae:.4f} "
          f"max {ref_max:.3f}")
    assert 1e-4 < d.mean() <= ref_mae and d.max() <= ref_max


@pytest.mark.parametrize("source", ["k9", "d128"])
def test_default_geometry_equals_generic_f16_bit_for_bit(source):
    """At 16 / 250 the mode runs generic-f16's kernels on generic-f16's numbers: signal, dwell and every debug stage equal."""
    sd, cfg = S.load_checkpoint(os.path.join(GOLDEN, "synthetic_k9.ckpt") if source == "k9" else sized_checkpoint_path(source))
    rng = np.random.default_rng(3)
    reads = ["".join(rng.choice(list("ACGT"), int(n))) for n in rng.integers(9, 2000, size=40)]
    bases, nv, _ = S.encode_reads(reads, int(cfg["seq_kmer"]))
    bases, nv = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    outs = {m: _run(sd, cfg, m, lambda e: (e.predict_chunks(bases, nv, S.PredictParams(seed=42), first_global_chunk=77),
                                           e.predict_chunks(bases, nv, S.PredictParams(seed=5, dwell_std=3.0, duration_sampling=False),
                                                            debug=True)))
            for m in ("generic-f16", MODE)}
    for a, b in zip(outs["generic-f16"], outs[MODE]):
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


@pytest.mark.parametrize("ts", [256, 257])
def test_both_sides_of_the_long_kernel_switch(ts):
    """r16x500's weights with the decoder position table cut to 256 samples (gen_attention_h_any_kernel) and to 257
    (gen_attention_long_h_kernel): the same dwell stream as "generic-geometry", the signal within r16x500's 16-mixed MAE of it."""
    sd, cfg = S.load_checkpoint(checkpoint_path("r16x500"))
    sd = dict(sd, **{"decoders.position_enc": sd["decoders.position_enc"][:, :ts].contiguous()})
    cfg = dict(cfg, max_signal_len=ts)
    bases, nv = _random_batch(int(cfg["seq_kmer"]), 16, 600, 8)
    p = S.PredictParams(seed=13)
    outs = {m: _run(sd, cfg, m, lambda e: e.predict_chunks(bases, nv, p, first_global_chunk=3)) for m in ("generic-geometry", MODE)}
    a, r = outs[MODE], outs["generic-geometry"]
    assert torch.equal(a["dur"], r["dur"]) and a["signal"].shape == (600, ts)
    y, t = a["signal"].cpu().numpy(), r["signal"].cpu().numpy()
    same = (y == 0) == (t == 0)
    assert same.mean() > 0.999 and (y > 0).any()
    ref_mae, _ = ref16_bar("r16x500", load_npz("geometry_r16x500.npz"))
    d = np.abs(y - t)[same]
    print(f"GENERIC_GEOMETRY_F16 r16x500 at {ts}: MAE to generic-geometry {d.mean():.4f} max {d.max():.3f}")
    assert 1e-4 < d.mean() <= ref_mae


def test_upper_edges_slices_determinism_packed_and_empty():
    """64 / 1024: a launch larger than one workspace slice equals itself and the same chunks in two launches, bit for bit; the
    packed entry point equals the plain one; B = 0 gives (0, 1024)."""
    sd, cfg = S.load_checkpoint(checkpoint_path("g64x1024"))
    eng = S.Engine(sd, cfg, mode=MODE)
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
    assert (whole["signal"] > 0).any() and torch.isfinite(whole["signal"]).all()
    assert eng.predict_chunks(bases[:0], nv[:0], p)["signal"].shape == (0, ts)
    reads = ["".join(np.random.default_rng(4).choice(list("ACGT"), L)) for L in (700, 64 + 8, 5000, 9, 1500)]
    rb, cs, pnv, _ = chunker.pack_reads(reads, k, te)
    ub, unv, _ = S.encode_reads(reads, k, te)
    packed = eng.predict_packed(torch.from_numpy(rb).cuda(), torch.from_numpy(cs).cuda(), torch.from_numpy(pnv).cuda(), p)
    plain = eng.predict_chunks(torch.from_numpy(ub).cuda(), torch.from_numpy(unv).cuda(), p)
    torch.cuda.synchronize()
    assert torch.equal(packed["signal"], plain["signal"]) and torch.equal(packed["dur"], plain["dur"])
    eng.close()


def test_decoder_operator_equals_the_full_launch():
    """modules.py's stand-alone Decoder on a generic-geometry-f16 engine at 16 / 500, fed the length-regulated rows of a full launch,
    returns that launch's y_scaled bit for bit."""
    from seq2squiggle_amd.modules import Stages
    sd, cfg = S.load_checkpoint(checkpoint_path("r16x500"))
    g = load_npz("geometry_r16x500.npz")
    eng = S.Engine(sd, cfg, mode=MODE)
    bases, nv = chunker.codes_to_bases(g["codes"])
    params = S.PredictParams(**P(noise_std=0.0))
    inj = torch.from_numpy(g["g"]).cuda()
    full = eng.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), params, debug=True, inject_g=inj)
    st = Stages(eng, params, inject_g=inj)                      # fresh context: every call below is the stand-alone operator
    lr, dur, _, _, _ = st.length_regulator(full["emb_out"].clone(), full["enc_out"].clone(), full["sigma"].unsqueeze(-1).clone())
    assert torch.equal(dur, full["dur"].float())
    y = st.decoder(lr)
    torch.cuda.synchronize()
    assert y.shape == (bases.shape[0], 500, 1)
    assert torch.equal(y[..., 0], full["y_scaled"])
    assert (full["y_scaled"] > 0).any()
    eng.close()


def test_cli_predict_generic_geometry_f16(tmp_path):
    """`predict -m <16 / 500 checkpoint> --compute-mode generic-geometry-f16 --profile rna-004-min` says which instance it runs and
    writes the reads of a "generic-geometry" run with the same seed: the same ids in the same order, each read's sample count within
    0.1 % (the dwell stream is the same; only zero-strip flips of samples at the ReLU's edge may differ)."""
    fa = tmp_path / "reads.fa"
    rng = np.random.default_rng(1)
    with open(fa, "w") as f:
        for i, n in enumerate([40, 333, 1200, 16 + 8, 2500, 700]):
            f.write(f">r{i}\n{''.join(rng.choice(list('ACGT'), n))}\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "S2S_ONE_GPU")}
    recs = {}
    for mode in ("generic-geometry", MODE):
        out = tmp_path / f"{mode}.blow5"
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "seq2squiggle_amd", "predict", str(fa), "--read-input",
                            "-o", str(out), "-m", checkpoint_path("r16x500"), "--profile", "rna-004-min", "--compute-mode", mode,
                            "--preserve-read-ids", "--seed", "9"], cwd=ROOT, capture_output=True, text=True, timeout=660, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert (r.stdout + r.stderr).count(f"predict instance: {mode} ") == 1
        recs[mode] = signal_io.read_blow5(str(out))[1]
    a, b = recs["generic-geometry"], recs[MODE]
    assert len(a) == 6 and [x["read_id"] for x in a] == [x["read_id"] for x in b]
    for x, y in zip(a, b):
        assert abs(int(x["len_raw_signal"]) - int(y["len_raw_signal"])) <= 0.001 * int(x["len_raw_signal"]), x["read_id"]
