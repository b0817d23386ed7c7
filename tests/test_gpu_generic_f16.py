"""The reduced-precision size-generic instance (S2S_MODE_GENERIC_F16, compute mode "generic-f16") on the GPU.

Its bar is the reference's own GPU arithmetic, as for S2S_MODE_F16 (tests/test_gpu_parity.py: test_reduced_precision_f16_mode):
the imported reference's predict_step under fp16 autocast on the same chunks with the same injected variates -- mixed16.npz at the
shipped size, sized_mixed16.npz at the sized cases (tools/make_sized_mixed16_goldens.py).  Against the fp32 golden the mode must be
at least as close as that reference, in MAE and max, with its own dwell indices bit-exact (the encoder side is S2S_MODE_GENERIC's
fp32 code: its stage outputs are bit-equal to a "generic" engine's)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import chunker, signal_io
from seq2squiggle_amd import utils as U
from conftest import GOLDEN, ROOT, load_npz
from _sized_models import checkpoint_path

pytestmark = pytest.mark.gpu
WORKSPACE_BYTES = 512 << 20                                              # S2S_GENERIC_WORKSPACE_BYTES (include/s2s_hip.h)
STAGES = ("emb_out", "enc_out", "sigma", "conc", "rate", "g", "dur")


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return base


def load(tag):
    return S.load_checkpoint(checkpoint_path(tag) if tag.startswith("d") else os.path.join(GOLDEN, f"synthetic_{tag}.ckpt"))


def ref16_bar(tag, g):
    """The reference 16-mixed's MAE / max against the fp32 golden where its dwell indices agree with fp32's, re-derived from the
    committed vectors."""
    m16 = load_npz("sized_mixed16.npz" if tag.startswith("d") else "mixed16.npz")
    r16, dur16 = m16[f"y_gamma_nsamp_16mixed_{tag}"], m16[f"dur_gamma_16mixed_{tag}"]
    agree = (dur16 == g["dur_gamma"]).all(1)
    d = np.abs(r16 - g["y_gamma_nsamp"])[agree]
    assert abs(d.mean() - float(m16[f"mae_vs_fp32_where_dwell_equal_{tag}"])) < 1e-6
    return d.mean(), d.max()


@pytest.mark.parametrize("tag", ["k9", "k6", "d32", "d128", "d512"])
def test_against_fp32_and_reference_16_mixed(tag):
    sd, cfg = load(tag)
    g = load_npz(f"sized_{tag}.npz" if tag.startswith("d") else f"stages_{tag}.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    b, n = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    kw = dict(inject_g=torch.from_numpy(g["g"]).cuda(), inject_z01=torch.from_numpy(np.ascontiguousarray(g["z01"])).cuda())
    out = {}
    for mode in ("generic", "generic-f16"):
        eng = S.Engine(sd, cfg, mode=mode)
        assert eng.mode == mode
        out[mode] = eng.predict_chunks(b, n, S.PredictParams(**P()), debug=True, **kw)
        torch.cuda.synchronize()
        eng.close()
    a = out["generic-f16"]
    for key in STAGES:                                           # the encoder side is the generic instance's own code
        assert torch.equal(a[key], out["generic"][key]), key
    assert np.array_equal(a["dur"].cpu().numpy(), g["dur_gamma"])
    y, t = a["signal"].cpu().numpy(), g["y_gamma_nsamp"]
    same = (y == 0) == (t == 0)
    assert same.mean() > 0.999
    d = np.abs(y - t)[same]
    ref_mae, ref_max = ref16_bar(tag, g)
    print(f"GENERIC_F16 {tag}: mode MAE {d.mean():.4f} max {d.max():.3f} | reference 16-mixed MAE {ref_mae:.4f} max {ref_max:.3f}")
    assert 1e-4 < d.mean() <= ref_mae and d.max() <= ref_max


def _random_batch(k, B, seed):
    rng = np.random.default_rng(seed)
    reads = ["".join(rng.choice(list("ACGT"), int(n))) for n in rng.integers(k, 3000, size=max(1, B // 8))]
    bases, nv, _ = S.encode_reads(reads, k)
    while bases.shape[0] < B:
        bases, nv = np.concatenate([bases, bases]), np.concatenate([nv, nv])
    return torch.from_numpy(bases[:B].copy()).cuda(), torch.from_numpy(nv[:B].copy()).cuda()


def test_builtin_samplers_slices_and_determinism_at_d128():
    """32,768 chunks with the built-in samplers: dwell bit-equal to "generic", the signal within test 1's bound of it; two runs
    bit-identical; the launch (several workspace slices) equals its slices launched one by one."""
    sd, cfg = load("d128")
    B = 32768
    bases, nv = _random_batch(int(cfg["seq_kmer"]), B, 21)
    p = S.PredictParams(seed=77)
    eng = S.Engine(sd, cfg, mode="generic")
    ref = eng.predict_chunks(bases, nv, p, first_global_chunk=5000)
    torch.cuda.synchronize()
    eng.close()
    eng = S.Engine(sd, cfg, mode="generic-f16")
    whole = eng.predict_chunks(bases, nv, p, first_global_chunk=5000)
    again = eng.predict_chunks(bases, nv, p, first_global_chunk=5000)
    torch.cuda.synchronize()
    assert torch.equal(whole["dur"], ref["dur"])
    y, r = whole["signal"].cpu().numpy(), ref["signal"].cpu().numpy()
    same = (y == 0) == (r == 0)
    assert same.mean() > 0.999 and (y > 0).any()
    ref_mae, _ = ref16_bar("d128", load_npz("sized_d128.npz"))
    assert np.abs(y - r)[same].mean() <= ref_mae
    assert torch.equal(whole["signal"], again["signal"]) and torch.equal(whole["dur"], again["dur"])
    d, f = int(cfg["dmodel"]), int(cfg["dff"])
    sl = WORKSPACE_BYTES // (4 * (16 * d + 250 * d + 250 * max(3 * d, f) + 16 + 250))
    assert B > 3 * sl + 17
    parts, s = [], 0
    for m in (sl, sl, sl, 17):
        parts.append(eng.predict_chunks(bases[s:s + m].contiguous(), nv[s:s + m].contiguous(), p, first_global_chunk=5000 + s))
        s += m
    torch.cuda.synchronize()
    for key in ("signal", "dur"):
        assert torch.equal(torch.cat([q[key] for q in parts]), whole[key][:s]), key
    st = eng.stats()
    assert st["chunks"] == 2 * B + s
    eng.close()


def test_decoder_operator_equals_the_full_launch():
    """modules.py's stand-alone Decoder on a generic-f16 engine, fed the length-regulated rows of a full launch, returns that
    launch's y_scaled bit for bit."""
    from seq2squiggle_amd.modules import Stages
    sd, cfg = load("d128")
    g = load_npz("sized_d128.npz")
    eng = S.Engine(sd, cfg, mode="generic-f16")
    bases, nv = chunker.codes_to_bases(g["codes"])
    params = S.PredictParams(**P(noise_std=0.0))
    inj = torch.from_numpy(g["g"]).cuda()
    full = eng.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), params, debug=True, inject_g=inj)
    st = Stages(eng, params, inject_g=inj)                      # fresh context: every call below is the stand-alone operator
    lr, dur, _, _, _ = st.length_regulator(full["emb_out"].clone(), full["enc_out"].clone(), full["sigma"].unsqueeze(-1).clone())
    assert torch.equal(dur, full["dur"].float())
    y = st.decoder(lr)
    torch.cuda.synchronize()
    assert y.shape == (bases.shape[0], 250, 1)
    assert torch.equal(y[..., 0], full["y_scaled"])
    assert (full["y_scaled"] > 0).any()
    eng.close()


def test_cli_predict_generic_f16(tmp_path):
    """`predict -m <dmodel-128 checkpoint> --compute-mode generic-f16` writes the reads of a "generic" run with the same seed: the
    same ids in the same order, each read's sample count within 0.1 % (the dwell stream is the same; only zero-strip flips of
    samples at the ReLU's edge may differ)."""
    fasta = os.path.join(GOLDEN, "example_test.fasta")
    recs = {}
    for mode in ("generic", "generic-f16"):
        out = tmp_path / f"{mode}.blow5"
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "seq2squiggle_amd", "predict", fasta, "--read-input",
                            "-o", str(out), "-m", checkpoint_path("d128"), "--compute-mode", mode, "--preserve-read-ids", "--seed", "3"],
                           cwd=ROOT, capture_output=True, text=True, timeout=660)
        assert r.returncode == 0, r.stderr[-2000:]
        assert (r.stdout + r.stderr).count(f"predict instance: {mode} ") == 1
        recs[mode] = signal_io.read_blow5(str(out))[1]
    ids = [n for _, n in U.read_fasta(fasta)]
    assert [x["read_id"] for x in recs["generic"]] == [x["read_id"] for x in recs["generic-f16"]] == ids
    for a, b in zip(recs["generic"], recs["generic-f16"]):
        assert abs(int(a["len_raw_signal"]) - int(b["len_raw_signal"])) <= 0.001 * int(a["len_raw_signal"]), a["read_id"]
