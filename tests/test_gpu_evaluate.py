"""s2s_evaluate_chunks on the GPU (Engine.evaluate_chunks, seq2squiggle_amd.evaluate, model.validation_step, the evaluate command)
against the reference's own validation_step (tests/golden/eval_<tag>.npz, tools/make_eval_goldens.py).

Bounds, one per quantity:
  y (teacher-forced decoder output) against prediction_ref: the predict parity bound of the mode -- MAE < 1e-4 pA for the fp32-class
    modes (f32, f16x3, generic, generic-geometry); for the reduced-precision ones (f16, generic-f16, generic-geometry-f16) MAE and max
    no larger than the reference's own 16-mixed run of the same pass (y16_mae_pa / y16_max_pa);
  sigma, conc, rate: max relative error 1e-4 (every mode's frontend is fp32-class);
  per-chunk sums against the same sums recomputed in float64 from the GPU's own y / conc / rate / sigma: 1e-5 relative + 1e-7;
  the four dataset losses: within 1e-4 relative of the reference's logged values (fp32 class); for reduced precision no farther
  from them than the reference's 16-mixed run moves them chunk by chunk (finalize of |per_chunk16 - per_chunk|: the signed dataset
  sum of that run can cancel -- at k6 its logged signal loss is 1.4e-5 relative from fp32 while its per-chunk distance is larger).
Measured on an MI355X: y MAE 4.7e-05 pA (k9, f16x3); dataset losses of the fp32-class modes within 1e-6 relative; f16 / generic-f16
signal loss 1.2e-05 / 3.5e-06 relative at k9, 1.9e-05 / 3.0e-05 at k6; duration and noise losses within 1e-7 relative in every mode."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd.checkpoint import load_checkpoint
from conftest import ROOT
import _eval_data as ED

pytestmark = pytest.mark.gpu

ALL = ["f16x3", "f32", "f16", "generic", "generic-f16", "generic-geometry", "generic-geometry-f16"]
GENERIC = ["generic", "generic-f16", "generic-geometry", "generic-geometry-f16"]
GEOMETRY = ["generic-geometry", "generic-geometry-f16"]
# (the cases after r16x500: tests/_envelope_models.py and tests/_geometry_models.py -- te 1 / 5 / 23 / 16 / 64 / 64 / 17, ts 1 / 37 / 255 / 250
#  / 251 / 1024 / 1023, seq_kmer 1 at hd64 and 16 at hd24, 4 / 4 / 4 layers at hd96s; each holds a k-mer of dwell 32767)
MODES = {"k9": ALL, "k6": ALL, "d32": GENERIC, "r16x500": GEOMETRY, "hd1": GEOMETRY, "g5x37": GEOMETRY, "hd24": GEOMETRY, "hd64": GENERIC,
         "hd96s": GEOMETRY, "g64x1024": GEOMETRY, "hd208": GEOMETRY}
FP32_CLASS = {"f32", "f16x3", "generic", "generic-geometry"}
CASES = [(t, m) for t in ED.TAGS for m in MODES[t]]

_ENGINES = {}


def engine(tag, mode):
    if (tag, mode) not in _ENGINES:
        sd, cfg = load_checkpoint(ED.checkpoint(tag))
        _ENGINES[(tag, mode)] = S.Engine(sd, cfg, device=0, mode=mode)
    return _ENGINES[(tag, mode)]


def run(eng, g, lo=0, hi=None, **kw):
    a = ED.arrays(g)
    hi = a["chunks"].shape[0] if hi is None else hi
    scale = float(eng.config["scaling_max_value"])
    return EV.evaluate_batch(eng, a["chunks"][lo:hi], a["chunks_lengths"][lo:hi], (a["targets"][lo:hi] / scale).astype(np.float32),
                             (a["stdevs"][lo:hi] / scale).astype(np.float32), **kw)


def host_sums(out, g, scale):
    """The three per-chunk sums in float64 from the GPU's own stage outputs."""
    y, sg, c, r = (out[n].double().cpu().numpy() for n in ("y", "sigma", "conc", "rate"))
    t = (g["targets"].astype(np.float32) / scale).astype(np.float32).astype(np.float64)
    sd = (g["stdevs"] / scale).astype(np.float32).astype(np.float64)
    d = g["lengths"].astype(np.float64)
    x = np.where(d == 0, 1.0, np.abs(d))
    lg = np.vectorize(math.lgamma)(c)
    nll = -(c * np.log(r) + (c - 1) * np.log(x) - r * x - lg)
    return np.stack([((y - t) ** 2).sum(1), nll.sum(1), ((sd - sg) ** 2).sum(1)], 1)


@pytest.mark.parametrize("tag,mode", CASES)
def test_parity_with_reference(tag, mode):
    g = ED.load(tag)
    eng = engine(tag, mode)
    scale = float(eng.config["scaling_max_value"])
    out = run(eng, g, want_y=True, debug=True)
    y = out["y"].cpu().numpy()
    d = np.abs(y.astype(np.float64) - g["prediction_ref"]) * scale
    print(f"EVAL {tag} {mode}: y MAE {d.mean():.3e} pA max {d.max():.3e} | 16-mixed MAE {float(g['y16_mae_pa']):.3e} "
          f"max {float(g['y16_max_pa']):.3e}")
    if mode in FP32_CLASS:
        assert d.mean() < 1e-4
    else:
        assert d.mean() <= float(g["y16_mae_pa"]) and d.max() <= float(g["y16_max_pa"])
    for n in ("sigma", "conc", "rate"):
        ref = g[n].astype(np.float64)
        rel = np.abs(out[n].cpu().numpy() - ref) / np.abs(ref)
        assert rel.max() < 1e-4, (n, rel.max())
    loss = out["loss"].cpu().numpy().astype(np.float64)
    mine = host_sums(out, g, scale)
    assert np.all(np.abs(loss - mine) <= 1e-5 * np.abs(mine) + 1e-7), np.abs(loss - mine).max(0)
    te, ts = g["lengths"].shape[1], g["targets"].shape[1]
    fin = EV.finalize(loss, te, ts)
    # the reduced-precision bar: how far the reference's 16-mixed arithmetic moves each loss, chunk by chunk, without the
    # cancellation of the signed dataset sum (its logged 16-mixed loss can land closer to fp32 by luck)
    d16 = EV.finalize(np.abs(g["per_chunk16"] - g["per_chunk"]), te, ts)
    for i, name in enumerate(ED.LOSSES):
        ref = float(g["logged_bs32"][i])
        dist = abs(fin[name] - ref)
        print(f"EVAL {tag} {mode} {name}: {fin[name]:.9g} ref {ref:.9g} rel {dist / abs(ref):.2e} | 16-mixed per-chunk rel "
              f"{d16[name] / abs(ref):.2e}, logged 16-mixed rel {abs(float(g['logged16_bs32'][i]) - ref) / abs(ref):.2e}")
        if mode in FP32_CLASS:
            assert dist <= 1e-4 * abs(ref), name
        else:
            assert dist <= d16[name], name


@pytest.mark.parametrize("tag,mode", [("k9", "f16x3"), ("k9", "f32"), ("k9", "f16"), ("k6", "generic"), ("r16x500", "generic-geometry"),
                                      ("d32", "generic-f16")]
                         + [(t, m) for t in ("hd1", "g5x37", "hd24", "hd64", "hd96s", "g64x1024", "hd208") for m in MODES[t]])
def test_deterministic_under_slicing(tag, mode):
    """A chunk's sums depend on its own rows only: bit-identical for B = all, 1, 7, 64 and across two calls."""
    g = ED.load(tag)
    eng = engine(tag, mode)
    N = g["codes"].shape[0]
    whole = run(eng, g)["loss"].cpu().numpy()
    assert np.array_equal(whole, run(eng, g)["loss"].cpu().numpy())
    for step in (1, 7, 64):
        parts = np.concatenate([run(eng, g, lo, min(N, lo + step))["loss"].cpu().numpy() for lo in range(0, N, step)])
        assert np.array_equal(parts, whole), step


@pytest.mark.parametrize("mode", ["f16x3", "f32", "generic"])
def test_teacher_forced_y_matches_decoder_operator(mode):
    """Sliding-window chunks (where the predict path's encoder applies): the evaluate path's y equals the stand-alone Decoder fed
    the length regulator built in torch from the same dwell counts and the Encoder operator's enc_out."""
    eng = engine("k9", mode)
    k, te, ts = eng.k, eng.t_enc, eng.t_dec
    rng = np.random.default_rng(5)
    B = 40
    bases = rng.integers(1, 5, (B, te + k - 1))
    codes = np.stack([bases[:, c:c + k] for c in range(te)], 1).astype(np.uint8)          # [B,te,k] windows of one string
    dwell = rng.poisson(14, (B, te)).astype(np.int32)
    dwell[0] = 40                                                                          # cropped
    dwell[1, 3] = 0
    st = S.Stages(eng)
    enc_out, _ = st.encoder(torch.from_numpy(ED.onehot(codes)).to(eng.device))
    cum = torch.from_numpy(np.cumsum(dwell, 1)).to(eng.device)
    t = torch.arange(ts, device=eng.device)
    idx = (cum.unsqueeze(1) <= t.view(1, ts, 1)).sum(-1)                                   # [B,ts]: k-mer of sample t
    live = idx < te
    x = torch.gather(enc_out, 1, idx.clamp(max=te - 1).unsqueeze(-1).expand(B, ts, enc_out.shape[-1])) * live.unsqueeze(-1)
    y_op = st.decoder(x)[:, :, 0]
    kmers = torch.from_numpy(np.frombuffer(b"_ACGTN", np.uint8)[codes]).to(eng.device).contiguous()
    z = torch.zeros(B, ts, device=eng.device)
    out = eng.evaluate_chunks(kmers, torch.from_numpy(dwell).to(eng.device), z, torch.zeros(B, te, device=eng.device), want_y=True)
    d = (out["y"] - y_op).abs() * float(eng.config["scaling_max_value"])
    print(f"EVAL cross-check {mode}: MAE {d.mean().item():.3e} pA max {d.max().item():.3e}")
    assert d.mean().item() < 1e-4


def test_validation_step_matches_logged_losses():
    from seq2squiggle_amd.model import seq2squiggle
    g = ED.load("k9")
    m = seq2squiggle.load_from_checkpoint(ED.checkpoint("k9"), device=0, mode="f32")
    a = ED.arrays(g)
    scale = float(m.config["scaling_max_value"])
    sums = np.zeros(4)
    for i in range(0, 96, 32):
        batch = (torch.from_numpy(a["chunks"][i:i + 32]), torch.from_numpy(a["targets"][i:i + 32, :, None] / scale),
                 torch.from_numpy(a["chunks_lengths"][i:i + 32].astype(np.int16)), torch.from_numpy(a["targets_lengths"][i:i + 32]),
                 torch.from_numpy(a["stdevs"][i:i + 32] / scale))
        losses = m.validation_step(batch, i // 32)
        sums += 32 * np.array([losses[n] for n in ED.LOSSES])
    got = sums / 96
    assert np.all(np.abs(got - g["logged_bs32"]) <= 1e-4 * np.abs(g["logged_bs32"])), (got, g["logged_bs32"])


def test_cli_end_to_end(tmp_path):
    g = ED.load("k9")
    d = ED.write_dir(g, str(tmp_path / "data"), per_file=40)
    k9, k6 = ED.checkpoint("k9"), ED.checkpoint("k6")
    npz = str(tmp_path / "per_chunk.npz")
    r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "evaluate", d, "-m", k9, "-m", k9, "--compute-mode", "f32",
                        "--batch-size", "50", "--json", "--per-chunk", npz], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(rows) == 2 and rows[0]["mode"] == "f32" and rows[0]["chunks"] == 96 and rows[0]["chunks_per_s"] > 0
    for row in rows:
        for i, name in enumerate(ED.LOSSES):
            assert abs(row[name] - g["logged_bs32"][i]) <= 1e-4 * abs(g["logged_bs32"][i]), name
    z = np.load(npz)
    assert z["model0"].shape == (96, 3) and np.array_equal(z["model0"], z["model1"])
    assert np.allclose(z["model0"], g["per_chunk"], rtol=1e-3, atol=1e-6)
    # a checkpoint at another geometry (16 / 500), the compute mode chosen by the engine
    g5 = ED.load("r16x500")
    d5 = ED.write_dir(g5, str(tmp_path / "data500"), per_file=40)
    r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "evaluate", d5, "-m", ED.checkpoint("r16x500"), "--json"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(rows) == 1 and rows[0]["mode"] == "generic-geometry" and rows[0]["chunks"] == g5["codes"].shape[0]
    for i, name in enumerate(ED.LOSSES):
        print(f"EVAL cli r16x500 {name}: {rows[0][name]:.9g} ref {g5['logged_bs32'][i]:.9g}")
        assert abs(rows[0][name] - g5["logged_bs32"][i]) <= 1e-4 * abs(g5["logged_bs32"][i]), name
    # a checkpoint of another seq_kmer is refused with the expected shape
    r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "evaluate", d, "-m", k6], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "seq_kmer 6" in r.stderr + r.stdout
