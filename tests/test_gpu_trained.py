"""Every compute mode held to the project's stated bounds on weights the project's own trainer produced (tests/_trained.py: the
students k9, k9_far and g5x37), where every other numerical test runs on weights no optimiser has touched.

Inputs.  The 16 / 250 students run the 41 chunks of test_gpu_magnitudes.inputs() (one 392-base read, the ragged, N-rich and lower-case
reads) with that module's injected Gamma draws and normals, passes "g" (noise off) and "z" (noise on).  g5x37 runs its golden's 48
rows of k-mers re-encoded as predict input -- every row's bases rebuilt from its k-mers' first letters and its last real k-mer
(chunker.codes_to_bases), the oracle's codes then taken back from the windows of those bases; the all-pad row enters as one "_" k-mer,
n_valid 1, the smallest count s2s_predict_chunks admits -- with seeded draws of the same kind.  The fp32 and fp64 oracle
(oracle/s2s_oracle.py, CPU) are recomputed on each student.

Before any GPU figure: the reference alone must stay inside the caps that keep a bound from hiding a failure -- the fp32 oracle's
zero pattern agrees with the fp64 oracle's on more than 0.9995 of the samples and its distance to fp64 is > 0 (reference_inside_caps,
asserted when a case is built and by a test of its own).

A  predict parity: f32 / generic / generic-geometry within_bounds with zero flips in pass "g" and dwell indices equal among the
   instances; f16x3 on both attention paths within_bounds and the stage outputs at STAGE_TOL, the range condition of tests/_reparam.py
   asserted first; f16 / generic-f16 / generic-geometry-f16 dwell indices exact, signal finite, figures printed (no 16-mixed bar exists
   for weights the reference never ran).
B  the calibration launch: the path is "exact" exactly when the calibration rate exceeds s2s_attention_redo_threshold(), two handles
   agree, the counters obey test_peaked_attention_forces_the_rescale_fallback's identities, both paths hold A's bounds on one engine.
C  evaluate on each student's own training chunks in every mode that loads it: per-chunk sums against float64 sums of the GPU's own
   stage outputs (1e-5 relative + 1e-7), y of the fp32-class modes MAE < 1e-4 pA against the fp32 oracle's teacher-forced pass, a
   7-chunk launch bit-equal to the same rows of the full launch.
D  the backward pass at trained weights: test_gpu_train_gradients.compare's rule on B = 7 chunks, the loss rows bit-equal to
   evaluate's, a second call the same bits.

Every constant is an existing one (tests/_bounds.py, test_gpu_magnitudes.py, test_gpu_evaluate.py, test_gpu_train_gradients.py).
Every test prints its figures (TRAINED <student> <mode> <path> <pass>: ...) before it asserts.  Measured: LABNOTES.md round 43."""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import chunker
from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd import train as T
from seq2squiggle_amd.inference import redo_threshold
from oracle import s2s_oracle as O
import _eval_data as ED
import _reparam as R
import _train_ref as TREF
import _trained as TR
import test_gpu_magnitudes as M
import test_gpu_train_gradients as GD
from test_gpu_evaluate import FP32_CLASS, host_sums
from test_gpu_magnitudes import _no_attention_path_override  # noqa: F401  (autouse: no S2S_ATTENTION_PATH from the caller)

pytestmark = pytest.mark.gpu

EXACT = {"k9": ("f32", "generic", "generic-geometry"), "k9_far": ("f32", "generic", "generic-geometry"), "g5x37": ("generic-geometry",)}
REDUCED = {"k9": ("f16", "generic-f16", "generic-geometry-f16"), "k9_far": ("f16", "generic-f16", "generic-geometry-f16"),
           "g5x37": ("generic-geometry-f16",)}
LOADS = {n: EXACT[n] + (("f16x3",) if n in TR.TUNED_GEOMETRY else ()) + REDUCED[n] for n in TR.NAMES}
_CASES = {}


def predict_input_of(codes):
    """Rows of k-mers [B,te,k] -> (bases, n_valid, the codes of the windows of those bases: what predict sees of the rows)."""
    bases, nv = chunker.codes_to_bases(codes)
    nv = np.maximum(nv, 1).astype(np.uint8)
    B, te, k = codes.shape
    lut = np.full(256, 5, np.uint8)
    for i, ch in enumerate(b"_ACGT"):
        lut[ch] = i
    win = lut[bases][:, np.arange(te)[:, None] + np.arange(k)[None, :]]
    win[np.arange(te)[None, :] >= nv[:, None]] = 0
    return bases, nv, win


def reference_inside_caps(ref):
    """The caps share_same > 0.9995 and `agree64` must not be what makes a bound hold: on the oracle runs alone."""
    for name, (r32, r64) in ref.items():
        r, t = r32["signal"].numpy(), r64["signal"].numpy()
        agree = (r == 0) == (t == 0)
        err = float(np.abs(r - t)[agree].mean())
        assert agree.mean() > 0.9995 and err > 0, (name, float(agree.mean()), err)
        assert torch.equal(r32["dur"], r64["dur"]), name
    return True


def case(name, request):
    """The student, its predict inputs in the layout of test_gpu_magnitudes.inputs(), both oracles' runs and the fp64 taps."""
    if name in _CASES:
        return _CASES[name]
    st = TR.student(name, request)
    sd, cfg = st["sd"], st["cfg"]
    if name in TR.TUNED_GEOMETRY:
        base = M.inputs()
        inp = dict(cfg=cfg, codes=base["codes"], B=base["B"], g=base["g"], z=base["z"], dev=base["dev"])
    else:
        bases, nv, codes = predict_input_of(st["rows"]["codes"])
        B, te, ts = codes.shape[0], int(cfg["max_dna_len"]), int(cfg["max_signal_len"])
        gen = torch.Generator().manual_seed(37)
        g, z = torch.rand(B, te, generator=gen) * (1.6 * ts / te), torch.randn(B, ts, generator=gen)
        inp = dict(cfg=cfg, codes=codes, B=B, g=g, z=z,
                   dev=dict(bases=torch.from_numpy(bases).cuda(), nv=torch.from_numpy(nv).cuda(), g=g.cuda(), z=z.cuda()))
    inp.update(sd=sd, student=st, ref=M.oracle_runs(sd, cfg, inp), taps=R.intermediates(sd, cfg, inp["codes"], inp["g"]))
    assert reference_inside_caps(inp["ref"])
    _CASES[name] = inp
    return inp


def rows_of_instance(inp, mode):
    """One engine of an instance without attention paths -> {pass: (figures, dwell indices)}."""
    eng = S.Engine(inp["sd"], inp["cfg"], mode=mode)
    try:
        out = {}
        for name in M.PASSES:
            o = M.run(eng, inp, name)
            out[name] = (M.metrics(o, *inp["ref"][name]), o["dur"].cpu().numpy())
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("name", TR.NAMES)
def test_students_moved(name, request):
    """Printed for LABNOTES.md (the builder's time, the movement figures); asserted: the weights are finite and left their start, the
    position tables did not, and -- what no synthetic checkpoint has -- LayerNorm gains and biases are no longer 1 and 0."""
    inp = case(name, request)
    st = inp["student"]
    print(f"\nTRAINED {name}: builder {st['seconds']:.2f} s, last epoch " + " ".join(f"{k} {v:.6g}" for k, v in st["records"][-1].items()))
    for k, v in TR.movement(st["sd"], st["start"], st["cfg"], inp["codes"], inp["g"], inp["taps"]).items():
        print(f"TRAINED {name} moved: {k}: {v}")
    sd, start = st["sd"], st["start"]
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    for k in sd:
        if k.endswith("position_enc"):
            assert torch.equal(sd[k], start[k]), k
        elif not k.endswith("w_ks.bias"):                 # (its gradient is mathematically zero: softmax is shift invariant)
            assert not torch.equal(sd[k], start[k]), k
        if k.endswith("layer_norm.weight"):
            assert not torch.equal(sd[k], torch.ones_like(sd[k])), k
        if k.endswith("layer_norm.bias"):
            assert bool(sd[k].any()), k


@pytest.mark.parametrize("name", TR.NAMES)
def test_reference_stays_inside_the_caps(name, request):
    inp = case(name, request)
    for p, (r32, r64) in inp["ref"].items():
        r, t = r32["signal"].numpy(), r64["signal"].numpy()
        agree = (r == 0) == (t == 0)
        print(f"TRAINED {name} oracle {p}: zero pattern fp32 = fp64 on {agree.mean():.6f}, fp32 to fp64 {np.abs(r - t)[agree].mean():.3e} pA, "
              f"{int((r != 0).sum())} of {r.size} samples live")
    assert reference_inside_caps(inp["ref"])


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", TR.NAMES)
def test_exact_modes_hold_the_bounds(name, request):
    inp = case(name, request)
    rows = {mode: rows_of_instance(inp, mode) for mode in EXACT[name]}
    for mode, per in rows.items():
        for p, (m, _) in per.items():
            print(f"TRAINED {name} {mode} - {p}: {M.fmt(m)}")
    for mode, per in rows.items():
        for p, (m, dur) in per.items():
            assert M.within_bounds(m, fp64_rule=(p == "g")), (name, mode, p, m)
            if p == "g":
                assert m["flips"] == 0, (name, mode, m)
            assert np.array_equal(dur, rows[EXACT[name][0]][p][1]), (name, mode, p)


@pytest.mark.parametrize("name", TR.TUNED_GEOMETRY)
def test_split_f16_holds_the_bounds(name, request):
    inp = case(name, request)
    worst = max(inp["taps"].values())
    print(f"TRAINED {name} f16x3 range: largest intermediate {worst:.4g} of {R.RANGE_LIMIT:g}")
    assert worst < R.RANGE_LIMIT, f"student {name} is outside S2S_MODE_F16X3's stated range: {worst:.4g} >= {R.RANGE_LIMIT:g}"
    rows = M.envelope_rows(inp["sd"], inp, "f16x3")
    for (path, p), m in rows.items():
        print(f"TRAINED {name} f16x3 {path} {p}: {M.fmt(m)}")
    ref = inp["ref"]["g"][0]
    eng = S.Engine(inp["sd"], inp["cfg"], mode="f16x3")
    stage = {}
    try:
        for path in ("fast", "exact"):
            eng.attention_path = path
            out = M.run(eng, inp, "g", debug=True)
            torch.cuda.synchronize()
            stage[path] = {k: out[k].cpu().numpy() for k in ("enc_out", "sigma", "conc", "rate", "dur")}
    finally:
        eng.close()
    for path, o in stage.items():
        d_enc = float(np.abs(o["enc_out"] - ref["enc_out"].numpy()).max())
        d_sig = float(np.abs(o["sigma"] - ref["sigma"].numpy()).max())
        print(f"TRAINED {name} f16x3 {path} stages: enc_out {d_enc:.2e} sigma {d_sig:.2e}")
    for (path, p), m in rows.items():
        assert M.within_bounds(m, fp64_rule=(p == "g")), (name, path, p, m)
    for path, o in stage.items():
        assert float(np.abs(o["enc_out"] - ref["enc_out"].numpy()).max()) < M.STAGE_TOL["enc"], (name, path)
        assert float(np.abs(o["sigma"] - ref["sigma"].numpy()).max()) < M.STAGE_TOL["sig"], (name, path)
        for key in ("conc", "rate"):
            assert np.allclose(o[key], ref[key].numpy(), rtol=M.STAGE_TOL["rel"], atol=M.STAGE_TOL["rel"]), (name, path, key)
        assert np.array_equal(o["dur"], ref["dur"].numpy()), (name, path)


@pytest.mark.parametrize("name", TR.NAMES)
def test_reduced_precision_modes_stay_finite(name, request):
    """Recorded only, as test_f16_mode_stays_finite: outside the parity bound by design."""
    inp = case(name, request)
    for mode in REDUCED[name]:
        if mode == "f16":
            rows = M.envelope_rows(inp["sd"], inp, mode)
        else:
            rows = {("-", p): m for p, (m, _) in rows_of_instance(inp, mode).items()}
        for (path, p), m in rows.items():
            print(f"TRAINED {name} {mode} {path} {p}: {M.fmt(m)}")
        for (path, p), m in rows.items():
            assert m["dur_equal"] and m["finite"], (name, mode, path, p)


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
@pytest.mark.parametrize("name", TR.TUNED_GEOMETRY)
def test_calibration_launch(name, mode, request):
    inp = case(name, request)
    B, layers = inp["B"], int(inp["cfg"]["decoder_layers"])
    eng, twin = (S.Engine(inp["sd"], inp["cfg"], mode=mode) for _ in range(2))
    try:
        calib, chosen = eng.calibration_redo_rate, eng.attention_path
        assert 0.0 <= calib <= 1.0 and (chosen == "exact") == (calib > redo_threshold()), (name, mode, calib, chosen)
        assert (twin.calibration_redo_rate, twin.attention_path) == (calib, chosen)
        rows, stats = {}, {}
        for path in ("fast", "exact"):
            eng.attention_path = path
            for p in M.PASSES:
                eng.stats()
                rows[(path, p)] = M.metrics(M.run(eng, inp, p), *inp["ref"][p])
                stats[(path, p)] = eng.stats()
    finally:
        eng.close()
        twin.close()
    print(f"TRAINED {name} {mode} calibration: rate {calib:.4f} against threshold {redo_threshold():.4f} -> {chosen}; the 41 chunks on the "
          f"fast path: redo {stats[('fast', 'g')]['redo_rate']:.4f}")
    for (path, p), m in rows.items():
        m["redo"] = stats[(path, p)]["redo_rate"]
        print(f"TRAINED {name} {mode} {path} {p}: {M.fmt(m)}")
    for (path, p), st in stats.items():
        assert st["chunks"] == B and st["softmax_runs"] == B * 8 * 8 * layers, (name, mode, path, p, st)
        assert st["softmax_redone"] <= st["softmax_runs"]
        if path == "fast":
            assert st["chunks_on_exact_path"] == 0, st
        else:
            assert st["chunks_on_exact_path"] == B and st["softmax_redone"] == 0, st
    for (path, p), m in rows.items():
        if mode == "f16x3":
            assert M.within_bounds(m, fp64_rule=(p == "g")), (name, mode, path, p, m)
        else:
            assert m["dur_equal"] and m["finite"], (name, mode, path, p)


# ---------------------------------------------------------------------------------------------------------------- C
def eval_reference(inp):
    """The fp32 oracle's teacher-forced pass on the student's training chunks, once per student."""
    if "eval_ref" not in inp:
        st = inp["student"]
        rows, scale = st["rows"], float(st["cfg"]["scaling_max_value"])
        target, stdev = ED.scaled(rows, scale)
        inp["eval_ref"] = O.evaluate_chunks(st["sd"], st["cfg"], rows["codes"], rows["lengths"], target, stdev)["y"].numpy()
    return inp["eval_ref"]


@pytest.mark.parametrize("name,mode", [(n, m) for n in TR.NAMES for m in LOADS[n]])
def test_evaluate_on_training_chunks(name, mode, request):
    inp = case(name, request)
    st = inp["student"]
    rows, scale = st["rows"], float(st["cfg"]["scaling_max_value"])
    a = ED.arrays(rows)
    target, stdev = ED.scaled(rows, scale)
    N = rows["codes"].shape[0]
    eng = S.Engine(st["sd"], st["cfg"], device=0, mode=mode)
    try:
        out = EV.evaluate_batch(eng, a["chunks"], a["chunks_lengths"], target, stdev, want_y=True, debug=True)
        lo = min(5, N - 7)
        part = EV.evaluate_batch(eng, a["chunks"][lo:lo + 7], a["chunks_lengths"][lo:lo + 7], target[lo:lo + 7], stdev[lo:lo + 7],
                                 first_chunk=lo, want_y=True)
        torch.cuda.synchronize()
    finally:
        eng.close()
    loss = out["loss"].cpu().numpy().astype(np.float64)
    mine = host_sums(out, rows, scale)
    d = np.abs(out["y"].cpu().numpy().astype(np.float64) - eval_reference(inp)) * scale
    fin = EV.finalize(loss, rows["lengths"].shape[1], rows["targets"].shape[1])
    print(f"TRAINED {name} {mode} evaluate: {N} chunks, y MAE {d.mean():.3e} pA max {d.max():.3e}, sums off by at most "
          f"{float((np.abs(loss - mine) / (1e-5 * np.abs(mine) + 1e-7)).max()):.3f} of the tolerance; "
          + " ".join(f"{k} {v:.6g}" for k, v in fin.items()))
    assert np.isfinite(loss).all()
    assert np.all(np.abs(loss - mine) <= 1e-5 * np.abs(mine) + 1e-7), np.abs(loss - mine).max(0)
    if mode in FP32_CLASS:
        assert d.mean() < 1e-4
    assert torch.equal(part["loss"], out["loss"][lo:lo + 7]) and torch.equal(part["y"], out["y"][lo:lo + 7])


# ---------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("name", ["k9", "g5x37"])
def test_backward_pass_at_trained_weights(name, request):
    inp = case(name, request)
    st = inp["student"]
    sd, cfg, rows = st["sd"], st["cfg"], st["rows"]
    N = rows["codes"].shape[0]
    idx = TREF.rows_with_every_kind(rows["kind"], 7) if "kind" in rows else np.linspace(0, N - 1, 7).astype(np.int64)
    target, stdev = ED.scaled(rows, float(cfg["scaling_max_value"]))
    codes, lengths, target, stdev = rows["codes"][idx], rows["lengths"][idx], target[idx], stdev[idx]
    _, _, g64 = TREF.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float64)
    _, _, g32 = TREF.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float32)
    tr = T.Trainer(sd, cfg, 0)
    eng = S.Engine(sd, cfg, 0, "generic-geometry")
    try:
        args = GD.on_device(codes, lengths, target, stdev)
        out = tr.gradients(*args)
        again = tr.gradients(*args)
        ev = eng.evaluate_chunks(*args)
        torch.cuda.synchronize()
        dev = T.split_blob(out["grad"].cpu().numpy(), cfg)
    finally:
        eng.close()
        tr.close()
    _, _, bad = GD.compare(f"TRAINED {name}", dev, g64, g32)
    assert torch.equal(out["loss"], ev["loss"]), "per-chunk loss sums differ from s2s_evaluate_chunks'"
    assert torch.equal(out["loss"], again["loss"]) and torch.equal(out["grad"], again["grad"]), "a second call gives other bits"
    assert bool(torch.isfinite(out["grad"]).all())
    for n in TREF.POSITION_TABLES:
        assert not dev[n].any(), f"{n} has a gradient"
    assert not bad, bad
