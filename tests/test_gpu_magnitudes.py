"""GPU parity across operand magnitudes: function-preserving power-of-two rescalings of the FFT blocks (tests/_reparam.py).

The fp32 oracle's output is bit-equal for every variant (tests/test_reparam_cpu.py), so every expectation here is the e = 0
expectation, and whatever moves on the GPU is the operand range a mode sees.  The exact modes must not move at all; the split-f16
mode, whose lo halves turn subnormal below |x| = 2^-3, must hold the project's parity bounds over the band recorded in
tests/_reparam.py (LABNOTES.md round 16) and stay finite with exact dwell indices everywhere the range condition admits.

Inputs: one 392-base random read (24 chunks: past the group of 16) and the ragged reads of
test_gpu_parity.py::test_edge_inputs_and_parameters, 41 chunks in all; pass "g": injected Gamma draws, noise off; pass "z": the same
draws, injected normals, the noise sampler on.  Every test builds its own engines (s2s_create is a few milliseconds)."""
import functools

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from oracle import s2s_oracle as O
from conftest import load_ckpt
from _bounds import MAE_TOL, MAX_TOL
import _reparam as R

pytestmark = pytest.mark.gpu
TAG, K = "k9", 9
RAGGED = ["ACGTACGTA", "ACGTACGTAC" * 2 + "ACGT", "ACGTACGTAC" * 2 + "ACGTA", "N" * 60, "acgtacgtacgtacgtacgtacgtacgt",
          "ACGT_ACGT__ACGTACGTACGTAC", "ACGTNNNNNNNNNACGTACGTRYKMACGTACGTACGATCGATCGATCGATTTTTTTTTTTTTTTTTTTGGGGGGGGGGGGG"]
STAGE_TOL = dict(emb=1e-5, enc=6e-5, sig=1e-5, rel=3e-5)       # test_gpu_parity.py::test_stage_outputs, split-f16 frontend
PASSES = {"g": dict(noise_std=0.0), "z": dict()}


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return base


@pytest.fixture(scope="module", autouse=True)
def _no_attention_path_override():
    import os
    saved = os.environ.pop("S2S_ATTENTION_PATH", None)
    yield
    if saved is not None:
        os.environ["S2S_ATTENTION_PATH"] = saved


def oracle_runs(sd, cfg, inp):
    """-> {pass: (fp32 oracle output with stages, fp64 oracle output)}."""
    out = {}
    for name, over in PASSES.items():
        z = None if name == "g" else inp["z"]
        out[name] = (O.predict_chunks(sd, cfg, inp["codes"], O.PredictParams(**P(**over)), inject_g=inp["g"], inject_z01=z, stages=True),
                     O.predict_chunks(sd, cfg, inp["codes"], O.PredictParams(**P(**over)), inject_g=inp["g"], inject_z01=z,
                                      dtype=torch.float64))
    return out


@functools.lru_cache(maxsize=None)
def inputs():
    """The chunks, the injected variates, the oracle's e = 0 expectation of both passes (fp32 and fp64) and the fp64 taps the range
    condition is evaluated from: computed once for the module and never written to."""
    sd, cfg = load_ckpt(TAG)
    rng = np.random.default_rng(392)
    reads = ["".join(rng.choice(list("ACGT"), 392))] + RAGGED
    bases, nv, _ = S.encode_reads(reads, K)
    codes = np.concatenate([O.encode_read(r, K) for r in reads], 0)
    B = bases.shape[0]
    assert B == codes.shape[0] == 41 and O.encode_read(reads[0], K).shape[0] == 24
    gen = torch.Generator().manual_seed(17)
    inp = dict(sd=sd, cfg=cfg, codes=codes, B=B, g=torch.rand(B, 16, generator=gen) * 25, z=torch.randn(B, 250, generator=gen))
    inp["ref"] = oracle_runs(sd, cfg, inp)
    inp["taps"] = R.intermediates(sd, cfg, codes, inp["g"])
    inp["dev"] = dict(bases=torch.from_numpy(bases).cuda(), nv=torch.from_numpy(nv).cuda(), g=inp["g"].cuda(), z=inp["z"].cuda())
    return inp


def run(eng, inp, name, debug=False):
    d = inp["dev"]
    return eng.predict_chunks(d["bases"], d["nv"], S.PredictParams(**P(**PASSES[name])), inject_g=d["g"],
                              inject_z01=None if name == "g" else d["z"], debug=debug)


def metrics(out, ref, ref64):
    """The figures of test_gpu_parity.py::_parity_both_paths for one launch: over the samples whose zero pattern agrees with the fp32
    oracle's, MAE and max against it and the mean distance to the fp64 oracle beside the fp32 oracle's own; the flips counted, with
    their largest |difference|."""
    y = out["signal"].cpu().numpy()
    r, t = ref["signal"].numpy(), ref64["signal"].numpy()
    agree64 = (r == 0) == (t == 0)
    m = dict(dur_equal=bool(np.array_equal(out["dur"].cpu().numpy(), ref["dur"].numpy())), finite=bool(np.isfinite(y).all()))
    if not m["finite"]:
        return m
    same = (y == 0) == (r == 0)
    d = np.abs(y - r)
    m.update(flips=int((~same).sum()), flip_max=float(d[~same].max()) if (~same).any() else 0.0, share_same=float(same.mean()),
             mae=float(d[same].mean()), max=float(d[same].max()), err64=float(np.abs(y - t)[same & agree64].mean()),
             err64_ref=float(np.abs(r - t)[agree64].mean()))
    m["ratio64"] = m["err64"] / m["err64_ref"]
    return m


def within_bounds(m, fp64_rule):
    """The project's parity bounds (tests/_bounds.py, _parity_both_paths) on one set of figures."""
    return (m["dur_equal"] and m["finite"] and m["share_same"] > 0.9995 and m["flip_max"] < MAX_TOL and m["mae"] < MAE_TOL
            and m["max"] < MAX_TOL and (not fp64_rule or m["err64"] < 5 * m["err64_ref"]))


def envelope_rows(sd, inp, mode, ref=None):
    """One engine of `mode` on these weights -> {(attention path, pass): figures [+ redo rate on the fast path]}."""
    ref = ref or inp["ref"]
    eng = S.Engine(sd, inp["cfg"], mode=mode)
    rows = {}
    try:
        for path in ("fast", "exact"):
            eng.attention_path = path
            for name in PASSES:
                eng.stats()
                m = metrics(run(eng, inp, name), *ref[name])
                st = eng.stats()
                assert st["chunks"] == inp["B"]
                assert st["chunks_on_exact_path"] == (inp["B"] if path == "exact" else 0)
                m["redo"] = st["redo_rate"]
                rows[(path, name)] = m
    finally:
        eng.close()
    return rows


def fmt(m):
    if not m.get("finite", False):
        return f"dur {'ok' if m['dur_equal'] else 'DIFFERS'} NON-FINITE"
    return (f"dur {'ok' if m['dur_equal'] else 'DIFFERS'} MAE {m['mae']:.2e} max {m['max']:.2e} fp64 x{m['ratio64']:.2f} "
            f"flips {m['flips']} (<= {m['flip_max']:.1e}) redo {m.get('redo', 0.0):.4f}")


@pytest.mark.parametrize("scope", R.SCOPES)
@pytest.mark.parametrize("pair", R.PAIRS)
@pytest.mark.parametrize("mode", ["f32", "generic"])
def test_exact_modes_are_invariant(mode, pair, scope):
    """S2S_MODE_F32 and S2S_MODE_GENERIC evaluate these blocks in fp32 (the f32 engine's encoder blocks included): signal and dwell
    indices of every admitted variant are bit-equal to the mode's own e = 0 run, in both passes -- no denormal flush in the
    f32-input MFMA and no rounding in the order of the softmax scale on Q reaches the output (measured: LABNOTES.md round 16)."""
    inp = inputs()
    base = S.Engine(inp["sd"], inp["cfg"], mode=mode)
    want = {name: {k: v.clone() for k, v in run(base, inp, name).items()} for name in PASSES}
    base.close()
    for name in PASSES:                                 # ... and that run is itself inside the parity bounds, zero pattern exact
        m = metrics(want[name], *inp["ref"][name])
        assert m["flips"] == 0 and within_bounds(m, fp64_rule=(name == "g")), (mode, name, m)
    for e in R.admitted(inp["sd"], inp["taps"], pair, scope):
        eng = S.Engine(R.variant(inp["sd"], pair, e, scope), inp["cfg"], mode=mode)
        for name in PASSES:
            out = run(eng, inp, name)
            assert torch.equal(out["dur"], want[name]["dur"]), (mode, pair, scope, e, name)
            assert torch.equal(out["signal"], want[name]["signal"]), (mode, pair, scope, e, name)
        eng.close()


@pytest.mark.parametrize("scope", R.SCOPES)
@pytest.mark.parametrize("pair", R.PAIRS)
def test_split_f16_envelope(pair, scope):
    """S2S_MODE_F16X3 on both attention paths (switched on one engine).  Every admitted variant: dwell indices equal to the oracle's
    and a finite signal.  Inside the recorded band (which holds e = -1, 0, +1 at least: one binade changes only which lo halves are
    subnormal, and a parity contract that does not survive that is a defect): MAE < 1e-4 pA and max < 2e-3 pA against the fp32
    oracle over the samples whose zero pattern agrees, every flipped sample below 2e-3 pA, and -- pass "g", as in
    _parity_both_paths -- no further from the fp64 oracle than 5 x the fp32 oracle is."""
    inp = inputs()
    inside = R.band(pair, scope)
    assert {-1, 0, 1} <= set(inside)
    ok = R.admitted(inp["sd"], inp["taps"], pair, scope)
    assert set(inside) <= set(ok)
    for e in ok:
        rows = envelope_rows(R.variant(inp["sd"], pair, e, scope), inp, "f16x3")
        for (path, name), m in rows.items():
            print(f"ENVELOPE f16x3 {pair} {scope} e {e:+d} {path} {name}: {fmt(m)}")
            assert m["dur_equal"] and m["finite"], (pair, scope, e, path, name)
            if e in inside:
                assert within_bounds(m, fp64_rule=(name == "g")), (pair, scope, e, path, name, m)


@pytest.mark.parametrize("pair", R.PAIRS)
def test_stage_outputs_of_encoder_variants(pair):
    """The frontend is split-f16 in every tuned mode and its outputs feed the samplers: enc_out, sigma, conc and rate of the
    encoder-scope variants against the oracle at test_stage_outputs' tolerances, inside the recorded band; dwell indices exact."""
    inp = inputs()
    ref = inp["ref"]["g"][0]
    for e in R.band(pair, "encoder"):
        eng = S.Engine(R.variant(inp["sd"], pair, e, "encoder"), inp["cfg"], mode="f16x3")
        out = run(eng, inp, "g", debug=True)
        torch.cuda.synchronize()
        d_enc = float(np.abs(out["enc_out"].cpu().numpy() - ref["enc_out"].numpy()).max())
        d_sig = float(np.abs(out["sigma"].cpu().numpy() - ref["sigma"].numpy()).max())
        print(f"STAGES f16x3 {pair} encoder e {e:+d}: enc_out {d_enc:.2e} sigma {d_sig:.2e}")
        assert d_enc < STAGE_TOL["enc"] and d_sig < STAGE_TOL["sig"], (pair, e, d_enc, d_sig)
        for key in ("conc", "rate"):
            assert np.allclose(out[key].cpu().numpy(), ref[key].numpy(), rtol=STAGE_TOL["rel"], atol=STAGE_TOL["rel"]), (pair, e, key)
        assert np.array_equal(out["dur"].cpu().numpy(), ref["dur"].numpy())
        eng.close()


@pytest.mark.parametrize("scope", R.SCOPES)
@pytest.mark.parametrize("pair", R.PAIRS)
def test_f16_mode_stays_finite(pair, scope):
    """Recorded only (LABNOTES.md round 16): S2S_MODE_F16, outside the parity bound by design, over the same sweep -- dwell indices exact
    (the frontend is the split-f16 one) and a finite signal."""
    inp = inputs()
    for e in R.admitted(inp["sd"], inp["taps"], pair, scope):
        for (path, name), m in envelope_rows(R.variant(inp["sd"], pair, e, scope), inp, "f16").items():
            print(f"ENVELOPE f16 {pair} {scope} e {e:+d} {path} {name}: {fmt(m)}")
            assert m["dur_equal"] and m["finite"], (pair, scope, e, path, name)


def test_trained_like_checkpoint_stays_finite():
    """Recorded only: every Linear weight and bias of every FFT block x 2^-2 -- NOT function-preserving, the oracle is recomputed --
    through the split-f16 mode: dwell indices exact and a finite signal."""
    inp = inputs()
    sd = R.trained_like(inp["sd"])
    taps = R.intermediates(sd, inp["cfg"], inp["codes"], inp["g"])
    assert max(taps.values()) < R.RANGE_LIMIT
    ref = oracle_runs(sd, inp["cfg"], inp)
    assert not torch.equal(ref["g"][0]["signal"], inp["ref"]["g"][0]["signal"])
    for (path, name), m in envelope_rows(sd, inp, "f16x3", ref=ref).items():
        print(f"ENVELOPE f16x3 trained-like x2^-2 {path} {name}: {fmt(m)}")
        assert m["dur_equal"] and m["finite"], (path, name)


def test_trained_checkpoint_holds_the_bounds(request):
    """THIS test, not test_trained_like_checkpoint_stays_finite above, is the evidence about trained weights: that one rescales the
    synthetic checkpoint (a stand-in from before the project had a trainer) and asserts a finite signal only; this one takes the
    student "k9" of tests/_trained.py -- 300 Adam steps of the project's trainer from a fresh initialisation -- through the same
    envelope_rows call, the oracle recomputed on it, and asserts the full parity bounds on both attention paths in both passes."""
    import _trained as TR
    inp = inputs()
    st = TR.student("k9", request)
    sd = st["sd"]
    taps = R.intermediates(sd, inp["cfg"], inp["codes"], inp["g"])
    assert max(taps.values()) < R.RANGE_LIMIT
    ref = oracle_runs(sd, inp["cfg"], inp)
    assert not torch.equal(ref["g"][0]["signal"], inp["ref"]["g"][0]["signal"])
    for name, (r32, r64) in ref.items():              # the caps of within_bounds do not carry it: the reference alone stays inside them
        r, t = r32["signal"].numpy(), r64["signal"].numpy()
        agree64 = (r == 0) == (t == 0)
        assert agree64.mean() > 0.9995 and np.abs(r - t)[agree64].mean() > 0, name
    rows = envelope_rows(sd, inp, "f16x3", ref=ref)
    for (path, name), m in rows.items():
        print(f"TRAINED k9 f16x3 {path} {name}: {fmt(m)}")
    for (path, name), m in rows.items():
        assert within_bounds(m, fp64_rule=(name == "g")), (path, name, m)
