"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the committed goldens.

Tolerances (floating point path; stated per BASELINE.json north_star):
  * dwell indices: bit-exact;
  * zero pattern of the signal (ReLU zeros / pad / clamp): exact;
  * signal: MAE < 1e-4 pA vs the fp32 reference goldens, max |diff| < 2e-3 pA.
"""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import chunker
from seq2squiggle_amd.inference import redo_threshold
from oracle import s2s_oracle as O
from conftest import load_ckpt, load_npz
from _f16_bar import QK, variant as _variant     # (the variant checkpoints are shared with the tests of the f16 instance)

pytestmark = pytest.mark.gpu
MAE_TOL, MAX_TOL = 1e-4, 2e-3


@pytest.fixture(scope="module", autouse=True)
def _no_attention_path_override():
    """The tests below read what s2s_create's calibration launch decided: an S2S_ATTENTION_PATH left in the caller's environment
    would skip that launch (calibration_redo_rate = -1) for every engine of the module."""
    import os
    saved = os.environ.pop("S2S_ATTENTION_PATH", None)
    yield
    if saved is not None:
        os.environ["S2S_ATTENTION_PATH"] = saved


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return base


@pytest.fixture(scope="module", params=[("k9", "f32"), ("k6", "f32"), ("k9", "f16x3"), ("k6", "f16x3"),
                                        ("k9", "f16x3", "exact"), ("k6", "f16x3", "exact")],
                ids=lambda p: "-".join(p))
def case(request):
    """(checkpoint, arithmetic[, attention path]): the committed checkpoints calibrate to the fast softmax path; the "exact"
    cases run every test of this file on the other one too (s2s_set_attention_path: the online softmax as the only path)."""
    tag, mode = request.param[:2]
    sd, cfg = load_ckpt(tag)
    eng = S.Engine(sd, cfg, mode=mode)
    if mode != "f32":
        assert eng.attention_path == "fast" and 0.0 <= eng.calibration_redo_rate < 0.1
    if len(request.param) > 2:
        eng.attention_path = request.param[2]
        assert eng.attention_path == "exact"
    g = load_npz(f"stages_{tag}.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    dev = eng.device
    yield dict(tag=tag, sd=sd, cfg=cfg, eng=eng, g=g, bases=torch.from_numpy(bases).to(dev),
               nv=torch.from_numpy(nv).to(dev), dev=dev)
    eng.close()


def dev_t(case, key):
    return torch.from_numpy(np.ascontiguousarray(case["g"][key])).to(case["dev"])


def test_stage_outputs(case):
    """Intermediate tensors against the reference's (scaled units).  The split-f16 arithmetic carries 22-bit
    operands, so its stage tolerances are a few 1e-6 wider than the exact-fp32 path's."""
    g, eng = case["g"], case["eng"]
    t = dict(emb=2e-6, enc=2e-5, sig=2e-6, rel=2e-6, y=2e-5) if eng.mode == "f32" else \
        dict(emb=1e-5, enc=6e-5, sig=1e-5, rel=3e-5, y=6e-5)
    out = eng.predict_chunks(case["bases"], case["nv"], S.PredictParams(**P(noise_std=0.0)),
                             inject_g=dev_t(case, "g"), debug=True)
    torch.cuda.synchronize()
    assert np.abs(out["emb_out"].cpu().numpy() - g["emb_out"]).max() < t["emb"]
    assert np.abs(out["enc_out"].cpu().numpy() - g["enc_out"]).max() < t["enc"]
    assert np.abs(out["sigma"].cpu().numpy() - g["sigma"]).max() < t["sig"]
    assert np.allclose(out["conc"].cpu().numpy(), g["conc"], rtol=t["rel"], atol=t["rel"])
    assert np.allclose(out["rate"].cpu().numpy(), g["rate"], rtol=t["rel"], atol=t["rel"])
    assert np.array_equal(out["dur"].cpu().numpy(), g["dur_gamma"])
    assert np.abs(out["y_scaled"].cpu().numpy() - g["y_scaled_gamma"]).max() < t["y"]


CASES = [
    ("y_gamma_nsamp", dict(), True, True, False),
    ("y_gamma_nsamp_minnoise", dict(noise_std=1.5, min_noise=0.02), True, True, False),
    ("y_gamma_nconst", dict(noise_sampling=False), True, True, False),
    ("y_gamma_nonoise", dict(noise_std=0.0), True, False, False),
    ("y_ideal", dict(noise_std=0.0, noise_sampling=False, duration_sampling=False), False, False, False),
    ("y_ideal_nsamp", dict(duration_sampling=False), False, True, False),
    ("y_normal_nsamp", dict(duration_sampling=False, dwell_std=4.0), False, True, True),
    ("y_ideal_dwell31", dict(noise_std=0.0, noise_sampling=False, duration_sampling=False,
                             dwell_mean=4000 / 130), False, False, False),
]


def test_submodule_call_surface(case):
    """The reference's Encoder / NoiseSampler / LengthRegulator / Decoder signatures (modules.py:65-89, 275-278, 396-441,
    133-142), chained as predict_step chains them (model.py:197-221), against the stage goldens -- including the two the
    kernel never materialises: the length-regulated tensor (through its row sums) and the expanded sigma."""
    from seq2squiggle_amd.modules import Stages
    g, eng = case["g"], case["eng"]
    codes = torch.from_numpy(g["codes"].astype(np.int64))
    onehot = torch.zeros(*codes.shape, 5)
    known = codes < 5
    onehot[known] = torch.nn.functional.one_hot(codes[known], 5).float()        # unknown letters: all-zero rows (utils.py:86)
    st = Stages(eng, S.PredictParams(**P(noise_std=0.0)), inject_g=dev_t(case, "g"))
    x = onehot.reshape(codes.shape[0], 16, -1).to(case["dev"])                  # model.py:197-198
    enc_out, emb_out = st.encoder(x)
    sigma = st.noise_sampler(emb_out)
    out, dur, dist, noise_ext, _ = st.length_regulator(emb_out, enc_out, sigma, dwell_mean=12.5, dwell_std=0.0,
                                                       duration_sampling=True, min_length=3)
    y = st.decoder(out)
    tol = 2e-5 if eng.mode == "f32" else 6e-5
    assert enc_out.shape == emb_out.shape == (codes.shape[0], 16, 64) and sigma.shape == (codes.shape[0], 16, 1)
    assert np.abs(enc_out.cpu().numpy() - g["enc_out"]).max() < tol and np.abs(emb_out.cpu().numpy() - g["emb_out"]).max() < tol
    assert np.abs(sigma[..., 0].cpu().numpy() - g["sigma"]).max() < tol
    assert np.array_equal(dur.cpu().numpy(), g["dur_gamma"].astype(np.float32))
    assert out.shape == (codes.shape[0], 250, 64) and noise_ext.shape == (codes.shape[0], 250, 1) and y.shape == (codes.shape[0], 250, 1)
    assert np.abs(out.sum(-1).cpu().numpy() - g["lr_rowsum_gamma"]).max() < 64 * tol
    assert np.abs(noise_ext[..., 0].cpu().numpy() - g["sigma_ext_gamma"]).max() < tol
    assert np.abs(y[..., 0].cpu().numpy() - g["y_scaled_gamma"]).max() < tol
    assert torch.allclose(dist.concentration.cpu(), torch.from_numpy(g["conc"]), rtol=3e-5, atol=3e-5)
    with pytest.raises(ValueError):
        st.length_regulator(emb_out, enc_out, sigma, dwell_mean=9.0)             # contradicts the context's PredictParams


def test_standalone_submodule_operators(case):
    """The sub-modules as operators on ARBITRARY tensors, as a user of the reference may call them (modules.py: NoiseSampler
    259-278, LengthRegulator 344-441, Decoder 97-142): random emb_out / x / sigma / decoder inputs that no encoder produced,
    against the oracle's restatement of each module.  (The kernel's test instance takes the stage input from memory:
    s2s_debug.emb_in / dec_in.)"""
    from seq2squiggle_amd.modules import Stages
    eng, dev, sd, cfg = case["eng"], case["dev"], case["sd"], case["cfg"]
    gen = torch.Generator().manual_seed(11)
    B = 37                                                           # not a multiple of the group of 16
    emb = torch.rand(B, 16, 64, generator=gen) * 1.5                 # (emb_out is a ReLU output: non-negative)
    x = torch.randn(B, 16, 64, generator=gen)
    sig = torch.rand(B, 16, 1, generator=gen)
    g_inj = torch.rand(B, 16, generator=gen) * 22
    tol = 2e-5 if eng.mode == "f32" else 6e-5
    st = Stages(eng, S.PredictParams(**P(noise_std=0.0)), inject_g=g_inj.to(dev))
    # NoiseSampler on a foreign emb_out
    got = st.noise_sampler(emb.to(dev))
    assert got.shape == (B, 16, 1)
    assert np.abs(got[..., 0].cpu().numpy() - O.noise_sampler(sd, emb).numpy()).max() < tol
    # LengthRegulator on foreign tensors: Gamma parameters from emb, dwell from the injected draws, expansion of x and sigma
    out, dur, dist, noise_ext, _ = st.length_regulator(emb.to(dev), x.to(dev), sig.to(dev), dwell_mean=12.5, dwell_std=0.0,
                                                       duration_sampling=True, min_length=3)
    conc, rate = O.duration_params(sd, emb)
    ref_dur = O.durations(O.PredictParams(**P(noise_std=0.0)), B, g=g_inj)
    ref_out, ref_sx = O.length_regulate(x, sig[..., 0], ref_dur)
    assert np.array_equal(dur.cpu().numpy(), ref_dur.numpy().astype(np.float32))
    assert torch.equal(out.cpu(), ref_out) and torch.equal(noise_ext[..., 0].cpu(), ref_sx)       # pure indexing: exact
    assert torch.allclose(dist.concentration.cpu(), conc, rtol=3e-5, atol=3e-5) and torch.allclose(dist.rate.cpu(), rate, rtol=3e-5, atol=3e-5)
    # Decoder on a foreign [B,250,64] (position_enc is added inside, modules.py:136)
    h = torch.randn(B, 250, 64, generator=gen) * 0.7
    y = st.decoder(h.to(dev))
    ref_y = O.decoder(sd, cfg, h)
    assert y.shape == (B, 250, 1)
    yn, rn = y[..., 0].cpu().numpy(), ref_y.numpy()
    mism = (yn == 0) != (rn == 0)
    print(f"STANDALONE {eng.mode}: decoder zero-pattern mismatches {int(mism.sum())} of {mism.size}, max |diff| {np.abs(yn - rn).max():.3e}")
    assert not mism.any()
    assert np.abs(yn - rn).max() < 3 * tol
    # and chained use still continues the encoder's launch (the tensors of one fused launch, no second one)
    codes = torch.from_numpy(case["g"]["codes"].astype(np.int64))
    onehot = torch.zeros(*codes.shape, 5)
    onehot[codes < 5] = torch.nn.functional.one_hot(codes[codes < 5], 5).float()
    st2 = Stages(eng, S.PredictParams(**P(noise_std=0.0)), inject_g=dev_t(case, "g"))
    enc_out, emb_out = st2.encoder(onehot.reshape(codes.shape[0], 16, -1).to(dev))
    lr, _, _, _, _ = st2.length_regulator(emb_out, enc_out, st2.noise_sampler(emb_out))
    assert st2.decoder(lr).data_ptr() == st2._ctx.out["y_scaled"].data_ptr()


@pytest.mark.parametrize("key,over,use_g,use_z,use_zdw", CASES)
def test_predict_modes_vs_reference_goldens(case, key, over, use_g, use_z, use_zdw):
    g, eng = case["g"], case["eng"]
    out = eng.predict_chunks(case["bases"], case["nv"], S.PredictParams(**P(**over)),
                             inject_g=dev_t(case, "g") if use_g else None,
                             inject_z01=dev_t(case, "z01") if use_z else None,
                             inject_zdw=dev_t(case, "zdw") if use_zdw else None)
    y, ref = out["signal"].cpu().numpy(), g[key]
    assert np.array_equal(y == 0, ref == 0)
    d = np.abs(y - ref)
    assert d.mean() < MAE_TOL and d.max() < MAX_TOL, (d.mean(), d.max())
    if key == "y_normal_nsamp":
        assert np.array_equal(out["dur"].cpu().numpy(), g["dur_normal"])
    if key == "y_ideal":
        assert (out["dur"].cpu().numpy() == 12).all()


def test_wide_reference_goldens(case):
    """Round 6: ~220 chunks per chemistry of real (lambda) sequence, homopolymers, a repeat, an N-rich read and short tails, through
    the IMPORTED reference's predict_step with injected variates (tests/golden/wide_*.npz, tools/make_goldens.py wide): the HIP path
    against the reference itself on four times the chunks of the stage goldens, in both arithmetic modes and on both attention
    paths.  The bound is the file's: dwell indices and zero pattern exact, MAE < 1e-4 pA, max < 2e-3 pA."""
    eng, dev = case["eng"], case["dev"]
    g = load_npz(f"wide_{case['tag']}.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    b, n = torch.from_numpy(bases).to(dev), torch.from_numpy(nv).to(dev)
    z = torch.from_numpy(g["z01"].astype(np.float32)).to(dev)
    out = eng.predict_chunks(b, n, S.PredictParams(**P()), inject_g=torch.from_numpy(g["g"]).to(dev), inject_z01=z)
    assert np.array_equal(out["dur"].cpu().numpy(), g["dur_gamma"])
    y, ref = out["signal"].cpu().numpy(), g["y_gamma_nsamp"]
    assert np.array_equal(y == 0, ref == 0)
    d = np.abs(y - ref)
    assert d.mean() < MAE_TOL and d.max() < MAX_TOL, (d.mean(), d.max())
    out = eng.predict_chunks(b, n, S.PredictParams(**P(noise_std=1.0, noise_sampling=False, duration_sampling=False)), inject_z01=z)
    y2, ref2 = out["signal"].cpu().numpy(), g["y_ideal_nconst"]
    assert (out["dur"].cpu().numpy() == 12).all() and np.array_equal(y2 == 0, ref2 == 0)
    d2 = np.abs(y2 - ref2)
    assert d2.mean() < MAE_TOL and d2.max() < MAX_TOL, (d2.mean(), d2.max())
    print(f"WIDE {case['tag']} {eng.mode} {eng.attention_path}: {y.shape[0]} chunks, gamma + sampled noise MAE {d.mean():.2e} max {d.max():.2e}; "
          f"ideal + constant noise MAE {d2.mean():.2e} max {d2.max():.2e}")


def test_random_batch_vs_oracle(case):
    """Seeded random chunks (with N and short tails) at a size the oracle does in seconds."""
    k, eng, dev = case["cfg"]["seq_kmer"], case["eng"], case["dev"]
    rng = np.random.default_rng(42)
    reads = ["".join(rng.choice(list("ACGTN"), int(n), p=[.245, .245, .245, .245, .02]))
             for n in rng.integers(k, 400, size=40)]
    bases, nv, first = S.encode_reads(reads, k)
    codes = np.concatenate([O.encode_read(r, k) for r in reads], 0)
    B = bases.shape[0]
    gen = torch.Generator().manual_seed(3)
    ginj = (torch.rand(B, 16, generator=gen) * 25).float()
    z = torch.randn(B, 250, generator=gen)
    p = P()
    ref = O.predict_chunks(case["sd"], case["cfg"], codes, O.PredictParams(**p), inject_g=ginj, inject_z01=z)
    out = eng.predict_chunks(torch.from_numpy(bases).to(dev), torch.from_numpy(nv).to(dev), S.PredictParams(**p),
                             inject_g=ginj.to(dev), inject_z01=z.to(dev))
    assert np.array_equal(out["dur"].cpu().numpy(), ref["dur"].numpy())
    y, r = out["signal"].cpu().numpy(), ref["signal"].numpy()
    assert np.array_equal(y == 0, r == 0)
    assert np.abs(y - r).mean() < MAE_TOL and np.abs(y - r).max() < MAX_TOL


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("scale", [4.0, 16.0])
def test_peaked_attention_forces_the_rescale_fallback(mode, scale):
    """Scores spread over hundreds of units (w_qs, w_ks scaled up): later key passes beat the pass-0 maximum by far
    more than the f16 range of P allows, so the f16x3 block must detect the overflowed row sums and redo those
    heads on its safe path (running max raised every pass).  An input that forces the rare branch, checked
    against the full-tensor CPU oracle (cdna_hip_programming.md rule 26)."""
    sd, cfg = load_ckpt("k9")
    sd = {k: v.clone() for k, v in sd.items()}
    for k in sd:
        if k.startswith("decoders.") and k.endswith(("w_qs.weight", "w_ks.weight", "w_qs.bias", "w_ks.bias")):
            sd[k] *= scale
    g = load_npz("stages_k9.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    p = P(noise_std=0.0)
    ref = O.predict_chunks(sd, cfg, g["codes"], O.PredictParams(**p), inject_g=torch.from_numpy(g["g"]), stages=True)
    ref64 = O.predict_chunks(sd, cfg, g["codes"], O.PredictParams(**p), inject_g=torch.from_numpy(g["g"]), dtype=torch.float64)
    eng = S.Engine(sd, cfg, mode=mode)
    r, t = ref["signal"].numpy(), ref64["signal"].numpy()
    err_ref = np.abs(r - t)[(r == 0) == (t == 0)].mean()
    b_d, n_d, g_d = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), torch.from_numpy(g["g"]).cuda()
    if mode == "f16x3":                    # s2s_create's calibration launch saw what these weights do to the fast path
        assert eng.attention_path == "exact" and eng.calibration_redo_rate > 0.5
    ys = {}
    for path in (("fast", "exact") if mode == "f16x3" else ("fast",)):
        if mode == "f16x3":
            eng.attention_path = path
        eng.stats()
        out = eng.predict_chunks(b_d, n_d, S.PredictParams(**p), inject_g=g_d)
        y = ys[path] = out["signal"].cpu().numpy()
        st = eng.stats()                   # the production counters (s2s_stats_read)
        assert st["chunks"] == bases.shape[0] and st["softmax_runs"] == bases.shape[0] * 8 * 8 * 2
        assert 1.0 < st["in_kernel_clock_ghz"] < 2.6 and st["workgroups"] == min(256, bases.shape[0])
        if mode == "f32":
            assert st["softmax_redone"] == 0 and st["chunks_on_exact_path"] == 0
        elif path == "fast":               # ... saw the rare branch (the out-of-line online softmax)
            assert 0.5 * st["softmax_runs"] < st["softmax_redone"] <= st["softmax_runs"], st
            assert st["chunks_on_exact_path"] == 0
        else:                              # exact path at once: nothing to redo
            assert st["softmax_redone"] == 0 and st["chunks_on_exact_path"] == st["chunks"]
        assert eng.stats()["chunks"] == 0  # read-and-reset
        assert np.isfinite(y).all()
        same = ((y == 0) == (t == 0))
        assert same.mean() > 0.999
        # near-one-hot softmax amplifies rounding: judge both fp32 implementations by their distance to fp64
        err_gpu = np.abs(y - t)[same].mean()
        assert err_gpu < max(5 * err_ref, 2e-4), (path, err_gpu, err_ref)
    if mode == "f16x3":                    # two roundings of the same (near-one-hot, rounding-amplifying) softmax
        assert np.abs(ys["fast"] - ys["exact"]).mean() < max(5 * err_ref, 2e-4)
    eng.close()


def test_attention_path_calibration_and_overrides(monkeypatch):
    """s2s_create picks the attention path per checkpoint from one calibration launch on a fixed input (include/s2s_hip.h:
    s2s_set_attention_path): the committed checkpoints (0.006 % / 1.7 % of the heads redone) stay on the fast path, the decoder's
    w_qs / w_ks x 4 (79 %) goes to the exact instance; the answer is the same for every handle of the same weights; the
    environment variable and the setter override it; the counters say which instance ran."""
    sd, cfg = load_ckpt("k9")
    g = load_npz("stages_k9.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    b, n = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    def scaled(f):
        return {k: (v * f if k.startswith("decoders.") and k.endswith(("w_qs.weight", "w_ks.weight", "w_qs.bias", "w_ks.bias")) else v.clone())
                for k, v in sd.items()}
    from oracle import redo_model as R
    gi = torch.from_numpy(g["g"])
    for f in (1.0, 2.0, 4.0):
        # the decision rule, and the kernel's redo counter on the golden chunks against the CPU model of the fast path on the same
        # chunks (oracle/redo_model.py: rows whose maximum beats their pass-0 maximum by more than 18 log2 units; pass 0 = the key
        # blocks b = 0 mod 4).  x 2: 59 % with pass 0 = the first 64 keys (round 3), 6-7 % now -- near the threshold (5.5 %: where the exact instance costs the same), which is
        # why the RATE is compared with the model instead of being pinned to a window that decides the path
        eng = S.Engine(scaled(f), cfg, mode="f16x3")
        assert (eng.attention_path == "exact") == (eng.calibration_redo_rate > redo_threshold()) and 0.0 <= eng.calibration_redo_rate <= 1.0
        eng.attention_path = "fast"
        eng.stats()
        eng.predict_chunks(b, n, S.PredictParams(**P(noise_std=0.0)), inject_g=gi.cuda())
        measured = eng.stats()["redo_rate"]
        model = R.predicted_redo_rate(scaled(f), cfg, g["codes"], gi)
        first64 = R.predicted_redo_rate(scaled(f), cfg, g["codes"], gi, scheme="first64")
        print(f"REDO x{f:g}: calibration {eng.calibration_redo_rate:.4f}, golden chunks measured {measured:.4f}, model {model:.4f} (first 64 keys: {first64:.4f})")
        assert abs(measured - model) <= max(0.02, 0.35 * model), (f, measured, model)
        if f == 2.0:
            assert 0.0 < measured < 0.25 < first64                 # the interleaved pass 0 is what keeps this checkpoint off the redo path
        eng.close()
    sharp = scaled(4.0)
    rates = []
    for _ in range(2):
        eng = S.Engine(sharp, cfg, mode="f16x3")
        assert eng.attention_path == "exact" and 0.6 < eng.calibration_redo_rate < 0.9
        rates.append(eng.calibration_redo_rate)
        eng.stats()
        a = eng.predict_chunks(b, n, S.PredictParams(**P(seed=5)))
        st = eng.stats()
        assert st["chunks_on_exact_path"] == st["chunks"] == bases.shape[0] and st["softmax_redone"] == 0
        eng.attention_path = "fast"
        c = eng.predict_chunks(b, n, S.PredictParams(**P(seed=5)))
        st = eng.stats()
        assert st["chunks_on_exact_path"] == 0 and st["softmax_redone"] > 0.3 * st["softmax_runs"]
        assert torch.equal(a["dur"], c["dur"]) and float((a["signal"] - c["signal"]).abs().mean()) < MAE_TOL
        eng.close()
    assert rates[0] == rates[1]                                   # a fixed input: deterministic per set of weights
    for env, want in (("fast", "fast"), ("exact", "exact"), ("Exact", "exact"), ("FAST", "fast")):
        monkeypatch.setenv("S2S_ATTENTION_PATH", env)
        for weights in (sd, sharp):
            eng = S.Engine(weights, cfg, mode="f16x3")
            assert eng.attention_path == want and eng.calibration_redo_rate == -1.0      # no calibration launch
            eng.close()
    for env in ("auto", ""):                                      # ... means: calibrate
        monkeypatch.setenv("S2S_ATTENTION_PATH", env)
        eng = S.Engine(sharp, cfg, mode="f16x3")
        assert eng.attention_path == "exact" and eng.calibration_redo_rate == rates[0]
        eng.close()
    for env in ("sideways", "e", "1", "exactly"):                 # a typo must not pin a path silently
        monkeypatch.setenv("S2S_ATTENTION_PATH", env)
        with pytest.raises(ValueError, match="S2S_ATTENTION_PATH must be fast, exact or auto"):
            S.Engine(sd, cfg, mode="f16x3")
    monkeypatch.delenv("S2S_ATTENTION_PATH")
    eng = S.Engine(sharp, cfg, mode="f32")                        # the f32 block has one softmax path
    eng.predict_chunks(b, n, S.PredictParams(**P(seed=5)))
    assert eng.stats()["chunks_on_exact_path"] == 0
    with pytest.raises(ValueError):
        eng.attention_path = "sideways"
    eng.close()


def test_closer_to_fp64_truth_than_tolerance(case):
    """Report-style: distance to an fp64 evaluation of the same model is at the fp32 noise floor."""
    g, eng = case["g"], case["eng"]
    p = P(noise_std=0.0)
    o64 = O.predict_chunks(case["sd"], case["cfg"], g["codes"], O.PredictParams(**p),
                           inject_g=torch.from_numpy(g["g"]), dtype=torch.float64)
    out = eng.predict_chunks(case["bases"], case["nv"], S.PredictParams(**p), inject_g=dev_t(case, "g"))
    y = out["signal"].cpu().numpy().astype(np.float64)
    t = o64["signal"].numpy()
    same = (y == 0) == (t == 0)
    assert same.mean() > 0.999
    assert np.abs(y - t)[same].mean() < MAE_TOL


@pytest.mark.parametrize("mode", ["f32", "f16x3", "f16", "f16x3-exact", "f16-exact"])
@pytest.mark.parametrize("tag", ["k9", "k6"])
def test_production_instance_equals_test_instance(tag, mode):
    """`s2s_fused_kernel<MODE, false>` -- the production instance that bench.py, run_streaming and every un-instrumented
    call launch -- against `<MODE, true>`, the instance every injected-variate / stage-output parity test above runs
    (s2s_hip.hip: `test = dbg || inject_*`).  Same source, TEST only gates pointers; with the built-in Philox samplers
    (Gamma dwell modules.py:221-223, Normal noise model.py:224-240) and a fixed seed both must give the same bits.
    5,003 chunks: more than one per workgroup and not a multiple of the group of 16, ragged read tails, N bases, a read
    of length k; also through s2s_predict_packed, and in the Normal-dwell and constant-noise modes."""
    sd, cfg = load_ckpt(tag)
    k = cfg["seq_kmer"]
    eng = S.Engine(sd, cfg, mode=mode.split("-")[0])
    if mode.endswith("-exact"):
        eng.attention_path = "exact"
    dev = eng.device
    rng = np.random.default_rng(20263)
    lens = list(rng.integers(k, 900, size=170)) + [k, k + 15, k + 16, 5000]
    reads = ["".join(rng.choice(list("ACGTN"), int(n), p=[.2475, .2475, .2475, .2475, .01])) for n in lens]
    while sum(chunker.n_chunks(len(r), k) for r in reads) < 5003:
        reads.append("".join(rng.choice(list("ACGT"), int(rng.integers(k, 900)))))
    bases, nv, first = S.encode_reads(reads, k)
    bases, nv = bases[:5003], nv[:5003]
    assert int(nv.min()) < 16 and bases.shape[0] % 16 != 0
    b, n = torch.from_numpy(bases).to(dev), torch.from_numpy(nv).to(dev)
    for over in (dict(), dict(duration_sampling=False, dwell_std=3.0), dict(noise_sampling=False, noise_std=1.5)):
        pp = S.PredictParams(**P(seed=77, **over))
        prod = eng.predict_chunks(b, n, pp, first_global_chunk=123456789012)
        test = eng.predict_chunks(b, n, pp, first_global_chunk=123456789012, debug=True)
        assert torch.equal(prod["dur"], test["dur"]) and torch.equal(prod["signal"], test["signal"]), over
        assert int((prod["signal"] != 0).sum()) > 100 * 5003 and bool(torch.isfinite(prod["signal"]).all())
        # the test instance hands out the variates it drew: re-injecting them reproduces the production output again
        if not over:
            again = eng.predict_chunks(b, n, pp, first_global_chunk=123456789012, inject_g=test["g"].contiguous(),
                                       inject_z01=test["z01"].contiguous())
            assert torch.equal(again["dur"], prod["dur"])
            assert torch.equal(again["signal"], prod["signal"])         # (z01 is recorded for all 250 positions of a chunk)
    flat, cs, nv2, rf = chunker.pack_reads(reads, k)
    pp = S.PredictParams(**P(seed=77))
    packed = eng.predict_packed(torch.from_numpy(flat).to(dev), torch.from_numpy(cs).to(dev), torch.from_numpy(nv2).to(dev), pp,
                                first_global_chunk=123456789012)
    prod = eng.predict_chunks(b, n, pp, first_global_chunk=123456789012)
    assert torch.equal(packed["signal"][:5003], prod["signal"]) and torch.equal(packed["dur"][:5003], prod["dur"])
    eng.close()


def test_batch_and_offset_invariance(case):
    """Counter-based RNG: the same chunk gives the same samples whatever the batch split."""
    eng = case["eng"]
    pp = S.PredictParams(**P(seed=1234))
    full = eng.predict_chunks(case["bases"], case["nv"], pp, first_global_chunk=1000)
    s = 17
    a = eng.predict_chunks(case["bases"][:s].contiguous(), case["nv"][:s].contiguous(), pp, first_global_chunk=1000)
    b = eng.predict_chunks(case["bases"][s:].contiguous(), case["nv"][s:].contiguous(), pp, first_global_chunk=1000 + s)
    assert torch.equal(full["signal"], torch.cat([a["signal"], b["signal"]]))
    assert torch.equal(full["dur"], torch.cat([a["dur"], b["dur"]]))
    other = eng.predict_chunks(case["bases"], case["nv"], S.PredictParams(**P(seed=1235)), first_global_chunk=1000)
    assert not torch.equal(full["dur"], other["dur"])


def test_packed_reads_equal_chunk_windows(case):
    """s2s_predict_packed (chunks addressed inside the packed read buffer) == s2s_predict_chunks on the windows."""
    from seq2squiggle_amd import chunker
    eng, dev, k = case["eng"], case["dev"], case["cfg"]["seq_kmer"]
    rng = np.random.default_rng(5)
    reads = ["".join(rng.choice(list("ACGTN"), int(n))) for n in rng.integers(k, 700, size=40)] + ["A" * k, "ACGT" * 4000]
    flat, cs, nv, rf = chunker.pack_reads(reads, k)
    bases, nv2, rf2 = chunker.encode_reads(reads, k)
    assert np.array_equal(nv, nv2) and np.array_equal(rf, rf2)
    pp = S.PredictParams(**P(seed=99))
    a = eng.predict_chunks(torch.from_numpy(bases).to(dev), torch.from_numpy(nv).to(dev), pp, first_global_chunk=7)
    b = eng.predict_packed(torch.from_numpy(flat).to(dev), torch.from_numpy(cs).to(dev), torch.from_numpy(nv).to(dev), pp,
                           first_global_chunk=7)
    assert torch.equal(a["signal"], b["signal"]) and torch.equal(a["dur"], b["dur"])
    with pytest.raises(ValueError):
        eng.predict_packed(torch.from_numpy(flat).to(dev), torch.from_numpy(cs[:-1]).to(dev), torch.from_numpy(nv).to(dev), pp)


def test_empty_batch_and_bad_args(case):
    eng, dev = case["eng"], case["dev"]
    nb = 16 + case["cfg"]["seq_kmer"] - 1
    out = eng.predict_chunks(torch.zeros(0, nb, dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev),
                             S.PredictParams())
    assert out["signal"].shape == (0, 250)
    with pytest.raises(ValueError):
        eng.predict_chunks(torch.zeros(2, nb + 1, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev),
                           S.PredictParams())
    with pytest.raises(RuntimeError):
        eng.predict_chunks(case["bases"], case["nv"], S.PredictParams(min_duration=-1.0))


def test_philox_known_answers(case):
    eng = case["eng"]
    # Random123 kat_vectors: philox4x32-10
    r = eng.philox_u32(0, 0, 0, 0, 0, 1).cpu().numpy().view(np.uint32)[0]
    assert [hex(x) for x in r] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    r = eng.philox_u32(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1).cpu().numpy().view(np.uint32)[0]
    assert [hex(x) for x in r] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]


def test_sampler_statistics(case):
    """Built-in Philox samplers vs torch's own Gamma / Normal at the same parameters."""
    eng, dev, k = case["eng"], case["dev"], case["cfg"]["seq_kmer"]
    rng = np.random.default_rng(0)
    reads = ["".join(rng.choice(list("ACGT"), 16 * 64 + k - 1))]
    bases, nv, _ = S.encode_reads(reads * 64, k)
    bt, nvt = torch.from_numpy(bases).to(dev), torch.from_numpy(nv).to(dev)
    out = eng.predict_chunks(bt, nvt, S.PredictParams(**P(min_duration=0.0, seed=7)), debug=True)
    conc, rate, gd = out["conc"].cpu(), out["rate"].cpu(), out["g"].cpu()
    gen = torch.Generator().manual_seed(1)
    ref = (torch._standard_gamma(conc, generator=gen) / rate).clamp(min=1.0)
    # the 64 copies of the read share conc/rate per position but have distinct chunk counters
    assert abs(gd.mean().item() - ref.mean().item()) < 0.05 * ref.mean().item()
    assert abs(gd.std().item() - ref.std().item()) < 0.08 * ref.std().item()
    qs = torch.tensor([0.1, 0.25, 0.5, 0.75, 0.9])
    assert torch.allclose(torch.quantile(gd.flatten(), qs), torch.quantile(ref.flatten(), qs), rtol=0.06)
    z = out["z01"].cpu().flatten()
    assert abs(z.mean().item()) < 0.01 and abs(z.std().item() - 1.0) < 0.01
    assert abs((z ** 4).mean().item() - 3.0) < 0.15
    # (the laws themselves -- KS tests incl. the alpha < 1 Gamma branch, and the bit-exact noise formula -- are held in
    #  tests/test_gpu_samplers.py; this is the quick moment check that runs for every checkpoint x arithmetic mode)


def test_export_zero_strip_and_dac(case):
    tag, g, eng, dev = case["tag"], case["g"], case["eng"], case["dev"]
    sig = load_npz(f"signals_{tag}.npz")
    out = eng.predict_chunks(case["bases"], case["nv"], S.PredictParams(**P()), inject_g=dev_t(case, "g"),
                             inject_z01=dev_t(case, "z01"))
    names = [str(n) for n in g["names"]]
    order = [str(n) for n in sig["read_order"]]
    first = [0]
    for rid in order:
        first.append(first[-1] + names.count(rid))
    rf = torch.tensor(first, dtype=torch.int32, device=dev)
    prof = load_npz("profiles.npz")
    pname = "dna-r10-prom" if tag == "k9" else "dna-r9-min"
    dig, _, _, rng_, off = prof[pname + "__profile"][:5]
    ex = eng.export_reads(out["signal"], rf, dig, rng_, off, rna=False, want_pa=True, want_dac=True)
    offs = ex["offsets"].cpu().numpy()
    pa, dac = ex["pa"].cpu().numpy(), ex["dac"].cpu().numpy()
    host_sig = out["signal"].cpu()
    for r, rid in enumerate(order):
        ref = sig["sig__" + rid]
        got = pa[offs[r]:offs[r + 1]]
        assert got.shape == ref.shape, rid
        assert np.abs(got - ref).max() < MAX_TOL
        mine = O.strip_zeros([host_sig[i] for i in range(first[r], first[r + 1])]).numpy()
        assert np.array_equal(got, mine)                      # compaction itself is exact
        assert np.array_equal(dac[offs[r]:offs[r + 1]], O.to_dac(mine, dig, rng_, off))
    exr = eng.export_reads(out["signal"], rf, dig, rng_, off, rna=True, want_pa=False, want_dac=True)
    dr = exr["dac"].cpu().numpy()
    for r in range(len(order)):
        assert np.array_equal(dr[offs[r]:offs[r + 1]], dac[offs[r]:offs[r + 1]][::-1])


def test_full_size_properties():
    """BASELINE.json configs[1] size (1000 reads x 5 kb = 312,000 chunks, one launch): size-independent
    properties the domain offers -- determinism (same seed -> identical samples), tile/batch invariance of the
    counter-based RNG (any split of the batch gives the same chunks) and the strip/offset bookkeeping of the export."""
    sd, cfg = load_ckpt("k9")
    eng = S.Engine(sd, cfg, mode="f16x3")
    rng = np.random.default_rng(1234)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = [lut[rng.integers(0, 4, 5000)].tobytes().decode() for _ in range(1000)]
    bases, nv, first = S.encode_reads(reads, 9)
    assert bases.shape[0] == 312000
    b, n = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    pp = S.PredictParams(seed=42)
    a = eng.predict_chunks(b, n, pp)
    a_sig, a_dur = a["signal"].clone(), a["dur"].clone()
    again = eng.predict_chunks(b, n, pp)
    assert torch.equal(a_sig, again["signal"]) and torch.equal(a_dur, again["dur"])
    cut = 100003                                               # not a multiple of the group of 16 or of the grid
    lo = eng.predict_chunks(b[:cut].contiguous(), n[:cut].contiguous(), pp)
    hi = eng.predict_chunks(b[cut:].contiguous(), n[cut:].contiguous(), pp, first_global_chunk=cut)
    assert torch.equal(a_sig, torch.cat([lo["signal"], hi["signal"]])) and torch.equal(a_dur, torch.cat([lo["dur"], hi["dur"]]))
    assert torch.isfinite(a_sig).all() and (a_sig >= 0).all() and (a_dur >= 3).all()
    # (rows past sum(dur) are NOT forced to zero: as in the reference, the decoder sees zero rows + position_enc
    # there and only samples its ReLU/clamp zeroes are stripped, model.py:284-286)
    nz = (a_sig != 0).sum(1)
    ex = eng.export_reads(a_sig, torch.from_numpy(first).cuda(), 2048.0, 281.345551, -127.5655735, want_pa=True, want_dac=True)
    offs = ex["offsets"].cpu().numpy()
    per_read = nz.cpu().numpy().reshape(1000, 312).sum(1)
    assert np.array_equal(np.diff(offs), per_read) and offs[-1] == int(nz.sum())
    pa = ex["pa"][: offs[-1]]
    assert (pa != 0).all() and torch.equal(pa, a_sig[a_sig != 0])        # compaction keeps order and values
    eng.close()


@pytest.mark.parametrize("tag,per_read,noise_std", [("k9", 312, 2.0), ("k6", 500, 1.5)])
def test_maximum_batch_in_one_call(tag, per_read, noise_std):
    """BASELINE.json configs[2] / configs[3] per-GPU share (12,500 reads x 5 kb ~ 3.9 M chunks, 4 GB of fp32 signal; k = 6 with
    noise_std 1.5: 12,500 x 8 kb = 6.25 M chunks, 6.25 GB) in ONE call: four / six launches of <= 2^20 chunks, 64-bit row offsets,
    RNG counters beyond 2^32; spot windows across the batch must equal small separate calls (counter-based RNG), and the export
    of the whole batch must add up."""
    sd, cfg = load_ckpt(tag)
    eng = S.Engine(sd, cfg, mode="f16x3")
    rng = np.random.default_rng(7)
    B = 12500 * per_read
    nb = 16 + cfg["seq_kmer"] - 1
    bases = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (4096, nb))]).cuda()
    bases = bases.repeat(B // 4096 + 1, 1)[:B].contiguous()             # 4096 distinct chunks tiled (the RNG still differs per chunk)
    nv = torch.full((B,), 16, dtype=torch.uint8, device="cuda")
    pp = S.PredictParams(seed=3, noise_std=noise_std)
    full = eng.predict_chunks(bases, nv, pp, first_global_chunk=5_000_000_000)      # counters beyond 2^32
    sig, dur = full["signal"], full["dur"]
    assert sig.shape == (B, 250) and bool(torch.isfinite(sig[::997]).all()) and int(dur.min()) >= 3
    for lo in (0, 32768 * 57 - 5, (1 << 20) - 2050, B - 4099):         # (the third window straddles the first launch boundary)
        part = eng.predict_chunks(bases[lo:lo + 4099].contiguous(), nv[lo:lo + 4099].contiguous(), pp,
                                  first_global_chunk=5_000_000_000 + lo)
        assert torch.equal(part["signal"], sig[lo:lo + 4099]) and torch.equal(part["dur"], dur[lo:lo + 4099])
    assert not torch.equal(sig[:4096], sig[4096:8192])                  # same bases, different chunk index: different draws
    first = torch.arange(0, B + 1, per_read, dtype=torch.int32, device="cuda")
    ex = eng.export_reads(sig, first, 2048.0, 281.345551, -127.5655735, want_pa=False, want_dac=True)
    offs = ex["offsets"].cpu().numpy()
    assert offs[-1] == int((sig != 0).sum()) > 2 ** 29 and (np.diff(offs) > 0).all()
    eng.close()


EDGE_PARAMS = [
    dict(),                                                           # defaults (injected variates below)
    dict(duration_sampling=False, dwell_mean=0.0, noise_std=0.0),     # zero dwell: every row is pad + position_enc
    dict(duration_sampling=False, dwell_mean=0.4, noise_std=0.0),     # rounds to 0 as well
    dict(duration_sampling=False, dwell_mean=250.0, noise_std=0.0),   # first k-mer fills the whole chunk
    dict(min_duration=300.0),                                         # clamp beyond the chunk length
    dict(min_duration=0.0, noise_std=-1.0),                           # Gamma values below 1 clamp to 1; negative noise_std = off
    dict(noise_sampling=True, min_noise=5.0, noise_std=0.5),          # sigma clamp dominates
    dict(noise_sampling=False, noise_std=50.0),                       # large constant noise: many samples clamp to 0
]

EDGE_READS = ["ACGTACGTA", "ACGTACGTAC" * 2 + "ACGT", "ACGTACGTAC" * 2 + "ACGTA", "N" * 60, "acgtacgtacgtacgtacgtacgtacgt",
              "ACGT_ACGT__ACGTACGTACGTAC", "ACGTNNNNNNNNNACGTACGTRYKMACGTACGTACGATCGATCGATCGATTTTTTTTTTTTTTTTTTTGGGGGGGGGGGGG"]


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("over", EDGE_PARAMS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()) or "defaults")
def test_edge_inputs_and_parameters(mode, over):
    """Ragged and degenerate inputs the reference accepts (reads of length k, k+15, k+16; all-N; lower case = unknown
    letters; literal '_'), under parameter extremes, against the oracle."""
    sd, cfg = load_ckpt("k9")
    eng = S.Engine(sd, cfg, mode=mode)
    k = 9
    reads = EDGE_READS
    bases, nv, first = S.encode_reads(reads, k)
    codes = np.concatenate([O.encode_read(r, k) for r in reads], 0)
    B = bases.shape[0]
    assert B == codes.shape[0] and nv.tolist()[0] == 1
    gen = torch.Generator().manual_seed(5)
    g = torch.rand(B, 16, generator=gen) * 30                      # includes values < 1
    z = torch.randn(B, 250, generator=gen)
    p = P(**over)
    ref = O.predict_chunks(sd, cfg, codes, O.PredictParams(**p), inject_g=g, inject_z01=z)
    out = eng.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), S.PredictParams(**p),
                             inject_g=g.cuda(), inject_z01=z.cuda())
    assert np.array_equal(out["dur"].cpu().numpy(), ref["dur"].numpy())
    y, r = out["signal"].cpu().numpy(), ref["signal"].numpy()
    assert np.isfinite(y).all()
    mism = (y == 0) != (r == 0)
    assert not mism.any()                                          # (measured: 0 of 4,250 in every case; round 3 allowed 1e-3 of them)
    d = np.abs(y - r)
    print(f"EDGE {mode} {over}: mae {d.mean():.3e} max {d.max():.3e} mismatches {int(mism.sum())} of {mism.size}, |ref| there <= {np.abs(r[mism]).max() if mism.any() else 0:.2e}")
    assert d.mean() < MAE_TOL and d.max() < MAX_TOL, (d.mean(), d.max())      # (measured: <= 5.2e-5 / 2.5e-4)
    eng.close()


def layer_count_model(enc_l, dec_l, pre_l):
    """A checkpoint of enc_l / dec_l FFT blocks and pre_l pre-net layers, built from perturbed copies of the synthetic k=9 layers
    -> (state_dict, config, the generator the perturbations came from)."""
    sd0, cfg0 = load_ckpt("k9")
    cfg = dict(cfg0, encoder_layers=enc_l, decoder_layers=dec_l, pre_layers=pre_l)
    gen = torch.Generator().manual_seed(100 * enc_l + 10 * dec_l + pre_l)
    sd = {k: v.clone() for k, v in sd0.items() if ".layer_stack" not in k and "pre_net_stack" not in k}

    def perturbed(t):
        return t * (1.0 + 0.05 * torch.randn(t.shape, generator=gen)) + 0.01 * torch.randn(t.shape, generator=gen)
    for stack, n_src, n_dst in (("encoders.layer_stack", cfg0["encoder_layers"], enc_l),
                                ("decoders.layer_stack_FFT", cfg0["decoder_layers"], dec_l)):
        for l in range(n_dst):
            src = f"{stack}.{l % n_src}."
            for k, v in sd0.items():
                if k.startswith(src):
                    sd[f"{stack}.{l}." + k[len(src):]] = v.clone() if l < n_src else perturbed(v)
    for i in range(pre_l):
        for part in ("weight", "bias"):
            v = sd0[f"encoders.pre_net_stack.0.{part}"]
            sd[f"encoders.pre_net_stack.{i}.{part}"] = v.clone() if i == 0 else perturbed(v)
    return sd, cfg, gen


LAYER_COUNTS = [(1, 3, 0), (3, 1, 2), (4, 4, 4)]


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("enc_l,dec_l,pre_l", LAYER_COUNTS)
def test_other_layer_counts(mode, enc_l, dec_l, pre_l):
    """The C ABI takes 1..4 encoder/decoder layers and 0..4 pre-net layers (s2s_config): checkpoints of those shapes, built
    from perturbed copies of the synthetic k=9 layers, against the oracle (injected variates, both samplers on)."""
    sd, cfg, gen = layer_count_model(enc_l, dec_l, pre_l)
    eng = S.Engine(sd, cfg, mode=mode)
    rng = np.random.default_rng(enc_l + dec_l)
    reads = ["".join(rng.choice(list("ACGT"), 700)) for _ in range(2)]
    codes = np.concatenate([O.encode_read(r, 9) for r in reads])
    bases, nv = chunker.codes_to_bases(codes)
    B = codes.shape[0]
    g = torch.rand(B, 16, generator=gen) * 25
    z = torch.randn(B, 250, generator=gen)
    ref = O.predict_chunks(sd, cfg, codes, O.PredictParams(**P()), inject_g=g, inject_z01=z)
    for path in (("fast", "exact") if mode == "f16x3" else ("fast",)):           # both attention paths of the split-f16 block
        if mode == "f16x3":
            eng.attention_path = path
        out = eng.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), S.PredictParams(**P()),
                                 inject_g=g.cuda(), inject_z01=z.cuda())
        y, r = out["signal"].cpu().numpy(), ref["signal"].numpy()
        assert np.array_equal(out["dur"].cpu().numpy(), ref["dur"].numpy())
        assert np.array_equal(y == 0, r == 0)
        print(f"LAYERS {mode} {path} enc {enc_l} dec {dec_l} pre {pre_l}: mae {np.abs(y - r).mean():.3e} max {np.abs(y - r).max():.3e}")
        assert np.abs(y - r).mean() < MAE_TOL and np.abs(y - r).max() < MAX_TOL  # the same bound for any depth (measured: <= 5.3e-5 / 2.9e-4 with 4 + 4 layers)
    eng.close()


@pytest.mark.parametrize("tag", ["k9", "k6"])
def test_reduced_precision_f16_mode(tag):
    """S2S_MODE_F16 (decoder operands rounded to f16 once, one MFMA product per product) is OUTSIDE the 1e-4 pA parity bound by
    design.  Its bar is the reference's OWN GPU arithmetic: inference.py:403-404 runs "16-mixed" whenever a GPU is present, and
    tests/golden/mixed16.npz holds the imported reference's predict_step under fp16 autocast on these very chunks with the same
    injected variates (tools/make_goldens.py mixed16).  The mode must be at least as close to the fp32 golden as that -- MAE and
    max, measured where the reference's 16-mixed dwell indices agree with fp32's (one of its 816 / 896 indices rounds the other
    way and shifts a whole chunk; the mode's own indices are bit-exact, the frontend stays f16x3) -- and keep the zero pattern
    except where the pre-ReLU value is within that error of zero."""
    sd, cfg = load_ckpt(tag)
    g = load_npz(f"stages_{tag}.npz")
    m16 = load_npz("mixed16.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    eng = S.Engine(sd, cfg, mode="f16")
    b, n = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    kw = dict(inject_g=torch.from_numpy(g["g"]).cuda(), inject_z01=torch.from_numpy(np.ascontiguousarray(g["z01"])).cuda())
    a = eng.predict_chunks(b, n, S.PredictParams(**P()), **kw)
    assert np.array_equal(a["dur"].cpu().numpy(), g["dur_gamma"])
    y, t = a["signal"].cpu().numpy(), g["y_gamma_nsamp"]       # the reference's fp32 golden (tools/make_goldens.py)
    same = (y == 0) == (t == 0)
    assert same.mean() > 0.999
    d = np.abs(y - t)[same]
    # the reference under 16-mixed, re-derived from the committed vectors (not from the scalars stored beside them)
    r16, dur16 = m16[f"y_gamma_nsamp_16mixed_{tag}"], m16[f"dur_gamma_16mixed_{tag}"]
    agree = (dur16 == g["dur_gamma"]).all(1)
    assert 0 < (~agree).sum() <= 2 and int((dur16 != g["dur_gamma"]).sum()) == int(m16[f"dwell_indices_differing_{tag}"])
    ref_d = np.abs(r16 - t)[agree]
    assert abs(ref_d.mean() - float(m16[f"mae_vs_fp32_where_dwell_equal_{tag}"])) < 1e-6
    print(f"F16MODE {tag}: mode MAE {d.mean():.4f} max {d.max():.3f} | reference 16-mixed MAE {ref_d.mean():.4f} max {ref_d.max():.3f} "
          f"(all chunks: {np.abs(r16 - t).mean():.4f} / {np.abs(r16 - t).max():.1f})")
    assert 1e-4 < d.mean() <= ref_d.mean() and d.max() <= ref_d.max()      # measurably not the parity path; no worse than the reference's GPU path
    eng.close()


def _parity_both_paths(sd, cfg, reads, label, want_mixed=None):
    """reads -> chunks -> fast and exact path against the fp32 and fp64 oracle: dwell indices exact; the signal within the parity
    bound (MAE < 1e-4 pA, max < 2e-3 pA against the fp32 oracle -- no alternative branch: every variant has measured 4-6e-5 / 2-4e-4
    since round 5, profiles/r05/redo_and_mixed_regime_tests.txt) AND no further from the fp64 evaluation than 5 x the fp32 oracle
    itself is; the zero pattern equal except where a ReLU output sits within the parity bound of zero (a sample may be 0 on one side
    and < 2e-3 pA on the other -- counted, printed, and held below 0.05 % of the samples).
    -> (calibration redo rate, redo rate of this input on the fast path, the CPU model's)."""
    from oracle import redo_model as R
    k = cfg["seq_kmer"]
    bases, nv, _ = S.encode_reads(reads, k)
    codes = np.concatenate([O.encode_read(r, k) for r in reads], 0)
    B = bases.shape[0]
    gen = torch.Generator().manual_seed(11)
    gi = torch.rand(B, 16, generator=gen) * 20
    p = P(noise_std=0.0)
    ref = O.predict_chunks(sd, cfg, codes, O.PredictParams(**p), inject_g=gi)
    ref64 = O.predict_chunks(sd, cfg, codes, O.PredictParams(**p), inject_g=gi, dtype=torch.float64)
    r, t = ref["signal"].numpy(), ref64["signal"].numpy()
    agree64 = (r == 0) == (t == 0)
    err_ref = np.abs(r - t)[agree64].mean()
    eng = S.Engine(sd, cfg, mode="f16x3")
    calib = eng.calibration_redo_rate
    b_d, n_d, g_d = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), gi.cuda()
    live = None
    for path in ("fast", "exact"):
        eng.attention_path = path
        eng.stats()
        out = eng.predict_chunks(b_d, n_d, S.PredictParams(**p), inject_g=g_d)
        y = out["signal"].cpu().numpy()
        st = eng.stats()
        assert st["chunks"] == B and st["softmax_runs"] == B * 8 * 8 * cfg["decoder_layers"]
        assert np.array_equal(out["dur"].cpu().numpy(), ref["dur"].numpy()), (label, path)
        same = (y == 0) == (r == 0)
        assert same.mean() > 0.9995, (label, path, same.mean())
        flipped = int((~same).sum())
        if flipped:                                    # a sample that is zero on one side only is within the bound of zero on the other
            assert np.abs(y - r)[~same].max() < MAX_TOL, (label, path, flipped, np.abs(y - r)[~same].max())
        mae, mx = np.abs(y - r)[same].mean(), np.abs(y - r)[same].max()
        err_gpu = np.abs(y - t)[same & agree64].mean()
        assert mae < MAE_TOL and mx < MAX_TOL, (label, path, mae, mx)
        assert err_gpu < 5 * err_ref, (label, path, err_gpu, err_ref)
        if path == "fast":
            live = st["redo_rate"]
            if want_mixed:
                assert 0 < st["softmax_redone"] < 0.5 * st["softmax_runs"], (label, st)      # some heads of a launch redone, their partners not
        else:
            assert st["softmax_redone"] == 0 and st["chunks_on_exact_path"] == B
        print(f"MIXED {label} {path}: {B} chunks, redo {st['redo_rate']:.4f} (calibration {calib:.4f}), zero-pattern flips {flipped} of {same.size}, MAE {mae:.2e} max {mx:.2e} "
              f"vs fp64 {err_gpu:.2e} (fp32 oracle vs fp64 {err_ref:.2e})")
    eng.close()
    model = R.predicted_redo_rate(sd, cfg, codes, gi)
    assert abs(live - model) <= max(0.02, 0.35 * model), (label, live, model)
    return calib, live, model


@pytest.mark.parametrize("kind", ["x2", "pos2", "pos3"])
@pytest.mark.parametrize("tag", ["k9", "k6"])
def test_mixed_redo_regime_against_the_oracle(tag, kind):
    """the regime in which SOME heads of a launch are redone by the fast instance's out-of-line online softmax
    while their partner waves are not (the tested cases were 0 % and >= 79 % redone) -- against the fp32 and fp64 oracle, on both
    attention paths, on 240 chunks of random and lambda-genome sequence.  Reference: layers.py:20-40."""
    from oracle import redo_model as R
    sd, cfg = load_ckpt(tag)
    fam = R.input_families(seed=3, n_reads=5, read_len=384)
    reads = fam["random"] + fam["lambda"]
    _parity_both_paths(_variant(sd, kind), cfg, reads, f"{tag}-{kind}", want_mixed=True)


@pytest.mark.parametrize("tag", ["k9", "k6", "k9-x2"])
def test_redo_share_depends_on_the_input_and_parity_holds(tag):
    """the calibration launch decides on 512 pseudo-random chunks, but the redo share is a property of the
    weights AND the reads.  Real sequence (lambda), homopolymers, di- / tri-nucleotide repeats and N-rich reads through the
    committed checkpoints (and the x 2 one, which sits near the threshold): parity holds on both paths for every family, and the
    live redo share is reported beside the calibration's and the CPU model's (tools/redo_inputs.py prints the same table;
    inference_run warns when a run on the fast path ends above the threshold)."""
    from oracle import redo_model as R
    sd, cfg = load_ckpt(tag[:2])
    if tag.endswith("-x2"):
        sd = _variant(sd, "x2")
    rows = {}
    for name, reads in R.input_families(seed=5, n_reads=4, read_len=320).items():
        rows[name] = _parity_both_paths(sd, cfg, reads, f"{tag}-{name}")
    print("REDO_BY_INPUT", tag, {k: tuple(round(x, 4) for x in v) for k, v in rows.items()})
    if tag != "k9-x2":
        assert all(live < redo_threshold() for _, live, _ in rows.values()), rows      # the committed checkpoints stay on the fast path for every family
