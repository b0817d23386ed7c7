"""The Gamma and noise heads and everything that reads them, across their range (tests/_head_variants.py: the softplus's argument
spread over the clamp at 1e-8, over softplus = 1 and over nn.Softplus's threshold of 20), where the committed and seeded weights
keep sigma near 0.008, conc near 9 and rate near 0.8:
  * sigma / conc / rate of predict and of evaluate against the float64 oracle, the clamp decided exactly;
  * the Gamma dwell against the float64 restatement of the sampler on the kernel's own conc / rate (alpha from 1e-8 to 33, 1 / alpha
    up to 1e8, rate at 1e-8), its rounding and +-1e9 clamp, and the length regulator on dwells of 1e9 (the signal against the oracle
    fed the cropped dwells; align_chunks against its definition);
  * the noise formula bit for bit with sigma from 1e-13 to 30;
  * the duration and noise rows of the evaluate loss against float64 sums of the kernel's own heads, away from a ~ 9, r ~ 0.8.
tests/test_head_variants_cpu.py proves from the reference alone that these inputs populate the regimes and that float32 itself
stays inside the two shares / bounds used here.
Measured on an MI355X (LABNOTES round 34): heads within 1.5e-05 relative of float64 (the float32 oracle's own: 8.8e-06), every clamp
decision exact; every draw of every case agrees with the restatement; signal MAE at most 4.7e-05 pA; no sample off the noise formula;
loss rows at most 0.02 of their bound -- after s2s_eval_loss_kernel began to form each k-mer's term in double: with float32 parts
the all-zero dwell row of k6-generic-C (sum 2.19 from parts of about 60) lay 1.13 of the bound away."""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
import _head_variants as H
import _philox_ref as P
from _alignment_ref import ref_align
from _bounds import MAE_TOL, MAX_TOL
from oracle import s2s_oracle as O
from test_gpu_evaluate import host_sums

pytestmark = pytest.mark.gpu

# engine tag -> (weight set, compute mode)
ENGINES = {"k9-f16x3": ("k9", "f16x3"), "k9-f32": ("k9", "f32"), "k9-f16": ("k9", "f16"), "k6-generic": ("k6", "generic"),
           "e5x37": ("e5x37", None), "e64x1024": ("e64x1024", None)}
FP32_CLASS = [t for t in ENGINES if t != "k9-f16"]
CASES = [(t, c) for t in ENGINES for c in H.COMBOS]
F32_CLAMP = np.float32(1e-8)
_ENGINES, _PREDICT, _EVAL_IN, _EVAL = {}, {}, {}, {}


def engine(tag, combo):
    if (tag, combo) not in _ENGINES:
        weights, mode = ENGINES[tag]
        ref = H.reference(weights, combo)
        _ENGINES[(tag, combo)] = S.Engine(ref["sd"], ref["cfg"], mode=mode)
        if weights.startswith("e"):
            assert _ENGINES[(tag, combo)].mode == "generic-geometry"
    return _ENGINES[(tag, combo)]


def inputs(eng, ref):
    return torch.from_numpy(ref["bases"]).to(eng.device), torch.from_numpy(ref["n_valid"]).to(eng.device)


def predict(tag, combo):
    """The debug launch every predict-side test reads, once per session: duration sampling, min_duration 0, no noise, the batch
    starting at H.FIRST under H.SEED -> the arrays on the host."""
    if (tag, combo) not in _PREDICT:
        eng, ref = engine(tag, combo), H.reference(ENGINES[tag][0], combo)
        b, nv = inputs(eng, ref)
        out = eng.predict_chunks(b, nv, S.PredictParams(noise_std=0.0, min_duration=0.0, seed=H.SEED), first_global_chunk=H.FIRST, debug=True)
        _PREDICT[(tag, combo)] = {n: out[n].cpu().numpy() for n in ("signal", "dur", "sigma", "conc", "rate", "g")}
    return _PREDICT[(tag, combo)]


def eval_inputs(tag, combo):
    """The evaluate inputs of a case on the device, once per session: the k-mers that spell the chunks of predict(), the dwell rows
    of H.loss_dwells, seeded targets and stdevs -> (device tensors, the same as a dict host_sums reads, scale)."""
    if (tag, combo) not in _EVAL_IN:
        eng, ref = engine(tag, combo), H.reference(ENGINES[tag][0], combo)
        te, ts = eng.t_enc, eng.t_dec
        n = ref["kmers"].shape[0]
        rng = np.random.default_rng(11)
        g = dict(lengths=H.loss_dwells(n, te, ts), targets=rng.random((n, ts)).astype(np.float32) * 165.0,
                 stdevs=(rng.random((n, te)) * 4.0).astype(np.float32))
        scale = float(eng.config["scaling_max_value"])
        dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in
                    (ref["kmers"], g["lengths"], (g["targets"] / scale).astype(np.float32), (g["stdevs"] / scale).astype(np.float32)))
        _EVAL_IN[(tag, combo)] = dev, g, scale
    return _EVAL_IN[(tag, combo)]


def evaluate(tag, combo, lo=0, hi=None, **kw):
    dev = eval_inputs(tag, combo)[0]
    return engine(tag, combo).evaluate_chunks(*(t[lo:hi] for t in dev), **kw)


def evaluate_all(tag, combo):
    if (tag, combo) not in _EVAL:
        _EVAL[(tag, combo)] = evaluate(tag, combo, want_y=True, debug=True)
    return (_EVAL[(tag, combo)],) + eval_inputs(tag, combo)[1:]


@pytest.mark.parametrize("tag,combo", CASES)
def test_heads_against_the_float64_oracle(tag, combo):
    """sigma, conc and rate of predict and of evaluate: within max(1e-4, 5 x the float32 oracle's own largest relative distance to
    float64 on these k-mers); exactly float32(1e-8) where the float64 argument of the softplus lies below ln(1e-8) - 1e-3; the
    k-mers within 1e-3 of ln(1e-8) skipped and counted."""
    ref = H.reference(ENGINES[tag][0], combo)
    ev = evaluate_all(tag, combo)[0]
    runs = {"predict": predict(tag, combo), "evaluate": {n: ev[n].cpu().numpy() for n in ("sigma", "conc", "rate")}}
    for head in ("sigma", "conc", "rate"):
        x, want = ref["h64"][head]
        own = ref["h32"][head][1]
        clamped = head != "sigma"
        edge = clamped & (np.abs(x - H.LN_CLAMP) <= H.EDGE)
        below = clamped & (x < H.LN_CLAMP - H.EDGE)
        own_rel = float((np.abs(own - want) / want)[~edge].max())
        bar = max(1e-4, 5.0 * own_rel)
        for name, run in runs.items():
            got = run[head]
            assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
            rel = float((np.abs(got.astype(np.float64) - want) / want)[~edge].max())
            print(f"HEADS {tag} {combo} {name} {head}: {got.min():.3e} .. {got.max():.3e}, max relative distance to float64 {rel:.3e} "
                  f"(bar {bar:.3e}: 1e-4 or 5 x the float32 oracle's own {own_rel:.3e}), {int(below.sum())} clamped, {int(edge.sum())} skipped at the edge")
            assert rel <= bar
            assert edge.mean() < 1e-3
            if clamped:
                assert (got[below] == F32_CLAMP).all() and (got >= F32_CLAMP).all()
                assert (got[x >= H.LN_CLAMP + H.EDGE] > F32_CLAMP).all()
            else:
                assert (got > 0).all()


@pytest.mark.parametrize("tag,combo", CASES)
def test_draws_rounding_and_crop(tag, combo):
    weights = ENGINES[tag][0]
    eng, ref, out = engine(tag, combo), H.reference(weights, combo), predict(tag, combo)
    te, ts = eng.t_enc, eng.t_dec
    conc, rate, g, dur = out["conc"], out["rate"], out["g"], out["dur"]
    want = H.ref_dwell(conc, rate)                             # float64, on the kernel's own conc / rate
    share_all = H.agreement_all(g, want)
    share, counted = P.agreement(g, want) if (want > 1).any() else (1.0, 0)
    print(f"HEADS {tag} {combo} draws: {share_all:.6f} of all {g.size} agree with the float64 restatement within 1e-3; {counted} above "
          f"the clamp at 1 ({share:.6f} of them agree); g {g.min():.3e} .. {g.max():.3e}, {float((dur == 10 ** 9).mean()):.3f} of the dwells at 1e9")
    assert np.isfinite(g).all() and (g >= 1.0).all()
    assert g.size >= 4000 and share_all >= 0.999
    if combo in "ACE":
        assert counted >= 2000
    if combo == "B":
        assert (g == 1.0).all()
    assert dur.dtype == np.int32 and np.array_equal(dur, np.clip(np.rint(g.astype(np.float64)), -1e9, 1e9).astype(np.int64))
    if combo == "D":
        assert (dur == 10 ** 9).mean() >= 0.05 and (dur == 10 ** 9).all(1).any()
        assert (dur.astype(np.int64).sum(1) >= 2 ** 31).mean() > 0.9         # an int32 running sum of these would wrap
        seg = eng.align_chunks(torch.from_numpy(out["signal"]).to(eng.device), torch.from_numpy(dur).to(eng.device)).cpu().numpy()
        assert np.array_equal(seg, ref_align(out["signal"], dur))
    if tag not in FP32_CLASS:
        return
    # the signal: the oracle crops at ts, so it gives the same signal for the dwells cut at ts + 1 (test_head_variants_cpu.py), and
    # those fit its int32 round
    cfg = ref["cfg"]
    p = O.PredictParams(min_duration=0.0, noise_std=0.0, scaling_max_value=float(cfg["scaling_max_value"]))
    oracle = O.predict_chunks(ref["sd"], cfg, ref["codes"], p, inject_g=torch.from_numpy(np.minimum(g, np.float32(ts + 1))))
    assert np.array_equal(oracle["dur"].numpy(), np.minimum(dur, ts + 1))
    y, r = out["signal"], oracle["signal"].numpy()
    d = np.abs(y.astype(np.float64) - r)
    print(f"HEADS {tag} {combo} signal: MAE {d.mean():.3e} pA, max {d.max():.3e} pA, {float((r != 0).mean()):.3f} of the samples live")
    assert np.array_equal(y == 0, r == 0)
    assert d.mean() < MAE_TOL and d.max() < MAX_TOL


@pytest.mark.parametrize("min_noise", [0.0, 0.5])
@pytest.mark.parametrize("tag,combo", [(t, c) for t, c in CASES if c != "D"])
def test_noise_is_the_reference_formula(tag, combo, min_noise):
    """test_builtin_noise_is_the_reference_formula (tests/test_gpu_samplers.py) at the engine's te / ts with sigma from 1e-13 to 30:
    given the kernel's own z01, sigma and dur, bit for bit clamp(clean + z01 * max(sigma_ext, min_noise) * noise_std * scale, 0)
    where clean != 0, exactly clean elsewhere."""
    eng, ref = engine(tag, combo), H.reference(ENGINES[tag][0], combo)
    te, ts = eng.t_enc, eng.t_dec
    b, nv = inputs(eng, ref)
    noise_std = 1.5
    kw = dict(min_noise=min_noise, seed=21)
    noisy = eng.predict_chunks(b, nv, S.PredictParams(noise_std=noise_std, **kw), debug=True)
    clean = eng.predict_chunks(b, nv, S.PredictParams(noise_std=0.0, **kw), debug=True)
    assert torch.equal(noisy["dur"], clean["dur"])
    y, c, z = noisy["signal"].cpu(), clean["signal"].cpu(), noisy["z01"].cpu()
    dur, sigma = noisy["dur"].cpu().long().clamp(max=ts + 1), noisy["sigma"].cpu()
    idx = (dur.cumsum(1).view(-1, 1, te) <= torch.arange(ts).view(1, ts, 1)).sum(-1)      # [B, ts], te = past the last dwell
    sig_ext = torch.cat([sigma, torch.zeros(sigma.shape[0], 1)], 1).gather(1, idx)
    scale = torch.tensor(float(ref["cfg"]["scaling_max_value"]))
    sdv = (torch.clamp(sig_ext, min=min_noise) * torch.tensor(noise_std)) * scale           # model.py:227-232, float32 step by step
    expect = torch.where(c != 0, c + z * sdv, c).clamp(min=0.0)
    live = c != 0
    print(f"HEADS {tag} {combo} noise min_noise {min_noise}: sigma {sigma.min().item():.3e} .. {sigma.max().item():.3e}, noise sd "
          f"{sdv[live].min().item():.3e} .. {sdv[live].max().item():.3e} pA on {int(live.sum())} live samples, "
          f"{int((y != expect).sum())} samples differ from the formula")
    assert live.sum() > 1000 and torch.isfinite(y).all()
    assert torch.equal(y, expect)
    assert torch.equal(y[~live], torch.zeros_like(y[~live]))


@pytest.mark.parametrize("tag,combo", CASES)
def test_duration_and_noise_loss(tag, combo):
    """loss[:, 1] and loss[:, 2] against the float64 sums (math.lgamma) of the kernel's own conc / rate / sigma, on dwells from
    {0, 1, 2, 3, 12, 40, ts, ts + 1, 32767} with an all-zero row and a row of 32767: 1e-5 |sum| + 1e-7; rows bit-identical for
    B = all, 1 and 7."""
    out, g, scale = evaluate_all(tag, combo)
    loss = out["loss"].cpu().numpy()
    mine = host_sums(out, g, scale)
    n = loss.shape[0]
    assert np.isfinite(loss).all() and (g["lengths"][0] == 0).all() and (g["lengths"][1] == 32767).all()
    for col, name in ((1, "duration"), (2, "noise")):
        dist = np.abs(loss[:, col].astype(np.float64) - mine[:, col])
        ratio = dist / (1e-5 * np.abs(mine[:, col]) + 1e-7)
        print(f"HEADS {tag} {combo} {name} loss: at most {ratio.max():.3f} of the bound 1e-5 |sum| + 1e-7 (row {int(ratio.argmax())}, sum "
              f"{mine[int(ratio.argmax()), col]:.6e}, distance {dist[int(ratio.argmax())]:.3e}); |sum| {np.abs(mine[:, col]).min():.3e} .. "
              f"{np.abs(mine[:, col]).max():.3e}")
    for col in (1, 2):
        assert np.all(np.abs(loss[:, col] - mine[:, col]) <= 1e-5 * np.abs(mine[:, col]) + 1e-7), col
    for step in (1, 7):
        parts = np.concatenate([evaluate(tag, combo, lo, min(n, lo + step))["loss"].cpu().numpy() for lo in range(0, n, step)])
        assert np.array_equal(parts, loss), step
