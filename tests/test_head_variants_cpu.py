"""The inputs of tests/test_gpu_head_range.py do what they claim, from the reference alone (the float64 oracle, no GPU): for every
weight set and combination of tests/_head_variants.py, on the very chunks the GPU tests run,
  * the regimes are populated on both sides of their boundary, and almost no k-mer sits where float32 may decide the clamp either way;
  * the float32 restatement of the Gamma sampler stays within the draw-agreement bar of the float64 one, so that bar grades the
    kernel and not float32;
  * torch's float32 Gamma.log_prob stays within the loss bound of the float64 sum, likewise;
  * the oracle's length regulator gives the same signal for a dwell and for min(dwell, ts + 1), which is how the GPU test feeds it
    dwells that an int32 cannot hold.
Measured: the float32 oracle flips no clamp decision on these inputs (its x lies within 1.2e-5 of float64's); the float32 restatement
agrees with the float64 one on every draw of every case; the duration loss stays below 0.02 of its bound except on the all-zero
dwell row of C (conc ~ rate ~ 20 at x = 1: the parts of a term are about 60 and cancel below 1), where torch's float32 reaches 0.58."""
import numpy as np
import pytest
import torch

import _head_variants as H
import _philox_ref as P
from oracle import s2s_oracle as O

CASES = [(w, c) for w in H.WEIGHTS for c in H.COMBOS]
F32_CLAMP = float(np.float32(1e-8))


def test_preactivations_are_the_oracles_heads():
    """The helper that exposes the softplus's argument gives the oracle's own sigma / conc / rate bit for bit, in both precisions."""
    ref = H.reference("k9", "A")
    for dtype, h in ((torch.float64, ref["h64"]), (torch.float32, ref["h32"])):
        sd = {k: v.to(dtype) for k, v in ref["sd"].items()}
        _, emb = O.encoder(sd, ref["cfg"], O.one_hot(ref["codes"], dtype))
        conc, rate = O.duration_params(sd, emb)
        for name, t in (("sigma", O.noise_sampler(sd, emb)), ("conc", conc), ("rate", rate)):
            assert np.array_equal(t.double().numpy(), h[name][1]), (dtype, name)


def test_variant_scales_the_weight_and_sets_the_bias():
    sd, _ = H.base_weights("k6")
    v = H.variant(sd, "rate", 250.0, -3.5)
    p = H.HEADS["rate"]
    assert torch.equal(v[p + ".3.weight"], sd[p + ".3.weight"] * 250.0) and v[p + ".3.bias"].tolist() == [-3.5]
    assert all(v[k] is sd[k] for k in sd if k not in (p + ".3.weight", p + ".3.bias"))
    assert float(sd[p + ".3.bias"]) != -3.5                     # the copy, not the original


@pytest.mark.parametrize("weights,combo", CASES)
def test_regime_populations(weights, combo):
    ref = H.reference(weights, combo)
    for head in ("conc", "rate", "sigma"):
        regime = H.regime_of(combo, head)
        if regime is None:
            continue
        x, v = ref["h64"][head]
        x32, v32 = ref["h32"][head]
        edge = float((np.abs(x - H.LN_CLAMP) <= H.EDGE).mean())
        below = x < H.LN_CLAMP - H.EDGE
        flips = int(((v32 == F32_CLAMP) != (x < H.LN_CLAMP)).sum()) if head != "sigma" else 0
        shares = dict(clamped=float(below.mean()), band=float(((x >= H.LN_CLAMP + H.EDGE) & (x <= -10)).mean()),
                      below1=float((v < 1).mean()), above1=float((v > 1).mean()),
                      x15_20=float(((x >= 15) & (x < 20)).mean()), above20=float((x > 20).mean()))
        print(f"HEADS population {weights} {combo} {head} ({regime}): x {x.min():.2f} .. {x.max():.2f}, value {v.min():.3e} .. {v.max():.3e}, "
              + ", ".join(f"{k} {s:.3f}" for k, s in shares.items()) + f", within 1e-3 of the clamp {edge:.5f}, float32 clamp flips {flips}, "
              f"float32 max |x32 - x64| {np.abs(x32 - x).max():.2e}")
        assert head == "sigma" or edge < 1e-3                  # (sigma is not clamped: nothing to decide there)
        if regime == "clamp":
            assert shares["clamped"] >= 0.05 and shares["band"] >= 0.20
            if head != "sigma":                                # the float64 oracle clamps exactly those
                assert (v[below] == 1e-8).all() and (v[x >= H.LN_CLAMP + H.EDGE] > 1e-8).all()
        elif regime == "unit":
            assert shares["below1"] >= 0.20 and shares["above1"] >= 0.20
        elif regime == "threshold":
            assert shares["x15_20"] >= 0.20 and shares["above20"] >= 0.20
        else:                                                  # far: exp(x) overflows float32 at every k-mer
            assert x.min() > H.LN_FLT_MAX + 1 and np.array_equal(v, x)
    s = ref["h64"]["sigma"][1]
    assert (s > 0).all() and np.isfinite(s).all()              # sigma is never clamped
    if combo == "B":
        assert s.min() < 1e-12
    if combo == "C":
        assert s.max() > 27


@pytest.mark.parametrize("weights,combo", CASES)
def test_draw_agreement_cap(weights, combo):
    """float32 against float64 restatement of the sampler on the float32 oracle's conc / rate: at least 99.95 % of ALL draws agree
    within 1e-3 relative after the clamps (the GPU test asks 99.9 % of the kernel).  Also what the GPU test assumes of each
    combination: A and C keep 2,000 draws above the clamp at 1, every draw of B sits at it, and in D at least 5 % of the dwells
    round to 1e9 or beyond, whole chunks of them, so that an int32 running sum of the unclamped dwells would wrap."""
    ref = H.reference(weights, combo)
    conc, rate = (ref["h32"][h][1].astype(np.float32) for h in ("conc", "rate"))
    g64, g32 = H.ref_dwell(conc, rate, np.float64), H.ref_dwell(conc, rate, np.float32)
    share_all = H.agreement_all(g32, g64)
    share, counted = P.agreement(g32, g64) if (g64 > 1).any() else (1.0, 0)
    print(f"HEADS draw cap {weights} {combo}: float32 against float64 restatement, {share_all:.6f} of all {g64.size} draws agree within 1e-3; "
          f"{counted} above the clamp at 1 ({share:.6f} of them agree); conc {conc.min():.3e} .. {conc.max():.3e}, rate {rate.min():.3e} .. "
          f"{rate.max():.3e}, g up to {g64.max():.3e}")
    assert g64.size >= 4000 and share_all >= 0.9995
    if combo in "ACE":
        assert counted >= 2000
    if combo == "B":
        assert (g64 == 1.0).all()
    if combo == "D":
        dur = np.clip(np.rint(g64), -1e9, 1e9)
        full = (dur == 1e9).all(1)
        print(f"HEADS draw cap {weights} D: {float((dur == 1e9).mean()):.3f} of the dwells at 1e9, {int(full.sum())} chunks hold nothing else, "
              f"{int((np.rint(g64).sum(1) >= 2 ** 31).sum())} of {dur.shape[0]} chunks sum past 2^31")
        assert (dur == 1e9).mean() >= 0.05 and full.any()
        # the length regulator's k-mer of sample t, i(t) = #{j : cum[j] <= t}: with an int32 running sum of the dwells as they are
        # (no "a dwell past the crop acts like ts + 1") the sum wraps below zero and i(t) moves, so the signal test sees it
        ts = ref["cfg"]["max_signal_len"]
        t = np.arange(ts)[None, :, None]
        true = (np.cumsum(np.minimum(dur, ts + 1).astype(np.int64), 1)[:, None, :] <= t).sum(-1)
        wrapped = (np.cumsum(dur.astype(np.int64), 1).astype(np.int32)[:, None, :] <= t).sum(-1)
        moved = (true != wrapped).any(1)
        print(f"HEADS draw cap {weights} D: an unclamped int32 running sum moves i(t) in {int(moved.sum())} of {dur.shape[0]} chunks")
        assert moved[full].all() and moved.mean() > 0.5


@pytest.mark.parametrize("weights,combo", CASES)
def test_duration_loss_cap(weights, combo):
    """torch's float32 Gamma(conc, rate).log_prob, summed over a chunk in float32, against the float64 sum (math.lgamma) on the same
    float32 conc / rate and the dwell rows of the GPU test: inside the project's 1e-5 |sum| + 1e-7."""
    ref = H.reference(weights, combo)
    conc, rate = (torch.from_numpy(ref["h32"][h][1].astype(np.float32)) for h in ("conc", "rate"))
    te, ts = ref["cfg"]["max_dna_len"], ref["cfg"]["max_signal_len"]
    d = H.loss_dwells(conc.shape[0], te, ts)
    assert (d[0] == 0).all() and (d[1] == 32767).all() and set(np.unique(d)) == {0, 1, 2, 3, 12, 40, ts, ts + 1, 32767}
    x = torch.from_numpy(np.where(d == 0, 1, d).astype(np.float32))
    got = (-torch.distributions.Gamma(conc, rate).log_prob(x)).sum(1).double().numpy()
    want = H.loss_sums64(conc.numpy(), rate.numpy(), d)
    ratio = np.abs(got - want) / (1e-5 * np.abs(want) + 1e-7)
    print(f"HEADS loss cap {weights} {combo}: float32 log_prob at most {ratio.max():.3f} of the bound; sums {np.abs(want).min():.3e} .. "
          f"{np.abs(want).max():.3e}")
    assert np.isfinite(got).all() and ratio.max() <= 1.0


@pytest.mark.parametrize("weights", ["k9", "e5x37"])
def test_oracle_signal_is_the_same_for_a_dwell_and_its_crop(weights):
    """length_regulate crops at ts: the oracle gives bit for bit the same signal for g and for min(g, ts + 1), on dwells up to 32767
    (larger ones do not fit the oracle's int32 round; the GPU test therefore hands it the cropped ones)."""
    ref = H.reference(weights, "A")
    cfg = ref["cfg"]
    te, ts = cfg["max_dna_len"], cfg["max_signal_len"]
    n = 12
    rng = np.random.default_rng(3)
    values = np.array([1, 2, 3, 12, 40, ts - 1, ts, ts + 1, ts + 2, 1000, 32767], np.float32)
    g = values[rng.integers(0, len(values), (n, te))]
    g[0], g[1, 0] = 32767, ts + 1
    p = O.PredictParams(min_duration=0.0, noise_std=0.0, scaling_max_value=float(cfg["scaling_max_value"]))
    a = O.predict_chunks(ref["sd"], cfg, ref["codes"][:n], p, inject_g=torch.from_numpy(g))
    b = O.predict_chunks(ref["sd"], cfg, ref["codes"][:n], p, inject_g=torch.from_numpy(np.minimum(g, ts + 1)))
    assert torch.equal(a["signal"], b["signal"]) and (a["signal"] != 0).any()
    assert torch.equal(b["dur"], a["dur"].clamp(max=ts + 1))
