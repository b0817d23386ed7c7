"""The instrument of tests/test_gpu_magnitudes.py, checked on the CPU: the rescalings of tests/_reparam.py leave the fp32 oracle's
output unchanged bit for bit, and the range condition admits the exponents the GPU sweep relies on."""
import numpy as np
import pytest
import torch

from oracle import s2s_oracle as O
from conftest import load_ckpt, load_npz
import _reparam as R

N_CHUNKS = 6


@pytest.fixture(scope="module", params=["k9", "k6"])
def base(request):
    """Six golden chunks of the checkpoint, the fp32 oracle's output on them (injected g, noise off) and the fp64 taps."""
    tag = request.param
    sd, cfg = load_ckpt(tag)
    g = load_npz(f"stages_{tag}.npz")
    codes, gi = g["codes"][:N_CHUNKS], torch.from_numpy(g["g"][:N_CHUNKS])
    ref = O.predict_chunks(sd, cfg, codes, O.PredictParams(noise_std=0.0), inject_g=gi)
    return dict(tag=tag, sd=sd, cfg=cfg, codes=codes, gi=gi, ref=ref, taps=R.intermediates(sd, cfg, codes, gi))


def test_variant_touches_the_pair_in_scope_only():
    sd, _ = load_ckpt("k9")
    for pair in R.PAIRS:
        for scope in R.SCOPES:
            v = R.variant(sd, pair, 3, scope)
            changed = sorted(k for k in sd if not torch.equal(sd[k], v[k]))
            up, down = R._scaled_keys(sd, pair, scope)
            assert changed == sorted(up + down) and all(k.startswith(R.PREFIX[scope]) for k in changed)
            assert all(torch.equal(v[k], sd[k] * 8.0) for k in up) and all(torch.equal(v[k], sd[k] / 8.0) for k in down)
            layers = 2 * (scope != "both") + 4 * (scope == "both")        # the synthetic checkpoints have 2 + 2 FFT blocks
            assert len(up) == 2 * layers and len(down) == (2 if pair == "qk" else 1) * layers
            back = R.variant(v, pair, -3, scope)
            assert all(torch.equal(back[k], sd[k]) for k in sd)           # a power of two: the rewrite itself is exact
    t = R.trained_like(sd)
    touched = [k for k in sd if not torch.equal(sd[k], t[k])]
    assert len(touched) == 4 * 12 and all(torch.equal(t[k], sd[k] * 0.25) for k in touched)
    assert not any("layer_norm" in k or not k.startswith(R.PREFIX["both"]) for k in touched)


@pytest.mark.parametrize("scope", R.SCOPES)
@pytest.mark.parametrize("pair", R.PAIRS)
def test_fp32_oracle_is_bit_invariant(base, pair, scope):
    """signal and dur of the fp32 oracle equal the e = 0 run's for every listed exponent: whatever a GPU mode changes under these
    rewrites is its own arithmetic."""
    for e in R.EXPONENTS:
        out = O.predict_chunks(R.variant(base["sd"], pair, e, scope), base["cfg"], base["codes"], O.PredictParams(noise_std=0.0),
                               inject_g=base["gi"])
        assert torch.equal(out["dur"], base["ref"]["dur"]), (pair, scope, e)
        assert torch.equal(out["signal"], base["ref"]["signal"]), (pair, scope, e)


def test_taps_name_every_block(base):
    names = ("slf_attn.q", "slf_attn.k", "slf_attn.v", "slf_attn.attn_out", "pos_ffn.hidden")
    want = {f"{p}{l}.{n}" for p in R.PREFIX["both"] for l in range(2) for n in names}
    assert set(base["taps"]) == want and all(0.0 < v < R.RANGE_LIMIT for v in base["taps"].values())
    out = O.predict_chunks(base["sd"], base["cfg"], base["codes"], O.PredictParams(noise_std=0.0), inject_g=base["gi"], taps={})
    assert torch.equal(out["signal"], base["ref"]["signal"])              # recording changes nothing


@pytest.mark.parametrize("scope", R.SCOPES)
@pytest.mark.parametrize("pair", R.PAIRS)
def test_range_condition(base, pair, scope):
    """The condition from an fp64 oracle run on each variant; the one-run form the GPU sweep uses gives the same number; and at
    least e = -10 ... +6 is admitted."""
    direct = {}
    for e in R.EXPONENTS:
        direct[e] = R.variant_magnitude(base["sd"], base["cfg"], base["codes"], base["gi"], pair, e, scope)
        assert direct[e] == R.scaled_magnitude(base["sd"], base["taps"], pair, e, scope), (pair, scope, e)
    ok = tuple(e for e in R.EXPONENTS if direct[e] < R.RANGE_LIMIT)
    assert ok == R.admitted(base["sd"], base["taps"], pair, scope)
    print(f"RANGE {base['tag']} {pair} {scope}: admitted {ok}; magnitude at e = 6 {direct[6]:.4g}, at 10 {direct[10]:.4g}, at -10 {direct[-10]:.4g}")
    assert set(R.ADMITTED_AT_LEAST) <= set(ok), (pair, scope, ok)
    assert ok == tuple(e for e in R.EXPONENTS if ok[0] <= e <= ok[-1])    # contiguous around 0


def test_recorded_band_is_inside_the_admitted_range(base):
    """The band the GPU test asserts over is contiguous around 0, holds +-1 at least, and lies where the condition admits."""
    for pair in R.PAIRS:
        for scope in R.SCOPES:
            lo, hi = R.BAND[(pair, scope)]
            assert lo <= -1 and hi >= 1 and lo in R.EXPONENTS and hi in R.EXPONENTS
            if base["tag"] == "k9":                                       # the checkpoint the band was measured with
                assert set(R.band(pair, scope)) <= set(R.admitted(base["sd"], base["taps"], pair, scope))
