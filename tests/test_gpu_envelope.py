"""The generic instances across their size and geometry envelope, on the GPU (the cases of tests/_envelope_models.py: every head_dim,
key-count, tile-remainder and LDS-size class the kernels of s2s_generic.h / s2s_generic_h.h pick their code by).

fp32 ("generic-geometry", and "generic" at 16 / 250) against the imported reference's vectors (tests/golden/envelope_<tag>.npz) with
the project's bounds -- dwell indices bit-exact, zero pattern exact, MAE < 1e-4 pA, max < 2e-3 pA, stages within
tests/test_gpu_geometry.py's STAGE_TOL -- and no further from the fp64 oracle than 5 x the fp32 oracle is (tests/test_gpu_parity.py's
rule).  The stand-alone Decoder operator on dense signed rows against the oracle's.  The f16 modes against the reference's own
16-mixed distance at the same case (tests/golden/envelope_mixed16.npz), no margin.  Batch shapes (one chunk, B * T off the 64-row
tile, one workspace slice + 13 chunks, the packed entry point) as bit-equalities, with the chunks on either side of the slice
boundary held to the oracle.  Each test prints its measured distances (ENVELOPE ...) before it asserts."""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import chunker
from oracle import s2s_oracle as O
from conftest import load_npz
from _envelope_models import TAGS, checkpoint_path
from test_gpu_geometry import MAE_TOL, MAX_TOL, STAGE_TOL

pytestmark = pytest.mark.gpu
torch.set_float32_matmul_precision("highest")
F16_STAGES = ("emb_out", "enc_out", "sigma", "conc", "rate", "g", "dur")
MODES = [
    ("y_gamma_nsamp", dict(), True, True, False),
    ("y_gamma_nconst", dict(noise_sampling=False), True, True, False),
    ("y_ideal", dict(noise_std=0.0, noise_sampling=False, duration_sampling=False), False, False, False),
    ("y_normal_nsamp", dict(duration_sampling=False, dwell_std=4.0), False, True, True),
]
BATCH_TAGS = ["hd1", "hd40", "hd208"]          # head_dim 1 at 1 / 1, a long <8> and a long <32> decoder


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return base


def fp32_modes(cfg):
    at_default = (cfg["max_dna_len"], cfg["max_signal_len"]) == (16, 250)
    return ["generic-geometry"] + (["generic"] if at_default else [])


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))


@pytest.fixture(scope="module", params=TAGS)
def ecase(request):
    tag = request.param
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    g = load_npz(f"envelope_{tag}.npz")
    bases, nv = chunker.codes_to_bases(g["codes"])
    assert np.array_equal(nv, g["n_valid"])
    return dict(tag=tag, sd=sd, cfg=cfg, g=g, bases=torch.from_numpy(bases).cuda(), nv=torch.from_numpy(nv).cuda())


def run(case, mode, fn):
    eng = S.Engine(case["sd"], case["cfg"], mode=mode)
    assert eng.mode == mode and (eng.t_enc, eng.t_dec) == (case["cfg"]["max_dna_len"], case["cfg"]["max_signal_len"])
    out = fn(eng)
    torch.cuda.synchronize()
    eng.close()
    return out


def predict(case, eng, over, use_g=True, use_z=True, use_zdw=False, debug=False):
    g = case["g"]
    return eng.predict_chunks(case["bases"], case["nv"], S.PredictParams(**P(**over)), debug=debug,
                              inject_g=f32(g["g"]).cuda() if use_g else None, inject_z01=f32(g["z01"]).cuda() if use_z else None,
                              inject_zdw=f32(g["zdw"]).cuda() if use_zdw else None)


def oracle(case, over, use_g, use_z, use_zdw, dtype):
    g = case["g"]
    return O.predict_chunks(case["sd"], case["cfg"], g["codes"], O.PredictParams(**P(**over)), inject_g=f32(g["g"]) if use_g else None,
                            inject_z01=f32(g["z01"]) if use_z else None, inject_zdw=f32(g["zdw"]) if use_zdw else None, dtype=dtype)


def test_fp32_stage_outputs(ecase):
    g, t = ecase["g"], STAGE_TOL
    for mode in fp32_modes(ecase["cfg"]):
        out = run(ecase, mode, lambda e: predict(ecase, e, dict(noise_std=0.0), use_z=False, debug=True))
        o = {k: v.cpu().numpy() for k, v in out.items()}
        err = {k: float(np.abs(o[k] - g[r]).max()) for k, r in (("emb_out", "emb_out"), ("enc_out", "enc_out"), ("sigma", "sigma"),
                                                                 ("y_scaled", "y_scaled_gamma"))}
        print(f"ENVELOPE stages {ecase['tag']} {mode}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert o["emb_out"].shape == g["emb_out"].shape and o["y_scaled"].shape == g["y_scaled_gamma"].shape
        assert err["emb_out"] < t["emb"], (mode, err)
        assert err["enc_out"] < t["enc"], (mode, err)
        assert err["sigma"] < t["sig"], (mode, err)
        assert np.allclose(o["conc"], g["conc"], rtol=t["rel"], atol=t["rel"])
        assert np.allclose(o["rate"], g["rate"], rtol=t["rel"], atol=t["rel"])
        assert np.array_equal(o["dur"], g["dur_gamma"])
        assert err["y_scaled"] < t["y"], (mode, err)


@pytest.mark.parametrize("key,over,use_g,use_z,use_zdw", MODES)
def test_fp32_predict_modes(ecase, key, over, use_g, use_z, use_zdw):
    g, ref = ecase["g"], ecase["g"][key]
    o32 = oracle(ecase, over, use_g, use_z, use_zdw, torch.float32)["signal"].numpy()
    o64 = oracle(ecase, over, use_g, use_z, use_zdw, torch.float64)["signal"].numpy()
    agree64 = (o32 == 0) == (o64 == 0)
    err_ref = np.abs(o32 - o64)[agree64].mean()
    for mode in fp32_modes(ecase["cfg"]):
        out = run(ecase, mode, lambda e: predict(ecase, e, over, use_g, use_z, use_zdw))
        y, dur = out["signal"].cpu().numpy(), out["dur"].cpu().numpy()
        assert y.shape == ref.shape
        d = np.abs(y - ref)
        same = (y == 0) == (ref == 0)
        err_gpu = np.abs(y - o64)[same & agree64].mean()
        print(f"ENVELOPE fp32 {ecase['tag']} {mode} {key}: MAE {d.mean():.2e} max {d.max():.2e} pA | to fp64: mode {err_gpu:.2e} "
              f"fp32 oracle {err_ref:.2e} | zero-pattern flips {int((~same).sum())} of {same.size}")
        assert np.array_equal(dur, g["dur_gamma"] if use_g else g["dur_normal"] if use_zdw else np.full_like(dur, 12)), mode
        assert same.all(), (mode, int((~same).sum()))
        assert d.mean() < MAE_TOL and d.max() < MAX_TOL, (mode, d.mean(), d.max())
        assert err_gpu <= 5 * err_ref, (mode, err_gpu, err_ref)


def test_decoder_operator_on_dense_rows(ecase):
    """modules.py's stand-alone Decoder on rows no length regulator produced (dense, signed), against the oracle's Decoder.forward:
    the zero pattern equal and max < 6e-5 scaled units (tests/test_gpu_geometry.py's operator bound), and the mean distance to the
    fp64 oracle within 5 x the fp32 oracle's own."""
    from seq2squiggle_amd.modules import Stages
    sd, cfg = ecase["sd"], ecase["cfg"]
    ts, d = cfg["max_signal_len"], cfg["dmodel"]
    h = torch.randn(5, ts, d, generator=torch.Generator().manual_seed(11)) * 0.7
    r32 = O.decoder(sd, cfg, h).numpy()
    r64 = O.decoder({k: v.double() for k, v in sd.items()}, cfg, h.double()).numpy()
    agree64 = (r32 == 0) == (r64 == 0)
    err_ref = np.abs(r32 - r64)[agree64].mean()
    for mode in fp32_modes(cfg):
        y = run(ecase, mode, lambda e: Stages(e, S.PredictParams(**P(noise_std=0.0))).decoder(h.to(e.device))[..., 0].cpu().numpy())
        same = (y == 0) == (r32 == 0)
        err_gpu = np.abs(y - r64)[same & agree64].mean()
        print(f"ENVELOPE decoder-operator {ecase['tag']} {mode}: max {np.abs(y - r32).max():.2e} | to fp64: mode {err_gpu:.2e} "
              f"fp32 oracle {err_ref:.2e} | non-zero share {(r32 != 0).mean():.2f}")
        assert y.shape == (5, ts) and (r32 != 0).mean() > 0.25
        assert same.all() and np.abs(y - r32).max() < 6e-5, (mode, int((~same).sum()), np.abs(y - r32).max())
        assert err_gpu <= 5 * err_ref, (mode, err_gpu, err_ref)


def ref16_bar(tag, g):
    """The reference 16-mixed's MAE / max against the fp32 fixture on the chunks where its dwell indices agree with fp32's."""
    m16 = load_npz("envelope_mixed16.npz")
    agree = (m16[f"dur_gamma_16mixed_{tag}"] == g["dur_gamma"]).all(1)
    d = np.abs(m16[f"y_gamma_nsamp_16mixed_{tag}"] - g["y_gamma_nsamp"])[agree]
    assert abs(d.mean() - float(m16[f"mae_vs_fp32_where_dwell_equal_{tag}"])) < 1e-6
    return agree, d.mean(), d.max()


def test_f16_against_fp32_and_reference_16_mixed(ecase):
    tag, cfg, g = ecase["tag"], ecase["cfg"], ecase["g"]
    agree, ref_mae, ref_max = ref16_bar(tag, g)
    for mode32 in fp32_modes(cfg):
        mode = mode32 + "-f16"
        out = {m: run(ecase, m, lambda e: predict(ecase, e, dict(), debug=True)) for m in (mode32, mode)}
        a = out[mode]
        y, t = a["signal"].cpu().numpy(), g["y_gamma_nsamp"]
        same = (y == 0) == (t == 0)
        keep = same & agree[:, None]
        d = np.abs(y - t)[keep]
        print(f"ENVELOPE f16 {tag} {mode}: mode MAE {d.mean():.4f} max {d.max():.3f} | reference 16-mixed MAE {ref_mae:.4f} "
              f"max {ref_max:.3f} | zero pattern equal {same.mean():.5f} | chunks compared {int(agree.sum())} of {len(agree)}")
        for key in F16_STAGES:                                   # the encoder side is the fp32 instance's own code
            assert torch.equal(a[key], out[mode32][key]), (mode, key)
        assert np.array_equal(a["dur"].cpu().numpy(), g["dur_gamma"])
        assert y.shape == t.shape and np.isfinite(y).all()
        assert same.mean() > 0.999, (mode, same.mean())
        assert d.mean() <= ref_mae and d.max() <= ref_max, (mode, d.mean(), d.max(), ref_mae, ref_max)


def _random_chunks(k, te, B, seed):
    """B chunks of random bases, every 7th one short -> (bases uint8 [B, te + k - 1], n_valid uint8 [B], codes uint8 [B, te, k])."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    bases = letters[rng.integers(0, 4, size=(B, te + k - 1))]
    nv = np.full(B, te, np.uint8)
    nv[::7] = rng.integers(1, te + 1, size=len(nv[::7]))
    return bases, nv


def _codes(bases, nv, k, te):
    lut = np.zeros(256, np.uint8)
    for i, ch in enumerate(b"_ACGT"):
        lut[ch] = i
    codes = lut[bases][:, np.arange(te)[:, None] + np.arange(k)[None, :]]
    codes[np.arange(te)[None, :] >= nv[:, None]] = 0
    return codes


@pytest.mark.parametrize("mode", ["generic-geometry", "generic-geometry-f16"])
@pytest.mark.parametrize("tag", BATCH_TAGS)
def test_batch_shapes_are_bit_equal(tag, mode):
    """One chunk, three chunks (B * T off the 64-row tile) and the fixture's batch give the same rows; a launch of one workspace slice
    + 13 chunks equals itself and the same chunks in two launches; the packed entry point equals the plain one.  fp32: the chunks on
    either side of the slice boundary are also held to the oracle (two equal GPU runs could both be wrong)."""
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    g = load_npz(f"envelope_{tag}.npz")
    k, te, ts, d, f = (cfg[n] for n in ("seq_kmer", "max_dna_len", "max_signal_len", "dmodel", "dff"))
    eng = S.Engine(sd, cfg, mode=mode)
    dev = eng.device
    bases, nv = chunker.codes_to_bases(g["codes"])
    b_d, n_d, gi, z = torch.from_numpy(bases).to(dev), torch.from_numpy(nv).to(dev), f32(g["g"]).to(dev), f32(g["z01"]).to(dev)
    p = S.PredictParams(**P())
    full = eng.predict_chunks(b_d, n_d, p, inject_g=gi, inject_z01=z)
    assert (full["signal"] > 0).any()
    for B in (1, 3):
        assert B == 1 or (B * ts) % 64 and (B * te) % 64
        part = eng.predict_chunks(b_d[:B].contiguous(), n_d[:B].contiguous(), p, inject_g=gi[:B].contiguous(), inject_z01=z[:B].contiguous())
        assert torch.equal(part["signal"], full["signal"][:B]) and torch.equal(part["dur"], full["dur"][:B]), B
    # one workspace slice + 13 chunks
    slice_chunks = (512 << 20) // (4 * (te * d + te + ts * d + ts + max(te, ts) * max(3 * d, f)))
    # (include/s2s_hip.h: and few enough chunks that an attention launch, one workgroup per chunk and head, stays below 2^32 threads)
    slice_chunks = min(slice_chunks, (2 ** 32 - 1) // (max(cfg["encoder_heads"], cfg["decoder_heads"]) * max(1024, 256 * -(-ts // 64))))
    n = slice_chunks + 13
    hb, hnv = _random_chunks(k, te, n, 3)
    wb, wnv = torch.from_numpy(hb).to(dev), torch.from_numpy(hnv).to(dev)
    ps = S.PredictParams(seed=9)
    whole = eng.predict_chunks(wb, wnv, ps, first_global_chunk=100)
    again = eng.predict_chunks(wb, wnv, ps, first_global_chunk=100)
    m = n // 2
    a = eng.predict_chunks(wb[:m].contiguous(), wnv[:m].contiguous(), ps, first_global_chunk=100)
    b = eng.predict_chunks(wb[m:].contiguous(), wnv[m:].contiguous(), ps, first_global_chunk=100 + m)
    torch.cuda.synchronize()
    assert whole["signal"].shape == (n, ts) and whole["dur"].shape == (n, te)
    for key in ("signal", "dur"):
        assert torch.equal(whole[key], again[key]), key
        assert torch.equal(whole[key], torch.cat([a[key], b[key]])), key
    assert (whole["signal"] > 0).any() and torch.isfinite(whole["signal"]).all()
    del again, a, b
    # the chunks on either side of the slice boundary against the oracle, with injected variates
    lo, hi = slice_chunks - 6, n
    gen = torch.Generator().manual_seed(17)
    gw = torch.rand(n, te, generator=gen) * (2.2 * ts / te + 2)
    zw = torch.randn(n, ts, generator=gen)
    inj = eng.predict_chunks(wb, wnv, p, inject_g=gw.to(dev), inject_z01=zw.to(dev))
    edge = eng.predict_chunks(wb[lo:hi].contiguous(), wnv[lo:hi].contiguous(), p, inject_g=gw[lo:hi].to(dev), inject_z01=zw[lo:hi].to(dev))
    assert torch.equal(inj["signal"][lo:hi], edge["signal"]) and torch.equal(inj["dur"][lo:hi], edge["dur"])
    ref = O.predict_chunks(sd, cfg, _codes(hb[lo:hi], hnv[lo:hi], k, te), O.PredictParams(**P()), inject_g=gw[lo:hi], inject_z01=zw[lo:hi])
    y, r = inj["signal"][lo:hi].cpu().numpy(), ref["signal"].numpy()
    assert np.array_equal(inj["dur"][lo:hi].cpu().numpy(), ref["dur"].numpy())
    same = (y == 0) == (r == 0)
    dd = np.abs(y - r)[same]
    print(f"ENVELOPE slice-boundary {tag} {mode}: slice {slice_chunks} chunks, chunks {lo}..{hi - 1} to the fp32 oracle: MAE {dd.mean():.2e} "
          f"max {dd.max():.2e} pA, zero pattern equal {same.mean():.5f}")
    if mode == "generic-geometry":
        assert same.mean() > 0.9995 and dd.mean() < MAE_TOL and dd.max() < MAX_TOL, (same.mean(), dd.mean(), dd.max())
        if not same.all():                                      # a sample that is zero on one side only is within the bound of zero on the other
            assert np.abs(y - r)[~same].max() < MAX_TOL
    else:                                                       # the f16 decoder: the reference's 16-mixed MAE at this case's weights
        ref_mae = float(load_npz("envelope_mixed16.npz")[f"mae_vs_fp32_where_dwell_equal_{tag}"])
        assert same.mean() > 0.999 and dd.mean() <= ref_mae, (same.mean(), dd.mean(), ref_mae)
    # packed against plain
    rng = np.random.default_rng(4)
    reads = ["".join(rng.choice(list("ACGT"), L)) for L in (k, k + te - 1, k + te, 40 * te + k + 3, 7 * te + k)]
    rb, cs, pnv, _ = chunker.pack_reads(reads, k, te)
    ub, unv, _ = S.encode_reads(reads, k, te)
    packed = eng.predict_packed(torch.from_numpy(rb).to(dev), torch.from_numpy(cs).to(dev), torch.from_numpy(pnv).to(dev), ps)
    plain = eng.predict_chunks(torch.from_numpy(ub).to(dev), torch.from_numpy(unv).to(dev), ps)
    torch.cuda.synchronize()
    assert torch.equal(packed["signal"], plain["signal"]) and torch.equal(packed["dur"], plain["dur"])
    eng.close()
