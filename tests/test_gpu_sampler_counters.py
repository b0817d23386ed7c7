"""The samplers' counters against the layout include/s2s_hip.h states, from first principles (tests/_philox_ref.py): which Philox
counter every noise normal, dwell normal and Gamma draw of every compute mode and chunk geometry comes from -- chunk index split
into two words (batches that cross 2^32), position, kind, draw index -- rather than the laws of the draws, which
tests/test_gpu_samplers.py holds.  The normals are weight independent, so every element is pinned; the Gamma draws are restated in
float64 on the kernel's own conc / rate."""
import numpy as np
import pytest
import torch
from scipy import stats

import seq2squiggle_amd as S
import _geometry_models as GM
import _philox_ref as P
from conftest import load_ckpt
from test_gpu_events import CASES, engine as geometry_engine

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15                                     # bits in both words of the key
FIRSTS = [0, 2 ** 32 - 3, 123456789012]                       # the middle one: the batch crosses the carry into the high word
TUNED = ["tuned-f16x3", "tuned-f32", "tuned-f16"]
GEOMETRY = ["e16x250", "e1x1", "e5x37", "e64x1024", "e17x1023"]
B = 37
KS_ALPHA = 1e-3
_ENGINES, _RUNS = {}, {}


def eng_of(tag, biases=None):
    """"tuned-<mode>": the committed checkpoint on that tuned instance; otherwise the geometry engines of test_gpu_events.py.
    biases = (conc, rate): the same weights with the Gamma heads' output biases replaced."""
    key = (tag, biases)
    if key not in _ENGINES:
        if biases is None and not tag.startswith("tuned"):
            _ENGINES[key] = geometry_engine(tag)
        else:
            if tag.startswith("tuned"):
                sd, cfg = load_ckpt("k9")
                mode = tag[6:] or None
            else:
                sd, cfg, mode = GM.geometry_state_dict(tag, CASES), GM.geometry_config(tag, cases=CASES), None
            sd = dict(sd)
            if biases is not None:
                sd["length_regulator.duration_sampler.conc_layer.3.bias"] = torch.tensor([biases[0]])
                sd["length_regulator.duration_sampler.rate_layer.3.bias"] = torch.tensor([biases[1]])
            _ENGINES[key] = S.Engine(sd, cfg, mode=mode)
    return _ENGINES[key]


def chunks_of(eng, n, seed=0):
    """n full chunks of one random read -> (bases, n_valid) on the engine's device."""
    rng = np.random.default_rng(seed)
    read = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, eng.t_enc * n + eng.k - 1)].tobytes().decode()
    bases, nv, _ = S.encode_reads([read], eng.k, eng.t_enc)
    assert bases.shape[0] == n and (nv == eng.t_enc).all()
    return torch.from_numpy(bases).to(eng.device), torch.from_numpy(nv).to(eng.device)


def run(tag, first, dwell, n=B, biases=None):
    """One debug launch, once per session: dwell "gamma" (duration sampling, min_duration 0) or "normal" (dwell_mean 12.5,
    dwell_std 4, min_duration 3); noise_std 2 in both.  -> the debug arrays on the host."""
    key = (tag, first, dwell, n, biases)
    if key not in _RUNS:
        eng = eng_of(tag, biases)
        b, nv = chunks_of(eng, n)
        p = (S.PredictParams(noise_std=2.0, min_duration=0.0, seed=SEED) if dwell == "gamma" else
             S.PredictParams(noise_std=2.0, duration_sampling=False, dwell_mean=12.5, dwell_std=4.0, min_duration=3.0, seed=SEED))
        out = eng.predict_chunks(b, nv, p, first_global_chunk=first, debug=True)
        _RUNS[key] = {k_: out[k_].cpu().numpy() for k_ in ("z01", "g", "dur", "conc", "rate")}
    return _RUNS[key]


def chunk_ids(first, n):
    return (np.arange(n, dtype=np.uint64) + np.uint64(first))[:, None]


def test_reference_philox_equals_the_kernel():
    """1,000 random counters and keys: the numpy Philox (held to the Random123 vectors in tests/test_philox_ref_cpu.py) gives the
    words of Engine.philox_u32."""
    eng = eng_of("tuned-f16x3")
    rng = np.random.default_rng(5)
    c = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    seeds = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    got = torch.cat([eng.philox_u32(int(s), *(int(x) for x in ci), 1) for s, ci in zip(seeds, c)]).cpu().numpy().view(np.uint32)
    want = np.stack(P.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32)), -1)
    assert np.array_equal(got.astype(np.uint64), want)
    two = eng.philox_u32(7, 0xFFFFFFFF, 1, 2, 3, 2).cpu().numpy().view(np.uint32).astype(np.uint64)     # c0 + i wraps in its word
    assert np.array_equal(two, np.stack(P.philox4x32_10([0xFFFFFFFF, 0], 1, 2, 3, 7, 0), -1))


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("tag", TUNED + GEOMETRY)
def test_noise_normals_come_from_chunk_position_kind3(tag, first):
    """Every z01[b, t] is the normal of (first + b, t, kind 3, draw 0).  The bound of 1e-3 identifies the counter, it does not grade
    the hardware transcendentals (errors of the 1e-6 class, s2s_device.h): a draw from any other counter is an independent normal
    and lands within 1e-3 of the reference about 4e-4 of the time."""
    z = run(tag, first, "gamma")["z01"].astype(np.float64)
    ref = P.ref_normal(chunk_ids(first, B), np.arange(z.shape[1])[None, :], P.KIND_NOISE, SEED)
    assert z.shape == ref.shape and np.isfinite(z).all()
    dist = np.abs(z - ref).max()
    print(f"noise normals {tag} first {first}: max |z01 - reference| = {dist:.3e}")
    assert dist < 1e-3


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("tag", TUNED + GEOMETRY)
def test_dwell_normals_come_from_chunk_position_kind2(tag, first):
    """dwell_std > 0: g[b, c] = max(z * 4 + 12.5, min_duration) with z the normal of (first + b, c, kind 2, draw 0); 4e-3 is the
    noise test's bound times dwell_std."""
    out = run(tag, first, "normal")
    g = out["g"].astype(np.float64)
    z = P.ref_normal(chunk_ids(first, B), np.arange(g.shape[1])[None, :], P.KIND_DWELL, SEED)
    ref = np.maximum(z * 4.0 + 12.5, 3.0)
    dist = np.abs(g - ref).max()
    print(f"dwell normals {tag} first {first}: max |g - reference| = {dist:.3e}")
    assert g.shape == ref.shape and dist < 4e-3
    assert (ref > 3.0).mean() > 0.9 or g.size < 40
    assert np.array_equal(out["dur"], np.rint(out["g"]).astype(np.int32))


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("tag", GEOMETRY[1:])
def test_every_geometry_draws_the_normals_of_16x250(tag, first):
    """Same seed, same first chunk: bit for bit the normals of the generic instance at 16 / 250 on the positions both have."""
    a, b = run(tag, first, "gamma")["z01"], run("e16x250", first, "gamma")["z01"]
    n = min(a.shape[1], 250)
    assert np.array_equal(a[:, :n].view(np.uint32), b[:, :n].view(np.uint32))
    a, b = run(tag, first, "normal")["g"], run("e16x250", first, "normal")["g"]
    n = min(a.shape[1], 16)
    assert np.array_equal(a[:, :n].view(np.uint32), b[:, :n].view(np.uint32))


GAMMA_CHUNKS = {"tuned-f16x3": 1000, "e5x37": 16384, "e64x1024": 2000}
VARIANTS = {"seeded": None, "conc0.5": (-0.43, -6.0), "conc0.13": (-2.0, -9.0)}     # test_gamma_dwell_distribution's biases


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("tag", list(GAMMA_CHUNKS))
def test_gamma_draws_equal_the_float64_restatement(tag, variant):
    """The Gamma sampler restated in float64 on the same words (kind 1, the draw index counting the boost and every trip of the
    rejection loop) and fed the kernel's own conc / rate, then the clamps.  float32 against float64 can flip an accept / reject
    decision (tests/test_philox_ref_cpu.py: fewer than 1e-4 of the draws), hence a share: among the draws above the clamp at 1 at
    least 99.9 % agree within 1e-3 relative."""
    first = FIRSTS[1] - 100                                   # the carry falls inside the batch
    n = GAMMA_CHUNKS[tag] if variant == "seeded" else min(GAMMA_CHUNKS[tag], 4000)
    out = run(tag, first, "gamma", n, VARIANTS[variant])
    conc, rate, g = out["conc"], out["rate"], out["g"]
    te = g.shape[1]
    small = float((conc < 1).mean())
    assert variant == "seeded" or (conc < 1).sum() >= 1000, small            # the alpha < 1 boost runs
    s = P.ref_standard_gamma(conc, chunk_ids(first, n), np.arange(te)[None, :], SEED)
    ref = P.dwell_of_gamma(s, rate)
    share, counted = P.agreement(g, ref)
    print(f"gamma {tag} {variant}: {share:.6f} of {counted} draws above the clamp agree within 1e-3 (conc < 1: {small:.3f})")
    assert counted >= 2000 and share >= 0.999                # (2,000: the share then allows two draws)
    assert (g >= 1.0).all()
    assert np.array_equal(out["dur"], np.rint(g).astype(np.int32))
    if tag == "e64x1024":                                     # the probability-integral transform of test_gamma_dwell_distribution
        gd, a, sc = g.astype(np.float64).ravel(), conc.astype(np.float64).ravel(), 1.0 / rate.astype(np.float64).ravel()
        cens = gd <= 1.0
        u = np.where(cens, np.random.default_rng(3).random(gd.shape) * stats.gamma.cdf(1.0, a=a, scale=sc), stats.gamma.cdf(gd, a=a, scale=sc))
        ks = stats.kstest(u, "uniform")
        assert ks.pvalue > KS_ALPHA, ks


@pytest.mark.parametrize("tag", ["e64x1024", "e5x37"])
def test_no_correlation_between_neighbouring_positions_and_chunks(tag):
    """An indexing error that repeats or shifts draws between positions or chunks shows as lag-1 autocorrelation.  g is taken in
    the dwell_std > 0 mode, where it is a function of its own draw alone (the Gamma draws of neighbouring k-mers share letters and
    with them conc and rate).  A correct sampler's coefficient has a standard deviation of 1 / sqrt(pairs): 2,000 chunks put
    0.01 at 3.5 of them or more at 64 / 1024; at 5 / 37 a chunk holds four pairs of neighbouring dwells, so that geometry takes
    16,384 chunks (2.5 standard deviations for g along the positions, 7 for z01)."""
    n = GAMMA_CHUNKS[tag]
    first = FIRSTS[1] - 100
    for name, x in (("z01", run(tag, first, "gamma", n)["z01"]), ("g", run(tag, first, "normal", n)["g"])):
        x = x.astype(np.float64)
        along = np.corrcoef(x[:, :-1].ravel(), x[:, 1:].ravel())[0, 1]
        across = np.corrcoef(x[:-1].ravel(), x[1:].ravel())[0, 1]
        print(f"lag-1 autocorrelation {tag} {name}: positions {along:+.5f}, chunks {across:+.5f} ({x.size} draws)")
        assert abs(along) < 0.01 and abs(across) < 0.01, name
