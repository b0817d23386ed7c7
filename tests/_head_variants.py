"""Weights that move the three heads (noise_sampler.stdv_layer, duration_sampler.conc_layer / rate_layer: Linear(d, 1) + Softplus)
out of the slivers the committed and the seeded weights keep them in, shared by tests/test_head_variants_cpu.py (which proves from
the float64 oracle that the inputs populate the regimes) and tests/test_gpu_head_range.py (which holds the kernels on them).

A head's last layer is rescaled and shifted; the oracle is recomputed on the new weights, so nothing has to preserve the function.
With x the argument of the softplus, a regime spreads x over about 17 units around one boundary of the float32 code:
  clamp      [-30, -13]    crosses ln(1e-8) = -18.42, where clamp(min=1e-8) of conc / rate takes over (modules.py:215-218);
  unit       [-8.5, 8.5]   softplus on both sides of 1: Marsaglia-Tsang's alpha < 1 boost and the plain branch in one launch;
  threshold  [11.5, 28.5]  crosses nn.Softplus's threshold of 20;
  far        [96, 124]     the threshold regime 90 units up: past ln(FLT_MAX) = 88.72, where exp(x) is infinite in float32 and only the
                           branch above the threshold keeps the head finite (below it, log1p(exp(x)) differs from x by less than an
                           ulp, so nothing else can tell whether the branch is there).
SETTINGS holds (scale, bias) per weight set, head and regime, fitted once to the spread of x - bias over the chunks of `chunks()`
(float64 oracle) and rounded; COMBOS names the (conc, rate, sigma) combinations the tests run."""
import math

import numpy as np
import torch

from oracle import s2s_oracle as O

HEADS = {"sigma": "noise_sampler.stdv_layer", "conc": "length_regulator.duration_sampler.conc_layer",
         "rate": "length_regulator.duration_sampler.rate_layer"}
LN_CLAMP = math.log(1e-8)                                     # -18.42: softplus(x) ~ exp(x) falls below 1e-8 there
EDGE = 1e-3                                                   # |x - LN_CLAMP| below this: float32 may decide the clamp either way
REGIMES = ("clamp", "unit", "threshold", "far")
LN_FLT_MAX = math.log(float(np.finfo(np.float32).max))        # 88.72
# (conc, rate, sigma); None: the head as the weights have it.  D drives dwells past 1e9: conc above 11, rate down to the clamp.
COMBOS = {"A": ("unit", "unit", "unit"), "B": ("clamp", "clamp", "clamp"), "C": ("threshold", "threshold", "threshold"),
          "D": ("threshold", "clamp", None), "E": ("far", "far", "far")}
WEIGHTS = ("k9", "k6", "e5x37", "e64x1024")
# chunks per weight set: 300 on the tuned engines (both frontend_h16<1> and <2> run, with partial groups), otherwise enough for
# 4,000 dwell draws and more; the last PERIODIC chunks of every set come from reads of period 1 to 3 (one to three distinct k-mers
# per chunk, so that a whole chunk can sit on one side of a boundary)
N_CHUNKS = {"k9": 300, "k6": 300, "e5x37": 1000, "e64x1024": 80}


# weight set -> head -> regime -> (scale, bias) of <head>.3.  The scale is 17 / (the 1st to 99th percentile of x - bias); the biases put
# the median of x at -19.5 (clamp: above half of the k-mers clamped, the rest below -10), 0 (unit) and 20 (threshold).  Two departures,
# both so that the float64 restatement of the sampler alone meets what the GPU test asks of a combination (test_head_variants_cpu.py):
# the clamp regime of conc spreads over 12 units, not 17 (with conc up to 2.5e-3 one draw in 4,800 of B survived the boost
# (1 - u) ** (1 / alpha) and left the clamp at 1; with conc below 1e-4 none does), and the unit regime of rate sits one unit lower
# (A keeps 2,000 draws above the clamp at 1 with a margin).
def _head(scale, clamp, unit, threshold, clamp_scale=None):
    return {"clamp": (clamp_scale or scale, clamp), "unit": (scale, unit), "threshold": (scale, threshold), "far": (scale, threshold + 90.0)}


SETTINGS = {
    "k9": {"conc": _head(98.0, -12.8, 9.5, 29.5, 69.0), "rate": _head(350.0, -31.4, -12.9, 8.1), "sigma": _head(100.0, -2.1, 17.4, 37.4)},
    "k6": {"conc": _head(120.0, -12.0, 10.7, 30.7, 85.0), "rate": _head(300.0, -30.0, -11.5, 9.5), "sigma": _head(130.0, 1.0, 20.5, 40.5)},
    "e5x37": {"conc": _head(28.0, -33.1, -19.1, 0.9, 20.0), "rate": _head(88.0, -22.0, -3.5, 17.5), "sigma": _head(45.0, -1.8, 17.7, 37.7)},
    "e64x1024": {"conc": _head(21.0, -13.7, 8.1, 28.1, 15.0), "rate": _head(120.0, -28.7, -10.2, 10.8),
                 "sigma": _head(37.0, -13.9, 5.6, 25.6)},
}


def variant(sd: dict, head: str, scale: float, bias: float) -> dict:
    """A copy of the state dict with <head>.3.weight multiplied by `scale` and <head>.3.bias set to `bias` (head: a key of HEADS)."""
    p = HEADS[head]
    out = dict(sd)
    out[p + ".3.weight"] = sd[p + ".3.weight"].clone() * float(scale)
    out[p + ".3.bias"] = torch.full_like(sd[p + ".3.bias"], float(bias))
    return out


def combination(sd: dict, weights: str, combo: str) -> dict:
    """The weights of set `weights` with the heads in the regimes of COMBOS[combo]."""
    for head, regime in zip(("conc", "rate", "sigma"), COMBOS[combo]):
        if regime is not None:
            sd = variant(sd, head, *SETTINGS[weights][head][regime])
    return sd


def base_weights(weights: str):
    """-> (state dict, config) of a weight set: the two committed checkpoints, and the 5 / 37 and 64 / 1024 models of
    tests/test_gpu_events.py."""
    if weights in ("k9", "k6"):
        from conftest import load_ckpt
        sd, cfg = load_ckpt(weights)
        return {k: v.float() for k, v in sd.items()}, cfg
    import _geometry_models as GM
    from test_gpu_events import CASES
    return GM.geometry_state_dict(weights, CASES), GM.geometry_config(weights, cases=CASES)


_PERIODS = ("A", "C", "G", "T", "AC", "AG", "AT", "CG", "CT", "GT", "ACG", "ACT", "AGT", "CGT", "AAC", "GGT")


def chunks(weights: str, cfg: dict):
    """The chunks every test of a weight set runs on -> (bases uint8 [B, te + k - 1] letters, n_valid uint8 [B], codes uint8
    [B, te, k] for the oracle, kmers uint8 [B, te, k] letters for evaluate): one seeded random read cut into full chunks, then one
    chunk per entry of _PERIODS (a read of that period)."""
    import seq2squiggle_amd as S
    k, te = cfg["seq_kmer"], cfg["max_dna_len"]
    n = N_CHUNKS[weights] - len(_PERIODS)
    rng = np.random.default_rng(0)
    reads = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, te * n + k - 1)].tobytes().decode()]
    reads += [(p * (te + k))[:te + k - 1] for p in _PERIODS]
    bases, nv, _ = S.encode_reads(reads, k, te)
    codes = np.concatenate([O.encode_read(r, k, te) for r in reads], 0)
    assert bases.shape[0] == codes.shape[0] == N_CHUNKS[weights] and (nv == te).all()
    kmers = np.frombuffer(b"_ACGTN", np.uint8)[codes]
    return bases, nv, codes, np.ascontiguousarray(kmers)


def preactivations(sd: dict, cfg: dict, codes: np.ndarray, dtype=torch.float64) -> dict:
    """The oracle's heads in `dtype` -> {head: (x [B, te] the softplus's argument, value [B, te] the head's output, conc and rate
    after the clamp at 1e-8)}, float64 numpy arrays of the `dtype` results."""
    if dtype != torch.float32:
        sd = {k: v.to(dtype) for k, v in sd.items()}
    _, emb = O.encoder(sd, dict(cfg, encoder_layers=0), O.one_hot(codes, dtype))    # (emb_out alone: no layer runs)
    out = {}
    for head, p in HEADS.items():
        h = torch.relu(torch.nn.functional.linear(emb, sd[p + ".0.weight"], sd[p + ".0.bias"]))
        x = torch.nn.functional.linear(h, sd[p + ".3.weight"], sd[p + ".3.bias"]).flatten(1)
        v = torch.nn.functional.softplus(x)
        if head != "sigma":
            v = v.clamp(min=1e-8)
        out[head] = (x.double().numpy(), v.double().numpy())
    return out


SEED = 0x9E3779B97F4A7C15                                     # bits in both words of the Philox key
FIRST = 2 ** 32 - 103                                         # first_global_chunk: the carry into the high word falls inside the batch
LOSS_DWELLS = (0, 1, 2, 3, 12, 40, "ts", "ts+1", 32767)       # the measured dwells the duration loss is evaluated at

_REF = {}


def reference(weights: str, combo: str) -> dict:
    """Everything the oracle says about a weight set in a combination, once per process: sd, cfg, the arrays of chunks(), and the
    heads in float64 and float32 (`h64` / `h32`: preactivations())."""
    key = (weights, combo)
    if key not in _REF:
        sd, cfg = base_weights(weights)
        sd = combination(sd, weights, combo)
        bases, nv, codes, kmers = chunks(weights, cfg)
        _REF[key] = dict(sd=sd, cfg=cfg, bases=bases, n_valid=nv, codes=codes, kmers=kmers,
                         h64=preactivations(sd, cfg, codes, torch.float64), h32=preactivations(sd, cfg, codes, torch.float32))
    return _REF[key]


def regime_of(combo: str, head: str):
    return COMBOS[combo][("conc", "rate", "sigma").index(head)]


def chunk_ids(n: int):
    return (np.arange(n, dtype=np.uint64) + np.uint64(FIRST))[:, None]


def ref_dwell(conc, rate, dtype=np.float64):
    """The Gamma dwell of every k-mer of a batch that starts at FIRST under SEED, restated in `dtype` (tests/_philox_ref.py) on the
    given conc / rate [B, te], after the clamps at the smallest normal float32 and at 1 (min_duration 0)."""
    import _philox_ref as P
    conc = np.asarray(conc)
    s = P.ref_standard_gamma(conc.astype(dtype), chunk_ids(conc.shape[0]), np.arange(conc.shape[1])[None, :], SEED, dtype=dtype)
    return P.dwell_of_gamma(s, rate)


def agreement_all(got, ref, rel=1e-3) -> float:
    """_philox_ref.agreement's distance over ALL draws: the share within `rel` relative of the reference (two draws that both sit
    at the clamp at 1 are equal)."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float((np.abs(got - ref) <= rel * ref).mean())


def loss_dwells(n: int, te: int, ts: int) -> np.ndarray:
    """Measured dwells for the duration loss -> int32 [n, te] drawn from LOSS_DWELLS; row 0 all zero, row 1 all 32767."""
    values = np.array([ts if v == "ts" else ts + 1 if v == "ts+1" else v for v in LOSS_DWELLS], np.int32)
    d = values[np.random.default_rng(7).integers(0, len(values), (n, te))]
    d[0], d[1] = 0, 32767
    return d


def loss_sums64(conc, rate, dwell) -> np.ndarray:
    """sum over a chunk of -Gamma(conc, rate).log_prob(|d| + (d == 0)) in float64 with math.lgamma, as host_sums of
    tests/test_gpu_evaluate.py forms it -> [B]."""
    c, r, d = (np.asarray(v, np.float64) for v in (conc, rate, dwell))
    x = np.where(d == 0, 1.0, np.abs(d))
    return -(c * np.log(r) + (c - 1) * np.log(x) - r * x - np.vectorize(math.lgamma)(c)).sum(1)
