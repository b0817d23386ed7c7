"""The generic modes' envelope cases (tests/_envelope_models.py, tests/golden/envelope_*.npz) without a GPU: that the cases reach every
class of kernel code classes_of names, that its staging label follows the formula of s2s_generic.h, that the fixtures belong to the
weights the recipe writes, that the CPU oracle reproduces the reference's vectors at every case, and that the conditions the GPU
tests (tests/test_gpu_envelope.py) lean on hold for the reference alone."""
import os
import re

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import chunker
from seq2squiggle_amd import utils as U
from oracle import s2s_oracle as O
from conftest import GOLDEN, ROOT, load_npz
from _envelope_models import (CASES, GEN_ATTN_STAGE_BYTES, LABELS, TAGS, checkpoint_path, classes_of, envelope_config,
                              envelope_state_dict, gen_attn_lds_bytes, weights_sha256)

torch.set_float32_matmul_precision("highest")
TOL = 2e-6      # scaled units; two fp32 evaluation orders of the same aten ops (tests/test_oracle_golden.py)
Y_KEYS = ("y_gamma_nsamp", "y_gamma_nconst", "y_ideal", "y_normal_nsamp")
MODES = [
    ("y_gamma_nsamp", dict(), True, True, False),
    ("y_gamma_nconst", dict(noise_sampling=False), True, True, False),
    ("y_ideal", dict(noise_std=0.0, noise_sampling=False, duration_sampling=False), False, False, False),
    ("y_normal_nsamp", dict(duration_sampling=False, dwell_std=4.0), False, True, True),
]


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return O.PredictParams(**base)


def oracle_mode(sd, cfg, g, over, use_g, use_z, use_zdw, dtype=torch.float32):
    f = lambda key: torch.from_numpy(np.ascontiguousarray(g[key]).astype(np.float32))
    return O.predict_chunks(sd, cfg, g["codes"], P(**over), inject_g=f("g") if use_g else None, inject_z01=f("z01") if use_z else None,
                            inject_zdw=f("zdw") if use_zdw else None, dtype=dtype)


@pytest.fixture(scope="module", params=TAGS)
def ecase(request):
    tag = request.param
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    return tag, sd, cfg, load_npz(f"envelope_{tag}.npz")


def test_cases_reach_every_class():
    reached = {}
    for tag in TAGS:
        cfg = envelope_config(tag)
        c = classes_of(cfg)
        assert c <= LABELS, (tag, c - LABELS)
        for label in c:
            reached.setdefault(label, []).append(tag)
    assert set(reached) == LABELS, sorted(LABELS - set(reached))
    assert 12 <= len(TAGS) <= 16


def test_cases_are_inside_the_declared_envelope():
    for tag in TAGS:
        c = envelope_config(tag)
        d = c["dmodel"]
        assert d % 16 == 0 and 16 <= d <= 512 and c["dff"] % 8 == 0 and 8 <= c["dff"] <= 2048, tag
        for h in (c["encoder_heads"], c["decoder_heads"]):
            assert 1 <= h <= 16 and d % h == 0, tag
        assert 1 <= c["seq_kmer"] <= 16 and 1 <= c["max_dna_len"] <= 64 and 1 <= c["max_signal_len"] <= 1024, tag
        assert 0 <= c["pre_layers"] <= 4 and 1 <= c["encoder_layers"] <= 4 and 1 <= c["decoder_layers"] <= 4, tag


def test_staging_label_follows_the_kernel_header():
    """gen_attn_lds_bytes and GEN_ATTN_STAGE_BYTES as s2s_generic.h states them: the staged / unstaged label of every case is what the
    header's own formula and constant give, and the cases named for the switch sit next to it on both sides at 256 and 128 keys."""
    src = open(os.path.join(ROOT, "seq2squiggle_amd", "csrc", "s2s_generic.h")).read()
    m = re.search(r"#define GEN_ATTN_STAGE_BYTES \((\d+) \* 1024\)", src)
    limit = int(m.group(1)) * 1024
    assert limit == GEN_ATTN_STAGE_BYTES
    body = re.search(r"gen_attn_lds_bytes\(int T, int hd, bool stage\) \{\s*return (.*?);\s*\}", src, re.S).group(1)
    expr = body.replace("(size_t)", "").replace("sizeof(float)", "4").replace("?", "and").replace(": 0)", "or 0)")
    header = lambda T, hd, stage: eval(expr, {"T": T, "hd": hd, "stage": stage})
    for T in (1, 16, 64, 128, 250, 256):
        for hd in (1, 3, 36, 37, 38, 39, 40, 72, 76, 77, 80, 512):
            for stage in (True, False):
                assert header(T, hd, stage) == gen_attn_lds_bytes(T, hd, stage), (T, hd, stage)
    last = lambda T: max(h for h in range(1, 513) if header(T, h, True) <= limit)
    assert (last(250), last(256), last(128)) == (38, 37, 76)            # what the kernel's comment says for 250 keys
    for tag in TAGS:
        c = envelope_config(tag)
        labels = classes_of(c)
        want = set()
        for T, hd in ((c["max_dna_len"], c["dmodel"] // c["encoder_heads"]), (c["max_signal_len"], c["dmodel"] // c["decoder_heads"])):
            if T <= 256:
                want.add("attn:short_staged" if header(T, hd, True) <= limit else "attn:short_unstaged")
        assert {l for l in labels if l in ("attn:short_staged", "attn:short_unstaged")} == want, tag
    dec = lambda tag: (CASES[tag]["max_signal_len"], CASES[tag]["dmodel"] // CASES[tag]["decoder_heads"])
    for below, above in (("st36", "un40"), ("st72", "un80")):
        (Tb, hb), (Ta, ha) = dec(below), dec(above)
        assert Tb == Ta and hb <= last(Tb) < ha and ha - hb <= 8
        assert "attn_short:last_staged_hd-4..0" in classes_of(envelope_config(below))
        assert "attn_short:last_staged_hd+1..4" in classes_of(envelope_config(above))


def case_reads(tag):
    """The reads tools/make_envelope_goldens.py chunked for case `tag`."""
    cfg = envelope_config(tag)
    k, te = cfg["seq_kmer"], cfg["max_dna_len"]
    fasta = [(s, n) for s, n in U.read_fasta(os.path.join(GOLDEN, "example_test.fasta"))]
    g = load_npz(f"envelope_{tag}.npz")
    rng = np.random.default_rng(5)
    rand = list(rng.choice(list("ACGT"), k + te + te // 2))
    rand[len(rand) // 2] = "N"
    reads = [(fasta[0][0][:k], "len_k"), (fasta[1][0][:k + te - 1], "one_full_chunk"), (fasta[2][0][:k + te], "one_chunk_and_one"),
             ("".join(rand), "rand_with_N")]
    left = g["codes"].shape[0] - sum(chunker.n_chunks(len(s), k, te) for s, _ in reads)
    for seq, name in fasta[3:]:
        if left <= 0:
            break
        n = min(left, chunker.n_chunks(len(seq), k, te))
        reads.append((seq[:min(len(seq), k - 1 + n * te - te // 3)], name))
        left -= n
    return reads


def test_fixture_chunks_are_the_chunker_s(ecase):
    """The fixture's chunks are the package's own chunking of the case's reads; n_valid includes 1 and max_dna_len; <= 24 chunks."""
    tag, sd, cfg, g = ecase
    k, te = cfg["seq_kmer"], cfg["max_dna_len"]
    reads = case_reads(tag)
    bases, nv, first = chunker.encode_reads([s for s, _ in reads], k, te)
    assert bases.shape[0] == g["codes"].shape[0] <= 24 and g["codes"].shape[1:] == (te, k)
    assert np.array_equal(nv, g["n_valid"]) and {1, te} <= set(nv.tolist())
    assert [n for (s, n), a, b in zip(reads, first[:-1], first[1:]) for _ in range(b - a)] == [str(n) for n in g["names"]]
    ref_bases, ref_nv = chunker.codes_to_bases(g["codes"])
    assert np.array_equal(ref_nv, nv)
    for b in range(bases.shape[0]):
        n = int(nv[b]) + k - 1
        assert bytes(bases[b, :n]) == bytes(ref_bases[b, :n]), b
    assert (g["codes"] == 255).any()                                     # the N-bearing read
    assert np.array_equal(np.concatenate([O.encode_read(s, k, te) for s, _ in reads]), g["codes"])


def test_checkpoint_has_the_fixture_s_weights(ecase):
    tag, sd, cfg, g = ecase
    assert sd["encoders.position_enc"].shape == (1, cfg["max_dna_len"], cfg["dmodel"])
    assert sd["decoders.position_enc"].shape == (1, cfg["max_signal_len"], cfg["dmodel"])
    assert weights_sha256(sd, cfg) == weights_sha256(envelope_state_dict(tag), cfg) == str(g["weights_sha256"])
    assert str(load_npz("envelope_mixed16.npz")[f"weights_sha256_{tag}"]) == str(g["weights_sha256"])
    for key in Y_KEYS:
        assert g[key].shape == (g["codes"].shape[0], cfg["max_signal_len"])


def test_oracle_stages(ecase):
    tag, sd, cfg, g = ecase
    enc_out, emb_out = O.encoder(sd, cfg, O.one_hot(g["codes"]))
    assert np.abs(emb_out.numpy() - g["emb_out"]).max() < TOL
    assert np.abs(enc_out.numpy() - g["enc_out"]).max() < 5 * TOL
    assert np.abs(O.noise_sampler(sd, emb_out).numpy() - g["sigma"]).max() < TOL
    conc, rate = O.duration_params(sd, emb_out)
    assert np.allclose(conc.numpy(), g["conc"], rtol=1e-6, atol=1e-6)
    assert np.allclose(rate.numpy(), g["rate"], rtol=1e-6, atol=1e-6)
    gs = O.standard_gamma_to_sample(torch.from_numpy(g["sg"]), torch.from_numpy(g["rate"])).clamp(min=1.0)
    assert np.array_equal(gs.numpy(), g["g"])
    dur = O.durations(P(), g["codes"].shape[0], torch.from_numpy(g["g"]))
    h, _ = O.length_regulate(torch.from_numpy(g["enc_out"]), torch.from_numpy(g["sigma"]), dur, cfg["max_signal_len"])
    assert np.abs(O.decoder(sd, cfg, h).numpy() - g["y_scaled_gamma"]).max() < 10 * TOL


@pytest.mark.parametrize("key,over,use_g,use_z,use_zdw", MODES)
def test_oracle_reproduces_the_reference(ecase, key, over, use_g, use_z, use_zdw):
    """tests/test_oracle_golden.py's bounds at every envelope case: zero pattern exact, MAE < 1e-4 pA, max < 2e-3 pA, and both dwell
    arrays bit-exact -- the ideal and Normal dwell of the oracle at the case's max_dna_len."""
    tag, sd, cfg, g = ecase
    out = oracle_mode(sd, cfg, g, over, use_g, use_z, use_zdw)
    y, ref = out["signal"].numpy(), g[key]
    assert y.shape == ref.shape and out["dur"].shape == (g["codes"].shape[0], cfg["max_dna_len"])
    assert np.array_equal(y == 0, ref == 0), "zero pattern (ReLU / pad / clamp) must match exactly"
    assert np.abs(y - ref).mean() < 1e-4 and np.abs(y - ref).max() < 2e-3      # pA
    if use_g:
        assert np.array_equal(out["dur"].numpy(), g["dur_gamma"])
    elif use_zdw:
        assert np.array_equal(out["dur"].numpy(), g["dur_normal"])
    else:
        assert (out["dur"].numpy() == 12).all()                                # 12.5 -> 12 half-to-even


def test_conditions_the_gpu_tests_lean_on(ecase):
    """For the reference arithmetic alone: the fp32 and the fp64 oracle agree in zero pattern and dwell indices in every mode (so
    an exact zero-pattern assertion on the GPU is not a coin toss at a ReLU edge), at least a quarter of the reference's samples are
    non-zero (so it is not vacuous), and the injected Gamma draws end chunks before max_signal_len and crop others."""
    tag, sd, cfg, g = ecase
    ts = cfg["max_signal_len"]
    for key, over, use_g, use_z, use_zdw in MODES:
        o32 = oracle_mode(sd, cfg, g, over, use_g, use_z, use_zdw)
        o64 = oracle_mode(sd, cfg, g, over, use_g, use_z, use_zdw, dtype=torch.float64)
        assert torch.equal(o32["signal"] == 0, o64["signal"] == 0), (tag, key)
        assert torch.equal(o32["dur"], o64["dur"]), (tag, key)
        assert (g[key] != 0).mean() >= 0.25, (tag, key, (g[key] != 0).mean())
    sums = g["dur_gamma"].sum(1)
    assert (sums > ts).any()
    if cfg["max_dna_len"] * 3 < ts:                                           # (min_duration 3 per k-mer: below that every chunk is cropped)
        assert (sums < ts).any()
    # the 16-mixed reference vectors: the stored distances are those of the stored vectors
    m16 = load_npz("envelope_mixed16.npz")
    y16, d16 = m16[f"y_gamma_nsamp_16mixed_{tag}"], m16[f"dur_gamma_16mixed_{tag}"]
    agree = (d16 == g["dur_gamma"]).all(1)
    assert agree.sum() >= len(agree) // 2
    d = np.abs(y16 - g["y_gamma_nsamp"])[agree]
    assert abs(d.mean() - float(m16[f"mae_vs_fp32_where_dwell_equal_{tag}"])) < 1e-6
    assert abs(d.max() - float(m16[f"max_vs_fp32_where_dwell_equal_{tag}"])) < 1e-4


def test_fixtures_stay_small():
    files = [f for f in os.listdir(GOLDEN) if f.startswith("envelope_")]
    assert sorted(files) == sorted([f"envelope_{t}.npz" for t in TAGS] + ["envelope_mixed16.npz"])
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in files) < 2_000_000
