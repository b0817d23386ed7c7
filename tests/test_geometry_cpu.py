"""Chunk geometries other than max_dna_len 16 / max_signal_len 250 (S2S_MODE_GENERIC_GEOMETRY): the C ABI's limits and blob
size, the Python mode selection, the chunker against the reference's split_sequence at each max_dna_len, the fixtures' weights,
and the new attention kernel's register budget.  No GPU needed."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _build, _lib, chunker
from seq2squiggle_amd import utils as U
from seq2squiggle_amd.checkpoint import MODES, config_to_c, default_mode, is_default_geometry
from conftest import GOLDEN, ROOT, load_npz
from _geometry_models import CASES, checkpoint_path, geometry_config, geometry_state_dict, weights_sha256

GEOMETRY = 6
TAGS = list(CASES)


def blob_floats(c):
    return _lib.lib().s2s_blob_floats(ctypes.byref(c))


def err_of(c):
    h = ctypes.c_void_p()
    rc = _lib.lib().s2s_create(ctypes.byref(c), None, 0, 0, ctypes.byref(h))
    return rc, _lib.lib().s2s_last_error(None).decode()


def case_reads(tag):
    """The reads tools/make_geometry_goldens.py chunked for case `tag`."""
    reads = [(s, n) for s, n in U.read_fasta(os.path.join(GOLDEN, "example_test.fasta"))]
    rng = np.random.default_rng(5)
    rand = ("".join(rng.choice(list("ACGTN"), 150, p=[.24, .24, .24, .24, .04])), "rand150_with_N")
    if tag == "d512x288":
        return [(reads[0][0][:20], reads[0][1]), (rand[0][:30], rand[1])]
    n = {"r16x500": 1, "g12x300": 2, "g5x37": 7, "g64x1024": 2}[tag]
    return reads[:n] + [rand]


def test_mode_constant_and_selection():
    hdr = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()
    assert "#define S2S_MODE_GENERIC_GEOMETRY 6" in hdr and MODES["generic-geometry"] == GEOMETRY
    assert "#define S2S_GEOMETRY_MAX_DNA_LEN 64" in hdr and "#define S2S_GEOMETRY_MAX_SIGNAL_LEN 1024" in hdr
    base = geometry_config("r16x500")
    assert default_mode(base) == "generic-geometry"                        # the tuned sizes at another geometry
    assert default_mode(dict(base, max_signal_len=250)) == "f16x3"
    assert default_mode(dict(base, max_signal_len=250, dmodel=128)) == "generic"
    assert default_mode(dict(base, max_dna_len=12, max_signal_len=250)) == "generic-geometry"
    for tag in TAGS:
        assert not is_default_geometry(geometry_config(tag)) and default_mode(geometry_config(tag)) == "generic-geometry"
    assert config_to_c(base, "generic-geometry").compute_mode == GEOMETRY


@pytest.mark.parametrize("tag", TAGS)
def test_blob_size_matches_state_dict(tag):
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    c = config_to_c(cfg, "generic-geometry")
    n = blob_floats(c)
    assert n == sum(v.numel() for v in sd.values()) > 0
    assert S.state_dict_to_blob(sd, cfg).size == n
    for mode in ("f32", "f16x3", "f16", "generic", "generic-f16"):       # every other mode refuses the geometry
        assert blob_floats(config_to_c(cfg, mode)) == 0


@pytest.mark.parametrize("te,ts", [(1, 1), (64, 1024), (1, 1024), (64, 1), (16, 250)])
def test_blob_size_at_the_edges(te, ts):
    cfg = geometry_config("g12x300")
    c = config_to_c(dict(cfg, max_dna_len=te, max_signal_len=ts), "generic-geometry")
    d = cfg["dmodel"]
    at_default = config_to_c(dict(cfg, max_dna_len=16, max_signal_len=250), "generic")
    assert blob_floats(c) == blob_floats(at_default) + (te - 16) * d + (ts - 250) * d


@pytest.mark.parametrize("key,value", [("max_dna_len", 0), ("max_dna_len", 65), ("max_signal_len", 0), ("max_signal_len", 1025),
                                       ("dmodel", 72), ("dff", 4), ("decoder_heads", 5)])
def test_limits_name_their_key(key, value):
    _, cfg = S.load_checkpoint(checkpoint_path("g12x300"))
    c = config_to_c(cfg, "generic-geometry")
    setattr(c, key, value)
    assert blob_floats(c) == 0
    rc, msg = err_of(c)
    assert rc == -1 and key in msg, msg
    if key.startswith("max_"):
        assert "S2S_MODE_GENERIC_GEOMETRY" in msg, msg


@pytest.mark.parametrize("mode,word", [("f32", "max_signal_len must be 250"), ("f16x3", "max_signal_len must be 250"),
                                       ("f16", "max_signal_len must be 250"), ("generic", "max_signal_len must be 250"),
                                       ("generic-f16", "max_signal_len must be 250")])
def test_other_modes_keep_their_geometry_messages(mode, word):
    cfg = dict(geometry_config("r16x500"))
    c = config_to_c(cfg, mode)
    rc, msg = err_of(c)
    assert rc == -1 and msg == word, msg
    c.max_dna_len = 12
    rc, msg = err_of(c)
    assert rc == -1 and msg == "max_dna_len must be 16", msg


def test_engine_refuses_other_modes_at_another_geometry_and_names_generic_geometry(monkeypatch):
    sd, cfg = S.load_checkpoint(checkpoint_path("r16x500"))
    for mode in ("generic", "generic-f16", "f32", "f16x3", "f16"):
        with pytest.raises(ValueError) as e:
            S.Engine(sd, cfg, mode=mode)
        assert "generic-geometry" in str(e.value) and "max_signal_len 500" in str(e.value), str(e.value)
    # the mode checks come before the device: without a GPU the default and the explicit mode get as far as asking for one
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for mode in (None, "generic-geometry"):
        with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
            S.Engine(sd, cfg, mode=mode)


@pytest.mark.parametrize("tag", TAGS)
def test_chunker_matches_reference_split_sequence(tag):
    g = load_npz(f"geometry_{tag}.npz")
    cfg = geometry_config(tag)
    k, te = cfg["seq_kmer"], cfg["max_dna_len"]
    reads = case_reads(tag)
    bases, nv, first = chunker.encode_reads([s for s, _ in reads], k, te)
    assert bases.shape == (g["codes"].shape[0], te + k - 1) and g["codes"].shape[1] == te
    assert np.array_equal(nv, g["n_valid"])
    names = [n for (s, n), a, b in zip(reads, first[:-1], first[1:]) for _ in range(b - a)]
    assert names == [str(n) for n in g["names"]]
    ref_bases, ref_nv = chunker.codes_to_bases(g["codes"])
    assert np.array_equal(ref_nv, nv)
    for b in range(bases.shape[0]):
        n = int(nv[b]) + k - 1
        assert bytes(bases[b, :n]) == bytes(ref_bases[b, :n]), b
    # the packed form addresses the same windows, and counts the same chunks
    flat, cs, pnv, pfirst = chunker.pack_reads([s for s, _ in reads], k, te)
    assert np.array_equal(pfirst, first) and np.array_equal(pnv, nv)
    for b in range(bases.shape[0]):
        assert np.array_equal(flat[cs[b]: cs[b] + te + k - 1], bases[b])
    assert [chunker.n_chunks(len(s), k, te) for s, _ in reads] == list(np.diff(first))
    assert S.parallel.shard_reads([len(s) for s, _ in reads], k, 1, te) == [(0, len(reads), 0)]


@pytest.mark.parametrize("tag", TAGS)
def test_geometry_checkpoints_are_the_weights_the_goldens_were_made_with(tag):
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    assert sd["encoders.position_enc"].shape == (1, cfg["max_dna_len"], cfg["dmodel"])
    assert sd["decoders.position_enc"].shape == (1, cfg["max_signal_len"], cfg["dmodel"])
    g = load_npz(f"geometry_{tag}.npz")
    assert weights_sha256(sd, cfg) == weights_sha256(geometry_state_dict(tag), cfg) == str(g["weights_sha256"])
    assert g["y_ideal"].shape == (g["codes"].shape[0], cfg["max_signal_len"])


def test_fixtures_stay_small():
    assert sum(os.path.getsize(os.path.join(GOLDEN, f"geometry_{t}.npz")) for t in TAGS) < 2_000_000


def test_long_attention_kernel_has_no_scratch_or_spills(tmp_path):
    """gen_attention_long_kernel (three head-dim instances): 0 B scratch, no spills, no LDS (K and V come through the caches), so
    LDS never limits the workgroups per CU."""
    usage = _build.compile_to(str(tmp_path / "libcheck.so"), report=True)
    attn = {k: u for k, u in usage.items() if k.startswith("_Z25gen_attention_long_kernel")}
    assert sorted(re.search(r"ILi(\d+)E", k).group(1) for k in attn) == ["1", "32", "8"], sorted(usage)
    for k, u in attn.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["LDS Size [bytes/block]"] == 0, (k, u)
    # the export kernels: the tuned 250-sample rows and the run-time row length
    for name in ("s2s_count_kernel", "s2s_compact_kernel"):
        inst = [k for k in usage if re.match(rf"_Z\d+{name}ILi(250|0)EE", k)]
        assert len(inst) == 2, (name, sorted(usage))


def test_cli_accepts_compute_mode_generic_geometry():
    env = {k: v for k, v in dict(os.environ, S2S_DRY_LAUNCH="1").items() if k != "WORLD_SIZE"}
    base = [sys.executable, "-m", "seq2squiggle_amd", "predict", "g.fa", "-o", "o.blow5", "--gpus", "2", "-m",
            checkpoint_path("r16x500")]
    r = subprocess.run(base + ["--compute-mode", "generic-geometry"], cwd=ROOT, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["dry_launch"]
    assert cmd[cmd.index("--compute-mode") + 1] == "generic-geometry"
