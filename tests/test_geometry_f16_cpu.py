"""The reduced-precision chunk-geometry instance (S2S_MODE_GENERIC_GEOMETRY_F16, compute mode "generic-geometry-f16") without a GPU:
the mode constant, the C ABI's limits and blob size (those of S2S_MODE_GENERIC_GEOMETRY), the Python mode selection, the CLI option,
the reference's 16-mixed vectors at the geometry cases (tests/golden/geometry_mixed16.npz, written by
tools/make_geometry_mixed16_goldens.py), and the new attention kernel's register budget."""
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
from seq2squiggle_amd import _build, _lib
from seq2squiggle_amd.checkpoint import MODES, TUNED_MODES, config_to_c, default_mode
from conftest import GOLDEN, ROOT, load_npz
from _geometry_models import CASES, checkpoint_path, geometry_config, weights_sha256
from _sized_models import checkpoint_path as sized_checkpoint_path

GEOMETRY, GEOMETRY_F16 = 6, 7
MODE = "generic-geometry-f16"
TAGS = list(CASES)


def blob_floats(c):
    return _lib.lib().s2s_blob_floats(ctypes.byref(c))


def err_of(c):
    h = ctypes.c_void_p()
    rc = _lib.lib().s2s_create(ctypes.byref(c), None, 0, 0, ctypes.byref(h))
    return rc, _lib.lib().s2s_last_error(None).decode()


def test_mode_constant_and_never_the_default():
    hdr = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()
    assert "#define S2S_MODE_GENERIC_GEOMETRY_F16 7" in hdr
    assert MODES[MODE] == GEOMETRY_F16 and MODE not in TUNED_MODES
    for tag in TAGS:
        cfg = geometry_config(tag)
        assert default_mode(cfg) == "generic-geometry"                    # opt-in only
        assert config_to_c(cfg, MODE).compute_mode == GEOMETRY_F16
    for path in (os.path.join(GOLDEN, "synthetic_k9.ckpt"), sized_checkpoint_path("d128")):
        assert default_mode(S.load_checkpoint(path)[1]) != MODE
    assert default_mode(dict(geometry_config("r16x500"), max_signal_len=250)) == "f16x3"


@pytest.mark.parametrize("tag", TAGS)
def test_blob_size_equals_generic_geometry(tag):
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    n = blob_floats(config_to_c(cfg, MODE))
    assert n == blob_floats(config_to_c(cfg, "generic-geometry")) == sum(v.numel() for v in sd.values()) > 0


@pytest.mark.parametrize("te,ts", [(1, 1), (64, 1024), (1, 1024), (64, 1), (16, 250)])
def test_blob_size_at_the_edges(te, ts):
    cfg = dict(geometry_config("g12x300"), max_dna_len=te, max_signal_len=ts)
    assert blob_floats(config_to_c(cfg, MODE)) == blob_floats(config_to_c(cfg, "generic-geometry")) > 0


@pytest.mark.parametrize("key,value", [("max_dna_len", 0), ("max_dna_len", 65), ("max_signal_len", 0), ("max_signal_len", 1025),
                                       ("dmodel", 72), ("dmodel", 528), ("dff", 4), ("dff", 2056), ("decoder_heads", 5),
                                       ("decoder_heads", 17)])
def test_limits_name_their_key_and_the_mode(key, value):
    _, cfg = S.load_checkpoint(checkpoint_path("g12x300"))
    c = config_to_c(cfg, MODE)
    setattr(c, key, value)
    assert blob_floats(c) == 0
    rc, msg = err_of(c)
    assert rc == -1 and key in msg and "S2S_MODE_GENERIC_GEOMETRY_F16" in msg, msg
    c6 = config_to_c(cfg, "generic-geometry")                            # mode 6 keeps naming itself
    setattr(c6, key, value)
    rc, msg6 = err_of(c6)
    assert rc == -1 and key in msg6 and "GEOMETRY_F16" not in msg6, msg6


@pytest.mark.parametrize("tag", TAGS + ["k9"])
def test_engine_accepts_the_mode_at_every_geometry(tag, monkeypatch):
    """The mode checks come before the device: with no GPU the constructor gets as far as asking for one, 16 / 250 included."""
    sd, cfg = S.load_checkpoint(os.path.join(GOLDEN, "synthetic_k9.ckpt") if tag == "k9" else checkpoint_path(tag))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        S.Engine(sd, cfg, mode=MODE)


def test_f16_modes_at_another_geometry_name_both_geometry_modes():
    sd, cfg = S.load_checkpoint(checkpoint_path("r16x500"))
    for mode in ("generic-f16", "f16"):
        with pytest.raises(ValueError) as e:
            S.Engine(sd, cfg, mode=mode)
        msg = str(e.value)
        assert "'generic-geometry'" in msg and "'generic-geometry-f16'" in msg and "max_signal_len 500" in msg, msg
    with pytest.raises(ValueError) as e:
        S.Engine(sd, cfg, mode="f32")
    assert "generic-geometry-f16" not in str(e.value)


def test_cli_accepts_compute_mode_generic_geometry_f16():
    env = {k: v for k, v in dict(os.environ, S2S_DRY_LAUNCH="1").items() if k != "WORLD_SIZE"}
    base = [sys.executable, "-m", "seq2squiggle_amd", "predict", "g.fa", "-o", "o.blow5", "--gpus", "2", "-m",
            checkpoint_path("r16x500")]
    r = subprocess.run(base + ["--compute-mode", MODE], cwd=ROOT, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["dry_launch"]
    assert cmd[cmd.index("--compute-mode") + 1] == MODE


@pytest.mark.parametrize("tag", TAGS)
def test_geometry_mixed16_goldens_belong_to_the_case_weights(tag):
    """tests/golden/geometry_mixed16.npz: the reference's 16-mixed run of geometry_<tag>.npz's chunks, with the same weights; its
    stored distances re-derive from its vectors, and its arithmetic is measurably not fp32."""
    sd, cfg = S.load_checkpoint(checkpoint_path(tag))
    m16, g = load_npz("geometry_mixed16.npz"), load_npz(f"geometry_{tag}.npz")
    assert str(m16[f"weights_sha256_{tag}"]) == weights_sha256(sd, cfg) == str(g["weights_sha256"])
    r16, dur16, t = m16[f"y_gamma_nsamp_16mixed_{tag}"], m16[f"dur_gamma_16mixed_{tag}"], g["y_gamma_nsamp"]
    assert r16.shape == t.shape == (g["codes"].shape[0], cfg["max_signal_len"]) and dur16.shape == g["dur_gamma"].shape
    agree = (dur16 == g["dur_gamma"]).all(1)
    assert agree.sum() > 0.8 * len(agree)
    d = np.abs(r16 - t)[agree]
    assert abs(d.mean() - float(m16[f"mae_vs_fp32_where_dwell_equal_{tag}"])) < 1e-6
    assert abs(d.max() - float(m16[f"max_vs_fp32_where_dwell_equal_{tag}"])) < 1e-6
    assert d.mean() > 1e-3


def test_long_f16_attention_kernel_has_no_scratch_or_spills(tmp_path):
    """gen_attention_long_h_kernel (three head-dim instances) and gen_attention_h_any_kernel (the key count at run time; the 250-key
    gen_attention_h_kernel keeps its own signature): 0 B scratch, no spilled registers, LDS as the comments state (14,336 and
    40,960 bytes)."""
    usage = _build.compile_to(str(tmp_path / "libcheck.so"), report=True)
    attn = {k: u for k, u in usage.items() if k.startswith("_Z27gen_attention_long_h_kernel")}
    assert sorted(re.search(r"ILi(\d+)E", k).group(1) for k in attn) == ["1", "32", "8"], sorted(usage)
    assert "_Z22gen_attention_h_kernelPfii" in usage, sorted(usage)
    short = usage["_Z26gen_attention_h_any_kernelPfiii"]
    for k, u in {**attn, "any": short}.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
    for k, u in attn.items():
        assert u["LDS Size [bytes/block]"] == 14336, (k, u)
    assert short["LDS Size [bytes/block]"] == 40960 and short["VGPRs"] + short.get("AGPRs", 0) <= 128, short
