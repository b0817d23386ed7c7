"""Model sizes outside the shipped family (S2S_MODE_GENERIC): the C ABI's size rules and blob size, the Python mode
selection, and the CPU oracle against the imported reference's vectors for those sizes (tests/golden/sized_*.npz, written by
tools/make_sized_goldens.py from the weights of tests/_sized_models.py).  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _lib
from seq2squiggle_amd.checkpoint import MODES, config_to_c, default_mode, is_tuned_family
from oracle import s2s_oracle as O
from conftest import GOLDEN, load_npz
from _sized_models import checkpoint_path, weights_sha256

torch.set_float32_matmul_precision("highest")
TOL = 2e-6                 # scaled units, as tests/test_oracle_golden.py
SIZED = ["d128", "d32", "d512"]
GENERIC = 4


def sized(tag):
    return S.load_checkpoint(checkpoint_path(tag))


@pytest.mark.parametrize("tag", SIZED)
def test_sized_checkpoints_are_the_weights_the_goldens_were_made_with(tag):
    sd, cfg = sized(tag)
    assert all(t.dtype == torch.float32 for t in sd.values())
    assert weights_sha256(sd, cfg) == str(load_npz(f"sized_{tag}.npz")["weights_sha256"])


def err_of(c):
    h = ctypes.c_void_p()
    rc = _lib.lib().s2s_create(ctypes.byref(c), None, 0, 0, ctypes.byref(h))
    return rc, _lib.lib().s2s_last_error(None).decode()


def test_generic_mode_constant():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2s_hip.h")).read()
    assert "#define S2S_MODE_GENERIC 4" in hdr and MODES["generic"] == GENERIC


@pytest.mark.parametrize("tag", SIZED)
def test_generic_blob_size_matches_state_dict(tag):
    sd, cfg = sized(tag)
    assert not is_tuned_family(cfg) and default_mode(cfg) == "generic"
    c = config_to_c(cfg, "generic")
    assert c.compute_mode == GENERIC and c.decoder_heads == cfg["decoder_heads"]
    n = _lib.lib().s2s_blob_floats(ctypes.byref(c))
    assert n == sum(v.numel() for v in sd.values()) > 0
    assert S.state_dict_to_blob(sd, cfg).size == n
    # the same sizes in a tuned mode are refused
    for mode in ("f32", "f16x3", "f16"):
        assert _lib.lib().s2s_blob_floats(ctypes.byref(config_to_c(cfg, mode))) == 0


@pytest.mark.parametrize("tag", ["k9", "k6"])
def test_generic_blob_size_at_default_size(tag):
    sd, cfg = S.load_checkpoint(os.path.join(GOLDEN, f"synthetic_{tag}.ckpt"))
    assert is_tuned_family(cfg) and default_mode(cfg) == "f16x3"
    n_gen = _lib.lib().s2s_blob_floats(ctypes.byref(config_to_c(cfg, "generic")))
    assert n_gen == _lib.lib().s2s_blob_floats(ctypes.byref(config_to_c(cfg, "f32"))) == sum(v.numel() for v in sd.values())


@pytest.mark.parametrize("key,value,word", [
    ("dmodel", 8, "dmodel"), ("dmodel", 520, "dmodel"), ("dmodel", 72, "dmodel"),
    ("dff", 4, "dff"), ("dff", 2056, "dff"), ("dff", 12, "dff"),
    ("n_heads", 0, "n_heads"), ("n_heads", 17, "n_heads"), ("n_heads", 3, "n_heads"),
    ("decoder_heads", 32, "decoder_heads"), ("decoder_heads", 5, "decoder_heads"), ("decoder_heads", -1, "decoder_heads"),
    ("max_signal_len", 400, "max_signal_len"), ("max_dna_len", 32, "max_dna_len"),
    ("encoder_layers", 5, "encoder_layers"), ("decoder_layers", 0, "decoder_layers"), ("pre_layers", 5, "pre_layers"),
    ("seq_kmer", 17, "seq_kmer"),
])
def test_generic_limits_name_their_key(key, value, word):
    _, cfg = sized("d128")
    c = config_to_c(cfg, "generic")
    setattr(c, key, value)
    assert _lib.lib().s2s_blob_floats(ctypes.byref(c)) == 0
    rc, msg = err_of(c)
    assert rc == -1 and word in msg, msg


def test_generic_limits_accept_the_range_edges():
    _, cfg = sized("d32")
    c = config_to_c(cfg, "generic")
    for d, f, h, hd in ((16, 8, 1, 16), (512, 2048, 16, 1), (48, 24, 3, 16), (512, 8, 1, 0)):
        c.dmodel, c.dff, c.n_heads, c.decoder_heads = d, f, h, hd
        assert _lib.lib().s2s_blob_floats(ctypes.byref(c)) > 0, (d, f, h, hd)


def test_tuned_modes_refuse_as_before():
    sd, cfg = S.load_checkpoint(os.path.join(GOLDEN, "synthetic_k9.ckpt"))
    for mode in ("f32", "f16x3", "f16"):
        for key, value, word in (("dmodel", 128, "dmodel must be 64"), ("dff", 512, "dff must be 256"),
                                 ("n_heads", 4, "n_heads must be 8"), ("decoder_heads", 4, "decoder_heads")):
            c = config_to_c(cfg, mode)
            setattr(c, key, value)
            assert _lib.lib().s2s_blob_floats(ctypes.byref(c)) == 0
            rc, msg = err_of(c)
            assert rc == -1 and word in msg, (mode, key, msg)
        c = config_to_c(cfg, mode)
        c.decoder_heads = 8                       # explicit and equal: accepted
        assert _lib.lib().s2s_blob_floats(ctypes.byref(c)) > 0
        c.decoder_heads = 0                       # 0 = n_heads: what an old positional initialiser leaves
        assert _lib.lib().s2s_blob_floats(ctypes.byref(c)) > 0


def test_engine_refuses_tuned_mode_for_other_sizes():
    sd, cfg = sized("d128")
    with pytest.raises(ValueError, match="generic"):
        S.Engine(sd, cfg, mode="f32")


@pytest.mark.parametrize("tag", SIZED)
def test_oracle_holds_to_sized_goldens(tag):
    """oracle/s2s_oracle.py is size-generic: it must reproduce the reference at these sizes within test_oracle_golden.py's bounds."""
    sd, cfg = sized(tag)
    g = load_npz(f"sized_{tag}.npz")
    x = O.one_hot(g["codes"])
    enc_out, emb_out = O.encoder(sd, cfg, x)
    assert emb_out.shape[-1] == cfg["dmodel"]
    assert np.abs(emb_out.numpy() - g["emb_out"]).max() < TOL
    assert np.abs(enc_out.numpy() - g["enc_out"]).max() < 5 * TOL
    assert np.abs(O.noise_sampler(sd, emb_out).numpy() - g["sigma"]).max() < TOL
    conc, rate = O.duration_params(sd, emb_out)
    assert np.allclose(conc.numpy(), g["conc"], rtol=1e-6, atol=1e-6)
    assert np.allclose(rate.numpy(), g["rate"], rtol=1e-6, atol=1e-6)
    B = g["codes"].shape[0]
    p = O.PredictParams()
    dur = O.durations(p, B, torch.from_numpy(g["g"]))
    assert np.array_equal(dur.numpy(), g["dur_gamma"])
    h, sx = O.length_regulate(enc_out, torch.from_numpy(g["sigma"]), dur)
    assert np.array_equal(sx.numpy(), g["sigma_ext_gamma"])
    assert np.abs(O.decoder(sd, cfg, h).numpy() - g["y_scaled_gamma"]).max() < 10 * TOL
    out = O.predict_chunks(sd, cfg, g["codes"], O.PredictParams(min_duration=3.0), inject_g=torch.from_numpy(g["g"]),
                           inject_z01=torch.from_numpy(g["z01"]))
    y, ref = out["signal"].numpy(), g["y_gamma_nsamp"]
    assert np.array_equal(y == 0, ref == 0)
    assert np.abs(y - ref).mean() < 1e-4 and np.abs(y - ref).max() < 2e-3
