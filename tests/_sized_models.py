"""Synthetic checkpoints at model sizes outside the shipped family, built from a seeded recipe instead of being stored.

A d512 checkpoint holds three million weights: too large to keep in the repository.  The weights are therefore a pure function
of (tag, seed, sizes) -- numpy's PCG64 stream, nn.Linear's default init ranges, sinusoid position tables, the sharpened attention
and calibrated head biases of tools/make_goldens.make_model, every value rounded to fp16-representable fp32 -- and
tools/make_sized_goldens.py loads exactly these weights into the reference's own seq2squiggle(config=...) before it records
tests/golden/sized_<tag>.npz.  Each npz carries the SHA-256 of the weight blob it was made with (`weights_sha256`), so a recipe
that drifts fails loudly instead of comparing against vectors of other weights."""
import hashlib
import math
import os

import numpy as np
import torch

# tag: seed, seq_kmer, dmodel, dff, encoder_heads, decoder_heads, pre_layers, encoder_layers, decoder_layers
CASES = {
    "d128": dict(seed=11, seq_kmer=9, dmodel=128, dff=512, encoder_heads=16, decoder_heads=4, pre_layers=2, encoder_layers=2,
                 decoder_layers=3),
    "d32": dict(seed=12, seq_kmer=6, dmodel=32, dff=8, encoder_heads=4, decoder_heads=8, pre_layers=0, encoder_layers=1,
                decoder_layers=1),
    "d512": dict(seed=13, seq_kmer=9, dmodel=512, dff=32, encoder_heads=4, decoder_heads=4, pre_layers=0, encoder_layers=1,
                 decoder_layers=1),
}


def sized_config(tag: str, base: dict = None) -> dict:
    """The config of case `tag`: `base` (default: the package's copy of the reference's config.yaml) with the case's sizes."""
    if base is None:
        from seq2squiggle_amd.cli import set_config
        base = set_config(None)
    c = dict(base)
    c.update({k: v for k, v in CASES[tag].items() if k != "seed"})
    return c


def _sinusoid(n_position: int, d_hid: int) -> torch.Tensor:
    """get_sinusoid_encoding_table (reference layers.py:145-165): python-float64 angles -> fp32 -> sin / cos in fp32."""
    tab = torch.tensor([[pos / 10000 ** (2 * (j // 2) / d_hid) for j in range(d_hid)] for pos in range(n_position)])
    tab[:, 0::2] = torch.sin(tab[:, 0::2])
    tab[:, 1::2] = torch.cos(tab[:, 1::2])
    return tab.float()


def sized_state_dict(tag: str) -> dict:
    """The weights of case `tag`, keyed and shaped as the reference's state_dict (fp32 tensors, fp16-representable values)."""
    from seq2squiggle_amd.checkpoint import blob_names
    cfg = sized_config(tag)
    d, f, k = cfg["dmodel"], cfg["dff"], cfg["seq_kmer"]
    rng = np.random.default_rng(CASES[tag]["seed"])

    def linear(prefix, n_out, n_in):
        b = 1.0 / math.sqrt(n_in)                 # nn.Linear's default init range, weight and bias
        return {prefix + "weight": rng.uniform(-b, b, (n_out, n_in)), prefix + "bias": rng.uniform(-b, b, (n_out,))}

    def norm(prefix):
        return {prefix + "weight": 1.0 + 0.25 * rng.standard_normal(d), prefix + "bias": 0.1 * rng.standard_normal(d)}

    def layer(p):
        out = {}
        for n in ("w_qs", "w_ks", "w_vs", "fc"):
            out.update(linear(f"{p}slf_attn.{n}.", d, d))
        out[p + "slf_attn.w_qs.weight"] *= 3.0      # non-degenerate softmax rows (make_goldens.make_model)
        out[p + "slf_attn.w_ks.weight"] *= 3.0
        out.update(norm(p + "slf_attn.layer_norm."))
        out.update(linear(p + "pos_ffn.w_1.", f, d))
        out.update(linear(p + "pos_ffn.w_2.", d, f))
        out.update(norm(p + "pos_ffn.layer_norm."))
        return out

    sd = {"encoders.position_enc": _sinusoid(16, d).numpy()[None]}
    sd.update(linear("encoders.src_emb.", d, 5 * k))
    for i in range(cfg["pre_layers"]):
        sd.update(linear(f"encoders.pre_net_stack.{i}.", d, d))
    for l in range(cfg["encoder_layers"]):
        sd.update(layer(f"encoders.layer_stack.{l}."))
    for head in ("noise_sampler.stdv_layer.", "length_regulator.duration_sampler.conc_layer.",
                 "length_regulator.duration_sampler.rate_layer."):
        sd.update(linear(head + "0.", d, d))
        sd.update(linear(head + "3.", 1, d))
    sd["decoders.position_enc"] = _sinusoid(250, d).numpy()[None]
    for l in range(cfg["decoder_layers"]):
        sd.update(layer(f"decoders.layer_stack_FFT.{l}."))
    sd.update(linear("decoders.out_linear.", 1, d))
    # calibrated heads (make_goldens.make_model): Gamma(~9, ~0.8) dwell ~ 11, sigma ~ 0.01 scaled, ~80 pA with some ReLU zeros
    sd["length_regulator.duration_sampler.conc_layer.3.bias"][:] = 9.0
    sd["length_regulator.duration_sampler.rate_layer.3.bias"][:] = math.log(math.exp(0.8) - 1.0)
    sd["length_regulator.duration_sampler.conc_layer.3.weight"] *= 4.0
    sd["noise_sampler.stdv_layer.3.bias"][:] = math.log(math.exp(0.01) - 1.0)
    sd["noise_sampler.stdv_layer.3.weight"] *= 4.0
    sd["decoders.out_linear.bias"][:] = 0.5
    assert sorted(sd) == sorted(blob_names(cfg))
    return {n: torch.from_numpy(np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float32)) for n, v in sd.items()}


def weights_sha256(sd: dict, cfg: dict) -> str:
    from seq2squiggle_amd.checkpoint import state_dict_to_blob
    return hashlib.sha256(state_dict_to_blob(sd, cfg).tobytes()).hexdigest()


def write_checkpoint(tag: str, path: str) -> str:
    """Case `tag` as a Lightning-layout .ckpt at `path` (the layout tools/make_goldens.save_ckpt writes), weights stored as fp16."""
    sd = sized_state_dict(tag)
    ckpt = {
        "epoch": 0, "global_step": 0, "pytorch-lightning_version": "2.5.1.post0",
        "state_dict": {n: t.half() for n, t in sd.items()},
        "hyper_parameters": {"config": sized_config(tag), "save_valid_plots": True, "out_writer": None,
                             "dwell_mean": 9.0, "dwell_std": 0.0, "noise_std": -1, "noise_sampling": False,
                             "duration_sampling": False, "export_every_n_samples": 2000000, "min_noise": 0.5,
                             "min_duration": 1},
        "loops": {}, "callbacks": {}, "optimizer_states": [], "lr_schedulers": [],
    }
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(ckpt, path)
    return path


_WRITTEN = {}


def checkpoint_path(tag: str) -> str:
    """Case `tag` written once per process into a temporary directory; -> its path."""
    if tag not in _WRITTEN:
        import atexit, shutil, tempfile
        d = tempfile.mkdtemp(prefix="s2s_sized_")
        atexit.register(shutil.rmtree, d, True)
        _WRITTEN[tag] = write_checkpoint(tag, os.path.join(d, f"synthetic_{tag}.ckpt"))
    return _WRITTEN[tag]
