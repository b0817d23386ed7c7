"""Synthetic checkpoints at chunk geometries other than max_dna_len 16 / max_signal_len 250, from a seeded recipe.

The recipe of tests/_sized_models.py (numpy's PCG64 stream, nn.Linear's default init ranges, sharpened attention, calibrated head
biases, every value rounded to fp16-representable fp32) with the two position tables sized by the case's geometry: the encoder's
sinusoid table has max_dna_len rows and the decoder's max_signal_len rows, as the reference's Encoder / Decoder build them
(modules.py:25, 100).  tools/make_geometry_goldens.py loads exactly these weights into the reference's seq2squiggle(config=...)
and records tests/golden/geometry_<tag>.npz with the SHA-256 of the weight blob (`weights_sha256`)."""
import math
import os

import numpy as np
import torch

from _sized_models import _sinusoid, weights_sha256  # noqa: F401  (re-exported for the tests)

# tag: seed, seq_kmer, max_dna_len, max_signal_len, dmodel, dff, encoder_heads, decoder_heads, pre_layers, encoder_layers,
# decoder_layers (keys not given keep the shipped config's values)
CASES = {
    # the RNA-shaped checkpoint: the shipped sizes at 16 / 500 (rna-004 runs ~31 samples per base)
    "r16x500": dict(seed=21, seq_kmer=9, max_dna_len=16, max_signal_len=500),
    # neither length a multiple of 16 or 64; head_dim 32 on the decoder (the long attention's 8-tile instance)
    "g12x300": dict(seed=22, seq_kmer=6, max_dna_len=12, max_signal_len=300, dmodel=32, dff=64, encoder_heads=4, decoder_heads=1,
                    pre_layers=0, encoder_layers=1, decoder_layers=2),
    # short windows: the crop dominates
    "g5x37": dict(seed=23, seq_kmer=6, max_dna_len=5, max_signal_len=37, dmodel=48, dff=96, encoder_heads=3, decoder_heads=1,
                  pre_layers=1, encoder_layers=1, decoder_layers=1),
    # both upper edges
    "g64x1024": dict(seed=24, seq_kmer=9, max_dna_len=64, max_signal_len=1024, dmodel=16, dff=8, encoder_heads=2, decoder_heads=1,
                     pre_layers=0, encoder_layers=1, decoder_layers=1),
    # head_dim 512 on the long attention
    "d512x288": dict(seed=25, seq_kmer=9, max_dna_len=16, max_signal_len=288, dmodel=512, dff=32, encoder_heads=4, decoder_heads=1,
                     pre_layers=0, encoder_layers=1, decoder_layers=1),
}


def geometry_config(tag: str, base: dict = None, cases: dict = None) -> dict:
    """The config of case `tag` of the table `cases` (default: CASES above; tests/_envelope_models.py passes its own): `base`
    (default: the package's copy of the reference's config.yaml) with the case's keys."""
    if base is None:
        from seq2squiggle_amd.cli import set_config
        base = set_config(None)
    c = dict(base)
    c.update({k: v for k, v in (cases or CASES)[tag].items() if k != "seed"})
    return c


def geometry_state_dict(tag: str, cases: dict = None) -> dict:
    """The weights of case `tag`, keyed and shaped as the reference's state_dict (fp32 tensors, fp16-representable values)."""
    from seq2squiggle_amd.checkpoint import blob_names
    cfg = geometry_config(tag, cases=cases)
    d, f, k = cfg["dmodel"], cfg["dff"], cfg["seq_kmer"]
    rng = np.random.default_rng((cases or CASES)[tag]["seed"])

    def linear(prefix, n_out, n_in):
        b = 1.0 / math.sqrt(n_in)                 # nn.Linear's default init range, weight and bias
        return {prefix + "weight": rng.uniform(-b, b, (n_out, n_in)), prefix + "bias": rng.uniform(-b, b, (n_out,))}

    def norm(prefix):
        return {prefix + "weight": 1.0 + 0.25 * rng.standard_normal(d), prefix + "bias": 0.1 * rng.standard_normal(d)}

    def layer(p):
        out = {}
        for n in ("w_qs", "w_ks", "w_vs", "fc"):
            out.update(linear(f"{p}slf_attn.{n}.", d, d))
        out[p + "slf_attn.w_qs.weight"] *= 3.0      # non-degenerate softmax rows
        out[p + "slf_attn.w_ks.weight"] *= 3.0
        out.update(norm(p + "slf_attn.layer_norm."))
        out.update(linear(p + "pos_ffn.w_1.", f, d))
        out.update(linear(p + "pos_ffn.w_2.", d, f))
        out.update(norm(p + "pos_ffn.layer_norm."))
        return out

    sd = {"encoders.position_enc": _sinusoid(cfg["max_dna_len"], d).numpy()[None]}
    sd.update(linear("encoders.src_emb.", d, 5 * k))
    for i in range(cfg["pre_layers"]):
        sd.update(linear(f"encoders.pre_net_stack.{i}.", d, d))
    for l in range(cfg["encoder_layers"]):
        sd.update(layer(f"encoders.layer_stack.{l}."))
    for head in ("noise_sampler.stdv_layer.", "length_regulator.duration_sampler.conc_layer.",
                 "length_regulator.duration_sampler.rate_layer."):
        sd.update(linear(head + "0.", d, d))
        sd.update(linear(head + "3.", 1, d))
    sd["decoders.position_enc"] = _sinusoid(cfg["max_signal_len"], d).numpy()[None]
    for l in range(cfg["decoder_layers"]):
        sd.update(layer(f"decoders.layer_stack_FFT.{l}."))
    sd.update(linear("decoders.out_linear.", 1, d))
    # calibrated heads: Gamma(~9, ~0.8) dwell ~ 11, sigma ~ 0.01 scaled, ~80 pA with some ReLU zeros
    sd["length_regulator.duration_sampler.conc_layer.3.bias"][:] = 9.0
    sd["length_regulator.duration_sampler.rate_layer.3.bias"][:] = math.log(math.exp(0.8) - 1.0)
    sd["length_regulator.duration_sampler.conc_layer.3.weight"] *= 4.0
    sd["noise_sampler.stdv_layer.3.bias"][:] = math.log(math.exp(0.01) - 1.0)
    sd["noise_sampler.stdv_layer.3.weight"] *= 4.0
    sd["decoders.out_linear.bias"][:] = 0.5
    assert sorted(sd) == sorted(blob_names(cfg))
    return {n: torch.from_numpy(np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float32)) for n, v in sd.items()}


def write_checkpoint(tag: str, path: str, cases: dict = None) -> str:
    """Case `tag` as a Lightning-layout .ckpt at `path`, weights stored as fp16."""
    sd = geometry_state_dict(tag, cases)
    ckpt = {
        "epoch": 0, "global_step": 0, "pytorch-lightning_version": "2.5.1.post0",
        "state_dict": {n: t.half() for n, t in sd.items()},
        "hyper_parameters": {"config": geometry_config(tag, cases=cases), "save_valid_plots": True, "out_writer": None,
                             "dwell_mean": 9.0, "dwell_std": 0.0, "noise_std": -1, "noise_sampling": False,
                             "duration_sampling": False, "export_every_n_samples": 2000000, "min_noise": 0.5,
                             "min_duration": 1},
        "loops": {}, "callbacks": {}, "optimizer_states": [], "lr_schedulers": [],
    }
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(ckpt, path)
    return path


_WRITTEN = {}


def checkpoint_path(tag: str, cases: dict = None) -> str:
    """Case `tag` written once per process into a temporary directory; -> its path."""
    key = (id(cases or CASES), tag)
    if key not in _WRITTEN:
        import atexit, shutil, tempfile
        d = tempfile.mkdtemp(prefix="s2s_geometry_")
        atexit.register(shutil.rmtree, d, True)
        _WRITTEN[key] = write_checkpoint(tag, os.path.join(d, f"synthetic_{tag}.ckpt"), cases)
    return _WRITTEN[key]
