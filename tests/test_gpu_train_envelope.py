"""s2s_trainer_gradients on the configurations the envelope and geometry tables hold and no trainer test ran, and on attention rows
sharper than any checkpoint here has.  The rule, its constants and `compare` are tests/test_gpu_train_gradients.py's, unchanged.

Configurations (which class of the backward pass each adds: tests/_train_classes.py): the envelope cases hd3, hd6 (head_dim below a
small hp), hd40, hd112, hd136 (head_dim above 64 with a tail; dff 2048), st36 / un40 / st72 / un80 (T of 3, 4, 5 and 2 on the
encoder: idle waves beside live ones, fewer rows than row groups), the geometry case d512x288 (head_dim 512: wa / wb full; B = 2),
and hd2 of this module's own table (head_dim 2 on both sides, T = 3 on the encoder), all on
test_gpu_train_gradients.random_inputs: seeded k-mers, dwells with zeros and one stalled k-mer, targets and stdevs.  B = 3 where
max_signal_len > 256 or dmodel >= 128, else 7.  Per case, as test_gradients: the rule against float64 autograd, loss rows bit-equal
to evaluate_chunks' on a generic-geometry engine, a second call the same bits, a finite gradient, none on the position tables.

Sharp attention: g5x37 and k6 on rows 0..6 of their goldens with w_qs and w_ks (weight and bias) of every layer x 2 and x 4.
train_attention_bwd_kernel forms expf(s - max) / sum a second time in phase B from the row statistics phase A stored; at x 4 the
scores of a decoder row span more than -ln 2^-149 = 103.3, so the tail of the row is exactly 0 in fp32 and one key holds nearly
all of the weight.  The test measures that on the CPU (decoder layer 0, float64: the largest score range within a row and the
median over rows of the largest probability) before it touches the device and asserts range > 104 at x 4 and median > 0.5 at
both, so a recipe that drifts out of the regime fails instead of passing for another reason.

Every case prints its TRAIN-GRAD line before it asserts."""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import train as T
from seq2squiggle_amd.checkpoint import load_checkpoint
from oracle import s2s_oracle as O
import _envelope_models as EM
import _eval_data as ED
import _geometry_models as GM
import _train_ref as R
from test_gpu_train_gradients import FACTOR, FLOOR, NEGLIGIBLE, compare, on_device, random_inputs

pytestmark = pytest.mark.gpu
assert (FACTOR, FLOOR, NEGLIGIBLE) == (8.0, 2.0 ** -18, 1e-9)

# tag: seed, seq_kmer, max_dna_len, max_signal_len, dmodel, dff, encoder_heads, decoder_heads, pre / encoder / decoder layers
OWN_CASES = {
    # head_dim 2 on both sides (hp == 2: 32 row groups per wave), three encoder keys
    "hd2": dict(seed=56, seq_kmer=5, max_dna_len=3, max_signal_len=40, dmodel=32, dff=24, encoder_heads=16, decoder_heads=16,
                pre_layers=0, encoder_layers=1, decoder_layers=1),
}
CASES = [("hd3", 7), ("hd6", 3), ("hd40", 3), ("hd112", 3), ("hd136", 3), ("st36", 3), ("un40", 7), ("st72", 3), ("un80", 7),
         ("d512x288", 2), ("hd2", 7)]
SHARP = [("g5x37", 2.0), ("g5x37", 4.0), ("k6", 2.0), ("k6", 4.0)]
SHARP_ROWS = 7
UNDERFLOW = 104.0        # above -ln 2^-149 = 103.28: expf(s - max) is exactly 0 in fp32


def checkpoint_of(tag):
    if tag in OWN_CASES:
        return GM.checkpoint_path(tag, OWN_CASES)
    return EM.checkpoint_path(tag) if tag in EM.CASES else GM.checkpoint_path(tag)


def check(name, sd, cfg, codes, lengths, target, stdev):
    """test_gradients' assertions on one batch."""
    _, _, g64 = R.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float64)
    _, _, g32 = R.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float32)
    tr = T.Trainer(sd, cfg, 0)
    args = on_device(codes, lengths, target, stdev)
    out = tr.gradients(*args)
    again = tr.gradients(*args)
    torch.cuda.synchronize()
    eng = S.Engine(sd, cfg, 0, "generic-geometry")
    ev = eng.evaluate_chunks(*args)
    assert torch.equal(out["loss"], ev["loss"]), "per-chunk loss sums differ from s2s_evaluate_chunks'"
    assert torch.equal(out["loss"], again["loss"]) and torch.equal(out["grad"], again["grad"]), "a second call gives other bits"
    assert bool(torch.isfinite(out["grad"]).all())
    dev = T.split_blob(out["grad"].cpu().numpy(), cfg)
    for n in R.POSITION_TABLES:
        assert not dev[n].any(), f"{n} has a gradient"
    _, _, bad = compare(name, dev, g64, g32)
    eng.close()
    tr.close()
    assert not bad, bad


@pytest.mark.parametrize("tag,B", CASES, ids=[t for t, _ in CASES])
def test_gradients(tag, B):
    sd, cfg = load_checkpoint(checkpoint_of(tag))
    assert B == (2 if tag == "d512x288" else 3 if int(cfg["max_signal_len"]) > 256 or int(cfg["dmodel"]) >= 128 else 7)
    check(tag, sd, cfg, *random_inputs(cfg, B, 17))


def sharpened(sd, factor):
    out = dict(sd)
    for k, v in sd.items():
        if ".slf_attn.w_qs." in k or ".slf_attn.w_ks." in k:
            out[k] = v * factor
    return out


def decoder_layer0_rows(sd, cfg, codes, lengths):
    """-> (the largest score range within a row, the median over rows of the largest probability) of the first decoder layer's
    attention, float64 on the CPU."""
    p = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        enc_out, emb_out = O.encoder(p, cfg, O.one_hot(codes, torch.float64))
        sigma = O.noise_sampler(p, emb_out)
        h, _ = O.length_regulate(enc_out, sigma, torch.as_tensor(np.ascontiguousarray(lengths).astype(np.int64)), cfg["max_signal_len"])
        x = h + p["decoders.position_enc"][0]
        B, Tn, D = x.shape
        H = int(cfg["decoder_heads"])
        pre = "decoders.layer_stack_FFT.0.slf_attn."
        q = torch.nn.functional.linear(x, p[pre + "w_qs.weight"], p[pre + "w_qs.bias"]).view(B, Tn, H, D // H).permute(0, 2, 1, 3)
        k = torch.nn.functional.linear(x, p[pre + "w_ks.weight"], p[pre + "w_ks.bias"]).view(B, Tn, H, D // H).permute(0, 2, 1, 3)
        s = q @ k.transpose(2, 3) / (D // H) ** 0.5
        spread = float((s.max(-1).values - s.min(-1).values).max())
        top = float(torch.softmax(s, -1).max(-1).values.median())
    return spread, top


def sharp_inputs(tag, factor):
    g = ED.load(tag)
    sd, cfg = load_checkpoint(ED.checkpoint(tag))
    target, stdev = ED.scaled(g, float(cfg["scaling_max_value"]))
    rows = np.arange(SHARP_ROWS)
    return sharpened(sd, factor), cfg, g["codes"][rows], g["lengths"][rows], target[rows], stdev[rows]


@pytest.mark.parametrize("tag,factor", SHARP, ids=[f"{t}-x{int(f)}" for t, f in SHARP])
def test_sharp_attention(tag, factor):
    sd, cfg, codes, lengths, target, stdev = sharp_inputs(tag, factor)
    spread, top = decoder_layer0_rows(sd, cfg, codes, lengths)
    print(f"TRAIN-SHARP {tag} x{factor:g}: decoder layer 0 score range within a row {spread:.1f}, median row max of softmax {top:.3f}")
    assert top > 0.5
    if factor == 4.0:
        assert spread > UNDERFLOW
    check(f"{tag}-x{factor:g}", sd, cfg, codes, lengths, target, stdev)
