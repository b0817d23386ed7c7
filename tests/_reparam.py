"""Function-preserving rescalings of the FFT blocks, shared by tests/test_reparam_cpu.py and tests/test_gpu_magnitudes.py.

For s = 2^e three rewrites of a block leave its function unchanged, and -- s being a power of two -- every fp32 (and fp64)
evaluation bit for bit, barring overflow and underflow:

  ffn : pos_ffn.w_1.{weight,bias} * s,  pos_ffn.w_2.weight / s        (ReLU is positively homogeneous)
  vo  : slf_attn.w_vs.{weight,bias} * s, slf_attn.fc.weight / s
  qk  : slf_attn.w_qs.{weight,bias} * s, slf_attn.w_ks.{weight,bias} / s

What moves is the range of the operands a kernel sees and nothing else: the expected output of every variant is the
expected output at e = 0.
"""
import torch

from oracle import s2s_oracle as O

PAIRS = ("ffn", "vo", "qk")
SCOPES = ("decoder", "encoder", "both")
EXPONENTS = (-10, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8, 10)
PREFIX = {"decoder": ("decoders.layer_stack_FFT.",), "encoder": ("encoders.layer_stack.",),
          "both": ("decoders.layer_stack_FFT.", "encoders.layer_stack.")}

# pair -> (state_dict key suffixes multiplied by s, suffixes divided by s)
_UP = {"ffn": ("pos_ffn.w_1.weight", "pos_ffn.w_1.bias"), "vo": ("slf_attn.w_vs.weight", "slf_attn.w_vs.bias"),
       "qk": ("slf_attn.w_qs.weight", "slf_attn.w_qs.bias")}
_DOWN = {"ffn": ("pos_ffn.w_2.weight",), "vo": ("slf_attn.fc.weight",), "qk": ("slf_attn.w_ks.weight", "slf_attn.w_ks.bias")}
# pair -> (oracle taps multiplied by s, taps divided by s): the intermediates the rescaled Linear layers produce
_TAP_UP = {"ffn": ("pos_ffn.hidden",), "vo": ("slf_attn.v", "slf_attn.attn_out"), "qk": ("slf_attn.q",)}
_TAP_DOWN = {"ffn": (), "vo": (), "qk": ("slf_attn.k",)}

F16_MAX = 65504.0
# The range condition of the GPU sweep: a variant is admitted only if the largest magnitude among its rescaled weights and the
# intermediates of the fp64 oracle (FFN hidden activation, V, the attention output in front of fc, Q, K; every block) is below
# F16_MAX / 4.  A condition, not a measurement: every hi half of a split stays finite with two binades of margin, so the sweep
# never produces a non-finite value on purpose.
RANGE_LIMIT = F16_MAX / 4
# ... and what it has to admit at least, for every pair and scope on both committed checkpoints (tests/test_reparam_cpu.py)
ADMITTED_AT_LEAST = tuple(e for e in EXPONENTS if -10 <= e <= 6)

# The contiguous band of e around 0 in which S2S_MODE_F16X3 holds the project's parity bounds against the oracle (MAE < 1e-4 pA and
# max < 2e-3 pA against fp32, no further from fp64 than 5 x the fp32 oracle, every zero-pattern flip below 2e-3 pA, dwell indices
# exact) on BOTH attention paths and in both passes of tests/test_gpu_magnitudes.py, per (pair, scope), measured on one MI355X with
# the k9 checkpoint: LABNOTES.md "Round 16", table "Envelope of f16x3".  Outside the band the test asserts exact dwell indices and a
# finite signal only.  The rule that ends most bands is the fp64 one; MAE is then at 0.8-1.5e-4 pA.
BAND = {
    ("ffn", "decoder"): (-4, 3), ("ffn", "encoder"): (-4, 2), ("ffn", "both"): (-3, 2),
    ("vo", "decoder"): (-4, 2), ("vo", "encoder"): (-3, 4), ("vo", "both"): (-3, 2),
    ("qk", "decoder"): (-4, 4), ("qk", "encoder"): (-6, 4), ("qk", "both"): (-4, 6),
}


def _scaled_keys(sd, pair, scope):
    up, down = [], []
    for k in sd:
        if k.startswith(PREFIX[scope]):
            if k.endswith(_UP[pair]):
                up.append(k)
            elif k.endswith(_DOWN[pair]):
                down.append(k)
    return up, down


def variant(sd, pair, e, scope):
    """A copy of the state_dict with `pair` rewritten by s = 2^e in every FFT block of `scope`."""
    assert pair in PAIRS and scope in SCOPES
    s = 2.0 ** e
    out = {k: v.clone() for k, v in sd.items()}
    up, down = _scaled_keys(sd, pair, scope)
    assert up and down
    for k in up:
        out[k] = out[k] * s
    for k in down:
        out[k] = out[k] / s
    return out


def trained_like(sd, e=-2):
    """NOT function-preserving: every Linear weight and bias of every FFT block times 2^e (the oracle must be recomputed)."""
    out = {k: v.clone() for k, v in sd.items()}
    for k in out:
        if k.startswith(PREFIX["both"]) and ".layer_norm." not in k:
            out[k] = out[k] * 2.0 ** e
    return out


def intermediates(sd, cfg, codes, inject_g):
    """The fp64 oracle's taps on these chunks (noise off: the decoder does not see the noise): {block prefix + name: max |.|}."""
    taps = {}
    O.predict_chunks(sd, cfg, codes, O.PredictParams(noise_std=0.0), inject_g=inject_g, dtype=torch.float64, taps=taps)
    return taps


def magnitude(sd, taps, pair, scope):
    """The range condition's left side: the largest magnitude among the weights `pair` rescales in `scope` and the tapped
    intermediates (of every block: an unscaled one counts as it is)."""
    up, down = _scaled_keys(sd, pair, scope)
    w = max(float(sd[k].abs().max()) for k in up + down)
    return max(w, max(taps.values()))


def variant_magnitude(sd, cfg, codes, inject_g, pair, e, scope):
    """magnitude() of a variant, from an fp64 oracle run on the variant itself."""
    v = variant(sd, pair, e, scope)
    return magnitude(v, intermediates(v, cfg, codes, inject_g), pair, scope)


def scaled_magnitude(sd, taps0, pair, e, scope):
    """The same number from the taps of the UNSCALED model: in fp64 a power-of-two rescaling multiplies the intermediates a pair
    produces by exactly s (or 1 / s) and leaves every other one alone (tests/test_reparam_cpu.py holds this equal to
    variant_magnitude for every variant), so a sweep needs one fp64 run instead of one per variant."""
    s = 2.0 ** e
    up, down = _scaled_keys(sd, pair, scope)
    w = max([float(sd[k].abs().max()) * s for k in up] + [float(sd[k].abs().max()) / s for k in down])
    m = w
    for k, v in taps0.items():
        if k.startswith(PREFIX[scope]):
            if k.endswith(_TAP_UP[pair]):
                v = v * s
            elif _TAP_DOWN[pair] and k.endswith(_TAP_DOWN[pair]):
                v = v / s
        m = max(m, v)
    return m


def admitted(sd, taps0, pair, scope):
    """The exponents of EXPONENTS whose variant passes the range condition on the chunks taps0 was taken on."""
    return tuple(e for e in EXPONENTS if scaled_magnitude(sd, taps0, pair, e, scope) < RANGE_LIMIT)


def band(pair, scope):
    """The recorded band as the subset of EXPONENTS it covers."""
    lo, hi = BAND[(pair, scope)]
    return tuple(e for e in EXPONENTS if lo <= e <= hi)
