"""The bar of the tuned reduced-precision instance (S2S_MODE_F16, `--compute-mode f16`), computed at test time from the oracle.

The mode's contract (include/s2s_hip.h) is "decoder operands rounded to f16 once ... the precision class of the reference's own
fp16-autocast GPU path"; its frontend stays f16x3.  The plain reference of that operation is the oracle with ONLY decoder() under
torch.autocast("cpu", dtype=torch.float16) (oracle/s2s_oracle.py: predict_chunks(decoder_autocast16=True)): the policy of the
reference's inference.py:403-404 on the one stage the mode reduces.  Autocast also rounds every Linear / bmm OUTPUT to f16 where the
kernel keeps fp32 accumulators, so the bar is looser than the kernel by construction and `held` takes no multiplier.

Shared by tests/test_f16_bar_cpu.py (the bar is usable on every input the GPU tests take) and tests/test_gpu_f16_predict.py (the
instance against it); the variant checkpoints are shared with tests/test_gpu_parity.py."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from oracle import s2s_oracle as O
from conftest import load_ckpt, load_npz

QK = ("w_qs.weight", "w_ks.weight", "w_qs.bias", "w_ks.bias")
FLIP_SHARE = 1e-3          # zero-pattern flips against the fp32 oracle: at most 0.1 % of the samples
MIN_MAE = 1e-4             # the reduced instance is measurably not the parity path (pA)
REDONE_MOST = ("x4", "x16")
REDONE_SOME = ("x2", "pos2", "pos3")


def variant(sd, kind):
    """Checkpoints that make the fast softmax path redo heads.  "stock": a copy; "x2" / "x4" / "x16" = the decoder's w_qs / w_ks
    (weights and biases) scaled: x2 redoes SOME heads, x4 and x16 most; "pos2" / "pos3" = attention on the positional encoding alone
    (w_qs = w_ks = c I, biases 0: scores follow the sinusoid table, local attention), SOME heads redone."""
    out = {k: v.clone() for k, v in sd.items()}
    if kind == "stock":
        return out
    for k in out:
        if k.startswith("decoders.") and k.endswith(QK):
            if kind.startswith("x"):
                out[k] = out[k] * float(kind[1:])
            else:
                c = float(kind[3:])
                out[k] = c * torch.eye(64) if k.endswith("weight") else torch.zeros(64)
    return out


def P(**kw):
    base = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                min_noise=0.0, min_duration=3.0)
    base.update(kw)
    return base


@dataclass
class Oracles:
    ref32: dict
    bar16: dict
    ref64: Optional[dict]


_ORACLES = {}


def oracles(sd, cfg, codes, params, g=None, z01=None, zdw=None, want64=True, key=None) -> Oracles:
    """(weights, config, codes, parameter dict, injected variates) -> the fp32 oracle, the decoder-autocast oracle (the bar) and the
    fp64 oracle (`want64`; `held` does not read it).  `key`: results are kept per key for the life of the process."""
    if key is not None and key in _ORACLES and (_ORACLES[key].ref64 is not None or not want64):
        return _ORACLES[key]
    p = O.PredictParams(**params)
    kw = dict(inject_g=g, inject_z01=z01, inject_zdw=zdw)
    o = Oracles(ref32=O.predict_chunks(sd, cfg, codes, p, **kw),
                bar16=O.predict_chunks(sd, cfg, codes, p, decoder_autocast16=True, **kw),
                ref64=O.predict_chunks(sd, cfg, codes, p, dtype=torch.float64, **kw) if want64 else None)
    if key is not None:
        _ORACLES[key] = o
    return o


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def distance(y, ref32, mask=None):
    """-> (MAE, max, zero-pattern flips, the mask) of y against the fp32 oracle where their zero patterns agree (and `mask` holds)."""
    y, r = _np(y).astype(np.float64), _np(ref32).astype(np.float64)
    same = (y == 0) == (r == 0)
    m = same if mask is None else same & mask
    d = np.abs(y - r)[m]
    return (float(d.mean()) if d.size else 0.0, float(d.max()) if d.size else 0.0, int((~same).sum()), same)


def held(y, ref32, bar16, label="", check_max=True):
    """The f16 instance's output `y` against the fp32 oracle `ref32`, no worse than the decoder-autocast oracle `bar16` (all [B,250],
    pA): y finite; its zero pattern the fp32 oracle's except on at most 0.1 % of the samples, and on each of those the non-zero
    side no larger than the bar's max distance; on the samples where y AND the bar keep the fp32 zero pattern (one mask for both: a
    sample the bar itself flips carries a ReLU crossing, not a rounding distance) MAE <= the bar's MAE and max <= the bar's max,
    no multiplier; and MAE > 1e-4 pA, the instance is the reduced one.  `check_max=False` drops only the max clause (the x16 variant:
    a documented limit of the arithmetic class, DESIGN.md section 4, test_f16_bar_cpu.py::test_x16_max_belongs_to_the_arithmetic_class).
    (With the noise sampler on, a sample that crosses the ReLU carries its whole noise draw on the non-zero side, so the flip clause
    is at its strictest there; the instance meets it as it stands on every input of the GPU file.)
    -> dict(mae, max, bar_mae, bar_max, flips, bar_flips, n, flip_side)."""
    y, r, b = _np(y), _np(ref32), _np(bar16)
    assert np.isfinite(y).all(), (label, "not finite")
    _, _, bar_flips, bar_same = distance(b, r)
    _, _, flips, same = distance(y, r)
    mae, mx, _, _ = distance(y, r, bar_same)
    bar_mae, bar_mx, _, _ = distance(b, r, same)
    flip_side = float(np.maximum(np.abs(y), np.abs(r))[~same].max()) if flips else 0.0
    fig = dict(mae=mae, max=mx, bar_mae=bar_mae, bar_max=bar_mx, flips=flips, bar_flips=bar_flips, n=int(y.size), flip_side=flip_side)
    print(f"F16HELD {label}: mode MAE {mae:.4f} max {mx:.3f} | bar MAE {bar_mae:.4f} max {bar_mx:.3f} | flips {flips} (bar {bar_flips}) of "
          f"{y.size}, largest flipped sample {flip_side:.3f}")
    assert flips <= FLIP_SHARE * y.size, (label, fig)
    assert flip_side <= bar_mx, (label, fig)
    assert mae > MIN_MAE, (label, fig)
    assert mae <= bar_mae, (label, fig)
    if check_max:
        assert mx <= bar_mx, (label, fig)
    return fig


def decoder_f16_operands(sd, cfg, lr_out):
    """The mode's contract restated on the CPU, as plainly as it reads: every operand of a decoder matrix product (Linear inputs and
    weights, Q, K, V, the unnormalised P) rounded to f16 ONCE, the products accumulated exactly (float64), everything else -- biases,
    softmax shift and normalisation, residuals, LayerNorm -- in fp32.  lr_out [B,250,64] -> y_scaled [B,250].  Not a model of the
    kernel's instruction order; it tells a kernel defect from a property of the arithmetic class."""
    import math
    import torch.nn.functional as Fn

    def h(x):
        return x.half().float()

    def lin(x, p):
        return (h(x).double() @ h(sd[p + ".weight"]).double().t()).float() + sd[p + ".bias"]

    def norm(x, p):
        return Fn.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)
    x = lr_out + sd["decoders.position_enc"][0]
    nh = cfg["decoder_heads"]
    B, T, D = x.shape
    for l in range(cfg["decoder_layers"]):
        a, f = f"decoders.layer_stack_FFT.{l}.slf_attn.", f"decoders.layer_stack_FFT.{l}.pos_ffn."
        q, k, v = (lin(x, a + n).view(B, T, nh, D // nh).permute(0, 2, 1, 3) for n in ("w_qs", "w_ks", "w_vs"))
        s = (h(q).double() @ h(k).double().transpose(-1, -2)).float() * (math.log2(math.e) / math.sqrt(D // nh))
        p = h(torch.exp2(s - s.max(-1, keepdim=True).values))
        o = ((p.double() @ h(v).double()).float() / p.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B, T, D)
        x = norm(lin(o, a + "fc") + x, a + "layer_norm")
        x = norm(lin(torch.relu(lin(x, f + "w_1")), f + "w_2") + x, f + "layer_norm")
    return torch.relu(lin(x, "decoders.out_linear")).squeeze(-1)


def line(case, path, fig, redo=None):
    """The one line every GPU test of the instance prints."""
    return (f"F16 {case} {path}: mode {fig['mae']:.4f}/{fig['max']:.3f} | bar {fig['bar_mae']:.4f}/{fig['bar_max']:.3f} | "
            f"flips {fig['flips']} of {fig['n']} | redo {'-' if redo is None else format(redo, '.4f')}")


# --------------------------------------------------------------------------- the input sets of tests/test_gpu_f16_predict.py
@dataclass
class Case:
    label: str
    sd: dict
    cfg: dict
    codes: np.ndarray
    params: dict
    g: Optional[torch.Tensor] = None
    z01: Optional[torch.Tensor] = None
    extra: dict = field(default_factory=dict)

    def oracles(self, want64=False) -> Oracles:
        return oracles(self.sd, self.cfg, self.codes, self.params, self.g, self.z01, want64=want64, key=self.label)


def stage_case(tag, kind, noise=True) -> Case:
    """3a / 3b / 3f: the 51 / 56 chunks of stages_<tag>.npz with their injected g and z01."""
    sd, cfg = load_ckpt(tag)
    g = load_npz(f"stages_{tag}.npz")
    z = torch.from_numpy(np.ascontiguousarray(g["z01"]).astype(np.float32))
    return Case(f"{tag}-{kind}-{'noise' if noise else 'nonoise'}", variant(sd, kind), cfg, g["codes"],
                P() if noise else P(noise_std=0.0), torch.from_numpy(g["g"]), z if noise else None, dict(golden=g))


def mixed_reads():
    """3c: two random and two lambda reads of 384 bases (96 chunks)."""
    from oracle import redo_model as R
    fam = R.input_families(seed=3, n_reads=2, read_len=384)
    return fam["random"] + fam["lambda"]


def mixed_case(tag, kind) -> Case:
    sd, cfg = load_ckpt(tag)
    codes = np.concatenate([O.encode_read(r, cfg["seq_kmer"]) for r in mixed_reads()], 0)
    gen = torch.Generator().manual_seed(11)
    gi = torch.rand(codes.shape[0], 16, generator=gen) * 20
    return Case(f"{tag}-{kind}-mixed", variant(sd, kind), cfg, codes, P(noise_std=0.0), gi)


def edge_case(i) -> Case:
    """3d: the ragged reads of test_gpu_parity.py::test_edge_inputs_and_parameters under its i-th parameter set, its variates."""
    from test_gpu_parity import EDGE_PARAMS, EDGE_READS
    sd, cfg = load_ckpt("k9")
    codes = np.concatenate([O.encode_read(r, 9) for r in EDGE_READS], 0)
    gen = torch.Generator().manual_seed(5)
    g = torch.rand(codes.shape[0], 16, generator=gen) * 30
    z = torch.randn(codes.shape[0], 250, generator=gen)
    return Case(f"edge{i}", sd, cfg, codes, P(**EDGE_PARAMS[i]), g, z, dict(reads=EDGE_READS))


def depth_case(enc_l, dec_l, pre_l) -> Case:
    """3e: test_gpu_parity.py::test_other_layer_counts's checkpoints, reads and variates."""
    from test_gpu_parity import layer_count_model
    sd, cfg, gen = layer_count_model(enc_l, dec_l, pre_l)
    rng = np.random.default_rng(enc_l + dec_l)
    reads = ["".join(rng.choice(list("ACGT"), 700)) for _ in range(2)]
    codes = np.concatenate([O.encode_read(r, 9) for r in reads])
    g = torch.rand(codes.shape[0], 16, generator=gen) * 25
    z = torch.randn(codes.shape[0], 250, generator=gen)
    return Case(f"depth{enc_l}{dec_l}{pre_l}", sd, cfg, codes, P(), g, z)


def all_cases():
    """Every (checkpoint, variant, input set) the GPU file holds against the bar, as (id, builder)."""
    from test_gpu_parity import EDGE_PARAMS, LAYER_COUNTS
    out = []
    for tag in ("k9", "k6"):
        out.append((f"{tag}-stock-noise", lambda tag=tag: stage_case(tag, "stock")))
        for kind in REDONE_MOST:
            for noise in (False, True):
                out.append((f"{tag}-{kind}-{'noise' if noise else 'nonoise'}", lambda tag=tag, kind=kind, noise=noise: stage_case(tag, kind, noise)))
        for kind in REDONE_SOME:
            out.append((f"{tag}-{kind}-mixed", lambda tag=tag, kind=kind: mixed_case(tag, kind)))
    out += [(f"edge{i}", lambda i=i: edge_case(i)) for i in range(len(EDGE_PARAMS))]
    out += [(f"depth{e}{d}{p}", lambda e=e, d=d, p=p: depth_case(e, d, p)) for e, d, p in LAYER_COUNTS]
    return out
