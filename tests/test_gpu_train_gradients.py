"""s2s_trainer_gradients against autograd on the CPU oracle (tests/_train_ref.py), on the eleven evaluation goldens with their
checkpoints: one key and one row (hd1), T below a wave (g5x37), seq_kmer 1 and 16, 4 / 4 / 4 layers at 64 k-mers (hd96s), both
long-attention lengths (g64x1024, hd208 at 17 / 1023), dwell 0 rows and the k-mer stalled for 32767 samples (the goldens' kinds).
B = 3 at ts > 256 and 7 otherwise, the rows chosen so that every `kind` of the golden is among them; one more case repeats k9 with
B = 37 under a memory budget of 13 chunks: three micro-batches (13, 13, 11), 3,250 decoder rows each -- ragged against the
weight-gradient tile of 512 rows and several tiles long.

Per case, with g64 / g32 the CPU gradients in float64 / float32 and G = ||g64|| over all tensors:
  a tensor is negligible when ||g64_k|| <= 1e-9 G (the w_ks.bias tensors, whose gradient is mathematically zero: softmax is shift
  invariant; at hd1 also the tensors whose float64 gradient is exactly 0);
  r32 = max_k ||g32_k - g64_k|| / ||g64_k|| over the others;
  every other tensor:    ||g_dev_k - g64_k|| / ||g64_k|| <= max(8 r32, 2^-18);
  every negligible one:  ||g_dev_k|| <= 8 r32 G.
Factor 8: the device sums B T rows in fixed tiles where torch uses its own blocked reductions, and recomputes the softmax.  Floor
2^-18: 64 fp32 ulps, for the cases where torch's CPU kernels work in double internally.
Also: the per-chunk loss sums equal s2s_evaluate_chunks' on a generic-geometry engine bit for bit, a second call gives the same
bits, and the position tables' slots of the gradient are 0.

The sizes above the goldens' (tests/_sized_models.py: d128 = dmodel 128, dff 512, 16 encoder heads, 2 pre-net layers; d512 = dmodel
512, head_dim 128, no pre-net) have no evaluation golden: they run the same rule on seeded random k-mers, dwells (with zeros and one
stalled k-mer), targets and stdevs, B = 3.

Every case prints TRAIN-GRAD <tag>: r32, the device's worst ratio and dev / r32 before it asserts."""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import train as T
from seq2squiggle_amd.checkpoint import load_checkpoint
import _eval_data as ED
import _train_ref as R

pytestmark = pytest.mark.gpu

FACTOR, FLOOR, NEGLIGIBLE = 8.0, 2.0 ** -18, 1e-9
CASES = [(tag, None) for tag in ED.TAGS] + [("k9", 37)]


def case_inputs(tag, B):
    g = ED.load(tag)
    sd, cfg = load_checkpoint(ED.checkpoint(tag))
    if B is None:
        B = 3 if int(cfg["max_signal_len"]) > 256 else 7
    idx = R.rows_with_every_kind(g["kind"], B)
    target, stdev = ED.scaled(g, float(cfg["scaling_max_value"]))
    return sd, cfg, g["codes"][idx], g["lengths"][idx], target[idx], stdev[idx]


def on_device(codes, lengths, target, stdev):
    return (torch.from_numpy(R.kmers_of(codes)).cuda().contiguous(), torch.from_numpy(lengths.astype(np.int32)).cuda().contiguous(),
            torch.from_numpy(target).cuda().contiguous(), torch.from_numpy(stdev).cuda().contiguous())


def budget_for(tr, B, n):
    """Bisect the trainer's memory budget to n chunks per micro-batch of a batch of B, leave it set and return it."""
    lo, hi = 1, 1 << 40
    budget = hi
    tr.set_memory(budget)
    while tr.micro_batch(B) != n:
        assert hi - lo > 1, f"no budget gives {n} chunks per micro-batch"
        budget = (lo + hi) // 2
        tr.set_memory(budget)
        if tr.micro_batch(B) < n:
            lo = budget
        elif tr.micro_batch(B) > n:
            hi = budget
    return budget


def compare(name, dev: dict, g64: dict, g32: dict):
    """-> (r32, the device's worst relative distance, failures) by the module docstring's rule."""
    norm = {k: float(np.linalg.norm(v)) for k, v in g64.items()}
    G = float(np.sqrt(sum(n * n for n in norm.values())))
    small = {k for k, n in norm.items() if n <= NEGLIGIBLE * G}
    r32 = max(float(np.linalg.norm(g32[k].astype(np.float64) - g64[k])) / norm[k] for k in g64 if k not in small)
    worst, worst_name, bad = 0.0, None, []
    for k in g64:
        d = dev[k].astype(np.float64)
        if k in small:
            v = float(np.linalg.norm(d))
            if not v <= FACTOR * r32 * G:
                bad.append((k, "negligible", v, FACTOR * r32 * G))
        else:
            v = float(np.linalg.norm(d - g64[k])) / norm[k]
            if v > worst:
                worst, worst_name = v, k
            if not v <= max(FACTOR * r32, FLOOR):
                bad.append((k, "relative", v, max(FACTOR * r32, FLOOR)))
    print(f"TRAIN-GRAD {name}: r32 {r32:.3e} dev {worst:.3e} dev/r32 {worst / r32:.2f} negligible {len(small)} G {G:.3e} "
          f"worst tensor {worst_name}")
    return r32, worst, bad


@pytest.mark.parametrize("tag,B", CASES, ids=[t if b is None else f"{t}-B{b}" for t, b in CASES])
def test_gradients(tag, B):
    sd, cfg, codes, lengths, target, stdev = case_inputs(tag, B)
    _, _, g64 = R.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float64)
    _, _, g32 = R.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float32)
    tr = T.Trainer(sd, cfg, 0)
    if B is not None:                                              # 13 chunks per micro-batch: 37 = 13 + 13 + 11
        budget_for(tr, B, 13)
        assert tr.micro_batch(B) == 13
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
    _, _, bad = compare(tag if B is None else f"{tag}-B{B}", dev, g64, g32)
    eng.close()
    tr.close()
    assert not bad, bad


def random_inputs(cfg, B, seed):
    k, te, ts = int(cfg["seq_kmer"]), int(cfg["max_dna_len"]), int(cfg["max_signal_len"])
    rng = np.random.default_rng(seed)
    codes = rng.integers(1, 5, (B, te, k)).astype(np.uint8)
    lengths = rng.integers(0, 2 * ts // te, (B, te)).astype(np.int64)
    lengths[0, :min(2, te - 1)] = 0                                   # (below three k-mers the chunk keeps one that has samples)
    lengths[1 % B, te // 2] = 32767                                   # a stalled k-mer: everything behind it is cropped
    target = rng.random((B, ts), dtype=np.float32)
    stdev = (rng.random((B, te), dtype=np.float32) * 0.02).astype(np.float32)
    return codes, lengths, target, stdev


LARGE = ["d128", "d512"]


@pytest.mark.parametrize("tag", LARGE)
def test_gradients_at_the_large_sizes(tag):
    import _sized_models as SM
    sd, cfg = load_checkpoint(SM.checkpoint_path(tag))
    codes, lengths, target, stdev = random_inputs(cfg, 3, 17)
    _, _, g64 = R.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float64)
    _, _, g32 = R.loss_and_grads(sd, cfg, codes, lengths, target, stdev, torch.float32)
    tr = T.Trainer(sd, cfg, 0)
    args = on_device(codes, lengths, target, stdev)
    out = tr.gradients(*args)
    again = tr.gradients(*args)
    eng = S.Engine(sd, cfg, 0, "generic-geometry")
    ev = eng.evaluate_chunks(*args)
    assert torch.equal(out["loss"], ev["loss"]) and torch.equal(out["grad"], again["grad"])
    assert bool(torch.isfinite(out["grad"]).all())
    dev = T.split_blob(out["grad"].cpu().numpy(), cfg)
    _, _, bad = compare(tag, dev, g64, g32)
    eng.close()
    tr.close()
    assert not bad, bad
