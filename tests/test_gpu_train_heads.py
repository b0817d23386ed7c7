"""The heads' backward pass across their range: the weights of tests/_head_variants.py (sets e5x37 and k9, combinations A - E: the
clamp at 1e-8, both sides of 1, nn.Softplus's threshold of 20, and exp past FLT_MAX), its chunks(), dwells drawn from LOSS_DWELLS,
stdev 0.01.  Only the heads' own tensors (four per head) are compared, by the rule of tests/test_gpu_train_gradients.py (the floor of 2^-18 matters
here: torch's own fp32 is at 1e-7 to 5e-7); their CPU gradients come from the two head losses alone, which is all that reaches them.

A chunk is left out when a conc or rate pre-activation lies within EDGE of LN_CLAMP, or when float32 and float64 decide the clamp
differently (h64 / h32): the gradient jumps by O(1) across that boundary.  At most 2 % of a set's chunks may be left out.
Every gradient the device returns is finite in all five combinations."""
import numpy as np
import pytest
import torch

from seq2squiggle_amd import train as T
from oracle import s2s_oracle as O
import _head_variants as HV
import _train_ref as R
from test_gpu_train_gradients import compare, on_device

pytestmark = pytest.mark.gpu

STDEV = 0.01


def kept_chunks(ref) -> np.ndarray:
    drop = np.zeros(ref["codes"].shape[0], bool)
    for head in ("conc", "rate"):
        x64, v64 = ref["h64"][head]
        _, v32 = ref["h32"][head]
        near = np.abs(x64 - HV.LN_CLAMP) < HV.EDGE
        differ = (v64 <= 1e-8) != (v32 <= float(np.float32(1e-8)))
        drop |= (near | differ).any(1)
    return ~drop


def head_grads(sd, cfg, codes, dwell, stdev, dtype):
    p = R.leaves(sd, dtype)
    emb = R.head_input(p, cfg, codes, dtype)
    sigma = O.noise_sampler(p, emb)
    conc, rate = O.duration_params(p, emb)
    x = torch.as_tensor(dwell).abs().clamp(min=1).to(dtype)
    loss = R.DURATION_SCALE * (-torch.distributions.Gamma(conc, rate, validate_args=False).log_prob(x)).mean() \
        + ((torch.as_tensor(stdev).to(dtype) - sigma) ** 2).mean()
    loss.backward()
    return {k: v.grad.numpy().copy() for k, v in p.items() if any(k.startswith(h + ".") for h in HV.HEADS.values())}


@pytest.mark.parametrize("combo", sorted(HV.COMBOS))
@pytest.mark.parametrize("weights", ["e5x37", "k9"])
def test_head_gradients(weights, combo):
    ref = HV.reference(weights, combo)
    sd, cfg = ref["sd"], ref["cfg"]
    keep = kept_chunks(ref)
    n = int(keep.sum())
    print(f"TRAIN-HEADS {weights} {combo}: {len(keep) - n} of {len(keep)} chunks left out")
    assert len(keep) - n <= 0.02 * len(keep)
    te, ts = int(cfg["max_dna_len"]), int(cfg["max_signal_len"])
    codes = ref["codes"][keep]
    dwell = HV.loss_dwells(len(keep), te, ts)[keep]
    stdev = np.full((n, te), STDEV, np.float32)
    target = np.zeros((n, ts), np.float32)
    g64 = head_grads(sd, cfg, codes, dwell, stdev, torch.float64)
    g32 = head_grads(sd, cfg, codes, dwell, stdev, torch.float32)
    assert len(g64) == 12                                         # 0.weight, 0.bias, 3.weight, 3.bias of the three heads
    tr = T.Trainer(sd, cfg, 0)
    grad = tr.gradients(*on_device(codes, dwell, target, stdev))["grad"]
    tr.close()
    assert bool(torch.isfinite(grad).all())
    dev = T.split_blob(grad.cpu().numpy(), cfg)
    _, _, bad = compare(f"heads {weights} {combo}", {k: dev[k] for k in g64}, g64, g32)
    assert not bad, bad
