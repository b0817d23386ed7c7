"""Micro-batching past one split: s2s_trainer_gradients under budgets that cut a batch in other ways than k9's 13 / 13 / 11.

  k6, B = 7:       7 (unsplit), 3 / 3 / 1, 2 / 2 / 2 / 1, and set_memory(1): the `cap < 1 -> 1` floor, one chunk per micro-batch
  hd1, B = 7:      set_memory(1): seven micro-batches of M = 1 row on both sides
  g64x1024, B = 3: 3, 2 / 1 (2,048 decoder rows, four whole weight-gradient tiles, then 1,024) and 1 / 1 / 1: long attention split
  hd96s, B = 5:    2 / 2 / 1: 502 decoder rows, one tile, then 251
on the rows of the evaluation goldens that hold every `kind` (test_gpu_train_gradients.case_inputs).  The budget of a split is
found by test_gpu_train_gradients.budget_for's bisection on the trainer; tests/_train_classes.py restates train_micro_batch, and
the test asserts that the restatement's bisection lands on the same number of bytes and the same split, so the table of
_train_classes.RUNS is what runs here.

Per split: the loss rows are bit-equal to the unsplit call's and to evaluate_chunks' (a chunk's forward pass does not depend on
its neighbours), the gradient meets test_gpu_train_gradients' rule against float64 autograd (same constants), and the same split
run twice gives the same bits.  Across splits no gradient bits are compared: the header makes the budget an input of the result.
The float64 / float32 references and the unsplit answer are computed once per tag and shared."""
import functools

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import train as T
import _train_classes as TC
import _train_ref as R
from test_gpu_train_gradients import budget_for, case_inputs, compare, on_device

pytestmark = pytest.mark.gpu

# tag, B, chunks per micro-batch (B: unsplit; 1: by set_memory(1))
SPLITS = [("k6", 7, 7), ("k6", 7, 3), ("k6", 7, 2), ("k6", 7, 1), ("hd1", 7, 7), ("hd1", 7, 1),
          ("g64x1024", 3, 3), ("g64x1024", 3, 2), ("g64x1024", 3, 1), ("hd96s", 5, 5), ("hd96s", 5, 2)]


@functools.lru_cache(maxsize=None)
def reference(tag, B):
    """-> (sd, cfg, host inputs, g64, g32, the unsplit call's loss and the engine's, on the host)."""
    sd, cfg, *inputs = case_inputs(tag, B)
    _, _, g64 = R.loss_and_grads(sd, cfg, *inputs, torch.float64)
    _, _, g32 = R.loss_and_grads(sd, cfg, *inputs, torch.float32)
    args = on_device(*inputs)
    tr = T.Trainer(sd, cfg, 0)
    assert tr.micro_batch(B) == B
    whole = tr.gradients(*args)["loss"].cpu()
    tr.close()
    eng = S.Engine(sd, cfg, 0, "generic-geometry")
    ev = eng.evaluate_chunks(*args)["loss"].cpu()
    eng.close()
    return sd, cfg, inputs, g64, g32, whole, ev


@pytest.mark.parametrize("tag,B,n", SPLITS, ids=[f"{t}-B{b}-n{n}" for t, b, n in SPLITS])
def test_splits(tag, B, n):
    sd, cfg, inputs, g64, g32, whole, ev = reference(tag, B)
    tr = T.Trainer(sd, cfg, 0)
    if n == 1:
        tr.set_memory(1)
        assert TC.micro_batch(cfg, 1, B) == 1
    elif n < B:
        assert budget_for(tr, B, n) == TC.budget_for(cfg, B, n)
    assert tr.micro_batch(B) == n
    sizes = TC.split(B, n)
    assert (tag, B, n, tuple(sizes)) in [r[1:5] for r in TC.RUNS if r[0] == "splits.test_splits"]
    args = on_device(*inputs)
    out = tr.gradients(*args)
    again = tr.gradients(*args)
    loss, grad = out["loss"].cpu(), out["grad"].cpu()
    assert torch.equal(loss, whole), "a chunk's loss sums depend on the split"
    assert torch.equal(loss, ev), "per-chunk loss sums differ from s2s_evaluate_chunks'"
    assert torch.equal(loss, again["loss"].cpu()) and torch.equal(grad, again["grad"].cpu()), "the same split twice gives other bits"
    tr.close()
    assert bool(torch.isfinite(grad).all())
    dev = T.split_blob(grad.numpy(), cfg)
    for name in R.POSITION_TABLES:
        assert not dev[name].any(), f"{name} has a gradient"
    _, _, bad = compare(f"{tag}-B{B} in {' + '.join(map(str, sizes))}", dev, g64, g32)
    assert not bad, bad
