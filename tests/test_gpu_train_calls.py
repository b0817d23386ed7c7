"""The trainer's contract across calls (s2s_train.h: "a call's result depends on its inputs, B and the memory budget only"), on
g5x37 and on hd24 (seq_kmer 16: 5 k = 80 one-hot columns span two tiles of the src_emb gradient, which is stored transposed).

train_gradients reallocates the tape and the loss rows when B or the budget grows, carves a smaller tape out of a larger
allocation when they shrink, and takes the gradient, the partials and the statistics from whatever the call before left.  So:
  call sequence    one trainer: gradients(B = 7), gradients(B = 2), a budget for 3 chunks per micro-batch and gradients(B = 7) in
                   3 / 3 / 1, a large budget and gradients(B = 9), gradients(B = 1); every loss and gradient bit-equal to a fresh
                   trainer's that was given that budget and that call alone;
  stream           the same call inside torch.cuda.stream(torch.cuda.Stream()), its inputs copied in on that stream behind a delay
                   (late inputs, tests/_stream_order.py), gives the default stream's bits: gradients, and three steps (weights and
                   statistics);
  interleaved      a twelve-step trajectory with a gradients() call of another batch and another B between every two steps ends
                   with the bits of the trajectory without them, weights and every step's statistics: gradients() leaves m, v and
                   the weights alone;
  two trainers     of the two configurations taking alternate steps end with the bits each reaches alone;
  forward          after the twelve steps gradients()'s loss rows are bit-equal to evaluate_chunks' on an engine built from
                   state_dict() -- the arena the forward pass reads and the blob weights() hands out are one model -- and
                   state_dict_to_blob(state_dict()) is weights().
Everything here is bit equality the contract promises; no tolerance.  Batches are rows (start + i) mod N of the evaluation goldens,
targets x 1.3 as in test_gpu_train_steps; steps are Adam at lr 5e-4, clip 1.0."""
import functools

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import train as T
from seq2squiggle_amd.checkpoint import state_dict_to_blob
import _train_classes as TC
from test_gpu_train_gradients import budget_for, on_device
from test_gpu_train_steps import CLIP, LR, data

pytestmark = pytest.mark.gpu

TAGS = ["g5x37", "hd24"]
SEQUENCE = [(7, None), (2, None), (7, 3), (9, None), (1, None)]      # B, chunks per micro-batch (None: everything fits)
STREAM_B, STEP_B, OTHER_B, STEPS = 7, 8, 3, 12
LARGE = 1 << 40


@functools.lru_cache(maxsize=None)
def model(tag):
    return data(tag, 1.3)


def batch(tag, start, B):
    sd, cfg, *arrays = model(tag)
    rows = (start + np.arange(B)) % arrays[0].shape[0]
    return on_device(*(a[rows] for a in arrays))


def step(tr, args, s):
    return tr.step(*args, lr=LR, step=s + 1, optimizer="Adam", weight_decay=0.0, clip=CLIP)


@functools.lru_cache(maxsize=None)
def alone(tag):
    """The plain trajectory: STEPS steps of STEP_B rows -> (weights, [STEPS, 5] statistics), on the host."""
    sd, cfg = model(tag)[:2]
    tr = T.Trainer(sd, cfg, 0)
    stats = torch.stack([step(tr, batch(tag, s * STEP_B, STEP_B), s) for s in range(STEPS)]).cpu()
    w = tr.weights().cpu()
    tr.close()
    return w, stats


@pytest.mark.parametrize("tag", TAGS)
def test_call_sequence(tag):
    sd, cfg = model(tag)[:2]
    tr = T.Trainer(sd, cfg, 0)
    start = 0
    for B, n in SEQUENCE:
        if n is not None:
            budget = budget_for(tr, B, n)
            assert budget == TC.budget_for(cfg, B, n)
        else:
            budget = LARGE
            tr.set_memory(budget)
        assert tr.micro_batch(B) == (n or B)
        args = batch(tag, start, B)
        start += B
        got = tr.gradients(*args)
        fresh = T.Trainer(sd, cfg, 0, budget)
        assert fresh.micro_batch(B) == (n or B)
        want = fresh.gradients(*args)
        torch.cuda.synchronize()
        assert torch.equal(got["loss"], want["loss"]), f"B = {B}: the loss rows depend on the calls before"
        assert torch.equal(got["grad"], want["grad"]), f"B = {B}: the gradient depends on the calls before"
        assert bool(got["grad"].any())
        fresh.close()
    tr.close()


@pytest.mark.parametrize("tag", TAGS)
def test_stream(tag):
    """The side stream's inputs are LATE (tests/_stream_order.py): the input tensors hold other rows of the golden, a delay of ten times
    the default stream's run holds the side stream, the real rows are copied in behind it and the calls follow -- a launch, memset or
    copy that left the stream would read the other rows."""
    import _stream_order as SO
    sd, cfg = model(tag)[:2]
    tr = T.Trainer(sd, cfg, 0)

    def default_stream():
        want = tr.gradients(*batch(tag, 0, STREAM_B))
        wstats = torch.stack([step(tr, batch(tag, s * STREAM_B, STREAM_B), s) for s in range(3)]).cpu()
        return want, wstats, tr.weights().cpu()
    (want, wstats, wweights), t_solo = SO.timed(default_stream)
    want = {k: v.cpu() for k, v in want.items()}
    tr.close()
    tr = T.Trainer(sd, cfg, 0)
    tr.gradients(*batch(tag, 5, STREAM_B))              # (changes no weight: the tape grows here, not behind the delay)
    real = {(s, i): t for s in range(3) for i, t in enumerate(batch(tag, s * STREAM_B, STREAM_B))}
    decoy = {(s, i): t for s in range(3) for i, t in enumerate(batch(tag, 3 + s * STREAM_B, STREAM_B))}
    assert all(not torch.equal(real[k], decoy[k]) for k in real if k[1] in (0, 2))      # other k-mers, other targets
    side = SO.side_stream()
    ms = SO.delay_for(t_solo)
    ins, ev = SO.late(side, real, decoy, ms)
    rows = lambda s: tuple(ins[s, i] for i in range(4))                                            # noqa: E731
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        got = tr.gradients(*rows(0))
        stats = torch.stack([step(tr, rows(s), s) for s in range(3)])
        weights = tr.weights()
    before = SO.returned_before(side)
    snaps = SO.early(side, ins, decoy, dict(got, stats=stats, weights=weights))
    with torch.cuda.stream(side):
        got, stats, weights = {k: v.cpu() for k, v in got.items()}, stats.cpu(), weights.cpu()
    SO.lasted(f"test_gpu_train_calls.test_stream {tag}", ev, t_solo, ms)
    tr.close()
    assert before, "a trainer call waited for the stream"
    assert torch.equal(got["loss"], want["loss"]) and torch.equal(got["grad"], want["grad"])
    assert torch.equal(stats, wstats) and torch.equal(weights, wweights)
    assert not torch.equal(weights, torch.from_numpy(state_dict_to_blob(sd, cfg)))      # the steps did move the weights
    snaps = dict(snaps)
    assert torch.equal(snaps[".loss"].cpu(), want["loss"]) and torch.equal(snaps[".grad"].cpu(), want["grad"])
    assert torch.equal(snaps[".stats"].cpu(), wstats) and torch.equal(snaps[".weights"].cpu(), wweights)


@pytest.mark.parametrize("tag", TAGS)
def test_interleaved_gradients(tag):
    sd, cfg = model(tag)[:2]
    w, stats = alone(tag)
    tr = T.Trainer(sd, cfg, 0)
    got = []
    for s in range(STEPS):
        got.append(step(tr, batch(tag, s * STEP_B, STEP_B), s))
        g = tr.gradients(*batch(tag, 5 + s * OTHER_B, OTHER_B))["grad"]
        assert bool(g.any())
    assert torch.equal(torch.stack(got).cpu(), stats), "a gradients() call between two steps changed a later step"
    assert torch.equal(tr.weights().cpu(), w)
    tr.close()


def test_two_trainers():
    trs = {tag: T.Trainer(*model(tag)[:2], 0) for tag in TAGS}
    got = {tag: [] for tag in TAGS}
    for s in range(STEPS):
        for tag in TAGS:
            got[tag].append(step(trs[tag], batch(tag, s * STEP_B, STEP_B), s))
    for tag in TAGS:
        w, stats = alone(tag)
        assert torch.equal(torch.stack(got[tag]).cpu(), stats), tag
        assert torch.equal(trs[tag].weights().cpu(), w), tag
        trs[tag].close()


@pytest.mark.parametrize("tag", TAGS)
def test_forward_consistency(tag):
    sd, cfg = model(tag)[:2]
    tr = T.Trainer(sd, cfg, 0)
    for s in range(STEPS):
        step(tr, batch(tag, s * STEP_B, STEP_B), s)
    assert torch.equal(tr.weights().cpu(), alone(tag)[0])
    args = batch(tag, 3, STEP_B)
    loss = tr.gradients(*args)["loss"]
    now = tr.state_dict()
    eng = S.Engine(now, cfg, 0, "generic-geometry")
    assert torch.equal(loss, eng.evaluate_chunks(*args)["loss"]), "the forward pass of the trainer reads other weights than it hands out"
    eng.close()
    assert np.array_equal(state_dict_to_blob(now, cfg), tr.weights().cpu().numpy())
    tr.close()
