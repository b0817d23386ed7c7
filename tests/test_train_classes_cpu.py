"""tests/_train_classes.py without a GPU: that the calls the trainer's GPU tests make reach every class of the backward pass and of
the optimizer step that train_classes_of names, that the table of those calls is the tests' own case lists, and that
train_micro_batch's arithmetic, restated, gives the splits the table claims for the budgets the tests bisect to."""
import os
import re

import numpy as np

import _train_classes as TC
import test_gpu_train_calls as CALLS
import test_gpu_train_envelope as ENVELOPE
import test_gpu_train_gradients as GRADIENTS
import test_gpu_train_splits as SPLITS
import test_gpu_train_steps as STEPS
from conftest import ROOT


def rows_of_the_tests():
    """(test, tag, B, chunks per micro-batch, steps) of every trainer call the five modules parametrise over, from their own lists."""
    out = set()
    for tag, B in GRADIENTS.CASES:
        if B is None:
            B = 3 if int(TC.config_of(tag)["max_signal_len"]) > 256 else 7
            out.add(("gradients.test_gradients", tag, B, B, False))
        else:
            out.add(("gradients.test_gradients", tag, B, 13, False))
    out |= {("gradients.test_gradients_at_the_large_sizes", tag, 3, 3, False) for tag in GRADIENTS.LARGE}
    out |= {("envelope.test_gradients", tag, B, B, False) for tag, B in ENVELOPE.CASES}
    out |= {("envelope.test_sharp_attention", tag, ENVELOPE.SHARP_ROWS, ENVELOPE.SHARP_ROWS, False) for tag, _ in ENVELOPE.SHARP}
    out |= {("splits.test_splits", tag, B, n, False) for tag, B, n in SPLITS.SPLITS}
    for tag in CALLS.TAGS:
        out |= {("calls.test_call_sequence", tag, B, n or B, False) for B, n in CALLS.SEQUENCE}
        out |= {("calls.test_stream", tag, CALLS.STREAM_B, CALLS.STREAM_B, s) for s in (False, True)}
        out |= {("calls.test_interleaved_gradients", tag, CALLS.STEP_B, CALLS.STEP_B, True),
                ("calls.test_interleaved_gradients", tag, CALLS.OTHER_B, CALLS.OTHER_B, False)}
        out.add(("calls.test_two_trainers", tag, CALLS.STEP_B, CALLS.STEP_B, True))
        out |= {("calls.test_forward_consistency", tag, CALLS.STEP_B, CALLS.STEP_B, s) for s in (False, True)}
    for p in STEPS.ONE_STEP:
        tag = p.values[0]
        B = STEPS.one_step_batch(tag)
        out.add(("steps.test_one_step_is_adam", tag, B, B, True))
    out |= {("steps.test_trajectory", tag, B, B, True) for tag, B, _ in STEPS.TRAJECTORIES}
    _, sizes = STEPS.epoch_batches((np.zeros(48),), STEPS.SCHEDULED_B, STEPS.SCHEDULED_STEPS)
    out |= {("steps.test_scheduled_trajectory", STEPS.SCHEDULED_TAG, B, B, True) for B in sizes}
    return out


def test_the_table_is_the_tests_own_cases():
    table = {(test, tag, B, n, steps) for test, tag, B, n, sizes, steps in TC.RUNS}
    assert len(table) == len(TC.RUNS)
    want = rows_of_the_tests()
    assert table == want, (sorted(table - want), sorted(want - table))


def test_runs_reach_every_class():
    reached = {}
    for test, tag, B, n, sizes, steps in TC.RUNS:
        c = TC.train_classes_of(TC.config_of(tag), sizes, steps)
        assert c <= TC.LABELS, (tag, c - TC.LABELS)
        for label in c:
            reached.setdefault(label, []).append((test, tag, B, n))
    assert set(reached) == TC.LABELS, sorted(TC.LABELS - set(reached))
    # the classes this table was extended for, and the case that holds each
    cases = lambda label: {tag for _, tag, _, _ in reached[label]}
    assert "hd2" in cases("attn_bwd:hp==2") and {"hd3", "hd6"} <= cases("attn_bwd:hd<hp<=8")
    assert {"st36", "un80", "hd2"} <= cases("attn_bwd:T_2..3") and "d512x288" in cases("attn_bwd:hd==512")
    assert {"st36", "un40", "hd2"} <= cases("attn_bwd:1<T<ng")
    assert {"d128", "hd40", "d512"} <= cases("step:norm_blocks>256") and "hd40" in cases("mm:dff%64==0")
    assert ("splits.test_splits", "g64x1024", 3, 2) in reached["wgrad:whole_tiles"]
    assert ("splits.test_splits", "hd1", 7, 1) in reached["rows:M<4"]


def test_splits_are_what_the_budgets_give():
    """The restated train_micro_batch: the unsplit calls fit the budget they run under, set_memory(1) gives one chunk, and the
    budget the tests' bisection lands on gives the split of the table.  (The GPU tests assert that the trainer's own bisection lands
    on the same number of bytes.)"""
    for test, tag, B, n, sizes, steps in TC.RUNS:
        cfg = TC.config_of(tag)
        assert sizes == tuple(TC.split(B, n)) and sum(sizes) == B and max(sizes) == n, (test, tag)
        if n == B:
            assert TC.micro_batch(cfg, TC.DEFAULT_MEMORY, B) == B, (test, tag)
        elif n == 1:
            assert TC.micro_batch(cfg, 1, B) == 1 and sizes == (1,) * B, (test, tag)
        else:
            budget = TC.budget_for(cfg, B, n)
            assert TC.micro_batch(cfg, budget, B) == n, (test, tag)
            assert TC.tape_floats(cfg, n) * 4 <= budget < TC.tape_floats(cfg, n + 1) * 4, (test, tag)
    of = lambda t: {sizes for test, tag, B, n, sizes, steps in TC.RUNS if tag == t and test == "splits.test_splits"}
    assert of("k6") == {(7,), (3, 3, 1), (2, 2, 2, 1), (1,) * 7} and of("hd1") == {(7,), (1,) * 7}
    assert of("g64x1024") == {(3,), (2, 1), (1, 1, 1)} and of("hd96s") == {(5,), (2, 2, 1)}
    k9 = [sizes for test, tag, B, n, sizes, steps in TC.RUNS if (tag, B) == ("k9", 37)]
    assert k9 == [(13, 13, 11)]


def test_constants_are_the_headers():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    train = read("seq2squiggle_amd", "csrc", "s2s_train.h")
    assert int(re.search(r"#define TR_GRAD_ROWS (\d+)", train).group(1)) == TC.TR_GRAD_ROWS
    assert int(re.search(r"#define TR_TILE (\d+)", train).group(1)) == 64 and int(re.search(r"#define TR_RK (\d+)", train).group(1)) == 16
    assert (int(re.search(r"#define TRAIN_ATTN_MAX_T (\d+)", train).group(1)), int(re.search(r"#define TRAIN_ATTN_MAX_HD (\d+)", train).group(1))) == (1024, 512)
    api = read("include", "s2s_hip.h")
    assert int(re.search(r"#define S2S_GENERIC_WORKSPACE_BYTES \((\d+)u << 20\)", api).group(1)) << 20 == TC.WORKSPACE_BYTES
    assert int(re.search(r"#define S2S_TRAINER_DEFAULT_MEMORY \(\(size_t\)(\d+) << 30\)", api).group(1)) << 30 == TC.DEFAULT_MEMORY


def test_the_arena_s_padding_moves_no_case_across_one_trip():
    for tag in sorted({tag for _, tag, _, _, _, steps in TC.RUNS if steps}):
        lo, hi = TC.arena_blocks(TC.config_of(tag))
        assert (lo <= 256) == (hi <= 256), tag
    assert TC.arena_blocks(TC.config_of("k9"))[0] == 116 and TC.arena_blocks(TC.config_of("d128"))[0] == 545
