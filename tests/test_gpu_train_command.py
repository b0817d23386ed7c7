"""`train` end to end on the k9 golden written as a preprocess directory (TRAIN = VALID), --max-steps 6 from the k9 checkpoint: the
log's per-step losses equal a Python Trainer driven by hand over the same permutations, the written checkpoint's `evaluate` losses
equal the command's last valid_* line, the same command twice writes the same bytes; and without --init it writes a checkpoint
`predict` accepts."""
import json
import os

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

import seq2squiggle_amd as S
from seq2squiggle_amd import cli, train as T
from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd.checkpoint import load_checkpoint
import _eval_data as ED

pytestmark = pytest.mark.gpu

BS, STEPS = 32, 6


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_cmd")
    data = ED.write_dir(ED.load("k9"), str(root / "data"), per_file=40)
    sd, cfg = load_checkpoint(ED.checkpoint("k9"))
    cfg = dict(cfg, train_batch_size=BS, max_epochs=25, optimizer="AdamW", weight_decay=0.01, lr=5e-4, lr_schedule="warmup_cosine",
               warmup_ratio=0.34, gradient_clip_val=1.0)
    conf = str(root / "config.yaml")
    with open(conf, "w") as f:
        yaml.safe_dump(cfg, f)
    return root, data, conf, cfg, sd


def run(args):
    res = CliRunner().invoke(cli.main, ["train"] + args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    return [json.loads(line) for line in res.output.splitlines() if line.startswith("{")]


def test_train_from_a_checkpoint(setup):
    root, data, conf, cfg, sd = setup
    outs = []
    for name in ("a", "b"):
        out = str(root / name / "model.ckpt")
        rows = run([data, data, "-o", out, "-y", conf, "--init", ED.checkpoint("k9"), "--max-steps", str(STEPS), "--seed", "3", "--json"])
        outs.append((out, rows))
    (out, rows), (out_b, _) = outs
    assert open(out, "rb").read() == open(out_b, "rb").read(), "the same command wrote other bytes"
    steps = [r for r in rows if "step" in r]
    epochs = [r for r in rows if "epoch" in r]
    assert [r["step"] for r in steps] == list(range(1, STEPS + 1)) and [r["global_step"] for r in epochs] == [3, 6]
    # by hand
    td = T.TrainData(data, cfg, cfg.get("max_chunks_train"), seed=3)
    tr = T.Trainer(sd, cfg, 0)
    step = 0
    for epoch in range(2):
        for batch in td.epoch(epoch, BS):
            lr = T.lr_at("warmup_cosine", step, STEPS, 0.34, 5e-4)
            step += 1
            st = tr.step(*T.to_device(tr, *batch), lr=lr, step=step, optimizer="AdamW", weight_decay=0.01, clip=1.0).cpu().numpy()
            rec = steps[step - 1]
            assert rec["lr"] == lr
            assert [np.float32(rec[n]) for n in T.STAT_NAMES] == list(st), (step, rec, st)
    hand = tr.state_dict()
    tr.close()
    sd_out, cfg_out = load_checkpoint(out)
    assert cfg_out == cfg
    for k, v in hand.items():
        assert torch.equal(v, sd_out[k]), k
    eng = S.Engine.from_checkpoint(out, 0, "generic-geometry")          # the instance the command validates on
    losses, _, _ = EV.evaluate(eng, EV.EvalData(data, cfg_out, cfg_out.get("max_chunks_valid")))
    eng.close()
    print("TRAIN-CMD", epochs[-1])
    for k in ED.LOSSES:
        assert float(losses[k]) == epochs[-1][k], k


def test_train_from_the_default_initialisation(setup):
    root, data, conf, cfg, _ = setup
    out = str(root / "fresh" / "model.ckpt")
    rows = run([data, data, "-o", out, "-y", conf, "--max-steps", "2", "--json"])
    assert all(np.isfinite(r["train_total_loss"]) for r in rows if "step" in r)
    eng = S.Engine.from_checkpoint(out, 0)
    bases, nv, _ = S.encode_reads(["ACGT" * 60], cfg["seq_kmer"])
    p = S.PredictParams(dwell_mean=9.0, dwell_std=0.0, noise_std=0.0, noise_sampling=False, duration_sampling=False, min_noise=0.0,
                        min_duration=1.0)
    sig = eng.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), p)["signal"]
    eng.close()
    assert bool(torch.isfinite(sig).all())
