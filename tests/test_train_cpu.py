"""What `train` does without a device: the three schedules against their closed forms, TrainData's order and batches, the checkpoint
round trip, the default initialisation's bounds, and the command's refusals."""
import math
import os

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

from seq2squiggle_amd import cli, train as T
from seq2squiggle_amd.checkpoint import load_checkpoint, state_dict_to_blob
from oracle import s2s_oracle as O
import _eval_data as ED


@pytest.fixture(scope="module")
def k9():
    return load_checkpoint(ED.checkpoint("k9"))


@pytest.fixture(scope="module")
def k9_dir(tmp_path_factory):
    return ED.write_dir(ED.load("k9"), str(tmp_path_factory.mktemp("train_data")), per_file=40)


def test_schedules_are_the_closed_forms():
    total, ratio, lr = 1000, 0.1, 5e-4
    warm = int(total * ratio)
    for step in (0, warm - 1, warm, total // 2, total - 1):
        up = step / warm if step < warm else 1.0
        cos = up if step < warm else 0.5 * (1 + math.cos(math.pi * (step - warm) / (total - warm)))
        assert T.lr_at("warmup_cosine", step, total, ratio, lr) == pytest.approx(lr * cos, rel=1e-15, abs=0)
        assert T.lr_at("warmup_constant", step, total, ratio, lr) == pytest.approx(lr * up, rel=1e-15, abs=0)
        assert T.lr_at("constant", step, total, ratio, lr) == lr
    assert T.lr_at("warmup_cosine", 0, total, ratio, lr) == 0.0 and T.lr_at("warmup_cosine", warm, total, ratio, lr) == lr
    assert T.lr_at("warmup_cosine", 3, 5, 0.01, lr) == lr * 0.5 * (1 + math.cos(math.pi * 3 / 5))      # int(0.05) = 0 warm-up steps
    with pytest.raises(ValueError, match="linear"):
        T.lr_at("linear", 0, total, ratio, lr)


def test_train_data_order_batches_and_limits(k9, k9_dir):
    _, cfg = k9
    g = ED.load("k9")
    target, stdev = ED.scaled(g, float(cfg["scaling_max_value"]))
    td = T.TrainData(k9_dir, cfg, None, seed=5)
    assert td.n == 96 and td.steps_per_epoch(36) == 3
    for epoch in (0, 1):
        order = np.random.default_rng([5, epoch]).permutation(96)
        assert np.array_equal(td.order(epoch), order)
        seen, sizes = [], []
        for i, (chunks, dwell, tg, sv) in enumerate(td.epoch(epoch, 36)):
            idx = order[36 * i:36 * i + 36]
            sizes.append(len(dwell))
            seen += list(idx)
            assert np.array_equal(chunks, ED.onehot(g["codes"][idx])) and np.array_equal(dwell, g["lengths"][idx].astype(np.int32))
            assert np.array_equal(tg, target[idx]) and np.array_equal(sv, stdev[idx]) and tg.dtype == sv.dtype == np.float32
        assert sizes == [36, 36, 24] and sorted(seen) == list(range(96))          # the short last batch; every chunk once
    assert not np.array_equal(td.order(0), td.order(1))
    few = T.TrainData(k9_dir, cfg, 50, seed=5)
    assert few.n == 50 and sorted(few.order(0)) == list(range(50)) and sum(len(b[1]) for b in few.epoch(0, 16)) == 50


def test_checkpoint_round_trip(k9, tmp_path):
    sd, cfg = k9
    blob = torch.from_numpy(state_dict_to_blob(sd, cfg))
    back = T.blob_to_state_dict(blob, cfg)
    path = str(tmp_path / "m" / "model.ckpt")
    os.makedirs(os.path.dirname(path))
    T.save_checkpoint(path, back, cfg, 0, 7)
    sd2, cfg2 = load_checkpoint(path)
    assert cfg2 == cfg and set(sd2) == set(back)
    for k, v in sd2.items():
        assert v.shape == sd[k].shape and torch.equal(v, sd[k].float()), k
    assert np.array_equal(state_dict_to_blob(sd2, cfg2), blob.numpy())


@pytest.mark.gpu
def test_engine_accepts_the_checkpoint(k9, tmp_path):
    import seq2squiggle_amd as S
    sd, cfg = k9
    path = str(tmp_path / "model.ckpt")
    T.save_checkpoint(path, T.default_init(cfg, 1), cfg, 0, 0)
    for mode in ("f16x3", "f32", "f16", "generic", "generic-geometry"):
        S.Engine.from_checkpoint(path, 0, mode).close()


@pytest.mark.parametrize("tag", ["k9", "hd96s", "hd1"])
def test_default_initialisation(tag):
    sd, cfg = load_checkpoint(ED.checkpoint(tag))
    init = T.default_init(cfg, 4)
    assert list(init) == list(T.state_shapes(cfg)) and all(tuple(init[k].shape) == tuple(sd[k].shape) for k in init)
    again = T.default_init(cfg, 4)
    assert all(torch.equal(init[k], again[k]) for k in init) and not torch.equal(init["encoders.src_emb.weight"],
                                                                                  T.default_init(cfg, 5)["encoders.src_emb.weight"])
    for k, v in init.items():
        if k.endswith("position_enc"):
            assert torch.equal(v[0], O.sinusoid_table(v.shape[1], v.shape[2]))
        elif k.endswith("layer_norm.weight"):
            assert bool((v == 1).all())
        elif k.endswith("layer_norm.bias"):
            assert bool((v == 0).all())
        else:
            fan_in = init[k[:-4] + "weight"].shape[1] if k.endswith(".bias") else v.shape[1]
            bound = 1.0 / math.sqrt(fan_in)
            assert float(v.abs().max()) <= bound
            if v.numel() >= 256:
                assert float(v.abs().max()) > 0.9 * bound and abs(float(v.mean())) < 0.2 * bound


def invoke(args):
    return CliRunner().invoke(cli.main, ["train"] + args)


def test_command_refusals(k9, k9_dir, tmp_path):
    _, cfg = k9
    def conf(**kw):
        p = str(tmp_path / ("_".join(f"{k}-{v}" for k, v in kw.items()) + ".yaml"))
        with open(p, "w") as f:
            yaml.safe_dump({**cfg, **dict(train_batch_size=16, max_epochs=1, lr=5e-4, optimizer="Adam", lr_schedule="constant"), **kw}, f)
        return p
    out = str(tmp_path / "o" / "model.ckpt")
    r = invoke([k9_dir, k9_dir, "-o", out, "-y", conf(optimizer="SGD")])
    assert r.exit_code != 0 and "optimizer 'SGD'" in r.output
    r = invoke([k9_dir, k9_dir, "-o", out, "-y", conf(lr_schedule="linear")])
    assert r.exit_code != 0 and "lr_schedule 'linear'" in r.output
    r = invoke([k9_dir, k9_dir, "-o", "model.ckpt", "-y", conf()])
    assert r.exit_code != 0 and "directory part" in r.output
    r = invoke([k9_dir, k9_dir, "-o", str(tmp_path / "o" / "model.pt"), "-y", conf()])
    assert r.exit_code != 0 and ".ckpt" in r.output
    r = invoke([k9_dir, k9_dir, "-o", out, "-y", conf(dff=128), "--init", ED.checkpoint("k9")])
    assert r.exit_code != 0 and "dff is 256 in the checkpoint and 128 in the config" in r.output
    r = invoke([k9_dir, k9_dir, "-o", out, "-y", conf(), "--max-steps", "0"])
    assert r.exit_code != 0 and "--max-steps" in r.output
    assert not os.path.exists(out)
