"""tests/_train_ref.py held to itself: autograd's float64 gradient against central differences of the float64 loss along a dozen
seeded directions (a step of 1e-6 of the weight norm, agreement to 1e-6 relative; the heads' input held fixed, as detach() holds
it) on g5x37 and hd1, and the mathematically zero
gradient of every w_ks.bias (softmax is shift invariant)."""
import numpy as np
import pytest
import torch

from seq2squiggle_amd.checkpoint import load_checkpoint
import _eval_data as ED
import _train_ref as R


def case(tag, B=7):
    g = ED.load(tag)
    sd, cfg = load_checkpoint(ED.checkpoint(tag))
    idx = R.rows_with_every_kind(g["kind"], B)
    target, stdev = ED.scaled(g, float(cfg["scaling_max_value"]))
    return sd, cfg, g["codes"][idx], g["lengths"][idx], target[idx], stdev[idx]


@pytest.mark.parametrize("tag", ["g5x37", "hd1"])
def test_autograd_matches_central_differences(tag):
    sd, cfg, *batch = case(tag)
    _, _, g = R.loss_and_grads(sd, cfg, *batch, torch.float64)
    names = [k for k in sd if k not in R.POSITION_TABLES]
    wnorm = np.sqrt(sum(float((sd[k].double() ** 2).sum()) for k in names))
    fixed = R.head_input({k: v.double() for k, v in sd.items()}, cfg, batch[0])       # the detach(): the heads' input does not move
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(12):
        direction = {k: rng.standard_normal(tuple(sd[k].shape)) for k in names}
        dn = np.sqrt(sum(float((v ** 2).sum()) for v in direction.values()))
        direction = {k: v / dn for k, v in direction.items()}
        h = 1e-6 * wnorm
        vals = []
        for sign in (1.0, -1.0):
            p = {k: v.double() for k, v in sd.items()}
            for k in names:
                p[k] = p[k] + sign * h * torch.from_numpy(direction[k])
            with torch.no_grad():
                vals.append(float(R.total_loss(p, cfg, *batch, torch.float64, heads_read=fixed)[0]))
        fd = (vals[0] - vals[1]) / (2 * h)
        an = sum(float((g[k] * direction[k]).sum()) for k in names)
        worst = max(worst, abs(fd - an) / abs(an))
    print(f"TRAIN-REF {tag}: worst |fd - autograd| / |autograd| {worst:.3e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("tag", ["g5x37", "hd1", "k9"])
def test_w_ks_bias_gradient_is_zero(tag):
    sd, cfg, *batch = case(tag, 3)
    _, _, g = R.loss_and_grads(sd, cfg, *batch, torch.float64)
    G = np.sqrt(sum(float((v ** 2).sum()) for v in g.values()))
    keys = [k for k in g if k.endswith("w_ks.bias")]
    assert len(keys) == cfg["encoder_layers"] + cfg["decoder_layers"]
    for k in keys:
        assert np.linalg.norm(g[k]) <= 1e-9 * G, (k, np.linalg.norm(g[k]), G)
    for k in R.POSITION_TABLES:
        assert not g[k].any()
