"""s2s_trainer_step: the optimizer alone, and whole trajectories.

Unit: the update of one step against a float64 numpy restatement of torch.optim.Adam / AdamW (single-tensor form) on the gradient
the same trainer returned from gradients(): weight decay 0 and 0.01, clip below and above the norm, steps 1 and 1000 (m = v = 0, so
the bias corrections alone differ).  The device works in fp32 on fp32 state: per element
    |w_dev - w_ref| <= 2^-20 |w_ref| + 2^-20 lr R + D 2^-21 (|g s| + |wd w|)
-- an ulp-class rounding of the weight; a few of the update, whose size is at most lr R, R = the largest |update| / lr; and the
update's own conditioning: the direction g' = g s + wd w (s the clip scale) carries a few fp32 roundings of its two summands, and
the update u = step_size (1 - b1) g' / (c |g'| + eps) has du / dg' = D = step_size (1 - b1) eps / (c |g'| + eps)^2, which is
lr / eps-sized where coupled weight decay cancels a clipped gradient to below eps.  The position tables keep their bits.

Trajectory: twelve steps on k9 (B = 8, rows (s B + i) mod 96) and twenty-four on g5x37 (B = 16, mod 48), lr 5e-4, clip 1.0,
targets x 1.3 so that the weights move, against _train_ref.adam_run in float64, with adam_run in float32 on the CPU as yardstick:
every step's total loss within 8 x (fp32 CPU's largest relative loss difference), floor 2^-18, and
||w_dev - w64|| / ||w64 - w0|| over the whole model <= 8 x the same for fp32 CPU.  No test asks the loss to fall.

The unit also runs where train_norm_kernel makes more than one trip over train_sumsq_kernel's partials (one per 2,048 floats of the
arena, 256 a trip; k9 has 116) and train_adam_kernel's three ranges around the position tables are long: d128 (545 partials),
hd40 (544, dff 2048) and d512 (1,525), B = 2 on test_gpu_train_gradients.random_inputs, Adam and AdamW with weight decay 0.01, both
clips, step 1 -- same tolerance, same norm check against the float64 norm of the gradient the trainer returned.  clip = 0 (no
clipping: the reference's scale is 1) runs on k9.

Scheduled trajectories (g5x37, 24 steps): B = 20 on the 48-row golden, every epoch 20 / 20 / 8 in TrainData.epoch's order for
seed 0 (default_rng([0, epoch]).permutation(48)), the learning rate of every step lr_at("warmup_cosine", step, 24, 0.25, 5e-4) --
zero at the first step, a peak, a decay -- for AdamW with weight decay 0.01, Adam with coupled weight decay 0.01 and Adam without
clipping: b1 m and b2 v multiply moments that are not 0, the decay acts on weights that have moved, and a short batch follows two
full ones.  test_trajectory's two assertions and constants, _train_ref.adam_run taking the same per-step rates."""
import numpy as np
import pytest
import torch

from seq2squiggle_amd import train as T
from seq2squiggle_amd.checkpoint import load_checkpoint, state_dict_to_blob
import _eval_data as ED
import _train_ref as R
from test_gpu_train_gradients import on_device, random_inputs

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 8.0, 2.0 ** -18
LR, CLIP, EPS, B1, B2 = 5e-4, 1.0, 1e-7, 0.9, 0.999


def data(tag, scale_targets=1.0):
    g = ED.load(tag)
    sd, cfg = load_checkpoint(ED.checkpoint(tag))
    target, stdev = ED.scaled(g, float(cfg["scaling_max_value"]))
    return sd, cfg, g["codes"], g["lengths"], (target * np.float32(scale_targets)).astype(np.float32), stdev


def adam64(w, g, opt, lr, wd, clip, step):
    """One step from m = v = 0 in float64 -> (new weights, the norm before clipping)."""
    norm = float(np.sqrt((g * g).sum()))
    g = g * (clip / (norm + 1e-6) if clip > 0 and norm > clip else 1.0)
    if opt == "AdamW":
        w = w * (1.0 - lr * wd)
    else:
        g = g + wd * w
    m, v = (1 - B1) * g, (1 - B2) * g * g
    c = np.sqrt(1 - B2) / np.sqrt(1 - B2 ** step)
    cond = lr / (1 - B1 ** step) * (1 - B1) * EPS / (c * np.abs(g) + EPS) ** 2          # D of the module docstring
    return w - lr / (1 - B1 ** step) * m / (np.sqrt(v) / np.sqrt(1 - B2 ** step) + EPS), norm, cond


OPTIMIZERS = [("Adam", 0.0), ("Adam", 0.01), ("AdamW", 0.01)]
LARGE_TAGS = ["d128", "hd40", "d512"]
# tag, optimizer, weight decay, clip, step: the twelve k9 combinations under the ids they always had, then the large models and clip 0
ONE_STEP = ([pytest.param("k9", opt, wd, clip, step, id=f"{step}-{clip}-{opt}-{wd}")
             for step in (1, 1000) for clip in (0.05, 1e3) for opt, wd in OPTIMIZERS]
            + [pytest.param(tag, opt, wd, clip, 1, id=f"{tag}-1-{clip}-{opt}-{wd}")
               for tag in LARGE_TAGS for clip in (0.05, 1e3) for opt, wd in OPTIMIZERS[1:]]
            + [pytest.param("k9", opt, wd, 0.0, 1, id=f"k9-1-noclip-{opt}-{wd}") for opt, wd in OPTIMIZERS])


def one_step_batch(tag):
    return 8 if tag == "k9" else 2


def one_step_inputs(tag):
    """k9: rows 0..7 of its golden, targets x 1.3; the large models: B = 2 of random_inputs."""
    if tag == "k9":
        sd, cfg, codes, lengths, target, stdev = data("k9", 1.3)
        rows = np.arange(one_step_batch(tag))
        return sd, cfg, (codes[rows], lengths[rows], target[rows], stdev[rows])
    import _envelope_models as EM
    import _sized_models as SM
    sd, cfg = load_checkpoint(SM.checkpoint_path(tag) if tag in SM.CASES else EM.checkpoint_path(tag))
    return sd, cfg, random_inputs(cfg, one_step_batch(tag), 17)


@pytest.mark.parametrize("tag,opt,wd,clip,step", ONE_STEP)
def test_one_step_is_adam(tag, opt, wd, clip, step):
    sd, cfg, inputs = one_step_inputs(tag)
    args = on_device(*inputs)
    tr = T.Trainer(sd, cfg, 0)
    w0 = tr.weights().cpu().numpy().astype(np.float64)
    assert np.array_equal(w0.astype(np.float32), state_dict_to_blob(sd, cfg))
    g = tr.gradients(*args)["grad"].cpu().numpy().astype(np.float64)
    stats = tr.step(*args, lr=LR, step=step, optimizer=opt, weight_decay=wd, clip=clip).cpu().numpy()
    w1 = tr.weights().cpu().numpy().astype(np.float64)
    tr.close()
    ref, norm, cond = adam64(w0, g, opt, LR, wd, clip, step)
    assert (clip > 0 and norm > clip) == (clip == 0.05)
    assert abs(stats[4] - norm) <= 1e-6 * norm
    assert abs(stats[3] - (stats[0] + stats[1] + stats[2])) <= 1e-6 * abs(stats[3])
    pe = np.zeros(w0.size, bool)
    at = 0
    for n, s in T.state_shapes(cfg).items():
        num = int(np.prod(s))
        pe[at:at + num] = n in R.POSITION_TABLES
        at += num
    assert np.array_equal(w1[pe], w0[pe]), "a position table moved"
    moved = ~pe
    ratio = 1.0 / (1.0 - B1 ** step) * np.sqrt(1.0 - B2 ** step) * (1 - B1) / np.sqrt(1 - B2)   # |update| / lr at its largest
    scale = clip / (norm + 1e-6) if clip > 0 and norm > clip else 1.0
    summands = np.abs(g * scale) + (np.abs(wd * w0) if opt == "Adam" else 0.0)
    tol = 2.0 ** -20 * np.abs(ref[moved]) + 2.0 ** -20 * LR * max(ratio, 1.0) + (cond * 2.0 ** -21 * summands)[moved]
    err = np.abs(w1[moved] - ref[moved])
    print(f"TRAIN-STEP {tag} {opt} wd {wd} clip {clip} step {step}: norm {norm:.4g} worst err / tol {float((err / tol).max()):.3f} "
          f"mean |dw| {float(np.abs(ref[moved] - w0[moved]).mean()):.3e}")
    assert (err <= tol).all()
    assert np.abs(ref[moved] - w0[moved]).max() > 0.1 * LR           # the step did move the weights


def run_trajectory(name, sd, cfg, batches, opt="Adam", wd=0.0, clip=CLIP, lrs=None):
    """The device's trajectory over `batches` against adam_run in float64, adam_run in float32 the yardstick: the module
    docstring's two assertions; the position tables keep their bits."""
    steps = len(batches)
    lrs = [LR] * steps if lrs is None else lrs
    l64, n64, w64 = R.adam_run(sd, cfg, batches, torch.float64, opt, LR, wd, clip, EPS, lrs=lrs)
    l32, _, w32 = R.adam_run(sd, cfg, batches, torch.float32, opt, LR, wd, clip, EPS, lrs=lrs)
    tr = T.Trainer(sd, cfg, 0)
    stats = [tr.step(*on_device(*b), lr=lrs[s], step=s + 1, optimizer=opt, weight_decay=wd, clip=clip) for s, b in enumerate(batches)]
    ldev = torch.stack(stats).cpu().numpy().astype(np.float64)
    wdev = T.split_blob(tr.weights().cpu().numpy(), cfg)
    tr.close()
    l64 = np.asarray(l64)
    r32 = float((np.abs(np.asarray(l32) - l64) / np.abs(l64)).max())
    rdev = float((np.abs(ldev[:, 3] - l64) / np.abs(l64)).max())
    names = [k for k in w64 if k not in R.POSITION_TABLES]
    moved = np.sqrt(sum(float(((w64[k] - sd[k].double().numpy()) ** 2).sum()) for k in names))
    d32 = np.sqrt(sum(float(((w32[k].astype(np.float64) - w64[k]) ** 2).sum()) for k in names)) / moved
    ddev = np.sqrt(sum(float(((wdev[k].astype(np.float64) - w64[k]) ** 2).sum()) for k in names)) / moved
    print(f"TRAIN-TRAJ {name}: loss rel fp32 CPU {r32:.3e} dev {rdev:.3e}; weights fp32 CPU {d32:.3e} dev {ddev:.3e} "
          f"(dev / CPU {ddev / d32:.2f}); norm rel {float((np.abs(ldev[:, 4] - n64) / np.asarray(n64)).max()):.3e}")
    assert rdev <= max(FACTOR * r32, FLOOR)
    assert ddev <= FACTOR * d32
    for k in R.POSITION_TABLES:
        assert np.array_equal(wdev[k], sd[k].numpy())


TRAJECTORIES = [("k9", 8, 12), ("g5x37", 16, 24)]


@pytest.mark.parametrize("tag,B,steps", TRAJECTORIES)
def test_trajectory(tag, B, steps):
    sd, cfg, codes, lengths, target, stdev = data(tag, 1.3)
    N = codes.shape[0]
    batches = [tuple(a[(s * B + np.arange(B)) % N] for a in (codes, lengths, target, stdev)) for s in range(steps)]
    run_trajectory(tag, sd, cfg, batches)


SCHEDULED_TAG, SCHEDULED_B, SCHEDULED_STEPS = "g5x37", 20, 24
SCHEDULED = [("AdamW", 0.01, CLIP), ("Adam", 0.01, CLIP), ("Adam", 0.0, 0.0)]


def epoch_batches(arrays, B, steps):
    """TrainData.epoch's batches for seed 0 without a directory: per epoch default_rng([0, epoch]).permutation(N) in slices of B, the
    short last one kept -> (the first `steps` batches, their sizes)."""
    N = arrays[0].shape[0]
    out, epoch = [], 0
    while len(out) < steps:
        order = np.random.default_rng([0, epoch]).permutation(N)
        out += [tuple(a[order[i:i + B]] for a in arrays) for i in range(0, N, B)]
        epoch += 1
    out = out[:steps]
    return out, [b[0].shape[0] for b in out]


@pytest.mark.parametrize("opt,wd,clip", SCHEDULED, ids=[f"{o}-wd{w}-clip{c}" for o, w, c in SCHEDULED])
def test_scheduled_trajectory(opt, wd, clip):
    sd, cfg, *arrays = data(SCHEDULED_TAG, 1.3)
    assert arrays[0].shape[0] == 48
    batches, sizes = epoch_batches(arrays, SCHEDULED_B, SCHEDULED_STEPS)
    assert sizes == [20, 20, 8] * 8
    lrs = [T.lr_at("warmup_cosine", s, SCHEDULED_STEPS, 0.25, LR) for s in range(SCHEDULED_STEPS)]
    assert lrs[0] == 0.0 and max(lrs) == LR and 0.0 < lrs[-1] < 0.1 * LR
    run_trajectory(f"{SCHEDULED_TAG} scheduled {opt} wd {wd} clip {clip}", sd, cfg, batches, opt, wd, clip, lrs)
