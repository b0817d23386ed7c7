"""Students: checkpoints the project's own trainer produced, as test inputs (tests/test_gpu_trained.py,
tests/test_gpu_train_teacher_student.py, tests/test_gpu_magnitudes.py).

Each student is trained once per pytest process, on the GPU, by seq2squiggle_amd.train.train_run; the trainer is bit-deterministic
(include/s2s_hip.h: s2s_trainer_step), so a student is a fixed input on a given machine.  Nothing is committed: no checkpoint under
tests/golden/.

  k9      T.default_init(cfg, 0) of the synthetic k9 checkpoint's config; the chunks `preprocess` makes of the table `predict --events`
          wrote for six lambda reads (predict_run, the body of the `run` fixture, and GEOMETRY of
          tests/test_gpu_predict_preprocess.py); 300 steps, B = 32, Adam,
          lr 5e-4, warm-up cosine, clip 1.0 -- the teacher-student fit of tests/test_gpu_train_teacher_student.py.
  k9_far  the same start and chunks, a hotter and longer recipe (RECIPES), so that the weights move further.  16 / 250 like k9: the tuned
          instances load both.
  g5x37   the g5x37 evaluation golden's checkpoint and its 48 rows; 300 steps, B = 16, AdamW with weight decay 0.01.  Off 16 / 250
          (te 5, T below a wave): only the geometry instances load it.

student(name, request) -> dict(name, sd, cfg, start (the weights training began from), rows (the training chunks in the layout of
tests/_eval_data.py: codes, lengths, targets, stdevs [, kind]), data_dir, checkpoint, records (train_run's per-epoch records),
recipe, seconds (train_run on the wall)).  `request` is the calling test's: a builder takes its temporary directory from it."""
import time

import numpy as np
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd import preprocess as PP
from seq2squiggle_amd import train as T
from oracle import s2s_oracle as O
import _eval_data as ED

SCHEDULE = dict(lr_schedule="warmup_cosine", warmup_ratio=0.01, gradient_clip_val=1.0)
RECIPES = {
    "k9": dict(steps=300, batch=32, optimizer="Adam", weight_decay=0.0, lr=5e-4),
    "k9_far": dict(steps=600, batch=32, optimizer="Adam", weight_decay=0.0, lr=1e-2),      # chosen in LABNOTES.md round 43
    "g5x37": dict(steps=300, batch=16, optimizer="AdamW", weight_decay=0.01, lr=5e-4),
}
NAMES = tuple(RECIPES)
TUNED_GEOMETRY = ("k9", "k9_far")                        # 16 / 250: every instance loads them

_CACHE = {}


def recipe_config(cfg, name, n_chunks):
    r = RECIPES[name]
    epochs = -(-r["steps"] // -(-n_chunks // r["batch"]))
    return dict(cfg, train_batch_size=r["batch"], max_epochs=epochs, optimizer=r["optimizer"], weight_decay=r["weight_decay"], lr=r["lr"],
                **SCHEDULE)


def rows_of(data_dir, cfg):
    """A preprocess directory -> the layout of tests/_eval_data.py (letter codes 0-4, 5 for an all-zero one-hot row)."""
    data = EV.EvalData(str(data_dir), cfg)
    cat = {kind: np.concatenate([np.asarray(p[kind]) for p in data.parts]) for kind in ("chunks", "chunks_lengths", "targets", "stdevs")}
    hot = cat["chunks"].reshape(data.n, data.te, data.k, 5) != 0
    codes = np.where(hot.any(-1), hot.argmax(-1), 5).astype(np.uint8)
    return dict(codes=codes, lengths=cat["chunks_lengths"].astype(np.int64), targets=cat["targets"].reshape(data.n, data.ts),
                stdevs=cat["stdevs"])


def _train(name, data_dir, out_dir, cfg, init=None):
    out = str(out_dir / f"student_{name}.ckpt")
    r = RECIPES[name]
    t0 = time.perf_counter()
    recs = T.train_run(str(data_dir), str(data_dir), out, cfg, init=init, seed=0, max_steps=r["steps"], log=lambda s: None, log_every=0)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    sd, _ = S.load_checkpoint(out)
    print(f"\nTRAINED {name}: {r['steps']} steps of {r['batch']}, {r['optimizer']} lr {r['lr']:g} weight decay {r['weight_decay']:g}, "
          f"{len(recs)} epochs, {seconds:.2f} s")
    return dict(name=name, sd=sd, cfg=cfg, data_dir=str(data_dir), checkpoint=out, records=recs, recipe=r, seconds=seconds)


def _k9_chunks(request):
    if "k9 chunks" not in _CACHE:
        from test_gpu_kmer_model import CKPT
        from test_gpu_predict_preprocess import GEOMETRY, predict_run
        tmp = request.getfixturevalue("tmp_path_factory").mktemp("students_k9")
        d = predict_run(tmp)
        PP.preprocess_table(d / "truth.tsv", tmp / "chunks", *GEOMETRY)
        _, cfg = S.load_checkpoint(CKPT)
        _CACHE["k9 chunks"] = (tmp, cfg, rows_of(tmp / "chunks", cfg))
    return _CACHE["k9 chunks"]


def _build_k9(name, request):
    tmp, cfg, rows = _k9_chunks(request)
    cfg = recipe_config(cfg, name, rows["codes"].shape[0])
    st = _train(name, tmp / "chunks", tmp / name, cfg)
    st.update(start=T.default_init(cfg, 0), rows=rows)
    return st


def _build_g5x37(name, request):
    g = ED.load("g5x37")
    tmp = request.getfixturevalue("tmp_path_factory").mktemp("students_g5x37")
    start, cfg = S.load_checkpoint(ED.checkpoint("g5x37"))
    cfg = recipe_config(cfg, name, g["codes"].shape[0])
    ED.write_dir(g, str(tmp / "chunks"))
    st = _train(name, tmp / "chunks", tmp / name, cfg, init=ED.checkpoint("g5x37"))
    st.update(start=start, rows={k: g[k] for k in ("codes", "lengths", "targets", "stdevs", "kind")})
    return st


def student(name, request):
    if name not in _CACHE:
        _CACHE[name] = (_build_g5x37 if name == "g5x37" else _build_k9)(name, request)
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------ how far a student moved
FAMILIES = {"q/k": ("w_qs.weight", "w_ks.weight"), "v/fc": ("w_vs.weight", "fc.weight"), "ffn": ("w_1.weight", "w_2.weight"),
            "embedding": ("src_emb.weight",), "heads": ("layer.0.weight", "layer.3.weight"), "out": ("out_linear.weight",)}
QUANTILES = (0.5, 0.9, 0.99, 1.0)


def attention_row_maxima(sd, cfg, codes, inject_g):
    """The largest attention probability of every row of every head of every block, from the fp64 oracle (noise off): the oracle's
    `taps` hold magnitudes only, so torch.softmax is wrapped for the length of this one call.  -> float64 [rows]."""
    seen = []
    real = torch.softmax

    def recording(x, dim, *a, **kw):
        out = real(x, dim, *a, **kw)
        seen.append(out.max(dim=dim).values.reshape(-1).numpy().copy())
        return out

    torch.softmax = recording
    try:
        O.predict_chunks(sd, cfg, codes, O.PredictParams(noise_std=0.0), inject_g=inject_g, dtype=torch.float64)
    finally:
        torch.softmax = real
    return np.concatenate(seen)


def movement(sd, start, cfg, codes, inject_g, taps):
    """The figures LABNOTES.md records per student, from the weights and the fp64 oracle alone (no GPU output): per weight family
    max |w| now and at the start, the LayerNorm gain and bias range, the ranges of conc / rate / sigma on `codes`, the largest tapped
    intermediate and quantiles of the largest attention probability per row.  -> dict of printable values."""
    def fam(w, suffixes):
        return max(float(v.abs().max()) for k, v in w.items() if k.endswith(suffixes))
    out = {f"max|w| {n}": f"{fam(sd, s):.3g} (start {fam(start, s):.3g})" for n, s in FAMILIES.items()}
    gains = torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith("layer_norm.weight")])
    biases = torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith("layer_norm.bias")])
    out["LayerNorm gain"] = f"{float(gains.min()):.4f} .. {float(gains.max()):.4f}"
    out["LayerNorm bias"] = f"{float(biases.min()):+.4f} .. {float(biases.max()):+.4f}"
    sd64 = {k: v.double() for k, v in sd.items()}
    _, emb = O.encoder(sd64, cfg, O.one_hot(codes, torch.float64))
    conc, rate = O.duration_params(sd64, emb)
    for n, t in (("conc", conc), ("rate", rate), ("sigma", O.noise_sampler(sd64, emb))):
        out[n] = f"{float(t.min()):.4g} .. {float(t.max()):.4g}"
    out["largest intermediate"] = f"{max(taps.values()):.4g} ({max(taps, key=taps.get)})"
    p = attention_row_maxima(sd, cfg, codes, inject_g)
    out["attention row max (q50 / q90 / q99 / max)"] = " / ".join(f"{float(np.quantile(p, q)):.4f}" for q in QUANTILES)
    dist = float(np.sqrt(sum(float(((sd[k] - start[k]).double() ** 2).sum()) for k in sd)))
    norm = float(np.sqrt(sum(float((start[k].double() ** 2).sum()) for k in sd if not k.endswith("position_enc"))))
    out["||w - start|| / ||start||"] = f"{dist / norm:.4f}"
    return out
