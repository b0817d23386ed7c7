"""The loop closed once, measured, no bar set: `predict --read-input --events --events-samples` on the six lambda reads of
tests/test_gpu_predict_resquiggle.py with the synthetic k9 checkpoint (the teacher), `preprocess` of the table, `train` from a fresh
initialisation for 300 steps on those chunks, and the four `evaluate` losses of the student before and after and of the teacher.
A teacher-student fit on a handful of reads: it shows that a preprocess directory becomes a checkpoint every later command loads,
nothing about generalisation.  PRINTED (TRAIN-TEACHER-STUDENT ...); asserted only: every loss is finite, and the command's last valid_* record equals
`evaluate` on the checkpoint it wrote."""
import math

import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd import preprocess as PP
from seq2squiggle_amd import train as T
from test_gpu_kmer_model import CKPT
from test_gpu_predict_preprocess import GEOMETRY, run  # noqa: F401

pytestmark = pytest.mark.gpu
STEPS, BATCH = 300, 32


def losses_of(sd, cfg, data):
    eng = S.Engine(sd, cfg, 0, "generic-geometry")
    r, _, _ = EV.evaluate(eng, data)
    eng.close()
    return {k: float(v) for k, v in r.items()}


def test_teacher_student(run, tmp_path):  # noqa: F811
    d = run
    PP.preprocess_table(d / "truth.tsv", tmp_path / "chunks", *GEOMETRY)
    teacher, cfg = S.load_checkpoint(CKPT)
    cfg = dict(cfg, train_batch_size=BATCH, max_epochs=STEPS, optimizer="Adam", weight_decay=0.0, lr=5e-4, lr_schedule="warmup_cosine",
               warmup_ratio=0.01, gradient_clip_val=1.0)
    data = EV.EvalData(str(tmp_path / "chunks"), cfg)
    before = losses_of(T.default_init(cfg, 0), cfg, data)
    out = str(tmp_path / "m" / "student.ckpt")
    lines = []
    recs = T.train_run(str(tmp_path / "chunks"), str(tmp_path / "chunks"), out, cfg, seed=0, max_steps=STEPS, log=lines.append, log_every=0)
    student, _ = S.load_checkpoint(out)
    after = losses_of(student, cfg, data)
    print(f"\nTRAIN-TEACHER-STUDENT {data.n} chunks, {STEPS} steps of {BATCH}, {len(recs)} epochs")
    for name, v in (("student before", before), ("student after", after), ("teacher", losses_of(teacher, cfg, data))):
        print(f"TRAIN-TEACHER-STUDENT {name}: " + " ".join(f"{k} {x:.6g}" for k, x in v.items()))
    assert all(math.isfinite(x) for v in (before, after) for x in v.values())
    assert {k: recs[-1][k] for k in after} == after                  # the last valid_* line is the written checkpoint's
