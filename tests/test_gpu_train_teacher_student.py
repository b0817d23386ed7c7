"""The loop closed once, measured, no bar set: `predict --read-input --events --events-samples` on the six lambda reads of
tests/test_gpu_predict_resquiggle.py with the synthetic k9 checkpoint (the teacher), `preprocess` of the table, `train` from a fresh
initialisation for 300 steps on those chunks, and the four `evaluate` losses of the student before and after and of the teacher.
A teacher-student fit on a handful of reads: it shows that a preprocess directory becomes a checkpoint every later command loads,
nothing about generalisation.  PRINTED (TRAIN-TEACHER-STUDENT ...); asserted only: every loss is finite, and the command's last valid_* record equals
`evaluate` on the checkpoint it wrote.

The fit itself is tests/_trained.py's student "k9", built once per process: tests/test_gpu_trained.py holds every compute mode to
its parity bounds on the weights this test used to throw away."""
import math

import pytest

import seq2squiggle_amd as S
from seq2squiggle_amd import evaluate as EV
from test_gpu_kmer_model import CKPT
import _trained as TR

pytestmark = pytest.mark.gpu


def losses_of(sd, cfg, data):
    eng = S.Engine(sd, cfg, 0, "generic-geometry")
    r, _, _ = EV.evaluate(eng, data)
    eng.close()
    return {k: float(v) for k, v in r.items()}


def test_teacher_student(request):
    st = TR.student("k9", request)
    cfg, recs, recipe = st["cfg"], st["records"], st["recipe"]
    teacher, _ = S.load_checkpoint(CKPT)
    data = EV.EvalData(st["data_dir"], cfg)
    before = losses_of(st["start"], cfg, data)
    student, _ = S.load_checkpoint(st["checkpoint"])
    after = losses_of(student, cfg, data)
    print(f"\nTRAIN-TEACHER-STUDENT {data.n} chunks, {recipe['steps']} steps of {recipe['batch']}, {len(recs)} epochs")
    for name, v in (("student before", before), ("student after", after), ("teacher", losses_of(teacher, cfg, data))):
        print(f"TRAIN-TEACHER-STUDENT {name}: " + " ".join(f"{k} {x:.6g}" for k, x in v.items()))
    assert all(math.isfinite(x) for v in (before, after) for x in v.values())
    assert {k: recs[-1][k] for k in after} == after                  # the last valid_* line is the written checkpoint's
