"""The device-side refusals of the trainer's entries (B < 1, NULL pointers, a step below 1, betas / eps out of range, inputs on
another device where there is one), each with its message and without touching the weights; and the trainer alone in a fresh
process at a shape whose staged forward attention needs more than 64 KiB of dynamic LDS (dmodel 64 with 2 decoder heads at 250
samples: head_dim 32, 65,960 B), where no generic Engine has raised the kernel's limit before it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from seq2squiggle_amd import _lib, train as T
from seq2squiggle_amd.checkpoint import load_checkpoint
import _eval_data as ED
import _train_ref as R
from test_gpu_train_gradients import on_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_leave_the_weights_alone():
    g = ED.load("g5x37")
    sd, cfg = load_checkpoint(ED.checkpoint("g5x37"))
    target, stdev = ED.scaled(g, float(cfg["scaling_max_value"]))
    kmers, dwell, tg, sv = on_device(g["codes"][:4], g["lengths"][:4], target[:4], stdev[:4])
    tr = T.Trainer(sd, cfg, 0)
    L = _lib.lib()
    w0 = tr.weights().clone()
    loss = torch.empty(4, 3, device="cuda")
    grad = torch.empty(tr.n_floats, device="cuda")
    stats = torch.empty(5, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
    good = _lib.S2SAdam(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=0.0, clip=1.0, decoupled=0, step=1)

    def refused(rc, text):
        assert rc == -1 and text in L.s2s_trainer_last_error(tr._t).decode(), (rc, L.s2s_trainer_last_error(tr._t))

    for B in (0, -3):
        refused(L.s2s_trainer_gradients(tr._t, None, p(kmers), p(dwell), p(tg), p(sv), B, p(loss), p(grad)), "B < 1")
        refused(L.s2s_trainer_step(tr._t, None, p(kmers), p(dwell), p(tg), p(sv), B, C.byref(good), p(stats)), "B < 1")
    for hole in range(6):
        a = [p(kmers), p(dwell), p(tg), p(sv), p(loss), p(grad)]
        a[hole] = None
        refused(L.s2s_trainer_gradients(tr._t, None, a[0], a[1], a[2], a[3], 4, a[4], a[5]), "NULL argument")
    refused(L.s2s_trainer_step(tr._t, None, p(kmers), p(dwell), p(tg), p(sv), 4, None, p(stats)), "NULL argument")
    refused(L.s2s_trainer_step(tr._t, None, p(kmers), p(dwell), p(tg), p(sv), 4, C.byref(good), None), "NULL argument")
    refused(L.s2s_trainer_weights(tr._t, None, None), "NULL argument")
    for field, value, text in (("step", 0, "step counts from 1"), ("beta1", 1.0, "betas"), ("beta2", -0.1, "betas"), ("eps", 0.0, "eps")):
        bad = _lib.S2SAdam(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=0.0, clip=1.0, decoupled=0, step=1)
        setattr(bad, field, value)
        refused(L.s2s_trainer_step(tr._t, None, p(kmers), p(dwell), p(tg), p(sv), 4, C.byref(bad), p(stats)), text)
    refused(L.s2s_trainer_set_memory(tr._t, 0), "at least 1 byte")
    if torch.cuda.device_count() > 1:
        far = kmers.to("cuda:1")
        refused(L.s2s_trainer_gradients(tr._t, None, p(far), p(dwell), p(tg), p(sv), 4, p(loss), p(grad)), "another device")
    with pytest.raises(ValueError, match="optimizer 'SGD'"):
        tr.step(kmers, dwell, tg, sv, lr=5e-4, step=1, optimizer="SGD")
    with pytest.raises(ValueError, match="dwell must be contiguous"):
        tr.gradients(kmers, dwell.long(), tg, sv)
    torch.cuda.synchronize()
    assert torch.equal(tr.weights(), w0)
    tr.close()


FRESH = """
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch
import seq2squiggle_amd as S
from seq2squiggle_amd import train as T
sd, cfg = S.load_checkpoint({ckpt!r})
cfg = dict(cfg, decoder_heads=2)
sd = T.default_init(cfg, 2)
rng = np.random.default_rng(2)
B, k, te, ts = 5, cfg["seq_kmer"], cfg["max_dna_len"], cfg["max_signal_len"]
kmers = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (B, te, k))].copy()).cuda()
dwell = torch.from_numpy(rng.integers(0, 30, (B, te)).astype(np.int32)).cuda()
target = torch.rand(B, ts, device="cuda")
stdev = torch.rand(B, te, device="cuda") * 0.02
tr = T.Trainer(sd, cfg, 0)                       # no Engine exists yet in this process
out = tr.gradients(kmers, dwell, target, stdev)
torch.cuda.synchronize()
eng = S.Engine(sd, cfg, 0, "generic-geometry")
ev = eng.evaluate_chunks(kmers, dwell, target, stdev)
assert torch.equal(out["loss"], ev["loss"]), (out["loss"], ev["loss"])
assert bool(torch.isfinite(out["grad"]).all()) and float(out["grad"].abs().max()) > 0
print("FRESH_OK")
"""


def test_trainer_alone_in_a_fresh_process_above_64_kib_of_staged_lds(tmp_path):
    script = tmp_path / "fresh.py"
    script.write_text(FRESH.format(root=ROOT, ckpt=ED.checkpoint("k9")))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FRESH_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
