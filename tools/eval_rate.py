#!/usr/bin/env python
"""Evaluate against predict throughput (GPU box): chunks/s of Engine.evaluate_chunks (resident inputs: k-mer letters, dwell, targets,
stdevs already on the device) and of Engine.predict_chunks (resident bases, built-in samplers) for the same checkpoint and mode, in the
same process, at B chunks per call after a warm-up call.  Cases: f16x3, f32 and generic on the synthetic k9 checkpoint, and
generic-geometry on r16x500 (tests/_geometry_models.py).  One JSON line per case; the device clock is read with amd-smi after the
runs (read-only), as tools/geometry_rate.py does.
    python tools/eval_rate.py [chunks] [case ...]     (default 65536 chunks, every case)"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import seq2squiggle_amd as S
from seq2squiggle_amd.checkpoint import load_checkpoint

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
CASES = {"f16x3": ("k9", "f16x3"), "f32": ("k9", "f32"), "generic": ("k9", "generic"), "generic-geometry": ("r16x500", "generic-geometry")}


def clock():
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "--json"], capture_output=True, text=True, timeout=20)
        return r.stdout.strip()[:400] if r.returncode == 0 else None
    except (OSError, subprocess.SubprocessError):
        return None


def timed(fn):
    fn(0)                                                  # warm-up (grows the workspaces)
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < 2.0:
        fn(reps + 1)
        reps += 1
        torch.cuda.synchronize()
    return B * reps / (time.perf_counter() - t0), reps


def case(name):
    tag, mode = CASES[name]
    if tag == "k9":
        sd, cfg = load_checkpoint(os.path.join(ROOT, "tests", "golden", "synthetic_k9.ckpt"))
    else:
        import _geometry_models as GM
        sd, cfg = load_checkpoint(GM.checkpoint_path(tag))
    k, te, ts = int(cfg["seq_kmer"]), int(cfg["max_dna_len"]), int(cfg["max_signal_len"])
    eng = S.Engine(sd, cfg, mode=mode)
    rng = np.random.default_rng(0)
    dev = eng.device
    kmers = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (B, te, k))].copy()).to(dev)
    dwell = torch.from_numpy(rng.poisson(ts / te, (B, te)).astype(np.int32)).to(dev)
    target = torch.rand(B, ts, device=dev)
    stdev = torch.rand(B, te, device=dev) * 0.02
    ev, ev_calls = timed(lambda i: eng.evaluate_chunks(kmers, dwell, target, stdev))
    reads = ["".join(rng.choice(list("ACGT"), 5000)) for _ in range(B * te // 4900 + 1)]
    bases, nv, _ = S.encode_reads(reads, k, te)
    b, n = torch.from_numpy(bases[:B].copy()).to(dev), torch.from_numpy(nv[:B].copy()).to(dev)
    sig = torch.empty(B, ts, device=dev)
    dur = torch.empty(B, te, dtype=torch.int32, device=dev)
    p = S.PredictParams(seed=1)
    pr, pr_calls = timed(lambda i: eng.predict_chunks(b, n, p, out_signal=sig, out_dur=dur, first_global_chunk=i * B))
    eng.close()
    return {"case": name, "checkpoint": tag, "mode": mode, "chunks_per_call": B, "evaluate_chunks_per_s": ev, "evaluate_calls": ev_calls,
            "predict_chunks_per_s": pr, "predict_calls": pr_calls, "evaluate_vs_predict": ev / pr}


print(json.dumps({"device": torch.cuda.get_device_name(0)}))
for name in (sys.argv[2:] or list(CASES)):
    print(json.dumps(case(name)), flush=True)
print(json.dumps({"clock_after": clock()}))
