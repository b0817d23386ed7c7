#!/usr/bin/env python
"""Throughput of the size-generic instance (GPU box): chunks/s of predict_chunks in mode "generic" for the shipped size
(tests/golden/synthetic_k9.ckpt) and every size case of tests/_sized_models.py, next to the tuned "f32" instance at the default size, with
the built-in samplers.  One JSON line per case; the device clock is read with amd-smi where available (read-only).
    python tools/generic_rate.py [chunks] [tag:mode ...]     (default: every case below)"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import seq2squiggle_amd as S
from _sized_models import checkpoint_path

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32768


def clock():
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "--json"], capture_output=True, text=True, timeout=20)
        return r.stdout.strip()[:400] if r.returncode == 0 else None
    except (OSError, subprocess.SubprocessError):
        return None


def rate(tag, mode):
    sd, cfg = S.load_checkpoint(os.path.join(ROOT, "tests", "golden", f"synthetic_{tag}.ckpt") if tag == "k9" else checkpoint_path(tag))
    k = int(cfg["seq_kmer"])
    rng = np.random.default_rng(0)
    reads = ["".join(rng.choice(list("ACGT"), 5000)) for _ in range(B // 312 + 1)]
    bases, nv, _ = S.encode_reads(reads, k)
    b, n = torch.from_numpy(bases[:B].copy()).cuda(), torch.from_numpy(nv[:B].copy()).cuda()
    eng = S.Engine(sd, cfg, mode=mode)
    p = S.PredictParams(seed=1)
    sig = torch.empty(B, 250, device="cuda"); dur = torch.empty(B, 16, dtype=torch.int32, device="cuda")
    eng.predict_chunks(b, n, p, out_signal=sig, out_dur=dur)             # warm-up (grows the generic workspace)
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < 2.0:
        eng.predict_chunks(b, n, p, out_signal=sig, out_dur=dur, first_global_chunk=reps * B)
        reps += 1
        torch.cuda.synchronize()
    el = time.perf_counter() - t0
    eng.close()
    return {"tag": tag, "mode": mode, "dmodel": cfg["dmodel"], "dff": cfg["dff"], "heads": [cfg["encoder_heads"], cfg["decoder_heads"]],
            "layers": [cfg["pre_layers"], cfg["encoder_layers"], cfg["decoder_layers"]], "chunks_per_call": B, "calls": reps,
            "chunks_per_s": B * reps / el}


print(json.dumps({"device": torch.cuda.get_device_name(0), "clock_before": clock()}))
CASES = [("k9", "f32")] + [(t, m) for t in ("k9", "d32", "d128", "d512") for m in ("generic", "generic-f16")]
for tag, mode in ([tuple(a.split(":", 1)) for a in sys.argv[2:]] or CASES):
    print(json.dumps(rate(tag, mode)), flush=True)
print(json.dumps({"clock_after": clock()}))
