#!/usr/bin/env python
"""Throughput of the chunk-geometry instance (GPU box): chunks/s and padded samples/s (chunks x max_signal_len) of predict_chunks
in mode "generic-geometry" for every case of tests/_geometry_models.py, each beside mode "generic" at the same sizes and 16 / 250,
with the built-in samplers.  --f16: also mode "generic-geometry-f16" on the same chunks in the same process, and its ratio to
"generic-geometry".  One JSON line per case and mode; the device clock is read with amd-smi where available (read-only).
    python tools/geometry_rate.py [--f16] [chunks] [tag ...]     (default: every case)"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import seq2squiggle_amd as S
from _geometry_models import CASES, geometry_config, geometry_state_dict
from _sized_models import _sinusoid

F16 = "--f16" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--f16"]
B = int(ARGS[0]) if ARGS else 8192


def clock():
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "--json"], capture_output=True, text=True, timeout=20)
        return r.stdout.strip()[:400] if r.returncode == 0 else None
    except (OSError, subprocess.SubprocessError):
        return None


def rate(sd, cfg, mode):
    k, te, ts = int(cfg["seq_kmer"]), int(cfg["max_dna_len"]), int(cfg["max_signal_len"])
    rng = np.random.default_rng(0)
    reads = ["".join(rng.choice(list("ACGT"), 5000)) for _ in range(B * te // 4900 + 1)]
    bases, nv, _ = S.encode_reads(reads, k, te)
    b, n = torch.from_numpy(bases[:B].copy()).cuda(), torch.from_numpy(nv[:B].copy()).cuda()
    eng = S.Engine(sd, cfg, mode=mode)
    p = S.PredictParams(seed=1)
    sig = torch.empty(B, ts, device="cuda"); dur = torch.empty(B, te, dtype=torch.int32, device="cuda")
    eng.predict_chunks(b, n, p, out_signal=sig, out_dur=dur)             # warm-up (grows the workspace)
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < 2.0:
        eng.predict_chunks(b, n, p, out_signal=sig, out_dur=dur, first_global_chunk=reps * B)
        reps += 1
        torch.cuda.synchronize()
    el = time.perf_counter() - t0
    eng.close()
    return {"mode": mode, "max_dna_len": te, "max_signal_len": ts, "chunks_per_call": B, "calls": reps,
            "chunks_per_s": B * reps / el, "padded_samples_per_s": B * reps * ts / el}


print(json.dumps({"device": torch.cuda.get_device_name(0), "clock_before": clock()}))
for tag in (ARGS[1:] or list(CASES)):
    sd, cfg = geometry_state_dict(tag), geometry_config(tag)
    sizes = {k: cfg[k] for k in ("dmodel", "dff", "encoder_heads", "decoder_heads", "pre_layers", "encoder_layers", "decoder_layers")}
    r6 = rate(sd, cfg, "generic-geometry")
    print(json.dumps(dict(tag=tag, **sizes, **r6)), flush=True)
    if F16:
        r7 = rate(sd, cfg, "generic-geometry-f16")
        print(json.dumps(dict(tag=tag, **sizes, **r7, vs_generic_geometry=r7["chunks_per_s"] / r6["chunks_per_s"])), flush=True)
    # the same weights at 16 / 250: position tables of the default sizes (the timing does not depend on their values)
    base = dict(sd, **{"encoders.position_enc": _sinusoid(16, cfg["dmodel"])[None],
                       "decoders.position_enc": _sinusoid(250, cfg["dmodel"])[None]})
    print(json.dumps(dict(tag=tag, **sizes, **rate(base, dict(cfg, max_dna_len=16, max_signal_len=250), "generic"))), flush=True)
print(json.dumps({"clock_after": clock()}))
