#!/usr/bin/env python
"""The end of a predict launch (GPU box): per timed launch the kernel time from the handle's events against how long its
workgroups ran (Engine.stats: wg_span_ms_mean / _max / _min, thread 0's span per workgroup on the 100 MHz clock).  A launch lasts
as long as its slowest workgroup: gap = kernel - mean span is what a perfect split of the same work would save.

    python tools/tail_probe.py [--chunks N ...] [--steps K] [--warmup W] [--mode f16x3] [--schedule auto|static|dynamic]

Default --chunks: the headline workload (bench.py: 1000 reads x 5000 nt = 312,000 chunks).  Prints one line per launch, then ONE
JSON line with the per-size medians."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import seq2squiggle_amd as S  # noqa: E402
import bench  # noqa: E402

HEADLINE = 1000 * bench.CHUNKS_PER_READ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="*", default=[HEADLINE])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="f16x3")
    ap.add_argument("--schedule", default=None, choices=["auto", "static", "dynamic"])
    a = ap.parse_args()
    sd, cfg = S.load_checkpoint(os.path.join(ROOT, "tests", "golden", "synthetic_k9.ckpt"))
    eng = S.Engine(sd, cfg, mode=a.mode)
    if a.schedule:
        eng.schedule = a.schedule
    schedule = eng.schedule if hasattr(eng, "schedule") else "static"
    n_max = max(a.chunks)
    bases, nv, _ = S.encode_reads(bench.make_reads(-(-n_max // bench.CHUNKS_PER_READ), 1234), cfg["seq_kmer"])   # the headline's reads
    b_all, n_all = torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda()
    params = S.PredictParams(seed=42)
    rows = []
    for B in a.chunks:
        b, n = b_all[:B].contiguous(), n_all[:B].contiguous()
        sig = torch.empty(B, 250, dtype=torch.float32, device="cuda")
        dur = torch.empty(B, 16, dtype=torch.int32, device="cuda")
        for _ in range(a.warmup):
            eng.predict_chunks(b, n, params, out_signal=sig, out_dur=dur)
        torch.cuda.synchronize()
        eng.stats()
        eng.set_profiling(True)
        per = []
        for i in range(a.steps):
            eng.predict_chunks(b, n, params, out_signal=sig, out_dur=dur)
            ms, nl, _ = eng.kernel_ms()                 # (waits for the launch)
            st = eng.stats()
            assert nl == 1 and st["chunks"] == B
            row = {"kernel_ms": ms, "span_mean_ms": st["wg_span_ms_mean"], "span_max_ms": st["wg_span_ms_max"],
                   "span_min_ms": st["wg_span_ms_min"], "gap_ms": ms - st["wg_span_ms_mean"],
                   "clock_ghz": st["in_kernel_clock_ghz"], "dynamic": st["chunks_on_dynamic_schedule"] == B}
            per.append(row)
            print(f"chunks {B:7d} launch {i:2d}: kernel {ms:8.3f} ms  span mean {row['span_mean_ms']:8.3f} max {row['span_max_ms']:8.3f} "
                  f"min {row['span_min_ms']:8.3f}  gap {row['gap_ms']:6.3f} ms = {100 * row['gap_ms'] / ms:5.2f} %  "
                  f"clock {row['clock_ghz']:.4f} GHz  {'claims' if row['dynamic'] else 'static split'}", flush=True)
        eng.set_profiling(False)
        med = {k: statistics.median(r[k] for r in per) for k in ("kernel_ms", "span_mean_ms", "span_max_ms", "span_min_ms", "gap_ms", "clock_ghz")}
        rows.append(dict(med, chunks=B, launches=a.steps, gap_frac=med["gap_ms"] / med["kernel_ms"],
                         max_minus_min_ms=med["span_max_ms"] - med["span_min_ms"], dynamic=all(r["dynamic"] for r in per)))
    eng.close()
    print(json.dumps({"tool": "tail_probe", "mode": a.mode, "schedule": schedule, "device": torch.cuda.get_device_name(0),
                      "medians": rows}))


if __name__ == "__main__":
    main()
