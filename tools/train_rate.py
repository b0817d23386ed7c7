#!/usr/bin/env python
"""Training against evaluate throughput (GPU box): steps/s and chunks/s of Trainer.step (s2s_trainer_step: forward with the tape,
backward, norm, clip, Adam; resident inputs) beside Engine.evaluate_chunks on a generic-geometry engine of the same weights, in the
same process, at B chunks per call after a warm-up call, and the step-to-forward time ratio.  Cases: the synthetic k9 checkpoint
and the sized / geometry models of the tests (d32, d128, d512 of tests/_sized_models.py; r16x500, hd96s, g64x1024, hd208).  One JSON line per case; the device clock is
read with amd-smi after the runs (read-only), as tools/eval_rate.py does.  With --kernels the script runs itself once more under
`rocprofv3 --kernel-trace --stats` (a run of its own, one case, fresh process) and prints where the trace landed.
    python tools/train_rate.py [chunks] [case ...] [--kernels CASE]     (default 512 chunks, every case)"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import seq2squiggle_amd as S
from seq2squiggle_amd import train as T
from seq2squiggle_amd.checkpoint import load_checkpoint

CASES = ("k9", "d32", "d128", "d512", "r16x500", "hd96s", "g64x1024", "hd208")


def clock():
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "--json"], capture_output=True, text=True, timeout=20)
        return r.stdout.strip()[:400] if r.returncode == 0 else None
    except (OSError, subprocess.SubprocessError):
        return None


def timed(fn, B, seconds=1.5):
    fn(0)                                                  # warm-up (grows the workspaces)
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 3 or time.perf_counter() - t0 < seconds:
        fn(reps + 1)
        reps += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return reps / dt, B * reps / dt


def case(tag, B):
    import _eval_data as ED
    import _sized_models as SM
    sd, cfg = load_checkpoint(SM.checkpoint_path(tag) if tag in SM.CASES else ED.checkpoint(tag))
    k, te, ts = int(cfg["seq_kmer"]), int(cfg["max_dna_len"]), int(cfg["max_signal_len"])
    rng = np.random.default_rng(0)
    tr = T.Trainer(sd, cfg, 0)
    eng = S.Engine(sd, cfg, 0, "generic-geometry")
    dev = tr.device
    kmers = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (B, te, k))].copy()).to(dev)
    dwell = torch.from_numpy(rng.poisson(ts / te, (B, te)).astype(np.int32)).to(dev)
    target = torch.rand(B, ts, device=dev)
    stdev = torch.rand(B, te, device=dev) * 0.02
    stats = torch.empty(5, device=dev)
    ev_calls, ev_chunks = timed(lambda i: eng.evaluate_chunks(kmers, dwell, target, stdev), B)
    st_calls, st_chunks = timed(lambda i: tr.step(kmers, dwell, target, stdev, lr=1e-6, step=i + 1, clip=1.0, out=stats), B)
    row = dict(case=tag, chunks=B, micro_batch=tr.micro_batch(B), dmodel=cfg["dmodel"], dff=cfg["dff"], te=te, ts=ts,
               steps_per_s=st_calls, train_chunks_per_s=st_chunks, evaluate_chunks_per_s=ev_chunks, step_over_forward=ev_chunks / st_chunks)
    tr.close()
    eng.close()
    return row


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--kernels" in args:
        tag = args[args.index("--kernels") + 1]
        import tempfile
        out = tempfile.mkdtemp(prefix=f"train_rate_kernels_{tag}_")      # (outside the tree: traces are not source)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "64", tag]
        print(json.dumps(dict(kernels=tag, rc=subprocess.run(cmd, timeout=600).returncode, out=out)))
        sys.exit(0)
    B = int(args[0]) if args and args[0].isdigit() else 512
    names = [a for a in args if a in CASES] or CASES
    for name in names:
        print(json.dumps(case(name, B)), flush=True)
    print(json.dumps(dict(clock=clock())))
