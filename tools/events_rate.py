#!/usr/bin/env python
"""What `predict --events` costs (GPU box).
    python tools/events_rate.py kernels [chunks]      (default 32768)
        one predict launch of `chunks` chunks on the synthetic k9 checkpoint, then 20 x (export_reads, align_chunks, event_stats) on
        its signal / dur: HIP-event milliseconds per call of each.  Under `rocprofv3 --kernel-trace --stats -- python
        tools/events_rate.py kernels` the stats table puts s2s_event_stats_kernel beside s2s_align_kernel, which streams the same signal.
    python tools/events_rate.py e2e [runs] [--parent DIR] [-- extra predict options]      (default 3)
        wall seconds of BASELINE configs[1] (`predict example_lambda_genome.fasta -n 1000 -r 5000 -o x.blow5`, fixed seed) plain, with
        --events and with --events --events-samples, `runs` times each, interleaved, every run a fresh process, after one warm-up
        run; checks that the signal files hold the same bytes behind the header and reports the size of the tables.  --parent DIR:
        a built checkout of the parent commit; its plain run joins the interleaving as `parent_plain` and its file the comparison.
One JSON line per measurement."""
import json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def kernels(B):
    import numpy as np, torch
    import seq2squiggle_amd as S
    from seq2squiggle_amd.checkpoint import load_checkpoint
    sd, cfg = load_checkpoint(os.path.join(GOLDEN, "synthetic_k9.ckpt"))
    eng = S.Engine(sd, cfg)
    k, te = int(cfg["seq_kmer"]), eng.t_enc
    rng = np.random.default_rng(0)
    reads = ["".join(rng.choice(list("ACGT"), 5000)) for _ in range(B * te // 4900 + 1)]
    bases, nv, first = S.encode_reads(reads, k, te)
    dev = eng.device
    out = eng.predict_chunks(torch.from_numpy(bases[:B].copy()).to(dev), torch.from_numpy(nv[:B].copy()).to(dev), S.PredictParams(seed=1))
    first = torch.from_numpy(np.minimum(first, B).astype(np.int32)).to(dev)
    cal = (8192.0, 1400.0, 10.0)
    dac = torch.empty(B * eng.t_dec, dtype=torch.int16, device=dev)
    seg = torch.empty(B, te + 1, dtype=torch.uint16, device=dev)
    stats = torch.empty(eng.event_stats_layout(B, te)[3], dtype=torch.uint8, device=dev)

    def timed(fn, reps=20):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps
    ex = timed(lambda: eng.export_reads(out["signal"], first, *cal, want_pa=False, out_dac=dac))
    al = timed(lambda: eng.align_chunks(out["signal"], out["dur"], out=seg))
    ev = timed(lambda: eng.event_stats(out["signal"], out["dur"], *cal, out=stats))
    got = eng.event_stats(out["signal"], out["dur"], *cal, out=stats)
    rows = got["seg"].cpu().numpy().astype(np.int64)
    print(json.dumps({"chunks": B, "export_reads_ms": ex, "align_chunks_ms": al, "event_stats_ms": ev, "stored_samples": int(rows.sum()),
                      "counts_equal_align_chunks": bool(np.array_equal(rows, seg.cpu().numpy().astype(np.int64))),
                      "kmers_with_samples": int((rows[:, :te] > 0).sum()), "sum_of_sums": int(got["sum"].sum().item())}))
    eng.close()


def e2e(runs, extra, parent=None):
    d = tempfile.mkdtemp(prefix="s2s-events-")
    base = [sys.executable, "-m", "seq2squiggle_amd", "predict", os.path.join(GOLDEN, "example_lambda_genome.fasta"), "-n", "1000", "-r", "5000",
            "-m", os.path.join(GOLDEN, "synthetic_k9.ckpt"), "--seed", "7"] + extra
    variants = {"plain": [], "events": ["--events", os.path.join(d, "e.tsv")],
                "events_samples": ["--events", os.path.join(d, "es.tsv"), "--events-samples"]}
    if parent:
        variants = {"parent_plain": [], **variants}
    walls = {name: [] for name in variants}
    for i in range(runs + 1):                                   # (run 0: the warm-up, not reported)
        for name, opts in variants.items():
            out = os.path.join(d, f"{name}.blow5")
            t0 = time.perf_counter()
            r = subprocess.run(base + ["-o", out] + opts, cwd=parent if name == "parent_plain" else ROOT, capture_output=True, text=True,
                               timeout=900)
            if i:
                walls[name].append(time.perf_counter() - t0)
            if r.returncode != 0:
                print(r.stderr[-3000:], file=sys.stderr)
                sys.exit(r.returncode)
    a, *others = (open(os.path.join(d, f"{n}.blow5"), "rb").read() for n in variants)
    hdr = 64 + 4 + int.from_bytes(a[64:68], "little")
    with open(os.path.join(d, "e.tsv"), "rb") as f:
        n_rows = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b"")) - 1
    print(json.dumps({"runs": runs, **{f"{n}_s": w for n, w in walls.items()}, "event_rows": n_rows,
                      "events_bytes": os.path.getsize(os.path.join(d, "e.tsv")),
                      "events_samples_bytes": os.path.getsize(os.path.join(d, "es.tsv")), "blow5_bytes": len(a),
                      "records_identical": all(a[hdr:] == o[hdr:] for o in others)}))
    import shutil
    shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if what == "kernels":
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 32768)
    elif what == "e2e":
        rest = sys.argv[2:]
        extra = rest[rest.index("--") + 1:] if "--" in rest else []
        rest = rest[:rest.index("--")] if "--" in rest else rest
        parent = None
        if "--parent" in rest:
            parent = os.path.abspath(rest.pop(rest.index("--parent") + 1))
            rest.remove("--parent")
        e2e(int(rest[0]) if rest else 3, extra, parent)
    else:
        sys.exit(__doc__)
