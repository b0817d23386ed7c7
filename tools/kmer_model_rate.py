#!/usr/bin/env python
"""What `predict --kmer-model` costs (GPU box).
    python tools/kmer_model_rate.py kernels [chunks]      (default 32768)
        resident inputs, 20 x (event_stats, kmer_table_accumulate, kmer_model_accumulate) per case: a random genome and an all-A
        genome (every event of the launch adds to ONE row: what the per-workgroup cache is for), on the synthetic k9 checkpoint, on a
        k = 6 model of the same geometry and on a k = 3 one (the cache indexed directly), each on its own predict output; HIP-event
        milliseconds per call and a check of the model's counters against Engine.event_stats reduced on the host.
        Under `rocprofv3 --kernel-trace --stats -- python tools/kmer_model_rate.py kernels` (a run of its own, no counters) the
        trace puts s2s_kmer_model_kernel beside s2s_kmer_table_kernel and s2s_event_stats_kernel; every case dispatches each of the
        three 21 times (event_stats 22), in the order of the printed lines, so the kernel trace splits by case.
    python tools/kmer_model_rate.py e2e [runs] [--parent DIR] [-- extra predict options]      (default 3)
        wall seconds of BASELINE configs[1] (`predict example_lambda_genome.fasta -n 1000 -r 5000 -o x.blow5`, fixed seed) plain and
        with --kmer-model, `runs` times each, interleaved, every run a fresh process, after one warm-up run; checks that the signal
        files hold the same bytes behind the header and reports the size of the model.  --parent DIR: a built checkout of the parent
        commit; its plain run joins the interleaving as `parent_plain` and its file the comparison.
One JSON line per measurement."""
import json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def kernels(B):
    import numpy as np, torch
    import seq2squiggle_amd as S
    from seq2squiggle_amd.checkpoint import load_checkpoint
    from seq2squiggle_amd.chunker import pack_reads
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _geometry_models as GM
    from _kmer_model_ref import fixed_of_slots, reduce_by_code
    from _kmer_table_ref import kmer_codes
    cal = (8192.0, 1400.0, 10.0)
    sd9, cfg9 = load_checkpoint(os.path.join(GOLDEN, "synthetic_k9.ckpt"))
    small = {f"k{k}rate": dict(seed=k, seq_kmer=k, max_dna_len=16, max_signal_len=250, dmodel=16, dff=8, encoder_heads=2, decoder_heads=1,
                               pre_layers=0, encoder_layers=1, decoder_layers=1) for k in (6, 3)}
    engines = {9: S.Engine(sd9, cfg9)}
    for tag, c in small.items():
        engines[c["seq_kmer"]] = S.Engine(GM.geometry_state_dict(tag, small), GM.geometry_config(tag, cases=small), mode="generic")
    rng = np.random.default_rng(0)

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
    for k, eng in engines.items():
        te, dev = eng.t_enc, eng.device
        n_reads = B * te // 4900 + 1
        for genome in ("random", "poly_a"):
            reads = ["".join(rng.choice(list("ACGT"), 5000)) if genome == "random" else "A" * 5000 for _ in range(n_reads)]
            flat, start, nv, _ = pack_reads(reads, k, te)
            flat_d, start_d, nv_d = (torch.from_numpy(np.ascontiguousarray(x[:B] if i else x)).to(dev) for i, x in enumerate((flat, start, nv)))
            out = eng.predict_packed(flat_d, start_d, nv_d, S.PredictParams(seed=1))
            stats = torch.empty(eng.event_stats_layout(B, te)[3], dtype=torch.uint8, device=dev)
            table, model = eng.kmer_table_new(), eng.kmer_model_new()
            ev = timed(lambda: eng.event_stats(out["signal"], out["dur"], *cal, out=stats))
            kt = timed(lambda: eng.kmer_table_accumulate(out["signal"], out["dur"], flat_d, start_d, nv_d, *cal, table))
            km = timed(lambda: eng.kmer_model_accumulate(out["signal"], out["dur"], flat_d, start_d, nv_d, *cal, model))
            # the model's counters (21 calls) against event_stats' sections reduced on the host
            st = {n: v.cpu().numpy() for n, v in eng.event_stats(out["signal"], out["dur"], *cal).items()}
            want = reduce_by_code(*fixed_of_slots(st["seg"], st["sum"], st["sumsq"], te), kmer_codes(flat, start[:B], nv[:B], k, te), k)
            got = model.cpu().numpy()
            print(json.dumps({"k": k, "genome": genome, "chunks": B, "event_stats_ms": ev, "kmer_table_accumulate_ms": kt,
                              "kmer_model_accumulate_ms": km, "model_over_table": km / kt, "rows_hit": int((got[:, 0] > 0).sum()),
                              "n_events": int(got[:, 0].sum()) // 21, "model_equals_21x_reduction": bool(np.array_equal(got, 21 * want))}),
                  flush=True)
    for eng in engines.values():
        eng.close()


def e2e(runs, extra, parent=None):
    d = tempfile.mkdtemp(prefix="s2s-kmer-model-")
    base = [sys.executable, "-m", "seq2squiggle_amd", "predict", os.path.join(GOLDEN, "example_lambda_genome.fasta"), "-n", "1000", "-r", "5000",
            "-m", os.path.join(GOLDEN, "synthetic_k9.ckpt"), "--seed", "7"] + extra
    variants = {"plain": [], "kmer_model": ["--kmer-model", os.path.join(d, "m.model")]}
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
    with open(os.path.join(d, "m.model"), "rb") as f:
        n_rows = f.read().count(b"\n") - 3
    print(json.dumps({"runs": runs, **{f"{n}_s": w for n, w in walls.items()}, "kmer_model_rows": n_rows,
                      "kmer_model_bytes": os.path.getsize(os.path.join(d, "m.model")), "blow5_bytes": len(a),
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
