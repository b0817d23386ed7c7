#!/usr/bin/env python
"""What `--kmer-model-out` costs (GPU box).
    python tools/kmer_model_events_rate.py [--reads P] [--len N] [--kmers K] [--k K ...] [--host-threads T] [--reps R] [--long LOG2]
    [--command READS] [--parent-tree DIR] [--cpu] [--step-timeout S]
Every measurement is a STEP: a child process of this tool under its own time limit; the first step that fails ends the run.  A kernel
step generates P reads of N stored samples whose K k-mers own drawn dwells (the batch of tools/resquiggle_rate.py), copies them up
once and takes S and Q from s2s_event_sums on the device; then, in HIP-event milliseconds, R calls after a warm-up: s2s_event_sums and
s2s_kmer_model_events on the same buffers, with random k-mers and with one k-mer in every slot (an all-A read set: one row), per k;
--host-threads T > 0 also times s2s_kmer_model_events_host (which runs on one thread whatever T) and checks table and counters for
equality.  --long LOG2 adds a step with one read of 2^LOG2 samples (a tenth as many k-mers).  --command READS writes READS of the
reads as a BLOW5 file with a FASTA and a k = 6 model that explain them and takes the WHOLE-PROCESS wall time of `resquiggle`, three
runs each and interleaved: this tree without the option, with it, and -- with --parent-tree DIR, a built checkout of the commit
before -- that tree's, whose OUT must equal this tree's byte for byte (--cpu: these runs take the host path).  One JSON line per
measurement; the device clock is read with amd-smi after the runs."""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from preprocess_rate import dwells  # noqa: E402
from resquiggle_rate import clock  # noqa: E402


def kernel_step(a, P, N, K, tag):
    import ctypes as C
    import numpy as np, torch
    from seq2squiggle_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def check(rc):
        assert rc == 0, (rc, L.s2s_last_error(None))

    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()        # noqa: E731
    p = lambda t: t.data_ptr()                                               # noqa: E731
    x_h = rng.integers(-2000, 2000, P * N).astype(np.int16)
    st_h, ln_h = dwells(rng, P, N, K)
    offs_h, lo_h = np.arange(P + 1, dtype=np.int64) * N, np.arange(P + 1, dtype=np.int64) * K
    gain_h = rng.integers(2_800_000, 3_000_000, P).astype(np.int64)          # range / digitisation around 0.17 pA per count
    shift_h = rng.integers(-70_000, -50_000, P).astype(np.int64)             # offsets around -240 counts
    x, st, ln, offs, lo, gain, shift = (dev(v) for v in (x_h, st_h, ln_h, offs_h, lo_h, gain_h, shift_h))
    S, Q = torch.empty(P * K, dtype=torch.int64, device="cuda"), torch.empty(P * K, dtype=torch.int64, device="cuda")
    t_sums = timed(lambda: check(L.s2s_event_sums(0, stream, p(x), p(offs), p(st), p(ln), p(lo), P, p(S), p(Q))), a.reps)
    base = dict(what=tag, reads=P, samples=N, kmers=K, slots=P * K)
    print(json.dumps(dict(base, kernel="event_sums", ms=round(t_sums, 4))), flush=True)
    Sh, Qh = S.cpu().numpy(), Q.cpu().numpy()
    for k in a.k:
        for sequence in ("random", "all-A"):
            codes_h = (rng.integers(0, 4 ** k, P * K) if sequence == "random" else np.zeros(P * K)).astype(np.int32)
            codes = dev(codes_h)
            table = torch.zeros(4 ** k * 5 + 5 + 4, dtype=torch.int64, device="cuda")
            call = lambda: check(L.s2s_kmer_model_events(0, stream, p(codes), p(ln), p(S), p(Q), p(lo), P, p(gain), p(shift), k, 0,  # noqa: E731
                                                         p(table), p(table) + 8 * (4 ** k * 5 + 5)))
            t = timed(call, a.reps)
            table.zero_()
            call()
            got = table.cpu().numpy()
            row = dict(base, kernel="kmer_model_events", k=k, sequence=sequence, ms=round(t, 4), slots_per_s=round(P * K / t * 1e3),
                       over_event_sums=round(t / t_sums, 3), dropped=got[-4:].tolist())
            if a.host_threads > 0:
                want = np.zeros_like(got)
                q = lambda v: v.ctypes.data                                 # noqa: E731
                t0 = time.perf_counter()
                check(L.s2s_kmer_model_events_host(q(codes_h), q(ln_h), q(Sh), q(Qh), q(lo_h), P, q(gain_h), q(shift_h), k, q(want),
                                                   q(want) + 8 * (4 ** k * 5 + 5), a.host_threads))
                s = time.perf_counter() - t0
                row.update(host_ms=round(s * 1e3, 2), host_threads_asked=a.host_threads, host_over_gpu=round(s * 1e3 / t, 1),
                           equal_to_host=bool(np.array_equal(got, want)))
            print(json.dumps(row), flush=True)


def command_step(a):
    import numpy as np
    from seq2squiggle_amd import resquiggle as RSQ, signal_io, utils as U
    rng = np.random.default_rng(0)
    P, N, K, kk = a.command, a.len, a.kmers, 6
    pa = rng.permutation(4 ** kk) * (60.0 / 4 ** kk) + 60.0              # a model of 4^6 distinct levels, 60 .. 120 pA
    prof = U.get_profile("dna-r10-prom")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "m.model"), "w") as f:
            f.write("#k\t6\nkmer\tlevel_mean\n" + "".join("".join("ACGT"[(c >> (2 * (kk - 1 - t))) & 3] for t in range(kk)) + f"\t{pa[c]:.4f}\n"
                                                          for c in range(4 ** kk)))
        seqs = ["".join(rng.choice(list("ACGT"), K + kk - 1)) for _ in range(P)]
        _, ln_h = dwells(rng, P, N, K)
        sigs = []
        for q, s in enumerate(seqs):
            lev = np.repeat(pa[RSQ.kmer_codes(s, kk)], ln_h[q * K:(q + 1) * K]) + rng.normal(0, 1.5, N)
            sigs.append(np.rint(lev * prof["digitisation"] / prof["range"] - prof["offset_mean"]).astype(np.int16))
        ids = [f"read{q}" for q in range(P)]
        with open(os.path.join(d, "r.fasta"), "w") as f:
            f.write("".join(f">{i}\n{s}\n" for i, s in zip(ids, seqs)))
        w = signal_io.BLOW5Writer(os.path.join(d, "s.blow5"), prof, True, "dna-r10-prom", True)
        w.save_dac(ids, np.concatenate(sigs), np.concatenate([[0], np.cumsum([len(s) for s in sigs])]))
        files = [os.path.join(d, n) for n in ("r.fasta", "s.blow5")]
        trees = ([("parent", os.path.abspath(a.parent_tree), ())] if a.parent_tree else []) + [
            ("without the option", ROOT, ()), ("with the option", ROOT, ("--kmer-model-out", os.path.join(d, "new.model")))]
        wall = {name: [] for name, _, _ in trees}
        for run in range(-1, 3):                                         # (run -1 warms every tree's caches and is not counted)
            for name, tree, extra in trees:
                out = os.path.join(d, name.replace(" ", "_") + ".tsv")
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "resquiggle", *files, "--kmer-model", os.path.join(d, "m.model"),
                                    "-o", out, "--json", *extra, *(["--cpu"] if a.cpu else [])], cwd=tree, capture_output=True, text=True,
                                   timeout=a.step_timeout, env=dict(os.environ, PYTHONPATH=tree))
                s = time.perf_counter() - t0
                assert r.returncode == 0, (name, r.stderr[-2000:])
                if run >= 0:
                    wall[name].append(round(s, 3))
                last = json.loads(r.stdout.strip().splitlines()[-1])
                if extra and run == 2:
                    print(json.dumps(dict(what="command", kmer_model=last["kmer_model"], solve_s=round(last["solve_seconds"], 3))), flush=True)
        outs = {name: open(os.path.join(d, name.replace(" ", "_") + ".tsv"), "rb").read() for name, _, _ in trees}
        print(json.dumps(dict(what="command", reads=P, samples=N, kmers=K, k=kk, wall_s=wall,
                              out_equal=all(v == outs["without the option"] for v in outs.values()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--kmers", type=int, default=5000)
    ap.add_argument("--k", type=int, nargs="+", default=[6, 9])
    ap.add_argument("--host-threads", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--long", type=int, default=0)
    ap.add_argument("--command", type=int, default=0)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "batch":
        return kernel_step(a, a.reads, a.len, a.kmers, "batch")
    if a.step == "long":
        return kernel_step(a, 1, 1 << a.long, (1 << a.long) // 10, "one long read")
    if a.step == "command":
        return command_step(a)
    steps = ["batch"] + (["long"] if a.long else []) + (["command"] if a.command else [])
    for step in steps:                                                   # each in a process of its own, under its own limit
        limit = a.step_timeout * (12 if step == "command" else 1)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--step", step], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(step=step, failed=rc)), flush=True)
            return rc
    print(json.dumps({"clock_after": clock()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
