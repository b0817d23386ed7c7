#!/usr/bin/env python
"""What `preprocess` packs per second (GPU box).
    python tools/preprocess_rate.py [--reads P] [--len N] [--kmers K] [--geometry TE TS KMER] [--host-threads T] [--reps R]
    [--long LOG2] [--command READS]
P reads of N stored samples whose K k-mers own drawn dwells (every sample belongs to one k-mer) are generated on the host and copied
up once; S and Q come from s2s_event_sums on the device.  In HIP-event milliseconds, R calls after a warm-up: s2s_chunk_pack with the
raw source -> chunks/s and output bytes/s (per kept chunk te k 5 fp16 + te int64 + ts fp32 + int64 + te fp32), beside the copy
bandwidth the part reaches (6.29 TB/s, a float4 copy).  --host-threads T > 0 also times s2s_chunk_pack_host on T threads and checks
every output for equality.  --long LOG2 adds one read of 2^LOG2 samples (a tenth as many k-mers).  --command READS writes READS of the
reads as a BLOW5 file with a FASTA and a k = 6 model that explain them and runs, on the wall clock, `resquiggle --chunks` against
`resquiggle --samples` followed by `preprocess`: solve, pack, parse and write seconds.  One JSON line per measurement; the device clock
is read with amd-smi after the runs."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resquiggle_rate import clock  # noqa: E402

COPY_BANDWIDTH = 6.29e12            # bytes/s of a float4 copy on this part


def dwells(rng, P, N, K):
    """-> (start, len) int32 [P K]: K consecutive intervals that cover N samples, every one at least one sample."""
    import numpy as np
    cuts = np.sort(rng.integers(0, N - K + 1, (P, K - 1)), axis=1) + np.arange(1, K)
    edges = np.concatenate([np.zeros((P, 1), np.int64), cuts, np.full((P, 1), N)], axis=1)
    return edges[:, :-1].astype(np.int32).reshape(-1), np.diff(edges, axis=1).astype(np.int32).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--kmers", type=int, default=5000)
    ap.add_argument("--geometry", type=int, nargs=3, default=[16, 250, 9], metavar=("TE", "TS", "KMER"))
    ap.add_argument("--host-threads", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long", type=int, default=0)
    ap.add_argument("--command", type=int, default=0)
    a = ap.parse_args()
    import ctypes as C
    import numpy as np, torch
    from seq2squiggle_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    te, ts, k = a.geometry

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

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def measure(P, N, K, reps, tag):
        x_h = rng.integers(-2000, 2000, P * N).astype(np.int16)
        st_h, ln_h = dwells(rng, P, N, K)
        km_h = rng.choice(np.frombuffer(b"ACGT", np.uint8), (P * K, k))
        offs_h, lo_h = np.arange(P + 1, dtype=np.int64) * N, np.arange(P + 1, dtype=np.int64) * K
        cal_h = np.tile([8192.0, -243.0, 1437.976], P)
        cap = P * (K // te + 1)
        x, st, ln, km, offs, lo, cal = (dev(v) for v in (x_h, st_h, ln_h, km_h, offs_h, lo_h, cal_h))
        S, Q = torch.empty(P * K, dtype=torch.int64, device="cuda"), torch.empty(P * K, dtype=torch.int64, device="cuda")
        p = lambda t: t.data_ptr()                  # noqa: E731
        check(L.s2s_event_sums(0, stream, p(x), p(offs), p(st), p(ln), p(lo), P, p(S), p(Q)))
        sizes = dict(chunks=(np.uint16, te * k * 5), chunks_lengths=(np.int64, te), targets=(np.float32, ts), targets_lengths=(np.int64, 1),
                     stdevs=(np.float32, te))
        out = {n: torch.empty(cap * c, dtype=getattr(torch, np.dtype(dt).name), device="cuda") for n, (dt, c) in sizes.items()}
        n_rows, cnt = torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty(3, dtype=torch.int64, device="cuda")
        scratch = torch.empty(int(L.s2s_chunk_scratch_bytes(P * K, P, cap)), dtype=torch.uint8, device="cuda")
        t = timed(lambda: check(L.s2s_chunk_pack(0, stream, p(x), p(offs), P * N, 0, p(lo), P * K, p(st), p(ln), p(S), p(Q), p(cal), None,
                                                 p(km), P, k, te, ts, 0, 0, cap, p(scratch), *[p(out[n]) for n in sizes], p(n_rows),
                                                 p(cnt))), reps)
        formed, kept, _ = (int(v) for v in cnt.cpu().numpy())
        per_chunk = sum(np.dtype(dt).itemsize * c for dt, c in sizes.values())
        read_bytes = 2 * P * N + P * K * (4 + 4 + 8 + 8 + k)
        base = dict(what=tag, reads=P, samples=N, kmers=K, te=te, ts=ts, k=k)
        print(json.dumps(dict(base, kernel="chunk_pack", ms=round(t, 3), chunks_formed=formed, chunks_kept=kept, bytes_per_kept_chunk=per_chunk,
                              written_bytes=kept * per_chunk, written_bytes_per_s=round(kept * per_chunk / t * 1e3),
                              share_of_copy_bandwidth=round(kept * per_chunk / t * 1e3 / COPY_BANDWIDTH, 4),
                              moved_bytes_per_s=round((kept * per_chunk + read_bytes) / t * 1e3), chunks_per_s=round(formed / t * 1e3),
                              reads_per_s=round(P / t * 1e3, 1))), flush=True)
        if a.host_threads > 0:
            h = {n: np.zeros(cap * c, dt) for n, (dt, c) in sizes.items()}
            hn, hc = np.zeros(P, np.int32), np.zeros(3, np.int64)
            q = lambda v: v.ctypes.data             # noqa: E731
            Sh, Qh = S.cpu().numpy(), Q.cpu().numpy()
            t0 = time.perf_counter()
            check(L.s2s_chunk_pack_host(q(x_h), q(offs_h), P * N, 0, q(lo_h), P * K, q(st_h), q(ln_h), q(Sh), q(Qh), q(cal_h), None, q(km_h), P, k,
                                        te, ts, 0, 0, cap, *[q(h[n]) for n in sizes], q(hn), q(hc), a.host_threads))
            s = time.perf_counter() - t0
            equal = np.array_equal(hc, cnt.cpu().numpy()) and np.array_equal(hn, n_rows.cpu().numpy()) and all(
                h[n][:kept * c].tobytes() == out[n][:kept * c].cpu().numpy().tobytes() for n, (dt, c) in sizes.items())
            print(json.dumps(dict(base, kernel="chunk_pack_host", threads=a.host_threads, ms=round(s * 1e3, 1), equal_to_gpu=bool(equal),
                                  gpu_over_host=round(s * 1e3 / t, 2))), flush=True)

    measure(a.reads, a.len, a.kmers, a.reps, "batch")
    if a.long:
        measure(1, 1 << a.long, (1 << a.long) // 10, a.reps, "one long read")
    if a.command:
        from seq2squiggle_amd import preprocess as PP, resquiggle as RSQ, signal_io, utils as U
        P, N, K, kk = a.command, a.len, a.kmers, 6
        pa = rng.permutation(4 ** kk) * (60.0 / 4 ** kk) + 60.0          # a model of 4^6 distinct levels, 60 .. 120 pA
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
            files = [os.path.join(d, n) for n in ("r.fasta", "s.blow5", "m.model")]
            RSQ.resquiggle_files(*files, os.path.join(d, "warm.tsv"))
            t0 = time.perf_counter()
            s = RSQ.resquiggle_files(*files, os.path.join(d, "direct.tsv"), chunks=(os.path.join(d, "direct"), kk, te, ts))
            direct = time.perf_counter() - t0
            t0 = time.perf_counter()
            s2 = RSQ.resquiggle_files(*files, os.path.join(d, "text.tsv"), with_samples=True)
            t1 = time.perf_counter()
            s3 = PP.preprocess_table(os.path.join(d, "text.tsv"), os.path.join(d, "text"), kk, te, ts)
            t2 = time.perf_counter()
            c = s["chunks"]
            print(json.dumps(dict(what="command", reads=P, samples=N, kmers=K, te=te, ts=ts, k=kk,
                                  direct=dict(wall_s=round(direct, 3), solve_and_pack_s=round(s["solve_seconds"], 3),
                                              pack_s=round(c["pack_seconds"], 3), write_s=round(c["write_seconds"], 3),
                                              format_s=round(s["format_seconds"], 3), chunks_kept=c["chunks_kept"]),
                                  by_text=dict(wall_s=round(t2 - t0, 3), resquiggle_s=round(t1 - t0, 3), solve_s=round(s2["solve_seconds"], 3),
                                               format_s=round(s2["format_seconds"], 3), table_bytes=os.path.getsize(os.path.join(d, "text.tsv")),
                                               preprocess_s=round(t2 - t1, 3), parse_s=round(s3["parse_seconds"], 3),
                                               pack_s=round(s3["pack_seconds"], 3), write_s=round(s3["write_seconds"], 3),
                                               chunks_kept=s3["chunks_kept"]),
                                  text_over_direct=round((t2 - t0) / direct, 2))), flush=True)
    print(json.dumps({"clock_after": clock()}), flush=True)


if __name__ == "__main__":
    main()
