#!/usr/bin/env python
"""What `resquiggle` computes per second (GPU box).
    python tools/resquiggle_rate.py [--reads P] [--len N] [--kmers K] [--band R ...] [--host-threads T] [--reps K] [--long LOG2]
    [--command READS]
P reads of N samples against K k-mers (signal-like: every k-mer a level in units of 1/64 MAD, a drawn dwell, noise) are generated on
the host and copied up once.  Per band, in HIP-event milliseconds: s2s_resquiggle whole (the sweep with its decision stores, then the
walk back), the same call with empty scratch slots (the sweep without stores and a walk back that only writes -1 / 0: what is left
when nothing is traced), their difference (decision stores + walk back), and s2s_event_sums on the result -> reads/s and cell updates/s
(the cells inside the band, counted in closed form).  --host-threads T > 0 also times s2s_resquiggle_host on T threads on the same
inputs in the same process and checks cost, ev_start and ev_len for equality.  --long LOG2 adds one read of 2^LOG2 samples (a tenth
as many k-mers).  --command READS writes READS of the reads as a BLOW5 file with a FASTA and a k = 6 model that explain them and runs
resquiggle_files on the wall clock: solve and row-formatting seconds, rows/s of the Python formatter.  One JSON line per
measurement; the device clock is read with amd-smi after the runs.  For the split of the whole call into its two kernels run this tool
under `rocprofv3 --kernel-trace --stats` in a run of its own (profiles/r25)."""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock():
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "--json"], capture_output=True, text=True, timeout=20)
        return r.stdout.strip()[:400] if r.returncode == 0 else None
    except (OSError, subprocess.SubprocessError):
        return None


def band_cells(n, K, R):
    """Cells (i, j) with |i K - j n| <= R n, row by row in closed form."""
    import numpy as np
    i = np.arange(n, dtype=np.int64)
    jlo = np.maximum(0, -((-i * K) // n) - R)
    jhi = np.minimum(K - 1, i * K // n + R)
    return int((jhi - jlo + 1).sum())


def make_reads(rng, P, N, K):
    """-> (q int16 [P N], l int16 [P K]): levels of +-3 MAD in 1/64 MAD, dwell N / K on average (at least 1), noise of a quarter MAD."""
    import numpy as np
    lev = rng.integers(-192, 193, (P, K)).astype(np.int16)
    cuts = np.sort(rng.integers(0, N - K + 1, (P, K - 1)), axis=1) + np.arange(1, K) if K > 1 else np.zeros((P, 0), np.int64)
    j = np.zeros((P, N), np.int32)
    np.put_along_axis(j, cuts, 1, axis=1)
    j = np.cumsum(j, axis=1)
    q = np.take_along_axis(lev, j, axis=1).astype(np.int32) + rng.integers(-16, 17, (P, N), dtype=np.int16)
    return q.astype(np.int16).reshape(-1), lev.reshape(-1), j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--kmers", type=int, default=5000)
    ap.add_argument("--band", type=int, nargs="+", default=[512, 64])
    ap.add_argument("--skip-penalty", type=int, default=128)
    ap.add_argument("--unknown-cost", type=int, default=64)
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

    def measure(P, N, K, bands, reps, tag):
        q_h, l_h, _ = make_reads(rng, P, N, K)
        qo = (np.arange(P + 1, dtype=np.int64) * N)
        lo = (np.arange(P + 1, dtype=np.int64) * K)
        q, l, qo_d, lo_d = (torch.from_numpy(x).cuda() for x in (q_h, l_h, qo, lo))
        cost = torch.empty(P, dtype=torch.int64, device="cuda")
        ev = torch.empty(2 * P * K, dtype=torch.int32, device="cuda")
        SQ = torch.empty(2 * P * K, dtype=torch.int64, device="cuda")
        base = dict(what=tag, reads=P, samples=N, kmers=K)
        for R in bands:
            cells = P * band_cells(N, K, R)
            need = int(L.s2s_resquiggle_scratch_bytes(N, K, R))
            so = torch.from_numpy(np.concatenate([np.arange(P + 1, dtype=np.int64) * need, np.zeros(P + 1, np.int64)])).cuda()
            scratch = torch.empty(max(P * need, 16), dtype=torch.uint8, device="cuda")

            def run(slots_at):
                return lambda: check(L.s2s_resquiggle(0, stream, q.data_ptr(), qo_d.data_ptr(), l.data_ptr(), lo_d.data_ptr(), P, R, a.skip_penalty,
                                                      a.unknown_cost, cost.data_ptr(), scratch.data_ptr(), so.data_ptr() + 8 * slots_at,
                                                      ev.data_ptr(), ev.data_ptr() + 4 * P * K))
            bare = timed(run(P + 1), reps)
            ms = timed(run(0), reps)
            got, ev_h = cost.cpu().numpy(), ev.cpu().numpy()
            sums_ms = timed(lambda: check(L.s2s_event_sums(0, stream, q.data_ptr(), qo_d.data_ptr(), ev.data_ptr(), ev.data_ptr() + 4 * P * K,
                                                           lo_d.data_ptr(), P, SQ.data_ptr(), SQ.data_ptr() + 8 * P * K)), reps)
            print(json.dumps(dict(base, kernel="resquiggle", band=R, ms=round(ms, 3), no_scratch_ms=round(bare, 3),
                                  stores_and_walk_back_ms=round(ms - bare, 3), event_sums_ms=round(sums_ms, 3),
                                  reads_per_s=round(P / ms * 1e3, 2), cells=cells, cell_updates_per_s=round(cells / ms * 1e3),
                                  cell_updates_per_s_no_scratch=round(cells / bare * 1e3), scratch_bytes_per_read=need,
                                  mean_cost_per_sample=float((got / N / 64).mean()), skipped_kmers=int((ev_h[P * K:] == 0).sum()))), flush=True)
            if a.host_threads > 0:
                hc, hev = np.zeros(P, np.int64), np.zeros(2 * P * K, np.int32)
                t0 = time.perf_counter()
                check(L.s2s_resquiggle_host(q_h.ctypes.data, qo.ctypes.data, l_h.ctypes.data, lo.ctypes.data, P, R, a.skip_penalty, a.unknown_cost,
                                            hc.ctypes.data, hev.ctypes.data, hev.ctypes.data + 4 * P * K, a.host_threads))
                s = time.perf_counter() - t0
                print(json.dumps(dict(base, kernel="resquiggle_host", threads=a.host_threads, band=R, ms=round(s * 1e3, 1),
                                      cell_updates_per_s=round(cells / s), equal_to_gpu=bool(np.array_equal(hc, got) and np.array_equal(hev, ev_h)),
                                      gpu_over_host=round(s * 1e3 / ms, 2))), flush=True)
            del scratch

    measure(a.reads, a.len, a.kmers, a.band, a.reps, "batch")
    if a.long:
        measure(1, 1 << a.long, (1 << a.long) // 10, a.band[:1], 1, "one long read")
    if a.command:
        from seq2squiggle_amd import resquiggle as RSQ, signal_io, utils as U
        P, N, K, k = a.command, a.len, a.kmers, 6
        pa = rng.permutation(4 ** k) * (60.0 / 4 ** k) + 60.0           # a model of 4^6 distinct levels, 60 .. 120 pA
        prof = U.get_profile("dna-r10-prom")
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "m.model"), "w") as f:
                f.write("#k\t6\nkmer\tlevel_mean\n" + "".join("".join("ACGT"[(c >> (2 * (k - 1 - t))) & 3] for t in range(k)) + f"\t{pa[c]:.4f}\n"
                                                              for c in range(4 ** k)))
            seqs = ["".join(rng.choice(list("ACGT"), K + k - 1)) for _ in range(P)]
            _, _, j = make_reads(rng, P, N, K)
            sigs = []
            for p, s in enumerate(seqs):
                lev = pa[RSQ.kmer_codes(s, k)][j[p]] + rng.normal(0, 1.5, N)
                sigs.append(np.rint(lev * prof["digitisation"] / prof["range"] - prof["offset_mean"]).astype(np.int16))
            ids = [f"read{p}" for p in range(P)]
            with open(os.path.join(d, "r.fasta"), "w") as f:
                f.write("".join(f">{i}\n{s}\n" for i, s in zip(ids, seqs)))
            w = signal_io.BLOW5Writer(os.path.join(d, "s.blow5"), prof, True, "dna-r10-prom", True)
            w.save_dac(ids, np.concatenate(sigs), np.concatenate([[0], np.cumsum([len(s) for s in sigs])]))
            for R in a.band:
                t0 = time.perf_counter()
                s = RSQ.resquiggle_files(os.path.join(d, "r.fasta"), os.path.join(d, "s.blow5"), os.path.join(d, "m.model"),
                                         os.path.join(d, "out.tsv"), band=R)
                wall = time.perf_counter() - t0
                rows = {}
                for line in open(os.path.join(d, "out.tsv")).read().splitlines()[1:]:
                    v = line.split("\t")
                    rows.setdefault(v[0], []).append((int(v[1]), int(v[3]), int(v[4])))
                hit = total = 0
                for p, i in enumerate(ids):                # the share of samples that come back on the k-mer they were drawn for
                    mine = np.full(N, -1, np.int64)
                    for pos, b, e in rows.get(i, ()):
                        mine[b:e] = pos
                    hit += int((mine == j[p]).sum())
                    total += N
                print(json.dumps(dict(what="command", reads=P, samples=N, kmers=K, band=R, wall_s=round(wall, 3), solve_s=round(s["solve_seconds"], 3),
                                      format_s=round(s["format_seconds"], 3), format_share=round(s["format_seconds"] / wall, 4),
                                      rows=s["events"], rows_per_s=round(s["events"] / max(s["format_seconds"], 1e-9)), solved=s["solved"],
                                      skipped_kmers=s["skipped_kmers"], mean_cost_per_sample=s["mean_cost_per_sample"],
                                      samples_on_their_kmer=round(hit / total, 4))), flush=True)
    print(json.dumps({"clock_after": clock()}), flush=True)


if __name__ == "__main__":
    main()
