#!/usr/bin/env python
"""What `eventalign` computes per second, stage by stage (GPU box).
    python tools/eventalign_rate.py [--reads P] [--len N] [--kmers K] [--width W ...] [--resquiggle-band R] [--host-threads T]
    [--reps K] [--long LOG2] [--command READS]
P reads of N stored samples against K k-mers (signal-like: every k-mer a level, a drawn dwell, noise) are generated on the host and
copied up once.  In HIP-event milliseconds, after a warm-up call each: s2s_segment, s2s_event_sums, s2s_event_means, the median / MAD
and normalisation of the means, and s2s_eventalign per band width W (whole; with empty scratch slots, i.e. the sweep without stores
and a walk back that only writes "no path"; their difference) -> reads/s and band cells/s ((E + K - 1) W per read).
--resquiggle-band R times s2s_resquiggle at band R on the SAME reads (samples and levels normalised by the same entries) in the same
process: the baseline the ratio is quoted against.  --host-threads T > 0 also times s2s_eventalign_host on T threads and checks
every output for equality.  --long LOG2 adds one read of 2^LOG2 samples (a tenth as many k-mers).  --command READS writes READS of
the reads as a BLOW5 file with a FASTA and a k = 6 model that explain them and runs eventalign_files on the wall clock: solve and
row-formatting seconds.  One JSON line per measurement; the device clock is read with amd-smi after the runs.  For the split of
s2s_eventalign into its two kernels run this tool under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resquiggle_rate import clock, make_reads  # noqa: E402

SEG = (3, 6, 501, 20736)            # the defaults of `segment`


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--kmers", type=int, default=5000)
    ap.add_argument("--width", type=int, nargs="+", default=[64, 128, 1024])
    ap.add_argument("--skip-penalty", type=int, default=128)
    ap.add_argument("--trim-penalty", type=int, default=64)
    ap.add_argument("--unknown-cost", type=int, default=64)
    ap.add_argument("--resquiggle-band", type=int, default=512)
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

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def empty(n, dt):
        return torch.empty(max(int(n), 1), dtype=dt, device="cuda")

    def measure(P, N, K, widths, band, reps, tag):
        q_h, l_h, _ = make_reads(rng, P, N, K)
        x_h = (q_h.astype(np.int32) * 4 + 2000).astype(np.int16)              # stored samples: levels 4 ADC counts per unit, noise +-64
        offs_h, lo_h = np.arange(P + 1, dtype=np.int64) * N, np.arange(P + 1, dtype=np.int64) * K
        cap = max(1, N // SEG[0])
        eo_h = np.arange(P + 1, dtype=np.int64) * cap
        x, l_raw, offs, lo, eo = dev(x_h), dev(l_h), dev(offs_h), dev(lo_h), dev(eo_h)
        ET, KT = P * cap, P * K
        st, ln, ne, kmer = (empty(n, torch.int32) for n in (ET, ET, P, ET))
        S, Q, mo, cost = (empty(n, torch.int64) for n in (ET, ET, P + 1, P))
        means, mq, lq, xq = (empty(n, torch.int16) for n in (ET, ET, KT, P * N))
        stats = empty(4 * P, torch.int32)
        fe, ks = empty(2 * P, torch.int32), empty(3 * KT, torch.int32)
        seg_scratch = empty(L.s2s_segment_scratch_bytes(P * N, P), torch.uint8)
        p = lambda t, i=0: t.data_ptr() + i * t.element_size()                # noqa: E731
        base = dict(what=tag, reads=P, samples=N, kmers=K)
        ms = {}
        ms["segment"] = timed(lambda: check(L.s2s_segment(0, stream, p(x), p(offs), P, P * N, *SEG, p(seg_scratch), p(eo), p(st), p(ln), p(ne))), reps)
        ms["event_sums"] = timed(lambda: check(L.s2s_event_sums(0, stream, p(x), p(offs), p(st), p(ln), p(eo), P, p(S), p(Q))), reps)
        ms["event_means"] = timed(lambda: check(L.s2s_event_means(0, stream, p(S), p(ln), p(eo), p(ne), P, ET, p(mo), p(means))), reps)

        def norm(src, o, n, dst):
            check(L.s2s_signal_median_mad(0, stream, p(src), p(o), n, p(stats), p(stats, n)))
            check(L.s2s_signal_normalise(0, stream, p(src), p(o), n, p(stats), p(stats, n), 64, p(dst)))
        ms["normalise_means"] = timed(lambda: norm(means, mo, P, mq), reps)
        norm(l_raw, lo, P, lq)
        mo_h, ne_h = mo.cpu().numpy(), ne.cpu().numpy()
        E = np.diff(mo_h)
        print(json.dumps(dict(base, kernel="stages", **{k: round(v, 3) for k, v in ms.items()}, events_per_read=float(E.mean()),
                              samples_per_event=float(N / max(E.mean(), 1)))), flush=True)
        out = {}
        for W in widths:
            need = int(L.s2s_eventalign_scratch_bytes(cap, K, W))
            so = dev(np.concatenate([np.arange(P + 1, dtype=np.int64) * need, np.zeros(P + 1, np.int64)]))
            scratch = empty(P * need, torch.uint8)
            cells = int((E + K - 1).sum()) * W

            def run(slots_at):
                return lambda: check(L.s2s_eventalign(0, stream, p(mq), p(mo), p(lq), p(lo), p(st), p(ln), p(eo), P, W, a.skip_penalty,
                                                      a.trim_penalty, a.unknown_cost, p(cost), p(scratch), p(so, slots_at), p(fe), p(fe, P),
                                                      p(kmer), p(ks), p(ks, KT), p(ks, 2 * KT)))
            bare = timed(run(P + 1), reps)
            t = timed(run(0), reps)
            got = [v.cpu().numpy().copy() for v in (cost, fe, kmer, ks)]
            solved = got[0] >= 0
            out[W] = t
            print(json.dumps(dict(base, kernel="eventalign", width=W, ms=round(t, 3), no_scratch_ms=round(bare, 3),
                                  stores_and_walk_back_ms=round(t - bare, 3), reads_per_s=round(P / t * 1e3, 2), band_cells=cells,
                                  band_cells_per_s=round(cells / t * 1e3), bands_per_s_per_read=round(float((E + K - 1).mean()) / t * 1e3),
                                  scratch_bytes_per_read=need, solved=int(solved.sum()),
                                  mean_cost_per_event=float((got[0][solved] / np.maximum(E[solved], 1) / 64).mean()) if solved.any() else None,
                                  skipped_kmers=int((got[3][2 * KT:3 * KT] == 0).sum()))), flush=True)
            if a.host_threads > 0:
                h = [v.cpu().numpy() for v in (mq, mo, lq, lo, st, ln, eo)]
                hc, hfe, hk, hks = np.zeros(P, np.int64), np.zeros(2 * P, np.int32), np.zeros(max(ET, 1), np.int32), np.zeros(3 * KT, np.int32)
                t0 = time.perf_counter()
                check(L.s2s_eventalign_host(*[v.ctypes.data for v in h], P, W, a.skip_penalty, a.trim_penalty, a.unknown_cost, hc.ctypes.data,
                                            hfe.ctypes.data, hfe.ctypes.data + 4 * P, hk.ctypes.data, hks.ctypes.data, hks.ctypes.data + 4 * KT,
                                            hks.ctypes.data + 8 * KT, a.host_threads))
                s = time.perf_counter() - t0
                total = int(mo_h[-1])
                equal = (np.array_equal(hc, got[0]) and np.array_equal(hfe, got[1][:2 * P]) and np.array_equal(hk[:total], got[2][:total]) and
                         np.array_equal(hks, got[3][:3 * KT]))
                print(json.dumps(dict(base, kernel="eventalign_host", threads=a.host_threads, width=W, ms=round(s * 1e3, 1),
                                      band_cells_per_s=round(cells / s), equal_to_gpu=bool(equal), gpu_over_host=round(s * 1e3 / t, 2))), flush=True)
            del scratch
        if band:
            norm(x, offs, P, xq)
            need = int(L.s2s_resquiggle_scratch_bytes(N, K, band))
            so = dev(np.arange(P + 1, dtype=np.int64) * need)
            scratch = empty(P * need, torch.uint8)
            t = timed(lambda: check(L.s2s_resquiggle(0, stream, p(xq), p(offs), p(lq), p(lo), P, band, a.skip_penalty, a.unknown_cost, p(cost),
                                                     p(scratch), p(so), p(ks), p(ks, KT))), reps)
            chain = {W: ms["segment"] + ms["event_sums"] + ms["event_means"] + ms["normalise_means"] + v for W, v in out.items()}
            print(json.dumps(dict(base, kernel="resquiggle", band=band, ms=round(t, 3), scratch_bytes_per_read=need,
                                  solved=int((cost.cpu().numpy() >= 0).sum()),
                                  resquiggle_over_eventalign={str(W): round(t / v, 2) for W, v in out.items()},
                                  resquiggle_over_chain={str(W): round(t / v, 2) for W, v in chain.items()})), flush=True)

    measure(a.reads, a.len, a.kmers, a.width, a.resquiggle_band, a.reps, "batch")
    if a.long:
        measure(1, 1 << a.long, (1 << a.long) // 10, a.width, 0, 1, "one long read")
    if a.command:
        from seq2squiggle_amd import eventalign as EA, resquiggle as RSQ, signal_io, utils as U
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
            for q, s in enumerate(seqs):
                lev = pa[RSQ.kmer_codes(s, k)][j[q]] + rng.normal(0, 1.5, N)
                sigs.append(np.rint(lev * prof["digitisation"] / prof["range"] - prof["offset_mean"]).astype(np.int16))
            ids = [f"read{q}" for q in range(P)]
            with open(os.path.join(d, "r.fasta"), "w") as f:
                f.write("".join(f">{i}\n{s}\n" for i, s in zip(ids, seqs)))
            w = signal_io.BLOW5Writer(os.path.join(d, "s.blow5"), prof, True, "dna-r10-prom", True)
            w.save_dac(ids, np.concatenate(sigs), np.concatenate([[0], np.cumsum([len(s) for s in sigs])]))
            for W in a.width:
                t0 = time.perf_counter()
                s = EA.eventalign_files(os.path.join(d, "r.fasta"), os.path.join(d, "s.blow5"), os.path.join(d, "m.model"),
                                        os.path.join(d, "out.tsv"), band_width=W)
                wall = time.perf_counter() - t0
                rows = {}
                for line in open(os.path.join(d, "out.tsv")).read().splitlines()[1:]:
                    v = line.split("\t")
                    rows.setdefault(v[0], []).append((int(v[1]), int(v[3]), int(v[4])))
                hit = total = 0
                for q, i in enumerate(ids):                # the share of samples that come back on the k-mer they were drawn for
                    mine = np.full(N, -1, np.int64)
                    for pos, b, e in rows.get(i, ()):
                        mine[b:e] = pos
                    hit += int((mine == j[q]).sum())
                    total += N
                print(json.dumps(dict(what="command", reads=P, samples=N, kmers=K, width=W, wall_s=round(wall, 3), solve_s=round(s["solve_seconds"], 3),
                                      format_s=round(s["format_seconds"], 3), format_share=round(s["format_seconds"] / wall, 4),
                                      rows=s["events"], rows_per_s=round(s["events"] / max(s["format_seconds"], 1e-9)), solved=s["solved"],
                                      unreached=s["unreached"], aligned_events=s["aligned_events"], skipped_kmers=s["skipped_kmers"],
                                      mean_cost_per_event=s["mean_cost_per_event"], samples_on_their_kmer=round(hit / total, 4))), flush=True)
    print(json.dumps({"clock_after": clock()}), flush=True)


if __name__ == "__main__":
    main()
