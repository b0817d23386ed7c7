#!/usr/bin/env python
"""What `segment` computes per second (GPU box).
    python tools/segment_rate.py [--reads P] [--len N] [--long LOG2] [--host-threads T] [--reps K] [--command READS]
    [--window-short 3 --window-long 6 --threshold-short 1.4 --threshold-long 9.0]
P records of N signal-like samples (a level per 10 samples on average, noise on top) are generated ON THE DEVICE; --long LOG2 adds the
same measurement on one lone record of 2^LOG2 samples -- the pooled tiling exists so that the two rates agree.  Per shape, in
HIP-event milliseconds after a warm-up call: s2s_segment whole (its three launches) and s2s_event_sums on its result -> samples/s and
events/s.  --host-threads T > 0 also times s2s_segment_host on T threads on the same samples in the same process and checks n_events,
ev_start and ev_len for equality.  --command READS writes READS of the records as a BLOW5 file and runs segment_files on the wall
clock: solve and formatting seconds, the formatter's share, rows/s.  One JSON line per measurement; the device clock is read with
amd-smi after the runs.  For the split of the call into its three launches run this tool under `rocprofv3 --kernel-trace --stats` in a
run of its own (profiles/r26)."""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock():
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "--json"], capture_output=True, text=True, timeout=20)
        return r.stdout.strip()[:400] if r.returncode == 0 else None
    except (OSError, subprocess.SubprocessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--long", type=int, default=22)
    ap.add_argument("--host-threads", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--command", type=int, default=0)
    ap.add_argument("--window-short", type=int, default=3)
    ap.add_argument("--window-long", type=int, default=6)
    ap.add_argument("--threshold-short", type=float, default=1.4)
    ap.add_argument("--threshold-long", type=float, default=9.0)
    a = ap.parse_args()
    import ctypes as C
    import numpy as np, torch
    from seq2squiggle_amd import segment as SEG
    from seq2squiggle_amd._lib import lib
    L = lib()
    w_s, w_l, T_s, T_l = a.window_short, a.window_long, SEG.threshold_int(a.threshold_short), SEG.threshold_int(a.threshold_long)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(0)

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

    def signal(total):
        """Signal-like int16 on the device: levels of +-150 around 400 held for 4 .. 16 samples, +-12 of noise."""
        n_lev = total // 4 + 1
        dwell = torch.randint(4, 17, (n_lev,), device="cuda", generator=gen)
        lev = torch.randint(-150, 151, (n_lev,), device="cuda", generator=gen)
        x = torch.repeat_interleave(lev, dwell)[:total] + torch.randint(-12, 13, (total,), device="cuda", generator=gen) + 400
        return x.to(torch.int16).contiguous()

    def measure(P, N, reps, tag):
        total = P * N
        x = signal(total)
        offs = np.arange(P + 1, dtype=np.int64) * N
        eo = np.arange(P + 1, dtype=np.int64) * int(SEG.capacity(N, w_s))
        slots = int(eo[-1])
        offs_d, eo_d = torch.from_numpy(offs).cuda(), torch.from_numpy(eo).cuda()
        ev = torch.zeros(2 * slots + P, dtype=torch.int32, device="cuda")
        SQ = torch.zeros(2 * slots, dtype=torch.int64, device="cuda")
        scratch = torch.empty(int(L.s2s_segment_scratch_bytes(total, P)), dtype=torch.uint8, device="cuda")
        p = ev.data_ptr()
        ms = timed(lambda: check(L.s2s_segment(0, stream, x.data_ptr(), offs_d.data_ptr(), P, total, w_s, w_l, T_s, T_l, scratch.data_ptr(),
                                               eo_d.data_ptr(), p, p + 4 * slots, p + 8 * slots)), reps)
        sums_ms = timed(lambda: check(L.s2s_event_sums(0, stream, x.data_ptr(), offs_d.data_ptr(), p, p + 4 * slots, eo_d.data_ptr(), P,
                                                       SQ.data_ptr(), SQ.data_ptr() + 8 * slots)), reps)
        got = ev.cpu().numpy()
        events = int(got[2 * slots:].sum())
        base = dict(what=tag, records=P, samples=N, windows=[w_s, w_l], thresholds=[T_s, T_l])
        print(json.dumps(dict(base, kernel="segment", ms=round(ms, 4), event_sums_ms=round(sums_ms, 4), samples_per_s=round(total / ms * 1e3),
                              events=events, samples_per_event=round(total / max(events, 1), 3), events_per_s=round(events / ms * 1e3),
                              tiles=-(-total // 2048), scratch_bytes=scratch.numel())), flush=True)
        if a.host_threads > 0:
            x_h, hev = x.cpu().numpy(), np.zeros(2 * slots + P, np.int32)
            q = hev.ctypes.data
            t0 = time.perf_counter()
            check(L.s2s_segment_host(x_h.ctypes.data, offs.ctypes.data, P, total, w_s, w_l, T_s, T_l, eo.ctypes.data, q, q + 4 * slots,
                                     q + 8 * slots, a.host_threads))
            s = time.perf_counter() - t0
            print(json.dumps(dict(base, kernel="segment_host", threads=a.host_threads, ms=round(s * 1e3, 2), samples_per_s=round(total / s),
                                  equal_to_gpu=bool(np.array_equal(hev, got)), gpu_over_host=round(s * 1e3 / ms, 2))), flush=True)
        return x

    x = measure(a.reads, a.len, a.reps, "many records")
    if a.long:
        measure(1, 1 << a.long, a.reps, "one lone record")
    if a.command:
        from seq2squiggle_amd import signal_io, utils as U
        P, N = a.command, a.len
        sig = x[:P * N].cpu().numpy()
        ids = [f"read{p}" for p in range(P)]
        with tempfile.TemporaryDirectory() as d:
            w = signal_io.BLOW5Writer(os.path.join(d, "s.blow5"), U.get_profile("dna-r10-prom"), True, "dna-r10-prom", True)
            w.save_dac(ids, sig, np.arange(P + 1, dtype=np.int64) * N)
            for cpu in (False, True):
                t0 = time.perf_counter()
                s = SEG.segment_files(os.path.join(d, "s.blow5"), os.path.join(d, "out.tsv"), window_short=w_s, window_long=w_l,
                                      threshold_short=a.threshold_short, threshold_long=a.threshold_long, cpu=cpu)
                wall = time.perf_counter() - t0
                print(json.dumps(dict(what="command", cpu=cpu, records=P, samples=N, wall_s=round(wall, 3), solve_s=round(s["solve_seconds"], 3),
                                      format_s=round(s["format_seconds"], 3), format_share=round(s["format_seconds"] / wall, 4),
                                      rows=s["events"], rows_per_s=round(s["events"] / max(s["format_seconds"], 1e-9)),
                                      out_bytes=os.path.getsize(os.path.join(d, "out.tsv")))), flush=True)
    print(json.dumps({"clock_after": clock()}), flush=True)


if __name__ == "__main__":
    main()
