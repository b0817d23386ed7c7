#!/usr/bin/env python
"""What `compare` computes per second (GPU box).
    python tools/compare_rate.py [--pairs P] [--len N] [--band R ...] [--host-threads T] [--reps K]
P pairs of signal-like int16 records (levels of 8 samples plus noise; B's lengths N +- 2 %, so the band is sloped) are generated on the
device; per band: HIP-event milliseconds of s2s_dtw_banded on the normalised samples -> pairs/s and cell updates/s (the cells inside
the band, counted per pair in closed form on the host), and of the median and normalise kernels on the same records.
--host-threads T > 0 also times s2s_dtw_banded_host on T threads on the same inputs (the baseline) and checks that the costs are
equal.  --path adds the warping path per band: s2s_dtw_path whole (the recording sweep and the walk back), the recording sweep
alone (the same call with empty slots for the ops: the trace kernel then returns at once), their difference as the walk back, the
bytes of decision scratch, and with --host-threads s2s_dtw_path_host with an equality check of cost, steps and ops.  --parent-lib
LIB also times s2s_dtw_banded of another build of the library (the parent commit's) in the same process, on the same inputs.
--open-ends adds the anchor search of `compare --open-ends`: every B gets --pad further signal-like samples in front, the padded
records are normalised, and s2s_sdtw is timed on the 2 P anchors (--anchor samples of A's head and tail inside --anchor-window
samples of B's head and tail) -> anchors/s and cell updates/s (L H cells per anchor); with --host-threads s2s_sdtw_host on the same
problems with an equality check; then one batch through compare's own two stages (_anchors, then _run_batch on the trimmed B, at
the first --band) on the wall clock, host-to-device copies included: the share of stage 1 in the call.
One JSON line per measurement; the device clock is read with amd-smi after the runs."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock():
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "-c", "--json"], capture_output=True, text=True, timeout=20)
        return r.stdout.strip()[:400] if r.returncode == 0 else None
    except (OSError, subprocess.SubprocessError):
        return None


def band_cells(n, m, R):
    """Cells (i, j) with |i m - j n| <= R max(n, m), row by row in closed form."""
    import numpy as np
    i = np.arange(n, dtype=np.int64)
    T = R * max(n, m)
    jlo = np.maximum(0, -((T - i * m) // n))
    jhi = np.minimum(m - 1, (i * m + T) // n)
    return int((jhi - jlo + 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--band", type=int, nargs="+", default=[512, 64])
    ap.add_argument("--host-threads", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--path", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--open-ends", action="store_true")
    ap.add_argument("--pad", type=int, default=3000)
    ap.add_argument("--anchor", type=int, default=1024)
    ap.add_argument("--anchor-window", type=int, default=16384)
    a = ap.parse_args()
    import ctypes as C
    import numpy as np, torch
    from seq2squiggle_amd._lib import lib
    L = lib()
    P, N = a.pairs, a.len
    rng = np.random.default_rng(0)
    na = np.full(P, N, np.int64)
    nb = np.maximum(1, N + rng.integers(-N // 50, N // 50 + 1, P)) if N >= 50 else na.copy()
    nb = np.minimum(nb, 1 << 22)
    offs = np.concatenate([[0], np.cumsum(np.concatenate([na, nb]))]).astype(np.int64)
    total = int(offs[-1])
    g = torch.Generator(device="cuda").manual_seed(1)
    levels = torch.randint(-150, 150, (total // 8 + 1,), device="cuda", generator=g, dtype=torch.int32)
    x = (400 + levels.repeat_interleave(8)[:total] + torch.randint(-12, 13, (total,), device="cuda", generator=g, dtype=torch.int32)).to(torch.int16)
    del levels
    offs_d = torch.from_numpy(offs).cuda()
    med = torch.empty(2 * P, dtype=torch.int32, device="cuda")
    mad = torch.empty(2 * P, dtype=torch.int32, device="cuda")
    q = torch.empty(total, dtype=torch.int16, device="cuda")
    cost = torch.empty(P, dtype=torch.int64, device="cuda")
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
    base = dict(pairs=P, len_a=N, len_b_min=int(nb.min()), len_b_max=int(nb.max()), samples=total)
    ms = timed(lambda: check(L.s2s_signal_median_mad(0, stream, x.data_ptr(), offs_d.data_ptr(), 2 * P, med.data_ptr(), mad.data_ptr())), a.reps)
    print(json.dumps(dict(base, kernel="median_mad", ms=round(ms, 4), records_per_s=round(2 * P / ms * 1e3), samples_per_s=round(total / ms * 1e3))), flush=True)
    ms = timed(lambda: check(L.s2s_signal_normalise(0, stream, x.data_ptr(), offs_d.data_ptr(), 2 * P, med.data_ptr(), mad.data_ptr(), 64,
                                                    q.data_ptr())), a.reps)
    print(json.dumps(dict(base, kernel="normalise", ms=round(ms, 4), samples_per_s=round(total / ms * 1e3))), flush=True)
    q_h = q.cpu().numpy() if a.host_threads > 0 else None
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.s2s_dtw_banded.restype = C.c_int32
        parent.s2s_dtw_banded.argtypes = [C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_void_p]
    for R in a.band:
        cells = sum(band_cells(int(n), int(m), R) for n, m in zip(na, nb))
        run = lambda: check(L.s2s_dtw_banded(0, stream, q.data_ptr(), offs_d.data_ptr(), q.data_ptr(), offs_d.data_ptr() + 8 * P, P, R,  # noqa: E731
                                             cost.data_ptr()))
        ms = timed(run, a.reps)
        got = cost.cpu().numpy()
        print(json.dumps(dict(base, kernel="dtw_banded", band=R, ms=round(ms, 3), pairs_per_s=round(P / ms * 1e3, 2), cells=cells,
                              cell_updates_per_s=round(cells / ms * 1e3), mean_dtw_per_sample=float((got / (na + nb) / 64).mean()))), flush=True)
        if a.host_threads > 0:
            host = np.zeros(P, np.int64)
            t0 = time.perf_counter()
            check(L.s2s_dtw_banded_host(q_h.ctypes.data, offs.ctypes.data, q_h.ctypes.data, offs.ctypes.data + 8 * P, P, R, host.ctypes.data,
                                        a.host_threads))
            s = time.perf_counter() - t0
            print(json.dumps(dict(base, kernel="dtw_banded_host", threads=a.host_threads, band=R, ms=round(s * 1e3, 1),
                                  pairs_per_s=round(P / s, 2), cell_updates_per_s=round(cells / s), equal_to_gpu=bool(np.array_equal(host, got)),
                                  gpu_over_host=round(s * 1e3 / ms, 2))), flush=True)
        if parent is not None:
            pcost = torch.empty(P, dtype=torch.int64, device="cuda")
            pms = timed(lambda: check(parent.s2s_dtw_banded(0, stream, q.data_ptr(), offs_d.data_ptr(), q.data_ptr(), offs_d.data_ptr() + 8 * P, P, R,
                                                            pcost.data_ptr())), a.reps)
            print(json.dumps(dict(base, kernel="dtw_banded_parent", band=R, ms=round(pms, 3), this_over_parent=round(ms / pms, 4),
                                  equal_to_this=bool(np.array_equal(pcost.cpu().numpy(), got)))), flush=True)
        if a.path:
            need = np.array([L.s2s_dtw_path_scratch_bytes(int(n), int(m), R) for n, m in zip(na, nb)], np.int64)
            slots = np.concatenate([[0], np.cumsum(need), [0], np.cumsum(na + nb - 2), np.zeros(P + 1, np.int64)]).astype(np.int64)
            slots_d = torch.from_numpy(slots).cuda()       # scratch_offs, path_offs, and path_offs of empty slots
            scratch = torch.empty(int(slots[P]), dtype=torch.uint8, device="cuda")
            n_ops = int(slots[2 * P + 1])
            ops = torch.empty(max(n_ops, 1), dtype=torch.uint8, device="cuda")
            steps = torch.empty(P, dtype=torch.int64, device="cuda")
            pcost = torch.empty(P, dtype=torch.int64, device="cuda")

            def run_path(path_offs_at):
                return lambda: check(L.s2s_dtw_path(0, stream, q.data_ptr(), offs_d.data_ptr(), q.data_ptr(), offs_d.data_ptr() + 8 * P, P, R,
                                                    pcost.data_ptr(), scratch.data_ptr(), slots_d.data_ptr(), ops.data_ptr(),
                                                    slots_d.data_ptr() + 8 * path_offs_at, steps.data_ptr()))
            sweep_ms = timed(run_path(2 * P + 2), a.reps)
            assert int(steps.abs().sum()) == 0
            path_ms = timed(run_path(P + 1), a.reps)
            st = steps.cpu().numpy()
            print(json.dumps(dict(base, kernel="dtw_path", band=R, ms=round(path_ms, 3), sweep_ms=round(sweep_ms, 3),
                                  trace_ms=round(path_ms - sweep_ms, 3), sweep_over_cost_only=round(sweep_ms / ms, 4),
                                  scratch_bytes=int(slots[P]), ops_bytes=n_ops, mean_steps=float(st.mean()),
                                  cost_equal=bool(np.array_equal(pcost.cpu().numpy(), got)), pairs_per_s=round(P / path_ms * 1e3, 2))), flush=True)
            if a.host_threads > 0:
                hcost, hsteps, hops = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(max(n_ops, 1), np.uint8)
                po = slots[P + 1:2 * P + 2].copy()
                t0 = time.perf_counter()
                check(L.s2s_dtw_path_host(q_h.ctypes.data, offs.ctypes.data, q_h.ctypes.data, offs.ctypes.data + 8 * P, P, R, hcost.ctypes.data,
                                          hops.ctypes.data, po.ctypes.data, hsteps.ctypes.data, a.host_threads))
                s = time.perf_counter() - t0
                g_ops = ops.cpu().numpy()
                same_ops = all(np.array_equal(g_ops[e - k:e], hops[e - k:e]) for e, k in zip(po[1:], hsteps))
                print(json.dumps(dict(base, kernel="dtw_path_host", threads=a.host_threads, band=R, ms=round(s * 1e3, 1),
                                      equal_to_gpu=bool(np.array_equal(hcost, got) and np.array_equal(hsteps, st) and same_ops),
                                      gpu_over_host=round(s * 1e3 / path_ms, 2))), flush=True)
            del scratch, ops
    if a.open_ends:
        from seq2squiggle_amd import compare as CMP
        pad = a.pad
        nb2 = nb + pad
        offs2 = np.concatenate([[0], np.cumsum(np.concatenate([na, nb2]))]).astype(np.int64)
        total2 = int(offs2[-1])
        x2 = torch.empty(total2, dtype=torch.int16, device="cuda")
        x2[:int(offs[P])] = x[:int(offs[P])]
        lev = torch.randint(-150, 150, (P * pad // 8 + 1,), device="cuda", generator=g, dtype=torch.int32)
        junk = (400 + lev.repeat_interleave(8)[:P * pad] + torch.randint(-12, 13, (P * pad,), device="cuda", generator=g, dtype=torch.int32)).to(torch.int16)
        for p in range(P):                             # B' = pad fresh samples, then B
            o = int(offs2[P + p])
            x2[o:o + pad] = junk[p * pad:(p + 1) * pad]
            x2[o + pad:o + pad + int(nb[p])] = x[int(offs[P + p]):int(offs[P + p + 1])]
        offs2_d = torch.from_numpy(offs2).cuda()
        q2 = torch.empty(total2, dtype=torch.int16, device="cuda")
        check(L.s2s_signal_median_mad(0, stream, x2.data_ptr(), offs2_d.data_ptr(), 2 * P, med.data_ptr(), mad.data_ptr()))
        check(L.s2s_signal_normalise(0, stream, x2.data_ptr(), offs2_d.data_ptr(), 2 * P, med.data_ptr(), mad.data_ptr(), 64, q2.data_ptr()))
        la, hb = np.minimum(a.anchor, na), np.minimum(a.anchor_window, nb2)
        tab = np.concatenate([offs2[:P], offs2[:P] + na - la, la, la, offs2[P:2 * P], offs2[P:2 * P] + nb2 - hb, hb, hb]).astype(np.int64)
        rev = np.concatenate([np.zeros(P, np.uint8), np.ones(P, np.uint8)])
        tab_d, rev_d = torch.from_numpy(tab).cuda(), torch.from_numpy(rev).cuda()
        res = torch.empty(6 * P, dtype=torch.int64, device="cuda")
        N2 = 2 * P
        tp, rp = tab_d.data_ptr(), res.data_ptr()
        ms = timed(lambda: check(L.s2s_sdtw(0, stream, q2.data_ptr(), tp, tp + 8 * N2, q2.data_ptr(), tp + 16 * N2, tp + 24 * N2,
                                            rev_d.data_ptr(), N2, rp, rp + 8 * N2, rp + 16 * N2)), a.reps)
        got = res.cpu().numpy()
        cells = int(2 * (la * hb).sum())
        print(json.dumps(dict(base, kernel="sdtw", pad=pad, anchor=a.anchor, anchor_window=a.anchor_window, anchors=N2, ms=round(ms, 3),
                              anchors_per_s=round(N2 / ms * 1e3, 1), cells=cells, cell_updates_per_s=round(cells / ms * 1e3),
                              mean_b_start=float(got[N2:N2 + P].mean()))), flush=True)
        if a.host_threads > 0:
            q2_h, hres = q2.cpu().numpy(), np.zeros(6 * P, np.int64)
            hp, ho = tab.ctypes.data, hres.ctypes.data
            t0 = time.perf_counter()
            check(L.s2s_sdtw_host(q2_h.ctypes.data, hp, hp + 8 * N2, q2_h.ctypes.data, hp + 16 * N2, hp + 24 * N2, rev.ctypes.data, N2,
                                  ho, ho + 8 * N2, ho + 16 * N2, a.host_threads))
            sec = time.perf_counter() - t0
            print(json.dumps(dict(base, kernel="sdtw_host", threads=a.host_threads, ms=round(sec * 1e3, 1), cell_updates_per_s=round(cells / sec),
                                  equal_to_gpu=bool(np.array_equal(hres, got)), gpu_over_host=round(sec * 1e3 / ms, 2))), flush=True)
        # compare's own two stages on one batch, wall clock (copies included)
        x2_h = x2.cpu().numpy()
        al = [x2_h[offs2[p]:offs2[p + 1]] for p in range(P)]
        bl = [x2_h[offs2[P + p]:offs2[P + p + 1]] for p in range(P)]
        R = a.band[0]
        for rep in range(2):                           # the second pass is the measurement
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c1, s1, e1, hb1 = CMP._anchors(al, bl, True, False, 0, a.anchor, a.anchor_window)
            t1 = time.perf_counter()
            cut = [(int(s1[p]), len(bl[p]) - int(hb1[p]) + int(e1[P + p])) for p in range(P)]
            cut = [(s_, e_) if e_ - s_ >= 1 else (0, len(bl[p])) for p, (s_, e_) in enumerate(cut)]
            t2 = time.perf_counter()
            CMP._run_batch(al, [b_[s_:e_] for b_, (s_, e_) in zip(bl, cut)], R, True, False, 0)
            t3 = time.perf_counter()
        print(json.dumps(dict(base, kernel="open_ends_call", band=R, stage1_ms=round((t1 - t0) * 1e3, 1), stage2_ms=round((t3 - t2) * 1e3, 1),
                              stage1_share=round((t1 - t0) / ((t1 - t0) + (t3 - t2)), 4), sdtw_kernel_ms=round(ms, 3),
                              mean_trimmed=float(np.mean([e_ - s_ for s_, e_ in cut])))), flush=True)
    print(json.dumps({"clock_after": clock()}), flush=True)


if __name__ == "__main__":
    main()
