"""The stream-ordered entries of `compare` held to what include/s2s_hip.h states about them, by raw ctypes calls on device pointers
(no seq2squiggle_amd.compare wrapper in between: the wrappers refuse or size on the host everything checked here, so the
device-only branches run in no other test).  Every integer output is preset to 77 and every byte buffer to 0xAB.
  A1  members longer than 2^22 samples and members of exactly 2^22: s2s_signal_median_mad gives (0, 0) / the rank selection,
      s2s_dtw_banded gives S2S_DTW_COST_TOO_LONG / the plain sum against a one-sample partner, s2s_dtw_path leaves the slots of a
      too long pair alone.  The records declared too long really are that long, so an entry that wrongly did the work would give a
      wrong number, not a stray read.  The PATH of the 2^22 pair is left out on purpose: its scratch is 64 MiB and its walk back is
      a loop of one wave over 4 M steps.
  A2  the slots of s2s_dtw_path: too small, misaligned, empty, decreasing, negative -- cost as ever, steps 0, nothing written -- and a
      slot longer than the path, which comes out right-aligned.  `scratch` and `ops` point a margin inside a larger allocation; the
      margin is larger than any slot and every slot a refused pair could claim is reserved for it, so every address a wrong kernel
      could form from these tables lies inside the allocation and shows as a changed sentinel byte.  The offset tables are
      cumulative: pairs with an empty member (no path, no bytes) are the spacers where a slot starts or ends off the grid.
      One thing the header allows and the test therefore does not forbid: a pair refused for its slot of OPS alone has a valid
      scratch slot, and the sweep (which never sees path_offs) fills it.  "Nothing is written outside a slot" is what is held:
      every byte outside the scratch slots of pairs with a valid one and outside the right-aligned paths is still 0xAB.
  A3  a and b (q and t) in separate allocations with unrelated offset tables, record starts on odd and even sample indices, a
      samples pointer that is only 2-byte aligned, everything enqueued on a side stream with one synchronize before the read -- and
      the samples LATE on that stream (tests/_stream_order.py): behind a delay, over decoys, which are put back right after the calls.
  A4  s2s_signal_normalise with med / mad outside what int16 samples can give and with scale 1 and 8192.
Every comparison is an equality of integers or bytes; the seconds of the limit pairs are printed, not asserted."""
import time

import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd import compare as CMP
import _stream_order as SO
from _dtw_ref import ref_median_mad, ref_normalise
from test_compare_cpu import dtw_pair, mixed_pairs, rnd
from test_compare_open_ends_cpu import KINDS, SHAPES, make

pytestmark = pytest.mark.gpu

LIMIT = 1 << 22
I77, B77 = 77, 0xAB


def up(x):
    """A host array on the device, on the current stream."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def offsets(recs, first=0):
    return (first + np.concatenate([[0], np.cumsum([len(r) for r in recs])])).astype(np.int64)


def pool_of(recs, junk=0):
    return np.concatenate([np.full(junk, 12345, np.int16)] + [np.asarray(r, np.int16) for r in recs])


def full(n, value, dtype):
    import torch
    return torch.full((max(int(n), 1),), value, dtype=dtype, device="cuda")


def chunks_of(n, m, R):
    """Word pairs per diagonal (csrc/s2s_dtw.h: s2s_dtw_path_chunks), also for a pair the entry refuses."""
    return (2 * R * max(n, m) // (n + m) + 1 + 63) // 64


# ------------------------------------------------------------------ A1: too long, and at the limit
@pytest.fixture(scope="module")
def limits():
    rng = np.random.default_rng(22)
    return dict(too_long=rnd(rng, LIMIT + 1), limit=rnd(rng, LIMIT), small=[rnd(rng, n, -600, 900) for n in (300, 257, 1, 1000)],
                one_a=rnd(rng, 1), one_b=rnd(rng, 1), sm_a=rnd(rng, 120, -600, 900), sm_b=rnd(rng, 130, -600, 900),
                ord_a=[rnd(rng, n, -600, 900) for n in (150, 97)], ord_b=[rnd(rng, n, -600, 900) for n in (140, 300)])


def test_median_mad_of_too_long_and_limit_records(limits):
    import torch
    L = _lib.lib()
    s = limits["small"]
    recs = [s[0], limits["too_long"], s[1], limits["limit"], s[2], s[3]]
    d_pool, d_offs = up(pool_of(recs)), up(offsets(recs))
    out = full(2 * len(recs), I77, torch.int32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = L.s2s_signal_median_mad(0, torch.cuda.current_stream().cuda_stream, d_pool.data_ptr(), d_offs.data_ptr(), len(recs),
                                 out.data_ptr(), out.data_ptr() + 4 * len(recs))
    torch.cuda.synchronize()
    print(f"\ns2s_signal_median_mad, records of 2^22 + 1 and 2^22 samples among four small ones: {time.perf_counter() - t0:.3f} s")
    got = out.cpu().numpy()
    hmed, hmad = CMP.median_mad(s, cpu=True)
    host = [(int(a), int(b)) for a, b in zip(hmed, hmad)]
    assert rc == 0
    assert list(zip(got[:6].tolist(), got[6:].tolist())) == [host[0], (0, 0), host[1], ref_median_mad(limits["limit"]), host[2], host[3]]


def test_dtw_banded_of_too_long_and_limit_members(limits):
    import torch
    L = _lib.lib()
    al = [limits["too_long"], limits["sm_a"], limits["limit"], limits["one_a"]] + limits["ord_a"]
    bl = [limits["sm_b"], limits["too_long"], limits["one_b"], limits["limit"]] + limits["ord_b"]
    P = len(al)
    d_a, d_b, d_ao, d_bo = up(pool_of(al)), up(pool_of(bl)), up(offsets(al)), up(offsets(bl))
    cost = full(P, I77, torch.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = L.s2s_dtw_banded(0, torch.cuda.current_stream().cuda_stream, d_a.data_ptr(), d_ao.data_ptr(), d_b.data_ptr(), d_bo.data_ptr(), P, 1,
                          cost.data_ptr())
    torch.cuda.synchronize()
    print(f"\ns2s_dtw_banded, (2^22, 1) and (1, 2^22) at band 1 in one launch of six pairs: {time.perf_counter() - t0:.3f} s")
    x = limits["limit"].astype(np.int64)
    sums = [int(np.abs(x - int(limits["one_b"][0])).sum()), int(np.abs(x - int(limits["one_a"][0])).sum())]
    host = CMP.dtw_banded(limits["ord_a"], limits["ord_b"], 1, cpu=True).tolist()
    assert rc == 0 and min(sums) > 1 << 32
    assert cost.cpu().numpy().tolist() == [-2, -2] + sums + host


def test_dtw_path_leaves_the_slots_of_too_long_pairs_alone(limits):
    import torch
    L = _lib.lib()
    R = 1
    al = [limits["too_long"], limits["sm_a"]] + limits["ord_a"]
    bl = [limits["sm_b"], limits["too_long"]] + limits["ord_b"]
    P = len(al)
    # the slots a pair of these lengths would need if it were served: whatever a wrong kernel writes stays inside them
    need = [(len(a) + len(b) - 1) * chunks_of(len(a), len(b), R) * 16 for a, b in zip(al, bl)]
    cap = [len(a) + len(b) - 2 for a, b in zip(al, bl)]
    assert need[2:] == [CMP.path_scratch_bytes(len(a), len(b), R) for a, b in zip(al[2:], bl[2:])] and min(need[:2]) > 64 << 20
    so, po = np.concatenate([[0], np.cumsum(need)]).astype(np.int64), np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
    SM, OM = max(need[2:]) + 64, max(cap[2:]) + 64                    # margins: larger than the largest legitimate slot
    scratch, ops = full(SM + so[-1] + SM, B77, torch.uint8), full(OM + po[-1] + OM, B77, torch.uint8)
    d_a, d_b, d_ao, d_bo, d_so, d_po = up(pool_of(al)), up(pool_of(bl)), up(offsets(al)), up(offsets(bl)), up(so), up(po)
    out = full(2 * P, I77, torch.int64)
    rc = L.s2s_dtw_path(0, torch.cuda.current_stream().cuda_stream, d_a.data_ptr(), d_ao.data_ptr(), d_b.data_ptr(), d_bo.data_ptr(), P, R,
                        out.data_ptr(), scratch.data_ptr() + SM, d_so.data_ptr(), ops.data_ptr() + OM, d_po.data_ptr(), out.data_ptr() + 8 * P)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    hcost, hops = CMP.dtw_path(limits["ord_a"], limits["ord_b"], R, cpu=True)
    assert rc == 0
    assert got[:P].tolist() == [-2, -2] + hcost.tolist()
    assert got[P:].tolist() == [0, 0] + [len(o) for o in hops]
    # margins and the slots of the two refused pairs: still 0xAB (compared on the device: 128 MiB)
    assert bool((scratch[:SM + int(so[2])] == B77).all()) and bool((scratch[SM + int(so[-1]):] == B77).all())
    assert bool((ops[:OM + int(po[2])] == B77).all()) and bool((ops[OM + int(po[-1]):] == B77).all())
    raw = ops[OM + int(po[2]):OM + int(po[-1])].cpu().numpy()
    for k in (2, 3):
        slot, want = raw[po[k] - po[2]:po[k + 1] - po[2]], hops[k - 2]
        assert np.array_equal(slot[len(slot) - len(want):], want) and (slot[:len(slot) - len(want)] == B77).all()


# ------------------------------------------------------------------ A2: the slots of s2s_dtw_path
SLOT_KINDS = ("exact", "scratch 16 bytes short", "exact", "scratch starts 8 mod 16", "exact", "scratch of size 0", "exact",
              "scratch_offs decreasing", "exact", "scratch_offs negative", "exact", "ops of n + m - 3 bytes", "exact", "path_offs negative",
              "exact", "ops 7 bytes longer", "exact")
SCRATCH_REFUSED = SLOT_KINDS[1:10:2]
OPS_REFUSED = ("ops of n + m - 3 bytes", "path_offs negative")


@pytest.mark.parametrize("n,m,R", [(97, 300, 7), (700, 650, 300)])      # 64 threads and one word pair per diagonal; 256 threads and five
def test_dtw_path_slots(n, m, R):
    import torch
    L = _lib.lib()
    need, cap = CMP.path_scratch_bytes(n, m, R), n + m - 2
    assert need == (n + m - 1) * chunks_of(n, m, R) * 16 and chunks_of(n, m, R) == (1 if R == 7 else 5)
    SM, OM = need + 64, cap + 64
    # every pair reserves a whole slot of each kind at the cursors (x, y); the tables then claim less, or something else
    pairs, x, y = [], 0, 0
    for k, kind in enumerate(SLOT_KINDS):
        s0, s1, p0, p1, nx, ny = x, x + need, y, y + cap, x + need, y + cap
        if kind == "scratch 16 bytes short":
            s1 -= 16
        elif kind == "scratch starts 8 mod 16":
            s0, s1, nx = s0 + 8, s1 + 8, nx + 16
        elif kind == "scratch of size 0":
            s1 = s0
        elif kind == "scratch_offs decreasing":
            s1 = s0 - 32
        elif kind == "scratch_offs negative":
            s0, s1, nx = -need, 0, x                                                    # a whole slot, inside the margin
        elif kind == "ops of n + m - 3 bytes":
            p1 -= 1
        elif kind == "path_offs negative":
            p0, p1, ny = -cap, 0, y
        elif kind == "ops 7 bytes longer":
            p1, ny = p1 + 7, ny + 7
        else:
            assert kind == "exact"
        pairs.append(dict(kind=kind, ab=dtw_pair(n, m, seed=100 * R + k), s=(s0, s1), p=(p0, p1)))
        x, y = nx, ny
    # the cumulative tables: a spacer (empty a, three samples of b) wherever one pair's end is not the next pair's start
    rows, cs, cp = [], 0, 0
    spacer = (np.zeros(0, np.int16), np.array([1, 2, 3], np.int16))
    for pr in pairs:
        if (cs, cp) != (pr["s"][0], pr["p"][0]):
            rows.append((spacer, cs, cp, None))
        rows.append((pr["ab"], pr["s"][0], pr["p"][0], pr))
        cs, cp = pr["s"][1], pr["p"][1]
    so, po = np.array([r[1] for r in rows] + [cs], np.int64), np.array([r[2] for r in rows] + [cp], np.int64)
    al, bl = [r[0][0] for r in rows], [r[0][1] for r in rows]
    P = len(rows)
    assert sum(r[3] is None for r in rows) >= 6 and (np.diff(so) < 0).any() and so.min() == -need and po.min() == -cap
    scratch, ops = full(SM + x + SM, B77, torch.uint8), full(OM + y + OM, B77, torch.uint8)
    d_a, d_b, d_ao, d_bo, d_so, d_po = up(pool_of(al)), up(pool_of(bl)), up(offsets(al)), up(offsets(bl)), up(so), up(po)
    out = full(2 * P, I77, torch.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = L.s2s_dtw_path(0, torch.cuda.current_stream().cuda_stream, d_a.data_ptr(), d_ao.data_ptr(), d_b.data_ptr(), d_bo.data_ptr(), P, R,
                        out.data_ptr(), scratch.data_ptr() + SM, d_so.data_ptr(), ops.data_ptr() + OM, d_po.data_ptr(), out.data_ptr() + 8 * P)
    torch.cuda.synchronize()
    print(f"\ns2s_dtw_path, {P} pairs of ({n}, {m}) at band {R}: {time.perf_counter() - t0:.3f} s")
    got, scratch_h, ops_h = out.cpu().numpy(), scratch.cpu().numpy(), ops.cpu().numpy()
    hcost, hops = CMP.dtw_path([p["ab"][0] for p in pairs], [p["ab"][1] for p in pairs], R, cpu=True)
    assert rc == 0
    may_s, may_o = np.zeros(len(scratch_h), bool), np.zeros(len(ops_h), bool)          # the bytes the entry may have written
    k = 0
    for i, (_, _, _, pr) in enumerate(rows):
        if pr is None:
            assert (got[i], got[P + i]) == (-1, 0)                                      # a spacer: S2S_DTW_COST_EMPTY
            continue
        want, kind = hops[k], pr["kind"]
        assert got[i] == hcost[k], kind                                                 # the cost does not depend on the slots
        if kind in SCRATCH_REFUSED or kind in OPS_REFUSED:
            assert got[P + i] == 0, kind
        else:
            p1 = OM + pr["p"][1]
            assert got[P + i] == len(want) and np.array_equal(ops_h[p1 - len(want):p1], want), kind
            may_o[p1 - len(want):p1] = True
        if kind not in SCRATCH_REFUSED:
            may_s[SM + pr["s"][0]:SM + pr["s"][1]] = True
        if kind == "ops 7 bytes longer":                                                # right-aligned: the front of the slot is untouched
            p0 = OM + pr["p"][0]
            assert len(want) < cap and (ops_h[p0:p0 + 7 + cap - len(want)] == B77).all()
        k += 1
    assert k == len(pairs) and len(set(hcost.tolist())) > len(pairs) // 2
    # everything else -- both margins, every range a refused pair owns or was given room for, the front of every slot of ops
    assert (scratch_h[~may_s] == B77).all() and (ops_h[~may_o] == B77).all()
    assert not may_s[:SM].any() and not may_s[SM + x:].any() and not may_o[:OM].any() and not may_o[OM + y:].any()


# ------------------------------------------------------------------ A3: two pools, odd offsets, a side stream
def test_two_pools_odd_offsets_and_a_side_stream():
    import torch
    L = _lib.lib()
    R = 5
    al, bl = (v[:40] for v in mixed_pairs())
    P = len(al)
    need = np.array([CMP.path_scratch_bytes(len(a), len(b), R) for a, b in zip(al, bl)], np.int64)
    cap = np.array([len(a) + len(b) - 2 if len(a) and len(b) else 0 for a, b in zip(al, bl)], np.int64)
    so, po = np.concatenate([[0], np.cumsum(need)]).astype(np.int64), np.concatenate([[0], np.cumsum(cap)]).astype(np.int64)
    # s2s_sdtw: every open-ends shape and kind in both directions, q and t in pools of their own, then ranges that run over two
    # neighbouring queries / targets and so overlap the problems in front of them
    probs = [(k, L_, H_, rev) for k in KINDS for L_, H_ in SHAPES for rev in (0, 1)]
    qs, ts = [make(k, L_, H_)[0] for k, L_, H_, _ in probs], [make(k, L_, H_)[1] for k, L_, H_, _ in probs]
    q_pool, t_pool = pool_of(qs, junk=1), pool_of(ts, junk=3)
    qo, to = offsets(qs, 1), offsets(ts, 3)
    qb, ql, tb, tl, rv = qo[:-1].tolist(), np.diff(qo).tolist(), to[:-1].tolist(), np.diff(to).tolist(), [p[3] for p in probs]
    for i in (2, 9, 20, 31, 40):
        qb.append(qb[i] + 1); ql.append(ql[i] + ql[i + 1] - 1); tb.append(tb[i]); tl.append(tl[i] + tl[i + 1] // 2); rv.append(i % 2)
    N = len(qb)
    # a: three samples of junk in front, the pointer one sample into the allocation (2-byte aligned only); b: five samples of junk.
    # The four sample pools come LATE on the side stream (tests/_stream_order.py): the tensors hold other samples, a delay holds the
    # stream, the real samples are copied in behind it.  The offset tables carry addresses: they are in place before the delay.
    real = dict(a=pool_of(al, junk=3), b=pool_of(bl, junk=5), q=q_pool, t=t_pool)
    decoy = {k: SO.other_samples([v], 40 + i)[0] for i, (k, v) in enumerate(real.items())}
    real_d, decoy_d = SO.up(real), SO.up(decoy)
    d_ao, d_bo, d_so, d_po = up(offsets(al, 2)), up(offsets(bl, 5)), up(so), up(po)
    d_tab, d_rv = up(np.array(qb + ql + tb + tl, np.int64)), up(np.array(rv, np.uint8))
    tab = d_tab.data_ptr()

    def three(x):
        """The three entries on the current stream, on the pools x -> (return codes, cost1, out2, scratch, ops, out3)."""
        s_ptr = torch.cuda.current_stream().cuda_stream
        cost1, out2 = full(P, I77, torch.int64), full(2 * P, I77, torch.int64)
        scratch, ops = full(so[-1] + 64, B77, torch.uint8), full(po[-1] + 64, B77, torch.uint8)
        out3 = full(3 * N, I77, torch.int64)
        a_ptr = x["a"].data_ptr() + 2
        assert a_ptr % 4 == 2
        rcs = [L.s2s_dtw_banded(0, s_ptr, a_ptr, d_ao.data_ptr(), x["b"].data_ptr(), d_bo.data_ptr(), P, R, cost1.data_ptr()),
               L.s2s_dtw_path(0, s_ptr, a_ptr, d_ao.data_ptr(), x["b"].data_ptr(), d_bo.data_ptr(), P, R, out2.data_ptr(), scratch.data_ptr(),
                              d_so.data_ptr(), ops.data_ptr(), d_po.data_ptr(), out2.data_ptr() + 8 * P),
               L.s2s_sdtw(0, s_ptr, x["q"].data_ptr(), tab, tab + 8 * N, x["t"].data_ptr(), tab + 16 * N, tab + 24 * N, d_rv.data_ptr(), N,
                          out3.data_ptr(), out3.data_ptr() + 8 * N, out3.data_ptr() + 16 * N)]
        return rcs, cost1, out2, scratch, ops, out3
    three(real_d)                                       # (the kernels' first launch is not what is timed)
    solo, t_solo = SO.timed(lambda: three(real_d))
    of_decoy = three(decoy_d)
    assert not torch.equal(of_decoy[1], solo[1]) and not torch.equal(of_decoy[2], solo[2]) and not torch.equal(of_decoy[5], solo[5])
    side = SO.side_stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    ms = SO.delay_for(t_solo)
    ins, ev = SO.late(side, real_d, decoy_d, ms)
    with torch.cuda.stream(side):
        rcs, cost1, out2, scratch, ops, out3 = three(ins)
    before = SO.returned_before(side)
    snaps = SO.early(side, ins, decoy_d, [cost1, out2, ops, out3])
    side.synchronize()
    SO.lasted("test_gpu_compare_contract: dtw_banded, dtw_path, sdtw", ev, t_solo, ms)
    assert before, "an entry waited for the stream"
    assert rcs == [0, 0, 0]
    for (_, snap), now, alone in zip(snaps, (cost1, out2, ops, out3), (solo[1], solo[2], solo[4], solo[5])):
        assert torch.equal(snap, now) and torch.equal(now, alone)
    hcost, hops = CMP.dtw_path(al, bl, R, cpu=True)
    assert sum(c == -1 for c in hcost.tolist()) == 2
    assert cost1.cpu().numpy().tolist() == hcost.tolist() == CMP.dtw_banded(al, bl, R, cpu=True).tolist()
    got2, ops_h = out2.cpu().numpy(), ops.cpu().numpy()
    assert got2[:P].tolist() == hcost.tolist() and got2[P:].tolist() == [len(o) for o in hops]
    for k in range(P):
        slot = ops_h[po[k]:po[k + 1]]
        assert np.array_equal(slot[len(slot) - len(hops[k]):], hops[k]) and (slot[:len(slot) - len(hops[k])] == B77).all(), k
    assert (ops_h[po[-1]:] == B77).all() and bool((scratch[int(so[-1]):] == B77).all())
    host3 = CMP.sdtw([q_pool[b:b + n] for b, n in zip(qb, ql)], [t_pool[b:b + n] for b, n in zip(tb, tl)], reverse=[bool(r) for r in rv],
                     cpu=True)
    assert out3.cpu().numpy().tolist() == np.concatenate(host3).tolist()


# ------------------------------------------------------------------ A4: normalise outside the wrapper's habits
NORMALISE_CASES = ((10 ** 6, 5, 64), (-10 ** 6, 5, 64), (0, -5, 64), (0, 70000, 64), (3, 2 ** 31 - 1, 64), (-32768, 1, 8192),
                   (32767, 1, 8192), (0, 1, 1), (0, 65535, 8192))


def test_normalise_clamps_med_and_mad_at_any_scale():
    import torch
    L = _lib.lib()
    x = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    for scale in (64, 8192, 1):
        cases = [(med, mad) for med, mad, s in NORMALISE_CASES if s == scale]
        R = len(cases)
        med, mad = np.array([c[0] for c in cases], np.int32), np.array([c[1] for c in cases], np.int32)
        d_x, d_offs, d_mm = up(np.tile(x, R)), up(65536 * np.arange(R + 1, dtype=np.int64)), up(np.concatenate([med, mad]))
        out = full(65536 * R + 64, I77, torch.int16)
        rc = L.s2s_signal_normalise(0, torch.cuda.current_stream().cuda_stream, d_x.data_ptr(), d_offs.data_ptr(), R, d_mm.data_ptr(),
                                    d_mm.data_ptr() + 4 * R, scale, out.data_ptr())
        got = out.cpu().numpy()
        host = CMP.normalise([x] * R, med=med, mad=mad, scale=scale, cpu=True)
        assert rc == 0 and (got[65536 * R:] == I77).all()
        for r, (m, d) in enumerate(cases):
            want = ref_normalise(x, min(max(m, -32768), 32767), min(max(d, 1), 65535), scale)      # clamped as the header states
            assert np.array_equal(got[65536 * r:65536 * (r + 1)], want), (m, d, scale)
            assert np.array_equal(host[r], want), (m, d, scale)
    assert sum(len([c for c in NORMALISE_CASES if c[2] == s]) for s in (64, 8192, 1)) == len(NORMALISE_CASES) == 9
