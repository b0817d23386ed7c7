"""s2s_chunk_pack on raw device pointers, held to the sentences of include/s2s_hip.h that tests/test_gpu_preprocess.py cannot reach
through `preprocess.pack` (which always passes a sufficient capacity, well-formed offsets and buffers of its own): chunks beyond the
capacity, "nothing behind the kept prefix is written", a scratch that needs no initialisation, P = 0 / slots = 0, the limits, and
offsets the device can only skip.  Every buffer of every call, the scratch included, is preset to 0xAB and lies between guard margins
that must come back untouched (Buf of tests/test_gpu_segment.py); inputs must compare equal afterwards.  A handful of reads of at most
a few hundred slots per case, geometries 5 / 37 / 6 and 64 / 1024 / 10, both sample sources.  Nothing here provokes a fault: every
pointer is valid memory of the stated size, and every bad value lies closer to a valid one than a guard margin is wide."""
import numpy as np
import pytest

import _preprocess_cases as C
import _preprocess_ref as R
from seq2squiggle_amd import _lib
from seq2squiggle_amd import preprocess as PP
from test_gpu_segment import FILL, GUARD, Buf

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
GEOMETRIES = ((5, 37, 6), (64, 1024, 10))
SOURCES = (R.RAW, R.PA)
OUT = ("chunks", "chunks_lengths", "targets", "targets_lengths", "stdevs")
geometry = pytest.mark.parametrize("te,ts,k", GEOMETRIES)
sources = pytest.mark.parametrize("source", SOURCES, ids=("raw", "pa"))


def row_bytes(k, te, ts):
    return dict(chunks=2 * te * k * 5, chunks_lengths=8 * te, targets=4 * ts, targets_lengths=8, stdevs=4 * te)


def arrays(case, source, **over):
    """The inputs of one call as host arrays of the entry's types (None: a pointer the source does not use)."""
    a = dict(s_offs=case["s_offs"], l_offs=case["l_offs"], ev_start=case["ev_start"], ev_len=case["ev_len"], kmers=case["kmers"].reshape(-1),
             S=None, Q=None, cal=None, stdv=None)
    if source == R.RAW:
        a.update(pool=case["flat"], S=case["S"], Q=case["Q"], cal=np.asarray(case["cal"], np.float64))
    else:
        a.update(pool=case["pool"], stdv=case["stdv"])
    a.update(over)
    want = dict(s_offs=np.int64, l_offs=np.int64, ev_start=np.int32, ev_len=np.int32, kmers=np.uint8, S=np.int64, Q=np.int64, cal=np.float64,
                stdv=np.float32, pool=np.int16 if source == R.RAW else np.float32)
    for name, v in a.items():
        assert v is None or np.asarray(v).dtype == want[name], (name, np.asarray(v).dtype)
    return {name: None if v is None else np.ascontiguousarray(v) for name, v in a.items()}


class Result:
    pass


def device(case, source, te, ts, k=None, reverse=0, backwards=0, capacity=None, P=None, slots=None, total=None, null=(), scratch="exact",
           alloc=None, **over):
    """One call of s2s_chunk_pack on guarded 0xAB buffers -> Result(rc, out: the five outputs' bytes, n_rows, counters, untouched:
    every output byte, n_rows and counters included, is still 0xAB).  capacity, P, slots, total, k: by value, default the case's own;
    over: input arrays in place of the case's; null: pointers passed as NULL; scratch: "exact" (s2s_chunk_scratch_bytes to the byte),
    "shifted" (16 bytes into a larger allocation), "by8" (misaligned); alloc: (k, te, ts, capacity) the outputs are sized for, where a
    refused call names larger ones than the case has."""
    import torch
    L = _lib.lib()
    a = arrays(case, source, **over)
    k = case["k"] if k is None else k
    P = len(case["l_offs"]) - 1 if P is None else P
    slots = int(case["l_offs"][-1]) if slots is None else slots
    total = len(a["pool"]) if total is None else total
    capacity = PP.capacity(np.diff(case["l_offs"]), te) if capacity is None else capacity
    ak, ate, ats, acap = alloc or (k, te, ts, capacity)
    ins = {name: Buf(v.nbytes, v if v.nbytes else None) for name, v in a.items() if v is not None}
    rb = row_bytes(ak, ate, ats)
    outs = {name: Buf(acap * rb[name]) for name in OUT}
    outs.update(n_rows=Buf(4 * max(P, 0)), counters=Buf(24))
    need = int(L.s2s_chunk_scratch_bytes(slots, P, capacity))
    need = need if need > 0 else 16
    b_sc = Buf(need + (16 if scratch != "exact" else 0))
    sc_ptr = b_sc.ptr + dict(exact=0, shifted=16, by8=8)[scratch]
    ptr = lambda name: None if name in null or name not in {**ins, **outs} else {**ins, **outs}[name].ptr       # noqa: E731
    torch.cuda.synchronize()
    r = Result()
    r.rc = L.s2s_chunk_pack(0, None, ptr("pool"), ptr("s_offs"), total, source, ptr("l_offs"), slots, ptr("ev_start"), ptr("ev_len"), ptr("S"),
                            ptr("Q"), ptr("cal"), ptr("stdv"), ptr("kmers"), P, k, te, ts, reverse, backwards, capacity,
                            None if "scratch" in null else sc_ptr, *[ptr(name) for name in OUT], ptr("n_rows"), ptr("counters"))
    torch.cuda.synchronize()
    for name, b in list(ins.items()) + list(outs.items()) + [("scratch", b_sc)]:
        assert b.guards_intact(), name
    for name, b in ins.items():
        assert b.body(np.uint8).tobytes() == a[name].tobytes(), name
    r.out = {name: outs[name].body(np.uint8) for name in OUT}
    r.n_rows, r.counters = outs["n_rows"].body(np.int32), outs["counters"].body(np.int64)
    r.untouched = all((b.body(np.uint8) == FILL).all() for b in outs.values())
    r.row_bytes, r.capacity = rb, capacity
    if scratch == "shifted":
        assert (b_sc.body(np.uint8)[:16] == FILL).all()
    return r


def kept_prefix_equals(r, want, what=""):
    """The first `kept` rows of the five outputs are `want`'s bytes, everything behind them is still 0xAB; n_rows and counters equal."""
    N = len(want["targets_lengths"])
    for name in OUT:
        n = N * r.row_bytes[name]
        assert r.out[name][:n].tobytes() == want[name].tobytes(), (what, name)
        assert (r.out[name][n:] == FILL).all(), (what, name, "written behind the kept prefix")
    assert r.n_rows.tolist() == want["n_rows"].tolist() and r.counters.tolist() == want["counters"].tolist(), (what, r.counters, want["counters"])


def host_rc(case, source, te, ts, capacity):
    """The host twin's return code on the same call (outputs of `capacity` chunks)."""
    a = arrays(case, source)
    rb = row_bytes(case["k"], te, ts)
    out = [np.zeros(capacity * rb[name], np.uint8) for name in OUT] + [np.zeros(len(case["l_offs"]) - 1, np.int32), np.zeros(3, np.int64)]
    p = lambda v: None if v is None else v.ctypes.data      # noqa: E731
    return _lib.lib().s2s_chunk_pack_host(p(a["pool"]), p(a["s_offs"]), len(a["pool"]), source, p(a["l_offs"]), int(case["l_offs"][-1]),
                                          p(a["ev_start"]), p(a["ev_len"]), p(a["S"]), p(a["Q"]), p(a["cal"]), p(a["stdv"]), p(a["kmers"]),
                                          len(case["l_offs"]) - 1, case["k"], te, ts, 0, 0, capacity, *[p(v) for v in out], 1)


def batch(te, ts, k, seed=0, empty_at=0):
    """A handful of reads: none (the read `empty_at`), 1, te - 1, te + 1 and 2 te + 3 slots, lengths around ts / te (chunks on both
    sides of ts), two skipped slots, letters with N, two k-mers all N."""
    rng = np.random.default_rng([seed, te, ts, k])
    counts = [1, te - 1, te + 1, 2 * te + 3]
    counts.insert(empty_at, 0)
    lens = [C.row_lengths(rng, n, te, ts) for n in counts]
    lens[4][[1, te]] = 0
    case = C.make(rng, k, lens, letters=b"ACGTN")
    case["kmers"][[2, len(case["kmers"]) - 2]] = ord("N")
    return case


# ------------------------------------------------------------------ the plain call
@geometry
@sources
def test_plain_call_equals_the_host_twin_and_leaves_the_rest_alone(te, ts, k, source):
    case = batch(te, ts, k)
    for reverse, backwards in ((0, 0), (1, 1)):
        want = C.run(case, source, te, ts, reverse=bool(reverse), backwards=bool(backwards), cpu=True)
        r = device(case, source, te, ts, reverse=reverse, backwards=backwards)
        assert r.rc == OK and 0 < want["counters"][1] < want["counters"][0] < r.capacity and want["counters"][2] == 2
        kept_prefix_equals(r, want, (reverse, backwards))
        C.same(want, C.ref(case, source, te, ts, bool(reverse), bool(backwards)))


@geometry
@sources
def test_the_zero_tail_of_targets_is_written_by_the_kernel(te, ts, k, source):
    """Every row has one sample: every kept chunk has targets_length = te < ts, and targets[te:ts] must come out as zeros over the
    0xAB preset -- written by the kernel, not left over from an allocation that happened to be clean."""
    case = C.make(np.random.default_rng([1, te]), k, [[1] * (te + 2), [1] * 3])
    want = C.run(case, source, te, ts, cpu=True)
    r = device(case, source, te, ts)
    assert r.rc == OK and want["counters"].tolist() == [3, 3, 0] and (want["targets_lengths"] < ts).all()
    kept_prefix_equals(r, want)
    tg = r.out["targets"][:3 * 4 * ts].view(np.float32).reshape(3, ts)
    for c, tl in enumerate(want["targets_lengths"]):
        assert (tg[c, tl:].view(np.uint32) == 0).all() and (tg[c, :min(tl, 3)] != 0).any()


# ------------------------------------------------------------------ capacity below the chunks formed
@geometry
@sources
def test_chunks_beyond_the_capacity_are_not_formed_but_counted(te, ts, k, source):
    """Every capacity from P (the least the entry takes) to formed - 1: the first `capacity` pooled chunks of the restatement come
    out, counters[0] is the full count, counters[1] the kept among the formed, n_rows complete.  Among them are a cut in the middle
    of a read's chunks with the first cut chunk one that would be kept, one that would be dropped, and the cut between two reads (so
    the last chunk formed is of either kind too).  The host twin refuses the same call."""
    rng = np.random.default_rng([2, te, ts])
    short, long_ = [1] * te, [1] * (te - 1) + [ts]          # a chunk of te samples: kept; of ts + te - 1: dropped
    case = C.make(rng, k, [short + long_ + short + long_ + [1], [], long_ + short * 2 + [3]])
    full = C.ref(case, source, te, ts)
    P, formed = 3, int(full["counters"][0])
    assert formed == 5 + 4 and full["n_rows"].tolist() == [4 * te + 1, 0, 3 * te + 1]
    keep = [1, 0, 1, 0, 1, 0, 1, 1, 1]
    assert int(full["counters"][1]) == sum(keep)
    seen = set()
    for capacity in range(P, formed):
        want = C.ref(case, source, te, ts, capacity=capacity)
        assert want["counters"].tolist() == [formed, sum(keep[:capacity]), 0] and want["n_rows"].tolist() == full["n_rows"].tolist()
        for name in OUT:
            assert want[name].tobytes() == full[name][:sum(keep[:capacity])].tobytes()
        r = device(case, source, te, ts, capacity=capacity)
        assert r.rc == OK
        kept_prefix_equals(r, want, capacity)
        assert host_rc(case, source, te, ts, capacity) == ERR_ARG
        seen.add(("between reads" if capacity == 5 else "inside a read", "cut chunk kept" if keep[capacity] else "cut chunk dropped"))
    assert {("inside a read", "cut chunk kept"), ("inside a read", "cut chunk dropped"), ("between reads", "cut chunk dropped")} == seen
    assert host_rc(case, source, te, ts, formed) == OK


# ------------------------------------------------------------------ the scratch
@geometry
@sources
def test_scratch_to_the_byte_shifted_and_misaligned(te, ts, k, source):
    case = batch(te, ts, k, seed=3)
    want = C.run(case, source, te, ts, cpu=True)
    for how in ("exact", "shifted"):                # (the guards of `exact` are the proof that s2s_chunk_scratch_bytes suffices)
        r = device(case, source, te, ts, scratch=how)
        assert r.rc == OK
        kept_prefix_equals(r, want, how)
    r = device(case, source, te, ts, scratch="by8")
    assert r.rc == ERR_ARG and r.untouched


# ------------------------------------------------------------------ nothing to do
@geometry
@sources
def test_nothing_to_do_writes_the_counters_and_n_rows_only(te, ts, k, source):
    case = batch(te, ts, k, seed=4)
    z = np.zeros(1, np.int64)
    r = device(case, source, te, ts, P=0, slots=0, total=0, capacity=0, l_offs=z, s_offs=z)                   # P = 0
    assert r.rc == OK and r.counters.tolist() == [0, 0, 0] and all((v == FILL).all() for v in r.out.values()) and r.n_rows.size == 0
    P = len(case["l_offs"]) - 1
    r = device(case, source, te, ts, slots=0, l_offs=np.zeros(P + 1, np.int64), capacity=P)                   # slots = 0 with P > 0
    assert r.rc == OK and r.counters.tolist() == [0, 0, 0] and r.n_rows.tolist() == [0] * P and all((v == FILL).all() for v in r.out.values())
    none = dict(case, ev_len=np.zeros_like(case["ev_len"]))                                                     # reads without rows
    r = device(none, source, te, ts)
    assert r.rc == OK and r.counters.tolist() == [0, 0, 0] and r.n_rows.tolist() == [0] * P and all((v == FILL).all() for v in r.out.values())
    skipped = dict(case, ev_start=np.full_like(case["ev_start"], -1))
    r = device(skipped, source, te, ts)
    assert r.rc == OK and r.counters.tolist() == [0, 0, 0] and r.n_rows.tolist() == [0] * P and all((v == FILL).all() for v in r.out.values())


# ------------------------------------------------------------------ the limits
def small(k, te):
    return C.make(np.random.default_rng([5, k, te]), k, [[2, 1, 3], [1] * 2, [4]], letters=b"ACGTN")


@sources
def test_every_limit_of_the_header_one_call_each_side(source):
    """k 1 .. 10, te 1 .. 64, ts 1 .. 1,024, source 0 / 1, P <= capacity: the value outside is S2S_ERR_ARG with every output still
    0xAB (its buffers are sized for the value it names, so that even a launch would stay inside them); the neighbour inside runs and
    equals the host twin."""
    for k, te, ts in ((1, 5, 37), (10, 5, 37), (6, 1, 37), (6, 64, 1024), (6, 5, 5), (6, 5, 1), (6, 5, 1024), (6, 1, 1)):
        case = small(k, te)
        r = device(case, source, te, ts)
        assert r.rc == OK
        kept_prefix_equals(r, C.run(case, source, te, ts, cpu=True), (k, te, ts))
    case = small(6, 5)
    for k, te, ts in ((0, 5, 37), (11, 5, 37), (6, 0, 37), (6, 65, 37), (6, 5, 0), (6, 5, 1025), (-1, 5, 37), (6, -1, 37), (6, 5, -1)):
        r = device(case, source, te, ts, k=k, capacity=3, alloc=(max(k, 6), max(te, 5), max(ts, 37), 3))
        assert r.rc == ERR_ARG and r.untouched, (k, te, ts)
    P = 3
    r = device(case, source, 5, 37, capacity=P - 1, alloc=(6, 5, 37, P))
    assert r.rc == ERR_ARG and r.untouched
    r = device(case, source, 5, 37, capacity=P)     # all three chunks fit
    assert r.rc == OK and r.counters[0] == 3
    kept_prefix_equals(r, C.run(case, source, 5, 37, cpu=True))


def test_a_source_that_is_neither_is_refused():
    """(By hand: `device` chooses the pointers by the source.  Here every pointer of both sources is there: only the value is wrong.)"""
    case = small(6, 5)
    L = _lib.lib()
    import torch
    ins = {n: Buf(v.nbytes, v) for n, v in dict(arrays(case, R.RAW), stdv=case["stdv"]).items()}
    rb = row_bytes(6, 5, 37)
    outs = {n: Buf(3 * rb[n]) for n in OUT}
    outs.update(n_rows=Buf(12), counters=Buf(24))
    sc = Buf(int(L.s2s_chunk_scratch_bytes(6, 3, 3)))
    for bad, rc in ((-1, ERR_ARG), (2, ERR_ARG), (0, OK)):
        torch.cuda.synchronize()
        got = L.s2s_chunk_pack(0, None, ins["pool"].ptr, ins["s_offs"].ptr, len(case["flat"]), bad, ins["l_offs"].ptr, 6, ins["ev_start"].ptr,
                               ins["ev_len"].ptr, ins["S"].ptr, ins["Q"].ptr, ins["cal"].ptr, ins["stdv"].ptr, ins["kmers"].ptr, 3, 6, 5, 37, 0, 0,
                               3, sc.ptr, *[outs[n].ptr for n in OUT], outs["n_rows"].ptr, outs["counters"].ptr)
        torch.cuda.synchronize()
        assert got == rc and all(b.guards_intact() for b in list(ins.values()) + list(outs.values()) + [sc])
        assert (rc == OK) != all((b.body(np.uint8) == FILL).all() for b in outs.values()), bad


@sources
def test_every_null_pointer_the_entry_checks(source):
    case = small(6, 5)
    mine = ("S", "Q", "cal") if source == R.RAW else ("stdv",)
    for name in ("s_offs", "l_offs", "counters", "n_rows", "ev_start", "ev_len", "kmers", "scratch", "pool") + OUT + mine:
        r = device(case, source, 5, 37, null=(name,))
        assert r.rc == ERR_ARG and r.untouched, name
    r = device(case, source, 5, 37)                 # with every pointer it runs
    assert r.rc == OK and r.counters[0] == 3


# ------------------------------------------------------------------ offsets the device can only skip
def consistent(r, case, te, ts, k):
    """What the header promises of ANY offsets: counters[1] <= capacity, nothing behind counters[1] chunks, and every written chunk
    consistent in itself -- targets_lengths is the sum of the row lengths and <= ts, zeros behind it, a pad row ('_' k times) has
    length 1 and deviation 0, every other row the letters and length of one slot."""
    kept = int(r.counters[1])
    assert 0 <= kept <= r.capacity
    for name in OUT:
        assert (r.out[name][kept * r.row_bytes[name]:] == FILL).all(), name
    hot = r.out["chunks"][:kept * r.row_bytes["chunks"]].view(np.uint16).reshape(kept, te, k, 5)
    cl = r.out["chunks_lengths"][:kept * 8 * te].view(np.int64).reshape(kept, te)
    tg = r.out["targets"][:kept * 4 * ts].view(np.float32).reshape(kept, ts)
    tl = r.out["targets_lengths"][:kept * 8].view(np.int64)
    dev = r.out["stdevs"][:kept * 4 * te].view(np.float32).reshape(kept, te)
    assert (cl.sum(axis=1) == tl).all() and (tl <= ts).all() and (cl >= 1).all() and np.isin(hot, (0, 0x3C00)).all()
    pad = (hot[..., 0] == 0x3C00).all(axis=2)
    assert (cl[pad] == 1).all() and (dev[pad] == 0).all() and (hot[pad][..., 1:] == 0).all() and (hot[~pad][..., 0] == 0).all()
    for c in range(kept):
        assert (tg[c, tl[c]:].view(np.uint32) == 0).all()
        assert not pad[c, 0] or pad[c].all()        # pads only follow rows; a chunk that begins with one is all pads
    return kept


@geometry
@sources
def test_offsets_the_device_can_only_skip(te, ts, k, source):
    """One bad offset per call; the host twin refuses each.  Why every access stays inside the stated sizes (csrc/s2s_chunk.h,
    s2s_prims.h), whatever l_offs [P + 1] and s_offs [P + 1] hold:
      * s2s_record_find probes l_offs[m] for m in [ra, rb] inside [0, P - 1] and then reads l_offs[r + 1], r + 1 <= P; it says yes only
        if 0 <= l_offs[r] <= g < l_offs[r + 1] <= slots, and the flag kernel asks it only for g < slots: ev_start[g], ev_len[g],
        kmers[g k ..] are inside.  s_offs[r], s_offs[r + 1] are entries of the array; they are values handed to s2s_chunk_row, which
        says no unless 0 <= lo <= hi <= total and the interval lies in [lo, hi): no sample is read in launch 1 at all.
      * the compact kernel reads l_offs[p], l_offs[p + 1] for p < P and calls s2s_bitmap_rank only if 0 <= lo <= hi <= slots: positions up
        to slots <= tiles x S2S_SEG_TILE, where trank has tiles + 1 entries and a position that is no multiple of the tile has a word.
        rows[] is written at ranks below the number of flags <= slots.
      * s2s_chunk_load searches c_offs[0 .. P - 1] (the scan of launch 3's counts: written for every read), reads rows[r_offs + i] with
        i < n_rows, so below rank(hi) <= the number of flags: an entry launch 3 wrote, a slot < slots.  It tests the slot AGAIN against
        its own read's record: where two reads claim a slot (a decreasing l_offs makes the next read reach back), a slot flagged under
        the other read's record drops the chunk here instead of reading outside [lo, hi) and so outside [0, total).
      * the write kernel runs for c < min(c_offs[P], capacity) with krank[c + 1] != krank[c] only, writes row krank[c] < kept <=
        capacity, and reads samples lo + st + o with st + len <= hi - lo, hi <= total.
    Every bad value lies within 9 of 0, of slots / total or of the entry before it: 9 slots are 90 bytes of letters and 36 of an
    int32 array, 9 samples 36 bytes, a guard margin is 256 bytes.  A kernel that used one unchecked would touch a guard, not leave
    the allocation.
    Equality with the restatement is asserted only where the search is provably the same as for valid offsets: a bad s_offs entry
    (the search runs on l_offs alone; the two reads beside the entry lose their rows or, with a smaller start, see a wider record, as
    the definition says), l_offs[0] < 0 (the probe `l_offs[m] <= g` never reads entry 0; only read 0's own test fails) and l_offs[P] >
    slots (entry P is only ever read as read P - 1's end).  A bad INTERIOR l_offs entry can turn a probe and so lose rows of other
    reads: there only the unconditional promises are asserted."""
    case = batch(te, ts, k, seed=6, empty_at=2)
    assert GUARD == 256
    P, slots, total = len(case["l_offs"]) - 1, int(case["l_offs"][-1]), len(case["flat"])
    lo, so = case["l_offs"], case["s_offs"]
    assert lo.tolist() == [0, 1, te, te, 2 * te + 1, 4 * te + 4]

    def with_entry(offs, i, v):
        out = offs.copy()
        out[i] = v
        return out

    def own_pair_bad(offs, most):
        return [not 0 <= offs[p] <= offs[p + 1] <= most for p in range(P)]

    # s_offs: past `total` or decreasing, in the middle and at the end -> the restatement, whole
    for i, v in ((4, total + 4), (P, total + 4), (3, int(so[2]) - 5), (4, int(so[3]) - 9)):
        bad = dict(case, s_offs=with_entry(so, i, v))
        assert any(own_pair_bad(bad["s_offs"], total)) and host_rc(bad, source, te, ts, PP.capacity(np.diff(lo), te)) == ERR_ARG
        want = C.ref(bad, source, te, ts)
        r = device(bad, source, te, ts, total=total)
        assert r.rc == OK
        kept_prefix_equals(r, want, ("s_offs", i, v))
        consistent(r, case, te, ts, k)
        assert all(n == 0 for n, b in zip(r.n_rows, own_pair_bad(bad["s_offs"], total)) if b) and want["counters"][1] > 0
    # l_offs at its two ends -> the restatement, whole
    for i, v in ((0, -2), (P, slots + 3)):
        bad = dict(case, l_offs=with_entry(lo, i, v))
        want = C.ref(bad, source, te, ts)
        r = device(bad, source, te, ts, slots=slots, capacity=PP.capacity(np.diff(lo), te))
        assert r.rc == OK
        kept_prefix_equals(r, want, ("l_offs", i, v))
        consistent(r, case, te, ts, k)
        assert want["n_rows"][P - 1 if i else 0] == 0 and want["counters"][1] > 0
    # l_offs inside: negative, decreasing (the next read reaches back over 3 slots of the read before), past slots
    for i, v in ((2, -3), (3, int(lo[2]) - 1), (4, int(lo[3]) - 3), (4, slots + 5), (2, slots + 1)):
        bad = dict(case, l_offs=with_entry(lo, i, v))
        assert host_rc(bad, source, te, ts, PP.capacity(np.diff(lo), te)) == ERR_ARG
        r = device(bad, source, te, ts, slots=slots, capacity=PP.capacity(np.diff(lo), te))
        assert r.rc == OK
        consistent(r, case, te, ts, k)
        wrong = own_pair_bad(bad["l_offs"], slots)
        assert sum(wrong) >= 1 and all(n == 0 for n, b in zip(r.n_rows, wrong) if b), (i, v, r.n_rows)
        assert (r.n_rows >= 0).all() and r.n_rows.sum() <= 2 * slots and r.counters[0] >= r.counters[1]
