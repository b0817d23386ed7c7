"""The kernels of `segment` (csrc/s2s_segment.h) against the host twin s2s_segment_host, bit for bit, on the smallest shapes at which
the pooled tiling can go wrong: records around one and two tiles, steps at every offset around a tile border, more records than a tile
has positions, a lone long record.  Every buffer of every call is preset to 0xAB and lies between guard margins that must come back
untouched, as must every slot beyond a record's events.  Nothing here provokes a fault: every input is valid memory of the stated size."""
import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd import segment as SEG
from test_compare_cpu import squiggles
from test_segment_cpu import T_DEFAULT, WINDOWS, host

pytestmark = pytest.mark.gpu

TILE, GUARD, FILL = 2048, 256, 0xAB
FILL32 = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
TOO_LONG = -2


def halo(w_s, w_l):
    return max(2 * w_l, 3 * w_s)


class Buf:
    """nbytes of device memory between two guard margins, everything preset to 0xAB; data: what the body starts with."""

    def __init__(self, nbytes, data=None):
        import torch
        self.nbytes = int(nbytes)
        self.t = torch.full((2 * GUARD + (self.nbytes + 15) // 16 * 16,), FILL, dtype=torch.uint8, device="cuda:0")
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert len(raw) == self.nbytes
            self.t[GUARD:GUARD + self.nbytes] = torch.from_numpy(raw.copy())
        self.ptr = self.t.data_ptr() + GUARD

    def body(self, dtype):
        return self.t[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype)

    def guards_intact(self):
        return bool((self.t[:GUARD] == FILL).all()) and bool((self.t[GUARD + self.nbytes:] == FILL).all())


def device(flat, offs, total, w_s, w_l, T_s, T_l, eo, stream=None, scratch=None, t_solo=0.0):
    """s2s_segment on guarded buffers -> (rc, n_events [R], start slots, len slots, the scratch buffer).  stream: a side stream, on
    which the samples come LATE (tests/_stream_order.py): the buffer holds other samples, a delay of ten times t_solo (ms: the same
    call alone) holds the stream, the real samples are copied in behind it, the call follows, and the other samples are put back
    right behind it, before anything waits."""
    import torch
    L = _lib.lib()
    R = len(offs) - 1
    slots = int(eo[-1])
    b_x, b_offs, b_eo = Buf(2 * len(flat), flat), Buf(8 * len(offs), offs), Buf(8 * len(eo), eo)
    b_st, b_ln, b_ne = Buf(4 * slots), Buf(4 * slots), Buf(4 * R)
    need = int(L.s2s_segment_scratch_bytes(int(total), R))
    assert need >= 8
    b_sc = scratch if scratch is not None else Buf(need)
    assert b_sc.nbytes >= need
    args = (b_offs.ptr, R, int(total), w_s, w_l, T_s, T_l, b_sc.ptr, b_eo.ptr)
    if stream is None:
        torch.cuda.synchronize()
        rc = L.s2s_segment(0, None, b_x.ptr, *args, b_st.ptr, b_ln.ptr, b_ne.ptr)
        torch.cuda.synchronize()
    else:
        import _stream_order as SO
        other = np.ascontiguousarray(SO.other_samples([flat], 99)[0])
        d_st, d_ln, d_ne = Buf(4 * slots), Buf(4 * slots), Buf(4 * R)                  # what the other samples give, on the default stream
        b_other = Buf(2 * len(flat), other)
        torch.cuda.synchronize()
        assert L.s2s_segment(0, None, b_other.ptr, *args, d_st.ptr, d_ln.ptr, d_ne.ptr) == 0
        torch.cuda.synchronize()
        body = {"x": b_x.t[GUARD:GUARD + b_x.nbytes]}
        real, decoy = {"x": body["x"].clone()}, {"x": b_other.t[GUARD:GUARD + b_x.nbytes].clone()}
        body["x"].copy_(decoy["x"])
        torch.cuda.synchronize()
        ms = SO.delay_for(t_solo)
        ev = SO.hold(stream, body, real, ms)
        rc = L.s2s_segment(0, stream.cuda_stream, b_x.ptr, *args, b_st.ptr, b_ln.ptr, b_ne.ptr)
        before = SO.returned_before(stream)
        snaps = SO.early(stream, body, decoy, [b_st.t, b_ln.t, b_ne.t])
        stream.synchronize()
        SO.lasted("test_gpu_segment: segment", ev, t_solo, ms)
        assert before, "s2s_segment waited for the stream"
        assert all(torch.equal(snap, b.t) for (_, snap), b in zip(snaps, (b_st, b_ln, b_ne)))
        assert not torch.equal(d_st.t, b_st.t), "the other samples give the same events: the late input proves nothing"
        body["x"].copy_(real["x"])
        torch.cuda.synchronize()
    for b in (b_x, b_offs, b_eo, b_st, b_ln, b_ne, b_sc):
        assert b.guards_intact()
    assert (b_x.body(np.int16) == flat).all() and (b_offs.body(np.int64) == offs).all() and (b_eo.body(np.int64) == eo).all()
    return rc, b_ne.body(np.int32), b_st.body(np.int32), b_ln.body(np.int32), b_sc


def pool(records):
    recs = [np.ascontiguousarray(r, np.int16) for r in records]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return np.concatenate(recs + [np.zeros(0, np.int16)]), offs


def check(records, w_s=3, w_l=6, T=T_DEFAULT, caps=None, **kw):
    """Both on the same pool: equal n_events, equal events, and every slot beyond them still preset.  -> n_events, [starts]."""
    flat, offs = pool(records)
    caps = [int(c) for c in SEG.capacity([len(r) for r in records], w_s)] if caps is None else caps
    eo = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    hrc, hne, hst, hln, _, _ = host(records, w_s, w_l, *T, threads=16, caps=caps)
    rc, ne, st, ln, _ = device(flat, offs, int(offs[-1]), w_s, w_l, *T, eo, **kw)
    assert rc == 0 and ne.tolist() == hne
    for r in range(len(records)):
        k = max(int(ne[r]), 0)
        assert st[eo[r]:eo[r] + k].tolist() == hst[r] and ln[eo[r]:eo[r] + k].tolist() == hln[r], r
        assert (st[eo[r] + k:eo[r + 1]] == FILL32).all() and (ln[eo[r] + k:eo[r + 1]] == FILL32).all(), r
    assert hrc == (0 if min(hne + [0]) >= 0 else -1)
    return hne, hst


def noisy(seed, n):
    return squiggles(seed, [n])[0]


def test_records_around_one_and_two_tiles():
    H = halo(3, 6)
    lens = (TILE - 1, TILE, TILE + 1, 2 * TILE + H - 1, 2 * TILE + H + 1)
    recs = [noisy(50 + i, n) for i, n in enumerate(lens)]
    for r in recs:                                    # each alone: its ends against the tile borders
        ne, _ = check([r])
        assert ne[0] > 100
    check(recs)                                       # and pooled: every record but the first begins off a tile border
    check([noisy(7, 7), noisy(8, 5000)])              # a record that begins at an odd pooled offset


@pytest.mark.parametrize("w", ((3, 6), (32, 32)))
def test_steps_at_every_offset_around_a_tile_border(w):
    w_s, w_l = w
    H = halo(w_s, w_l)
    recs, at = [], []
    for off in range(-(H + 1), H + 2):                # records of three tiles: the pooled tile borders are the records' own
        x = noisy(100 + off, 3 * TILE).astype(np.int32)
        x[TILE + off:] += 3000
        recs.append(x.astype(np.int16))
        at.append(TILE + off)
    _, st = check(recs, w_s, w_l)
    assert all(p in s for p, s in zip(at, st))        # the planted step is a boundary wherever it lies


def test_more_records_than_a_tile_has_positions():
    rng = np.random.default_rng(5)
    recs = [rng.integers(-500, 500, int(n)).astype(np.int16) for n in rng.integers(0, 4, 5000)] + [noisy(9, 3000)]
    ne, _ = check(recs)
    assert sum(len(r) for r in recs[:-1]) > TILE and ne[-1] > 100 and set(ne[:-1]) == {0, 1}
    check([np.zeros(0, np.int16)] * 3 + [noisy(1, 10)] + [np.zeros(0, np.int16)] * 2)


def test_a_lone_record_of_300000_samples():
    ne, st = check([noisy(11, 300000)])
    assert ne[0] > 20000
    ne, _ = check([np.full(3 * TILE + 5, -7, np.int16)])          # one event across four tiles: its length runs to the record's end
    assert ne == [1]


@pytest.mark.parametrize("w", WINDOWS)
def test_the_windows_and_extreme_values_of_the_cpu_test(w):
    alt = np.tile(np.array([-32768, 32767], np.int16), 200)
    blocks = np.repeat(np.tile(np.array([-32768, 32767], np.int16), 40), 32)
    odd = np.concatenate([alt[:101], np.full(64, 32767, np.int16), np.full(64, -32768, np.int16)])
    saw = ((np.arange(3000) % 4) * 1000).astype(np.int16)        # ties inside a neighbourhood, across a tile border too
    lens = sorted({0, 1, 2 * w[0] - 1, 2 * w[0], 2 * w[1] - 1, 2 * w[1], 2 * w[1] + 1})
    recs = [noisy(10 + n, n) for n in lens] + [alt, blocks, odd, saw, noisy(3, 2500)]
    for T in (T_DEFAULT, (1, 1), (1 << 40, 1 << 40)):
        check(recs, *w, T=T)


def test_a_slot_one_event_too_small_is_refused_alone():
    recs = [noisy(1, 3000), noisy(2, 4000), noisy(3, 3500)]
    ne, _ = check(recs)
    caps = [int(c) for c in SEG.capacity([len(r) for r in recs], 3)]
    caps[1] = ne[1] - 1
    ne2, _ = check(recs, caps=caps)                  # check(): the slot is still preset, the neighbours are complete
    assert ne2 == [ne[0], -ne[1], ne[2]]


def test_a_too_long_record_is_marked_and_costs_nothing():
    a, b = noisy(1, 1000), noisy(2, 500)
    long_n = (1 << 22) + 1
    flat = np.concatenate([a, np.zeros(long_n, np.int16), b])
    offs = np.array([0, 1000, 1000 + long_n, 1000 + long_n + 500], np.int64)
    caps = [int(SEG.capacity(1000, 3)), 8, int(SEG.capacity(500, 3))]
    eo = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    rc, ne, st, ln, _ = device(flat, offs, int(offs[-1]), 3, 6, *T_DEFAULT, eo)
    _, hne, hst, hln, _, _ = host([a, b], 3, 6, *T_DEFAULT)
    assert rc == 0 and ne.tolist() == [hne[0], TOO_LONG, hne[1]]
    assert st[:hne[0]].tolist() == hst[0] and ln[:hne[0]].tolist() == hln[0]
    assert st[eo[2]:eo[2] + hne[1]].tolist() == hst[1] and ln[eo[2]:eo[2] + hne[1]].tolist() == hln[1]
    assert (st[eo[1]:eo[2]] == FILL32).all() and (ln[eo[1]:eo[2]] == FILL32).all()


def test_offsets_that_decrease_or_are_negative_count_as_empty_records():
    x = noisy(4, 700)
    for offs in ([400, 300, 300, 700], [-5, 300, 300, 700]):
        offs = np.array(offs, np.int64)
        caps = [4, 4, int(SEG.capacity(400, 3))]
        eo = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        rc, ne, st, ln, _ = device(x, offs, 700, 3, 6, *T_DEFAULT, eo)
        _, hne, hst, hln, _, _ = host([x[300:]], 3, 6, *T_DEFAULT)
        assert rc == 0 and ne.tolist() == [0, 0, hne[0]]
        assert st[8:8 + hne[0]].tolist() == hst[0] and ln[8:8 + hne[0]].tolist() == hln[0] and (st[:8] == FILL32).all()


def test_side_stream_scratch_reuse_and_argument_errors():
    import torch
    L = _lib.lib()
    import _stream_order as SO
    recs = [noisy(21, 5000), noisy(22, 100), noisy(23, 9000)]
    check(recs)
    _, t_solo = SO.timed(lambda: check(recs))             # (with the host twin's time: a delay of ten times that is long enough)
    ne, st = check(recs, stream=SO.side_stream(), t_solo=t_solo)
    scratch = Buf(int(L.s2s_segment_scratch_bytes(20000, 3)))
    for rs in (recs, [noisy(31, 9000), noisy(32, 5000), noisy(33, 100)], recs):      # one scratch, three calls: no state is carried over
        got = check(rs, scratch=scratch)
    assert got == (ne, st)
    flat, offs = pool(recs)
    eo = np.concatenate([[0], np.cumsum(SEG.capacity(np.diff(offs), 3))]).astype(np.int64)
    for bad in ((0, 1, 1, 1), (4, 3, 1, 1), (1, 33, 1, 1), (3, 6, 0, 1), (3, 6, 1, (1 << 40) + 1)):
        rc, ne_, st_, _, _ = device(flat, offs, int(offs[-1]), *bad, eo)
        assert rc == -1 and (ne_ == FILL32).all() and (st_ == FILL32).all()          # nothing was launched
    rc, ne_, _, _, _ = device(flat, offs, 0, 3, 6, 1, 1, eo)                          # total = 0 launches nothing
    assert rc == 0 and (ne_ == FILL32).all()
    a, b = SEG.segment(recs), SEG.segment(recs, cpu=True)
    assert [x.tolist() for x in a[0]] == [x.tolist() for x in b[0]] == st and [x.tolist() for x in a[1]] == [x.tolist() for x in b[1]]
