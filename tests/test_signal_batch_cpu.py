"""The batch layer (seq2squiggle_amd/signal_batch.py) by its own contracts, host side: the layout of a result buffer, the budget loop
and the dropping of device-only arguments.  What the layer computes through the solvers is held by the suites of compare, resquiggle
and segment."""
import ctypes

import numpy as np

from seq2squiggle_amd import _lib
from seq2squiggle_amd import signal_batch as SB

ODD_FIELDS = dict(a=(np.int64, 3), b=(np.int32, 5), c=(np.uint8, 7), d=(np.int64, 0))


def check_layout_and_round_trip(batch, write):
    """Every field aligned to its item size, no two fields overlapping (an empty one still owns an item), and fetch returns exactly what
    `write(buffer, pointer, bytes)` put behind every field's pointer."""
    res = batch.alloc(**ODD_FIELDS)
    spans, want = [], {}
    rng = np.random.default_rng(5)
    for name, (dt, count) in ODD_FIELDS.items():
        size = np.dtype(dt).itemsize
        assert res.ptr(name) % size == 0, name
        spans.append((res.ptr(name), res.ptr(name) + size * max(count, 1)))
        want[name] = rng.integers(0, 100, count).astype(dt)
        write(res, res.ptr(name), want[name].tobytes())
    spans.sort()
    assert all(e <= s for (_, e), (s, _) in zip(spans[:-1], spans[1:])), spans
    got = res.fetch()
    assert list(got) == list(ODD_FIELDS)
    for name, (dt, count) in ODD_FIELDS.items():
        assert got[name].dtype == np.dtype(dt) and got[name].shape == (count,) and np.array_equal(got[name], want[name]), name


def test_alloc_aligns_every_field_and_fetch_returns_what_was_written():
    check_layout_and_round_trip(SB.Batch([np.arange(3, dtype=np.int16)], cpu=True), lambda res, ptr, raw: ctypes.memmove(ptr, raw, len(raw)))


def test_alloc_starts_zeroed():
    got = SB.Batch([], cpu=True).alloc(**ODD_FIELDS).fetch()
    assert all(not v.any() for v in got.values())


def test_batch_packs_records_and_tables_once():
    recs = [np.array([1, 2, 3], np.int16), np.zeros(0, np.int16), np.array([-4], np.int16)]
    B = SB.Batch(recs, lambda offs: (np.diff(offs), np.array([7], np.uint8)), cpu=True, threads=2)
    assert B.n_rec == 3 and B.total == 4 and B.threads == 2
    assert np.array_equal(B.host_offs, [0, 3, 3, 4]) and np.array_equal(B.flat, [1, 2, 3, -4])
    assert np.array_equal(B.tables[0], [3, 0, 1]) and B.table(0) == B.tables[0].ctypes.data and B.table(1) == B.tables[1].ctypes.data
    assert B.offs() == B.host_offs.ctypes.data and B.offs(2) == B.host_offs.ctypes.data + 16 and B.samples == B.flat.ctypes.data


def batches(costs, limits):
    return list(SB.batches(range(len(costs)), lambda i: costs[i], limits))


def test_batches_one_limit():
    assert batches([(3,), (3,), (3,), (3,), (3,)], (6,)) == [[0, 1], [2, 3], [4]]
    assert batches([(3,), (4,)], (6,)) == [[0], [1]]
    assert batches([(3,), (3,)], (6,)) == [[0, 1]]                                      # a sum AT the limit stays


def test_batches_two_limits_end_at_whichever_comes_first():
    costs = [(2, 10), (2, 10), (2, 50), (5, 1), (5, 1), (1, 1)]
    assert batches(costs, (8, 60)) == [[0, 1], [2, 3], [4, 5]]


def test_batches_give_an_oversize_item_a_batch_to_itself():
    assert batches([(1,), (9,), (1,), (1,)], (4,)) == [[0], [1], [2, 3]]
    assert batches([(9,)], (4,)) == [[0]]
    assert batches([(1, 0), (1, 9), (1, 0)], (10, 4)) == [[0], [1], [2]]


def test_batches_zero_cost_item_after_an_oversize_one():
    """The running sum is past the limit already, so the batch ends before ANY further item, one that costs nothing included: it
    opens the next batch and ends none (segment's refused records)."""
    assert batches([(9,), (0,), (2,), (2,)], (4,)) == [[0], [1, 2, 3]]
    assert batches([(9,), (0,)], (4,)) == [[0], [1]]
    assert batches([(0,), (0,), (4,)], (4,)) == [[0, 1, 2]]


def test_batches_of_nothing():
    assert list(SB.batches([], lambda i: (1,), (4,))) == [] and list(SB.batches(iter(()), lambda i: (1, 1), (4, 4))) == []


def test_batches_pull_lazily():
    pulled = []

    def items():
        for i in range(7):
            pulled.append(i)
            yield i
    it = SB.batches(items(), lambda i: (1,), (3,))
    assert pulled == []
    assert next(it) == [0, 1, 2] and pulled == [0, 1, 2, 3]         # the batch that ends at 2 is out when 3 is seen, before 4 is pulled
    assert next(it) == [3, 4, 5] and pulled == [0, 1, 2, 3, 4, 5, 6]
    assert next(it) == [6] and next(it, None) is None


def test_call_drops_device_only_arguments_on_the_host():
    """s2s_dtw_path_host on one pair of 3 against 4 samples at band 1, through Batch.call with the device's scratch arguments in
    place, against the entry point called directly."""
    a, b = np.array([10, 40, 20], np.int16), np.array([12, 38, 41, 19], np.int16)
    path_offs = np.array([0, 3 + 4 - 2], np.int64)
    B = SB.Batch([a, b], (path_offs,), cpu=True, threads=1)
    res = B.alloc(cost=(np.int64, 1), steps=(np.int64, 1), ops=(np.uint8, 5))
    assert B.scratch(1 << 40).value is None                         # (nothing is allocated on the host)
    B.call("dtw_path", B.samples, B.offs(), B.samples, B.offs(1), 1, 1, res.ptr("cost"), B.scratch(64), SB.device_only(0xDEAD),
           res.ptr("ops"), B.table(0), res.ptr("steps"))
    got = res.fetch()
    flat, offs = np.concatenate([a, b]), np.array([0, 3, 7], np.int64)
    cost, steps, ops = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(5, np.uint8)
    rc = _lib.lib().s2s_dtw_path_host(flat.ctypes.data, offs.ctypes.data, flat.ctypes.data, offs[1:].ctypes.data, 1, 1, cost.ctypes.data,
                                      ops.ctypes.data, path_offs.ctypes.data, steps.ctypes.data, 1)
    assert rc == 0 and cost[0] >= 0 and 3 <= steps[0] <= 5
    assert np.array_equal(got["cost"], cost) and np.array_equal(got["steps"], steps) and np.array_equal(got["ops"], ops)


def test_call_raises_with_the_entry_points_name():
    B = SB.Batch([np.zeros(2, np.int16)] * 2, cpu=True, threads=1)
    res = B.alloc(cost=(np.int64, 1))
    try:
        B.call("dtw_banded", B.samples, B.offs(), B.samples, B.offs(1), 1, 0, res.ptr("cost"))      # band 0 is refused
    except RuntimeError as e:
        assert "s2s_dtw_banded_host failed" in str(e)
    else:
        raise AssertionError("band 0 was accepted")
