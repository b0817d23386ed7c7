"""The dynamic schedule's claim list (csrc/s2s_schedule.h through the C ABI: s2s_schedule_claim, s2s_schedule_is_dynamic), walked on
the CPU: no GPU.  The predict kernel computes the same function of (n, G, group) on the device, claim by claim."""
import ctypes as C

import pytest

from seq2squiggle_amd import _lib

SIZES = [1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 5003, 65520, 312000, 1 << 20]
GRIDS = [1, 8, 256]
GROUPS = [8, 16]


def claim(n, G, group, c):
    start, count = C.c_int64(-1), C.c_int32(-1)
    _lib.lib().s2s_schedule_claim(n, G, group, c, C.byref(start), C.byref(count))
    return start.value, count.value


def claims(n, G, group):
    """Every claim of the launch up to the first empty one (which ends the list for good: checked by the caller)."""
    out, c = [], 0
    while True:
        start, count = claim(n, G, group, c)
        if count == 0:
            return out, c
        out.append((start, count))
        c += 1
        assert c <= n, "more claims than chunks"


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("n", SIZES)
def test_claims_partition_the_launch_and_taper(n, G, group):
    got, n_claims = claims(n, G, group)
    # an exact partition of [0, n), in increasing order
    at = 0
    for start, count in got:
        assert start == at and 1 <= count <= group, (start, count, at)
        at += count
    assert at == n
    # whole groups first: everything in front of the taper zone (the last G * group chunks, plus a ragged remainder) is a full group
    sizes = [k for _, k in got]
    whole = max(0, (n - G * group) // group)
    assert sizes[:whole] == [group] * whole
    zone = sizes[whole:]
    assert sum(zone) == n - whole * group < (G + 1) * group
    # from the zone on the sizes never grow, and are the halvings of the group
    assert all(a >= b for a, b in zip(zone, zone[1:])), zone[:40]
    assert set(zone) <= {group >> i for i in range(1, group.bit_length())}
    # no size is dealt to more than G claims, except the singles
    for s in set(zone) - {1}:
        assert zone.count(s) <= G
    # the last thing any workgroup starts is one chunk
    if n >= 2 * G * group:
        assert len(zone) >= G and zone[-G:] == [1] * G
        assert zone.count(1) >= 2 * G
    # past the end: empty, for good
    for c in (n_claims, n_claims + 1, n_claims + G, n_claims + 100000, (1 << 31) - 1):
        assert claim(n, G, group, c) == (n, 0)


def test_full_taper_is_the_documented_one():
    """n a multiple of the group beyond the zone: G claims of 8, G of 4, G of 2 and 2 G of 1 behind the whole groups (group 16)."""
    G, group, n = 256, 16, 312000
    got, _ = claims(n, G, group)
    sizes = [k for _, k in got]
    whole = (n - G * group) // group
    assert sizes == [16] * whole + [8] * G + [4] * G + [2] * G + [1] * (2 * G)
    got8, _ = claims(8 * 100 + 3, 8, 8)
    assert [k for _, k in got8] == [8] * 92 + [4] * 8 + [2] * 8 + [1] * (16 + 3)


def test_out_of_range_arguments_claim_nothing():
    for args in ((0, 256, 16, 0), (-5, 256, 16, 0), (100, 256, 16, -1), (100, 0, 16, 0), (100, 256, 0, 0)):
        assert claim(*args)[1] == 0


def test_auto_decision_is_a_threshold_in_groups_per_workgroup():
    L = _lib.lib()
    for G in GRIDS:
        for group in GROUPS:
            t = None
            for n in range(0, 64 * G * group + 1, max(1, G * group // 4)):
                if L.s2s_schedule_is_dynamic(n, G, group):
                    t = n
                    break
            assert t is not None and t % (G * group) == 0 and t > 0            # a multiple of G x group
            assert not L.s2s_schedule_is_dynamic(t - 1, G, group) and L.s2s_schedule_is_dynamic(t, G, group)
            assert L.s2s_schedule_is_dynamic(1 << 20, G, group)                # monotone above
    # the shapes the GPU tests use stay on the static split under auto; the benchmark's launch takes claims
    assert not L.s2s_schedule_is_dynamic(5003, 256, 16) and not L.s2s_schedule_is_dynamic(5003, 256, 8)
    assert L.s2s_schedule_is_dynamic(312000, 256, 16)
