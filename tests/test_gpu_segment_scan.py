"""`segment` on pools of more than 1,024 and more than 2,048 tiles: launch 2, s2s_scan_kernel<1, S2SScanNext> (csrc/s2s_prims.h), scans
the tiles' counts 1,024 to a step with a carry, and every smaller pool of tests/test_gpu_segment.py is one step, three of sixteen waves
and carry 0.  Here: flags in every tile beyond tile 1,024 and beyond tile 2,048; pools of exactly 1,023 .. 2,049 tiles; a silent stretch
across the border of a step; the events of a record inside a big pool against the device's own answer for it in a small one; the
command with its batch border on either side of 1,024 tiles.  check() and Buf are those of tests/test_gpu_segment.py: the host twin
bit for bit, every buffer preset to 0xAB between guard margins, every slot beyond a record's events still preset."""
import numpy as np
import pytest

from seq2squiggle_amd import segment as SEG
from test_compare_cpu import squiggles, write_file
from test_gpu_segment import TILE, check, device, pool
from test_segment_cpu import SCAN_STEP, T_DEFAULT, silent_pool, three_step_pool, tiled_pool

pytestmark = pytest.mark.gpu

TOTALS = [T * TILE for T in (1023, 1024, 1025, 2048, 2049)] + [1024 * TILE + 1]      # (the last: a one-sample tile of a step of its own)


def test_three_scan_steps_with_flags_in_every_tile():
    """2,051 tiles: every wave's `before` and the carry are non-zero, twice; the next-flag search crosses both step borders."""
    recs = three_step_pool()
    ne, st = check(recs)
    per_tile = np.bincount(np.asarray(st[0][1:]) // TILE, minlength=2048)
    assert ne[0] == len(st[0]) and len(per_tile) == 2048 and per_tile.min() >= 1 and ne[1] > 100


@pytest.mark.parametrize("total", TOTALS)
def test_pools_around_one_and_two_scan_steps(total):
    recs = tiled_pool(total)
    _, offs = pool(recs)
    assert -(-total // TILE) in (1023, 1024, 1025, 2048, 2049) and (offs[1:-1] % TILE != 0).all()
    ne, _ = check(recs)
    assert min(ne[:-1]) > 100


@pytest.mark.parametrize("variant", ("one", "cut", "step"))
def test_silent_stretch_across_the_border_of_a_scan_step(variant):
    recs, k = silent_pool(variant)
    ne, st = check(recs)
    assert ne[k] == (2 if variant == "step" else 1) and min(ne[:k]) > 100 and min(ne[-20:]) > 100
    if variant == "cut":
        assert ne[k + 1] == 1 and sum(len(r) for r in recs[:k + 1]) == SCAN_STEP * TILE
    if variant == "step":
        assert st[k] == [0, 1030 * TILE + 77 - 3001 * k]


def events_of(recs):
    """The device alone (no host twin): -> [(starts, lengths)] per record."""
    flat, offs = pool(recs)
    eo = np.concatenate([[0], np.cumsum(SEG.capacity([len(r) for r in recs], 3))]).astype(np.int64)
    rc, ne, st, ln, _ = device(flat, offs, int(offs[-1]), 3, 6, *T_DEFAULT, eo)
    assert rc == 0 and (ne >= 0).all()
    return [(st[eo[r]:eo[r] + ne[r]].tolist(), ln[eo[r]:eo[r] + ne[r]].tolist()) for r in range(len(recs))]


@pytest.mark.parametrize("total", TOTALS)
def test_a_records_events_do_not_depend_on_the_pool_around_it(total):
    """Not via the host twin: the device's events of every record inside the big pool against the device's events of the same record
    in pools of 300 records (under 450 tiles: one step, carry 0)."""
    recs = tiled_pool(total)
    big = events_of(recs)
    small = [e for at in range(0, len(recs), 300) for e in events_of(recs[at:at + 300])]
    assert len(big) == len(small) == len(recs) and 300 * 3001 < 450 * TILE
    assert big == small


@pytest.fixture(scope="module")
def big_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("segment_scan")
    lens = [40_000, 7, 3001, 150_000, 900] * 12 + [5]
    sigs = squiggles(70, lens)
    ids = [f"read_{i}" for i in range(len(sigs))]
    return d, write_file(d / "s.blow5", ids, sigs), lens


def test_command_bytes_with_the_batch_border_on_either_side_of_1024_tiles(big_file):
    """2.3 M samples in records of mixed length: one batch on the GPU (1,137 tiles: two steps), --cpu, and --max-samples that end the
    first batch below (968 tiles) and above (1,042 tiles) 1,024 tiles."""
    d, path, lens = big_file
    total = sum(lens)
    assert total > 1070 * TILE

    def first_batch(m):                              # the batching rule of segment_files
        held = 0
        for n in lens:
            if held and held + n > m:
                return held
            held += n
        return held
    below, above = 1000 * TILE, 1060 * TILE
    assert 900 * TILE < first_batch(below) < SCAN_STEP * TILE < first_batch(above) < total
    got = {}
    for tag, kw in (("gpu", {}), ("cpu", dict(cpu=True)), ("below", dict(max_samples=below)), ("above", dict(max_samples=above))):
        s = SEG.segment_files(path, d / f"{tag}.tsv", summary_out=d / f"{tag}.sum", **kw)
        got[tag] = ((d / f"{tag}.tsv").read_bytes(), (d / f"{tag}.sum").read_bytes(), s["events"], s["batches"])
    assert got["gpu"][:3] == got["cpu"][:3] == got["below"][:3] == got["above"][:3]
    assert [got[t][3] for t in ("gpu", "cpu", "below", "above")] == [1, 1, 2, 2] and got["gpu"][2] > 200_000
