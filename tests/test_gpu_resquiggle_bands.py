"""s2s_resquiggle_kernel at every dealing of chunks to waves: the smallest and the largest band of every chunk count 1 .. 33
(REF.BANDS_BY_CHUNKS) -- the 16-wave workgroup of 1,024 threads at one chunk per wave (bands 480, 511) and at two (992, 1023) among
them, and the tightest ring, 64 c == 2 R + 2, at every c -- on shapes whose slots and level window wrap and whose window moves by two
columns (K = 2 n - 1, and K = 2 n, where a slot's old column is active one row before its new one and the answer is `unreached`); a path pressed against both edges of the band (REF.pressed); the slot contract at 16 waves; s2s_event_sums_kernel past one
stride of 128 k-mers.  Every answer is the host twin's, bit for bit; tests/test_resquiggle_cpu.py holds the host twin to the Python
restatement and to the invariants on the same inputs.  Every buffer is valid memory of its stated size: nothing provokes a fault."""
import functools

import numpy as np
import pytest

import _resquiggle_ref as REF
from seq2squiggle_amd import _lib
from seq2squiggle_amd import resquiggle as RSQ
from test_gpu_resquiggle import I77, launch
from test_resquiggle_cpu import event_sum_case, host

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def solved(reads_key):
    """The host twin on the reads of a key -> [(q, l, (cost, start, len))]; key: ("band", R) or ("pressed", R)."""
    what, R = reads_key
    if what == "band":
        reads = [REF.case(n, K, R, kind)[:2] for n, K, kind in REF.band_shapes(R)]
    else:
        reads = [REF.pressed(n, K, R) for n, K, band in REF.PRESSED if band == R]
    rc, c, st, ln = host(reads, R, threads=4)
    assert rc == 0 and all(int(c[p]) == (REF.UNREACHED if len(l) == 2 * len(q) else max(int(c[p]), 0)) for p, (q, l) in enumerate(reads))
    return [(q, l, (int(c[p]), st[p].tolist(), ln[p].tolist())) for p, (q, l) in enumerate(reads)]


def one_launch_and_alone(key):
    R = key[1]
    reads = solved(key)
    rc, cost, st, ln, _ = launch([r[:2] for r in reads], [(len(r[0]), len(r[1])) for r in reads], R)
    assert rc == 0
    for p, (q, l, want) in enumerate(reads):
        assert (int(cost[p]), st[p].tolist(), ln[p].tolist()) == want, (p, len(q), len(l), R)
        c1, s1, l1 = RSQ.resquiggle([q], [l], R, REF.SKIP, REF.UNK)
        assert (int(c1[0]), s1[0].tolist(), l1[0].tolist()) == want, (p, len(q), len(l), R)
    return reads


@pytest.mark.parametrize("R", REF.BANDS_BY_CHUNKS)
def test_every_chunk_count_in_one_launch_and_alone(R):
    """Chunk counts 1 .. 33; bands 480 / 511: 1,024 threads at one chunk per wave, 992 / 1023: at two; 1024: three chunks on 11 waves."""
    reads = one_launch_and_alone(("band", R))
    assert reads[0][2][0] == 0                          # the planted read: the one path of cost 0
    assert [(len(q), len(l)) for q, l, _ in reads] == [(n, K) for n, K, _ in REF.band_shapes(R)]


@pytest.mark.parametrize("R", sorted({R for _, _, R in REF.PRESSED}))
def test_pressed_paths_on_both_band_edges_in_one_launch_and_alone(R):
    for q, l, (cost, st, ln) in one_launch_and_alone(("pressed", R)):
        assert REF.edge_contact(len(q), len(l), R, st, ln) == (True, True)


def test_contract_slots_at_16_waves():
    """The slot part of test_contract_slots_and_bands at band 511: 16 chunks, one per wave, 1,024 threads."""
    L = _lib.lib()
    band = 511
    shapes = ((2600, 2400), (129, 64), (500, 70), (1200, 1500), (65, 9))
    reads = [REF.case(n, K, band, "noisy")[:2] for n, K in shapes]
    need = [int(L.s2s_resquiggle_scratch_bytes(n, K, band)) for n, K in shapes]
    assert need == [n * 16 * 16 for n, _ in shapes]
    want = [host([r], band) for r in reads]
    margin = 1 << 16
    # read 0: exact; read 1: 8 bytes short; read 2: large enough but misaligned by 8; read 3: exact again; read 4: an empty slot
    slots = np.cumsum([0, need[0], need[1] - 8, need[2] + 24, need[3], 0]).astype(np.int64)
    assert slots[2] % 16 == 8 and slots[3] % 16 == 0
    rc, cost, st, ln, scratch = launch(reads, shapes, band, slots=slots, margin=margin, scratch_bytes=int(slots[-1]))
    assert rc == 0
    for p in range(5):
        assert int(cost[p]) == int(want[p][1][0]) >= 0                           # the cost whatever the slot
        if p in (0, 3):
            assert st[p].tolist() == want[p][2][0].tolist() and ln[p].tolist() == want[p][3][0].tolist()
        else:
            assert set(st[p].tolist()) == {-1} and set(ln[p].tolist()) == {0}    # ... and no events
    assert I77 not in cost.tolist()
    body = scratch[margin:margin + int(slots[-1])]
    written = np.zeros(len(body), bool)
    for p in (0, 3):
        written[slots[p]:slots[p] + need[p]] = True
    assert (body[~written] == 0xAB).all() and (scratch[:margin] == 0xAB).all() and (scratch[margin + int(slots[-1]):] == 0xAB).all()


def test_event_sums_past_128_kmers_against_numpy():
    """Reads of 127, 128, 129 and 1,025 k-mers: the second to ninth trip of the stride of 16 * S2S_RSQ_SUM_SLICES = 128 k-mers."""
    recs, start, length, want = event_sum_case()
    S, Q = RSQ.event_sums(recs, start, length)
    Sh, Qh = RSQ.event_sums(recs, start, length, cpu=True)
    pairs = lambda S, Q: [list(zip(s.tolist(), q.tolist())) for s, q in zip(S, Q)]      # noqa: E731
    assert pairs(S, Q) == want == pairs(Sh, Qh)
