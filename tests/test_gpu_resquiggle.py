"""`resquiggle` on the GPU: s2s_resquiggle and s2s_event_sums (csrc/s2s_resquiggle.h) equal their host twins bit for bit -- and, on
the small shapes, the Python restatement of the definition (tests/_resquiggle_ref.py) -- every shape alone and all of them in one
launch with an empty and a too long member between them; the raw-pointer contract (slots of scratch too small or misaligned, bands
outside the limits) with every output preset to 77; and the command's bytes are the same for the GPU, --cpu and a split batch."""
import functools

import numpy as np
import pytest

import _resquiggle_ref as REF
from seq2squiggle_amd import _lib
from seq2squiggle_amd import resquiggle as RSQ
from test_resquiggle_cpu import files, host, run  # noqa: F401  (files: a fixture)

pytestmark = pytest.mark.gpu

LIMIT = 1 << 22
I77 = 77


def up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def full(n, value, dtype):
    import torch
    return torch.full((max(int(n), 1),), value, dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def reference(n, K, R, kind):
    """-> (q, l, planted, (cost, start, len) of the host twin); the small shapes are held to the restatement here, once."""
    q, l, plant = REF.case(n, K, R, kind)
    rc, c, st, ln = host([(q, l)], R)
    assert rc == 0
    want = (int(c[0]), st[0].tolist(), ln[0].tolist())
    if (n, K, R) in REF.SMALL:
        assert want == REF.solve(q, l, R, REF.SKIP, REF.UNK)
    return q, l, plant, want


@pytest.mark.parametrize("kind", REF.KINDS)
@pytest.mark.parametrize("n,K,R", REF.SMALL + REF.LARGE)
def test_every_shape_alone(n, K, R, kind):
    q, l, plant, want = reference(n, K, R, kind)
    cost, start, length = RSQ.resquiggle([q], [l], R, REF.SKIP, REF.UNK)
    assert (int(cost[0]), start[0].tolist(), length[0].tolist()) == want
    if plant is not None:
        assert int(cost[0]) == 0 and (start[0] == plant[0]).all() and (length[0] == plant[1]).all()
    elif want[0] >= 0:
        REF.check_invariants(q, l, R, REF.SKIP, REF.UNK, int(cost[0]), start[0], length[0])


def test_cost_passes_2_32():
    n, K, R = REF.EXTREME
    q, l = np.full(n, 32767, np.int16), np.full(K, -32767, np.int16)
    rc, c, st, ln = host([(q, l)], R)
    cost, start, length = RSQ.resquiggle([q], [l], R, REF.SKIP, REF.UNK)
    assert rc == 0 and int(cost[0]) == int(c[0]) == 65534 * n > 1 << 32
    assert start[0].tolist() == st[0].tolist() and length[0].tolist() == ln[0].tolist()


def launch(reads, lens, band, slots=None, skip=REF.SKIP, unk=REF.UNK, margin=0, scratch_bytes=None):
    """One raw s2s_resquiggle call.  reads: (q, l) per read (the arrays that exist); lens: (n, K) per read as the offset tables declare
    them.  slots: scratch_offs (default: exactly what every read needs).  -> (rc, cost, start, len, scratch bytes) with the outputs
    preset to 77 and the scratch to 0xAB; `margin` bytes of scratch lie in front of offset 0."""
    import torch
    L = _lib.lib()
    P = len(reads)
    q_pool = np.concatenate([np.asarray(r[0], np.int16) for r in reads] + [np.zeros(1, np.int16)])
    l_pool = np.concatenate([np.asarray(r[1], np.int16) for r in reads] + [np.zeros(1, np.int16)])
    qo = np.concatenate([[0], np.cumsum([x[0] for x in lens])]).astype(np.int64)
    lo = np.concatenate([[0], np.cumsum([x[1] for x in lens])]).astype(np.int64)
    assert qo[-1] <= len(q_pool) and lo[-1] <= len(l_pool)
    if slots is None:
        slots = np.concatenate([[0], np.cumsum([max(int(L.s2s_resquiggle_scratch_bytes(n, K, min(max(band, 1), 1024))), 0)
                                                for n, K in lens])]).astype(np.int64)
    total = int(scratch_bytes if scratch_bytes is not None else max(slots)) + 2 * margin
    scratch = full(total + 16, 0xAB, torch.uint8)
    cost, ev = full(P, I77, torch.int64), full(2 * (int(lo[-1]) + 1), I77, torch.int32)
    kt = int(lo[-1]) + 1
    d = [up(q_pool), up(qo), up(l_pool), up(lo), up(np.asarray(slots, np.int64))]
    rc = L.s2s_resquiggle(0, torch.cuda.current_stream().cuda_stream, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), P,
                          band, skip, unk, cost.data_ptr(), scratch.data_ptr() + margin, d[4].data_ptr(), ev.data_ptr(), ev.data_ptr() + 4 * kt)
    torch.cuda.synchronize()
    ev = ev.cpu().numpy()
    assert ev[kt - 1] == I77 and ev[2 * kt - 1] == I77
    return (rc, cost.cpu().numpy(), [ev[lo[p]:lo[p + 1]] for p in range(P)], [ev[kt + lo[p]:kt + lo[p + 1]] for p in range(P)],
            scratch.cpu().numpy())


@pytest.mark.parametrize("band", (1, 32, 1024))
def test_all_shapes_in_one_launch(band):
    """Every (n, K) at one band, kinds in turn, with an empty read, a read without k-mers and a too long one between them."""
    shapes = [s[:2] for s in REF.SMALL + REF.LARGE] + [REF.EXTREME[:2]]
    reads, lens = [], []
    for t, (n, K) in enumerate(shapes):
        q, l, _ = REF.case(n, K, band, REF.KINDS[t % 4])
        reads.append((q, l))
        lens.append((n, K))
        if t == 3:
            reads += [(np.zeros(0, np.int16), np.ones(4, np.int16)), (np.ones(9, np.int16), np.zeros(0, np.int16))]
            lens += [(0, 4), (9, 0)]
        if t == 6:                                       # declared too long, and really that long
            reads.append((np.zeros(LIMIT + 1, np.int16), np.ones(3, np.int16)))
            lens.append((LIMIT + 1, 3))
    rc, cost, st, ln, _ = launch(reads, lens, band)
    assert rc == 0
    for p, ((q, l), (n, K)) in enumerate(zip(reads, lens)):
        if n > LIMIT:
            assert cost[p] == REF.TOO_LONG and set(st[p].tolist()) == {I77} and set(ln[p].tolist()) == {I77}    # no work, nothing written
            continue
        hrc, c, hs, hl = host([(q, l)], band)
        assert hrc == 0 and (int(cost[p]), st[p].tolist(), ln[p].tolist()) == (int(c[0]), hs[0].tolist(), hl[0].tolist()), (p, n, K)
    assert cost[4] == REF.EMPTY and cost[5] == REF.EMPTY and set(st[4].tolist()) == {-1} and set(ln[4].tolist()) == {0}


def test_event_sums_against_numpy():
    rng = np.random.default_rng(8)
    recs = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (40_000, 700, 1, 0, 333)]
    start = [np.array([0, 5, -1, 5 + 30_000, 39_990], np.int32), np.array([0, 17, 16, 650], np.int32), np.array([0], np.int32),
             np.array([-1, 0], np.int32), np.concatenate([np.arange(0, 330, 3), [-1, 330, 340, -5]]).astype(np.int32)]
    length = [np.array([5, 30_000, 0, 9_985, 10], np.int32), np.array([16, 633, 1, 51], np.int32), np.array([1], np.int32),
              np.array([0, 1], np.int32), np.concatenate([np.full(110, 3), [0, 3, 3, 10]]).astype(np.int32)]
    S, Q = RSQ.event_sums(recs, start, length)
    Sh, Qh = RSQ.event_sums(recs, start, length, cpu=True)
    for p, x in enumerate(recs):
        x = x.astype(np.int64)
        for j, (s, n) in enumerate(zip(start[p].tolist(), length[p].tolist())):
            ok = s >= 0 and n > 0 and s + n <= len(x)            # a stall of 30,000 samples; intervals outside the record count as empty
            want = (int(x[s:s + n].sum()), int((x[s:s + n] ** 2).sum())) if ok else (0, 0)
            assert (int(S[p][j]), int(Q[p][j])) == want == (int(Sh[p][j]), int(Qh[p][j])), (p, j)


def test_contract_slots_and_bands():
    L = _lib.lib()
    band = 40                                            # two word pairs per row
    shapes = ((300, 40), (129, 64), (500, 70), (200, 260), (65, 9))
    reads = [REF.case(n, K, band, "noisy")[:2] for n, K in shapes]
    need = [int(L.s2s_resquiggle_scratch_bytes(n, K, band)) for n, K in shapes]
    assert need == [n * 32 for n, _ in shapes]
    want = [host([r], band) for r in reads]
    margin = 1 << 16
    # the offset table is cumulative.  read 0: exact; read 1: 8 bytes short; read 2: large enough but misaligned by 8; read 3: exact
    # again; read 4: an empty slot
    slots = np.cumsum([0, need[0], need[1] - 8, need[2] + 24, need[3], 0]).astype(np.int64)
    assert slots[2] % 16 == 8 and slots[3] % 16 == 0
    rc, cost, st, ln, scratch = launch(reads, shapes, band, slots=slots, margin=margin, scratch_bytes=int(slots[-1]))
    assert rc == 0
    for p in range(5):
        assert int(cost[p]) == int(want[p][1][0])                                # the cost whatever the slot
        if p in (0, 3):
            assert st[p].tolist() == want[p][2][0].tolist() and ln[p].tolist() == want[p][3][0].tolist()
        else:
            assert set(st[p].tolist()) == {-1} and set(ln[p].tolist()) == {0}    # ... and no events
    body = scratch[margin:margin + int(slots[-1])]
    written = np.zeros(len(body), bool)
    for p in (0, 3):
        written[slots[p]:slots[p] + need[p]] = True
    assert (body[~written] == 0xAB).all() and (scratch[:margin] == 0xAB).all() and (scratch[margin + int(slots[-1]):] == 0xAB).all()
    # a band, a penalty or a cost outside the limits, and a misaligned scratch pointer: S2S_ERR_ARG, nothing launched
    for b, skip, unk, mis in ((0, 1, 1, 0), (1025, 1, 1, 0), (8, -1, 1, 0), (8, (1 << 20) + 1, 1, 0), (8, 1, 65536, 0), (8, 1, 1, 8)):
        rc, cost, st, ln, scratch = launch(reads[:2], shapes[:2], b, skip=skip, unk=unk, margin=mis)
        assert rc == -1 and set(cost.tolist()) == {I77} and set(st[0].tolist()) == {I77} and (scratch == 0xAB).all()
    assert b"s2s_resquiggle" in L.s2s_last_error(None)


def test_command_bytes_gpu_cpu_and_split(files):  # noqa: F811
    d, blow5, slow5, reads, cal, adc = files
    outs = []
    for name, extra in (("gpu", ()), ("cpu", ("--cpu",)), ("split", ("--max-samples", 300))):
        r = run(d / "r.fasta", blow5, "--kmer-model", d / "m.model", "-o", d / f"g_{name}.tsv", "--samples", "--summary", d / f"g_{name}.sum",
                "--band", 64, *extra)
        assert r.exit_code == 0, r.output
        outs.append(((d / f"g_{name}.tsv").read_bytes(), (d / f"g_{name}.sum").read_bytes()))
    assert outs[0] == outs[1] == outs[2] and outs[0][0].count(b"\n") == 1 + sum(len(v[2]) for v in reads.values())
