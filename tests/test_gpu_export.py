"""The export kernels (s2s_count_kernel, s2s_scan_kernel<8, S2SScanInts>, s2s_read_offsets_kernel, s2s_compact_kernel behind s2s_export_reads)
against the numpy restatement of their definition (tests/_export_ref.py) on crafted, not predicted, signals: every chunk geometry,
RNA, empty reads, the scan's step and vector / tail boundaries, a workspace that grows and is reused, a capacity below the sample
count, B == 0.  Every comparison is between integers or bit patterns (pA as uint32)."""
import ctypes as C

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _lib
import _geometry_models as GM
from _export_ref import ref_export
from test_gpu_events import CAL, CASES, GEOMETRIES, engine, make_inputs, pa

pytestmark = pytest.mark.gpu

CAL2 = (2048.0, 281.345551, -127.5655735)                     # a profile's own numbers
# empty reads first, doubled in the middle and last; one-chunk and multi-chunk reads; [11, 12) is make_inputs' all-zero chunk
READ_FIRST = [0, 0, 1, 5, 5, 5, 11, 12, 13, 64, 65, 200, 257, 257]
GUARD = 64                                                    # untouched elements in front of and behind every view
FILL = 0xAB


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _same(got, want):
    """Bit patterns: float32 as uint32 (so -0.0 / subnormals / infinities count as what they are)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def cabi_export(eng, sig_d, rf_d, cal, rna, capacity, n_chunks=None):
    """ONE s2s_export_reads call with out_offsets, out_pa and out_dac as views into 0xAB-filled buffers that physically span
    B * ts samples plus GUARD elements on either side, whatever `capacity` says.  -> the three whole buffers as bytes.
    n_chunks: the B the library is told (default: the rows of sig_d)."""
    B, ts = (int(x) for x in sig_d.shape)
    R = int(rf_d.numel()) - 1
    bufs = {}
    for name, n, size in (("offsets", R + 1, 8), ("pa", B * ts, 4), ("dac", B * ts, 2)):
        bufs[name] = torch.full(((n + 2 * GUARD) * size,), FILL, dtype=torch.uint8, device=eng.device)
    at = lambda name, size: C.c_void_p(bufs[name].data_ptr() + GUARD * size)
    assert all(bufs[k_].data_ptr() % 8 == 0 for k_ in bufs)
    with torch.cuda.device(eng.device):
        rc = _lib.lib().s2s_export_reads(eng._h, eng._stream(), C.c_void_p(sig_d.data_ptr()), B if n_chunks is None else n_chunks, C.c_void_p(rf_d.data_ptr()), R,
                                         at("offsets", 8), at("pa", 4), at("dac", 2), int(capacity), *(float(x) for x in cal),
                                         int(bool(rna)))
    assert rc == 0, _lib.lib().s2s_last_error(eng._h)
    torch.cuda.synchronize()
    return {k_: v.cpu().numpy() for k_, v in bufs.items()}


def holds_exactly(buf, want):
    """buf: a whole 0xAB-filled buffer of cabi_export; want: the elements the call had to write at the front of its view.  True if
    those are there and EVERY other byte of the buffer, in front of the view, behind what was to be written and behind the view,
    still is 0xAB."""
    want = np.ascontiguousarray(want)
    lead, n = GUARD * want.dtype.itemsize, want.nbytes
    return bool((buf[:lead] == FILL).all() and np.array_equal(buf[lead:lead + n], _bits(want)) and (buf[lead + n:] == FILL).all())


def _crafted(tag):
    eng = engine(tag)
    sig, _, i_run = make_inputs(eng.t_enc, eng.t_dec)
    assert not sig[i_run + 1].any() and READ_FIRST[6:8] == [i_run + 1, i_run + 2]          # the read of the all-zero chunk alone
    return eng, sig, torch.from_numpy(sig).to(eng.device), torch.tensor(READ_FIRST, dtype=torch.int32, device=eng.device)


@pytest.mark.parametrize("tag", GEOMETRIES)
def test_export_equals_its_definition(tag):
    eng, sig, sig_d, rf_d = _crafted(tag)
    B, ts = sig.shape
    assert (np.signbit(sig) & (sig == 0)).any() and ((sig != 0) & (np.abs(sig) < 1e-38)).any() or ts == 1   # -0.0 and subnormals
    for cal in (CAL, CAL2):
        for rna in (False, True):
            offs, pa_, dac = ref_export(sig, READ_FIRST, *cal, rna)
            total = int(offs[-1])
            assert 0 < total < B * ts and offs[7] == offs[6] and offs[0] == offs[1] and offs[-1] == offs[-2]
            got = eng.export_reads(sig_d, rf_d, *cal, rna=rna, want_pa=True, want_dac=True)
            assert (got["offsets"].dtype, got["pa"].dtype, got["dac"].dtype) == (torch.int64, torch.float32, torch.int16)
            assert np.array_equal(got["offsets"].cpu().numpy(), offs), (cal, rna)
            assert _same(got["pa"].cpu().numpy()[:total], pa_), (cal, rna)            # never reversed
            assert _same(got["dac"].cpu().numpy()[:total], dac), (cal, rna)
    # once through the C ABI, into views of 0xAB-filled buffers: nothing from the total on, nothing around the views
    offs, pa_, dac = ref_export(sig, READ_FIRST, *CAL2, True)
    bufs = cabi_export(eng, sig_d, rf_d, CAL2, True, B * ts)
    assert holds_exactly(bufs["offsets"], offs) and holds_exactly(bufs["pa"], pa_) and holds_exactly(bufs["dac"], dac)


def _random_signal(rng, B, ts):
    """0-or-nonzero samples: about four in ten dropped, the others exact under CAL."""
    sig = pa(rng.integers(-3000, 3000, (B, ts))).astype(np.float32)
    sig[rng.random((B, ts)) < 0.4] = 0.0
    return sig


def _scan_case(eng, B, seed):
    rng = np.random.default_rng(seed)
    ts = eng.t_dec
    sig = _random_signal(rng, B, ts)
    sig_d = torch.from_numpy(sig).to(eng.device)
    own = np.arange(B + 1)                                                         # every chunk its own read
    cuts = rng.integers(0, B + 1, max(1, B // 3))                                  # random read lengths, zeros among them ...
    mixed = np.sort(np.concatenate([[0], cuts, cuts[:1], [B]]))                    # ... one cut twice: an empty read at any B
    assert (np.diff(mixed) == 0).any() and mixed[0] == 0 and mixed[-1] == B
    for rf, rna in ((own, False), (mixed, True)):
        offs, pa_, dac = ref_export(sig, rf, *CAL, rna)
        got = eng.export_reads(sig_d, torch.from_numpy(rf.astype(np.int32)).to(eng.device), *CAL, rna=rna, want_pa=True, want_dac=True)
        total = int(offs[-1])
        assert np.array_equal(got["offsets"].cpu().numpy(), offs), (B, rna)       # the numpy cumsum, at the reads' first chunks
        assert _same(got["dac"].cpu().numpy()[:total], dac), (B, rna)
        assert _same(got["pa"].cpu().numpy()[:total], pa_), (B, rna)


GROW = 5 * 32768 + 1            # a handle starts with export scratch for 5 * 32768 chunks and their total: this B outgrows it


@pytest.mark.parametrize("tag", ["e1x1", "e5x37"])
def test_scan_boundaries_and_workspace_growth(tag):
    """The scan walks 8,192 chunk counts per step, 8 per thread: a thread takes the vector loads if all 8 are inside B, else the
    guarded tail.  Then B = 9 again: its counts sit in front of the stale ones of the larger calls.  A handle is created with
    scratch for 163,840 chunks, so only a larger B makes s2s_export_reads grow it: on a FRESH e1x1 engine (one sample per chunk,
    less data than 16,389 chunks of 37) B = 163,841 grows it, a step of the scan ends inside the new allocation, and 9 and
    16,389 reuse it."""
    fresh = tag == "e1x1"
    eng = S.Engine(GM.geometry_state_dict(tag, CASES), GM.geometry_config(tag, cases=CASES)) if fresh else engine(tag)
    for i, B in enumerate((1, 7, 8, 9, 8191, 8192, 8193, 8199, 16384, 16389, 9) + ((GROW, 9, 16389) if fresh else ())):
        _scan_case(eng, B, 100 * i + eng.t_dec)
    if fresh:
        eng.close()


def test_scan_boundary_on_the_250_row_instance():
    _scan_case(engine("tuned"), 8193, 5)


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
@pytest.mark.parametrize("tag", ["e5x37", "tuned"])
def test_capacity_below_the_sample_count_truncates_by_index(tag, rna):
    """include/s2s_hip.h: out_offsets is complete whatever the capacity, and in each output exactly the elements whose own index is
    below capacity are written, with the value a call with enough capacity puts there (test_export_equals_its_definition holds that
    one to the reference); every other byte keeps 0xAB.  The buffers physically span B * ts samples plus guards."""
    eng, sig, sig_d, rf_d = _crafted(tag)
    B, ts = sig.shape
    offs, pa_, dac = ref_export(sig, READ_FIRST, *CAL, rna)
    total = int(offs[-1])
    keep = sig != 0
    chunk_offs = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    inside = int(chunk_offs[7]) + 3                  # chunk 7 of the read [5, 11): inside a multi-chunk read and a 64-sample pass
    assert keep[7, :64].sum() > 3 and offs[5] < chunk_offs[7] and inside < offs[6]
    for capacity in (0, 1, inside, total - 1, total):
        bufs = cabi_export(eng, sig_d, rf_d, CAL, rna, capacity)
        assert holds_exactly(bufs["offsets"], offs), capacity                      # offs[R] > capacity tells the caller
        assert holds_exactly(bufs["pa"], pa_[:capacity]), capacity
        assert holds_exactly(bufs["dac"], dac[:capacity]), capacity


@pytest.mark.parametrize("tag", ["tuned", "e5x37"])
def test_no_chunks(tag):
    """B == 0: every read is empty.  Engine.export_reads answers without the library (an empty tensor has no address to pass); the
    C ABI, given any non-NULL signal, writes the R + 1 zeros itself."""
    eng = engine(tag)
    sig_d = torch.zeros(0, eng.t_dec, device=eng.device)
    for R in (0, 1, 4):
        rf_d = torch.zeros(R + 1, dtype=torch.int32, device=eng.device)
        got = eng.export_reads(sig_d, rf_d, *CAL, want_pa=True, want_dac=True)
        assert got["offsets"].dtype == torch.int64 and got["offsets"].cpu().tolist() == [0] * (R + 1)
        assert got["pa"].numel() == 0 and got["dac"].numel() == 0
        mine = torch.full((R + 3,), -7, dtype=torch.int64, device=eng.device)
        got = eng.export_reads(sig_d, rf_d, *CAL, rna=True, want_pa=False, want_dac=True, out_offsets=mine)
        assert got["offsets"].data_ptr() == mine.data_ptr() and mine.cpu().tolist() == [0] * (R + 1) + [-7, -7]
    some = torch.ones(1, eng.t_dec, device=eng.device)
    bufs = cabi_export(eng, some, torch.zeros(4, dtype=torch.int32, device=eng.device), CAL, True, eng.t_dec, n_chunks=0)
    assert holds_exactly(bufs["offsets"], np.zeros(4, np.int64))
    assert holds_exactly(bufs["pa"], np.zeros(0, np.float32)) and holds_exactly(bufs["dac"], np.zeros(0, np.int16))
