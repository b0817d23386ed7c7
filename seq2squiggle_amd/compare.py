"""`compare A B -o OUT.tsv`: how far the signals of two files are apart -- per pair of records the banded dynamic-time-warping (DTW)
distance between their median / MAD normalised int16 samples.  Everything is defined in integers (include/s2s_hip.h, next to
s2s_dtw_banded, states the definitions; tests/_dtw_ref.py restates them): the GPU kernels (csrc/s2s_dtw.h), their host twins
(`--cpu`) and any batching give the same bytes.  Per batch of pairs: one host-to-device copy (offsets and samples of both
sides), the three kernels, one device-to-host copy (cost, med, mad).  The reference has no such command and no DTW tool was
at hand to compare against: what is pinned is that every number is the stated integer function of exactly the int16 samples the
two files store -- DESIGN.md section 6."""
import logging
import os
from typing import Iterable, Sequence

import click
import numpy as np

logger = logging.getLogger("seq2squiggle")

SCALE = 64                       # S2S_DTW_SCALE: one MAD is 64 units
MAX_SAMPLES = 1 << 22            # S2S_DTW_MAX_SAMPLES per record
DEFAULT_BAND = 512
DEFAULT_MAX_SAMPLES = 1 << 27    # samples of both sides per batch: 256 MiB of int16 on the device, twice with the normalised copy
COLUMNS = ("read_id", "n_a", "n_b", "med_a", "mad_a", "med_b", "mad_b", "band", "dtw", "dtw_per_sample")


def max_band() -> int:
    from ._lib import lib
    return int(lib().s2s_dtw_max_band())


def _host_threads() -> int:
    from .signal_io import cpu_share
    return cpu_share()


def _check(rc: int, what: str) -> None:
    if rc != 0:
        from ._lib import lib
        raise RuntimeError(f"{what} failed ({rc}): {lib().s2s_last_error(None).decode()}")


def _pack(records: Sequence[np.ndarray]):
    """int16 records -> (flat int16, int64 offsets [len + 1]); a record longer than the kernels' limit is refused here, where the
    lengths are known (the device entries cannot see them)."""
    recs = [np.ascontiguousarray(r, dtype=np.int16).reshape(-1) for r in records]
    offs = np.zeros(len(recs) + 1, np.int64)
    if recs:
        np.cumsum([len(r) for r in recs], out=offs[1:])
        if max(len(r) for r in recs) > MAX_SAMPLES:
            raise ValueError(f"a record holds more than {MAX_SAMPLES} samples")
    flat = np.concatenate(recs) if recs else np.zeros(0, np.int16)
    return flat, offs


def _check_band(band: int) -> int:
    band = int(band)
    if not 1 <= band <= max_band():
        raise ValueError(f"band must be 1..{max_band()}")
    return band


class _Device:
    """One batch on the GPU: a single uint8 buffer up (offsets, then samples) and a single one down (cost, med, mad)."""

    def __init__(self, flat: np.ndarray, offs: np.ndarray, device: int = 0):
        import torch
        self.torch, self.device = torch, int(device)
        self.n_rec, self.total = len(offs) - 1, int(offs[-1])
        host = np.empty(offs.nbytes + flat.nbytes, np.uint8)
        host[:offs.nbytes] = offs.view(np.uint8)
        host[offs.nbytes:] = flat.view(np.uint8)
        self.up = torch.from_numpy(host).to(f"cuda:{self.device}")
        self.offs_ptr = self.up.data_ptr()
        self.samples_ptr = self.offs_ptr + offs.nbytes                       # (8-byte aligned: behind int64s)
        self.stream = torch.cuda.current_stream(self.device).cuda_stream

    def down(self, n_pairs: int):
        """The result buffer: [cost int64 x n_pairs][med int32 x n_rec][mad int32 x n_rec] -> (tensor, cost ptr, med ptr, mad ptr)."""
        t = self.torch.empty(8 * n_pairs + 8 * self.n_rec + 8, dtype=self.torch.uint8, device=f"cuda:{self.device}")
        p = t.data_ptr()
        return t, p, p + 8 * n_pairs, p + 8 * n_pairs + 4 * self.n_rec

    def scratch(self):
        return self.torch.empty(max(self.total, 1), dtype=self.torch.int16, device=f"cuda:{self.device}")


def _split_down(raw: np.ndarray, n_pairs: int, n_rec: int):
    cost = raw[:8 * n_pairs].view(np.int64).copy()
    med = raw[8 * n_pairs:8 * n_pairs + 4 * n_rec].view(np.int32).copy()
    mad = raw[8 * n_pairs + 4 * n_rec:8 * n_pairs + 8 * n_rec].view(np.int32).copy()
    return cost, med, mad


def median_mad(records: Sequence[np.ndarray], cpu: bool = False, device: int = 0):
    """-> (med int32 [n], mad int32 [n]): the lower median of every int16 record and the lower median of its |x - med|."""
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    from ._lib import lib
    L = lib()
    flat, offs = _pack(records)
    n = len(offs) - 1
    if cpu:
        med, mad = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(L.s2s_signal_median_mad_host(flat.ctypes.data, offs.ctypes.data, n, med.ctypes.data, mad.ctypes.data, _host_threads()),
               "s2s_signal_median_mad_host")
        return med, mad
    dev = _Device(flat, offs, device)
    t, _, med_p, mad_p = dev.down(0)
    _check(L.s2s_signal_median_mad(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, n, med_p, mad_p), "s2s_signal_median_mad")
    _, med, mad = _split_down(t.cpu().numpy(), 0, n)
    return med, mad


def normalise(records: Sequence[np.ndarray], med=None, mad=None, scale: int = SCALE, cpu: bool = False, device: int = 0):
    """-> list of int16 arrays: q = clamp(floor((2 (x - med) scale + d) / (2 d)), -32767, 32767), d = max(mad, 1); med / mad default
    to the records' own (median_mad)."""
    if not cpu:
        import torch  # noqa: F401
    from ._lib import lib
    L = lib()
    flat, offs = _pack(records)
    n = len(offs) - 1
    if med is None or mad is None:
        med, mad = median_mad(records, cpu=cpu, device=device)
    med = np.ascontiguousarray(med, dtype=np.int32)
    mad = np.ascontiguousarray(mad, dtype=np.int32)
    if med.shape != (n,) or mad.shape != (n,):
        raise ValueError("med and mad must hold one value per record")
    if cpu:
        out = np.empty(len(flat), np.int16)
        _check(L.s2s_signal_normalise_host(flat.ctypes.data, offs.ctypes.data, n, med.ctypes.data, mad.ctypes.data, int(scale),
                                           out.ctypes.data, _host_threads()), "s2s_signal_normalise_host")
    else:
        import torch
        dev = _Device(flat, offs, device)
        mm = torch.from_numpy(np.concatenate([med, mad])).to(f"cuda:{dev.device}")
        q = dev.scratch()
        _check(L.s2s_signal_normalise(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, n, mm.data_ptr(), mm.data_ptr() + 4 * n,
                                      int(scale), q.data_ptr()), "s2s_signal_normalise")
        out = q.cpu().numpy()[:len(flat)]
    return [out[offs[i]:offs[i + 1]] for i in range(n)]


def _run_batch(a_list, b_list, band: int, norm: bool, cpu: bool, device: int = 0, threads: int = None):
    """One batch of pairs -> (cost int64 [P], med int32 [2 P], mad int32 [2 P]); records 0..P-1 are A's, P..2P-1 B's."""
    from ._lib import lib
    L = lib()
    P = len(a_list)
    flat, offs = _pack(list(a_list) + list(b_list))
    if cpu:
        threads = threads or _host_threads()
        med, mad, cost = np.zeros(2 * P, np.int32), np.zeros(2 * P, np.int32), np.zeros(P, np.int64)
        _check(L.s2s_signal_median_mad_host(flat.ctypes.data, offs.ctypes.data, 2 * P, med.ctypes.data, mad.ctypes.data, threads),
               "s2s_signal_median_mad_host")
        q = flat
        if norm:
            q = np.empty(len(flat), np.int16)
            _check(L.s2s_signal_normalise_host(flat.ctypes.data, offs.ctypes.data, 2 * P, med.ctypes.data, mad.ctypes.data, SCALE,
                                               q.ctypes.data, threads), "s2s_signal_normalise_host")
        _check(L.s2s_dtw_banded_host(q.ctypes.data, offs.ctypes.data, q.ctypes.data, offs.ctypes.data + 8 * P, P, band,
                                     cost.ctypes.data, threads), "s2s_dtw_banded_host")
        return cost, med, mad
    dev = _Device(flat, offs, device)
    t, cost_p, med_p, mad_p = dev.down(P)
    _check(L.s2s_signal_median_mad(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, 2 * P, med_p, mad_p), "s2s_signal_median_mad")
    q_ptr = dev.samples_ptr
    if norm:
        q = dev.scratch()
        q_ptr = q.data_ptr()
        _check(L.s2s_signal_normalise(dev.device, dev.stream, dev.samples_ptr, dev.offs_ptr, 2 * P, med_p, mad_p, SCALE, q_ptr),
               "s2s_signal_normalise")
    _check(L.s2s_dtw_banded(dev.device, dev.stream, q_ptr, dev.offs_ptr, q_ptr, dev.offs_ptr + 8 * P, P, band, cost_p), "s2s_dtw_banded")
    return _split_down(t.cpu().numpy(), P, 2 * P)


def dtw_banded(a_list: Sequence[np.ndarray], b_list: Sequence[np.ndarray], band: int, cpu: bool = False, device: int = 0) -> np.ndarray:
    """The banded DTW cost (int64 [P]) of the int16 records a_list[p] against b_list[p] AS THEY ARE (no normalisation); -1 for a
    pair with an empty member."""
    if len(a_list) != len(b_list):
        raise ValueError("a_list and b_list must pair up")
    band = _check_band(band)
    if not cpu:
        import torch  # noqa: F401
    if not len(a_list):
        return np.zeros(0, np.int64)
    return _run_batch(a_list, b_list, band, False, cpu, device)[0]


# ------------------------------------------------------------------ files
def _open_records(path: str) -> Iterable[dict]:
    """-> iterator over the records of a .blow5 / .slow5 file of ours; anything else is a ClickException that names the file (the
    file's extension, magic number and end marker are checked here, before anything is written)."""
    from . import signal_io
    path = str(path)
    if path.endswith(".pod5"):
        raise click.UsageError(f"{path}: compare reads .blow5 and .slow5 files; reading POD5 is not supported")
    if not path.endswith((".blow5", ".slow5")):
        raise click.UsageError(f"{path}: compare reads .blow5 and .slow5 files")
    if not os.path.isfile(path):
        raise click.ClickException(f"{path}: no such file")
    if path.endswith(".slow5"):
        try:
            return iter(signal_io.read_slow5(path)[1])
        except (ValueError, IndexError, UnicodeDecodeError) as e:
            raise click.ClickException(f"{path}: not a SLOW5 file this project writes ({type(e).__name__}: {e})")
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(68)
        f.seek(max(size - 5, 0))
        tail = f.read(5)
    if len(head) < 68 or head[:6] != b"BLOW5\x01":
        raise click.ClickException(f"{path}: not a BLOW5 file (no BLOW5 magic number)")
    if tail != signal_io.BLOW5Writer._EOF:
        raise click.ClickException(f"{path}: truncated BLOW5 file (no end-of-file marker)")
    if head[9] not in (0, 1, 2) or head[14] not in (0, 1):
        raise click.ClickException(f"{path}: BLOW5 record / signal compression {head[9]} / {head[14]} is not one this project reads")

    def records():
        it = signal_io.iter_blow5(path)
        try:
            next(it)                                # the header text
            yield from it
        except Exception as e:                      # a damaged record: struct / zlib / codec errors, asserts of the reader
            raise click.ClickException(f"{path}: damaged BLOW5 record ({type(e).__name__}: {e})")
    return records()


def _pairs(a_path: str, b_path: str, by_order: bool):
    """-> generator of (read_id, signal a, signal b), counters {"unpaired_a", "unpaired_b", "records_a", "records_b"} (filled while
    the generator runs).  By id: B is held in memory by read id, A streams; A's order."""
    counts = dict(records_a=0, records_b=0, unpaired_a=0, unpaired_b=0)
    ia, ib = _open_records(a_path), _open_records(b_path)

    def gen():
        if by_order:
            while True:
                ra, rb = next(ia, None), next(ib, None)
                if ra is None and rb is None:
                    return
                counts["records_a"] += ra is not None
                counts["records_b"] += rb is not None
                if ra is None or rb is None:
                    counts["unpaired_a" if rb is None else "unpaired_b"] += 1
                    continue
                yield ra["read_id"], np.asarray(ra["signal"], np.int16), np.asarray(rb["signal"], np.int16)
        else:
            b = {}
            for r in ib:
                counts["records_b"] += 1
                b.setdefault(r["read_id"], np.array(r["signal"], np.int16))
            used = set()
            for r in ia:
                counts["records_a"] += 1
                rid = r["read_id"]
                if rid not in b or rid in used:
                    counts["unpaired_a"] += 1
                    continue
                used.add(rid)
                yield rid, np.asarray(r["signal"], np.int16), b[rid]
            counts["unpaired_b"] = counts["records_b"] - len(used)
    return gen(), counts


def _row(rid, n_a, n_b, med_a, mad_a, med_b, mad_b, band, cost) -> str:
    per = "nan" if cost < 0 else "%.6f" % (float(cost) / float(n_a + n_b) / float(SCALE))
    return f"{rid}\t{n_a}\t{n_b}\t{med_a}\t{mad_a}\t{med_b}\t{mad_b}\t{band}\t{cost if cost >= 0 else 'nan'}\t{per}\n"


def compare_files(a_path, b_path, out, band: int = DEFAULT_BAND, normalise: str = "mad", by_order: bool = False,
                  max_samples: int = DEFAULT_MAX_SAMPLES, cpu: bool = False, device: int = 0) -> dict:
    """Write OUT.tsv (COLUMNS; one row per pair, A's order) and return the summary: pairs, records and unpaired records per file,
    mean and median of dtw_per_sample over the pairs that have one.  `normalise` = "mad" | "none" (`none`: the stored samples as they
    are, in units of 1 / 64 ADC count per sample in the last column).  A batch holds pairs until the samples of both sides pass
    max_samples (at least one pair)."""
    if normalise not in ("mad", "none"):
        raise ValueError("normalise must be 'mad' or 'none'")
    if int(max_samples) < 1:
        raise ValueError("max_samples must be >= 1")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    band = _check_band(band)
    pairs, counts = _pairs(str(a_path), str(b_path), by_order)
    per_sample = []
    n_pairs = 0
    with open(out, "w") as f:
        f.write("\t".join(COLUMNS) + "\n")

        def flush(batch):
            P = len(batch)
            cost, med, mad = _run_batch([p[1] for p in batch], [p[2] for p in batch], band, normalise == "mad", cpu, device)
            for i, (rid, a, b) in enumerate(batch):
                c = int(cost[i])
                f.write(_row(rid, len(a), len(b), int(med[i]), int(mad[i]), int(med[P + i]), int(mad[P + i]), band, c))
                if c >= 0:
                    per_sample.append(float(c) / float(len(a) + len(b)) / float(SCALE))

        batch, held = [], 0
        for rid, a, b in pairs:
            if len(a) > MAX_SAMPLES or len(b) > MAX_SAMPLES:
                raise click.ClickException(f"read {rid}: more than {MAX_SAMPLES} samples")
            if batch and held + len(a) + len(b) > max_samples:
                flush(batch)
                batch, held = [], 0
            batch.append((rid, a, b))
            held += len(a) + len(b)
            n_pairs += 1
        if batch:
            flush(batch)
    summary = dict(a=str(a_path), b=str(b_path), out=str(out), band=band, normalise=normalise, pairs=n_pairs,
                   records_a=counts["records_a"], records_b=counts["records_b"], unpaired_a=counts["unpaired_a"],
                   unpaired_b=counts["unpaired_b"],
                   mean_dtw_per_sample=float(np.mean(per_sample)) if per_sample else None,
                   median_dtw_per_sample=float(np.median(per_sample)) if per_sample else None)
    if counts["unpaired_a"] or counts["unpaired_b"]:
        logger.warning("compare: %d record(s) of %s and %d of %s have no partner", counts["unpaired_a"], a_path, counts["unpaired_b"], b_path)
    return summary
