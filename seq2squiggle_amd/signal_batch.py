"""The batch layer under `compare`, `resquiggle` and `segment`: the one place that knows whether a batch of stored int16 records is
solved by the GPU entry points (include/s2s_hip.h) or by their host twins (`--cpu`).  A `Batch` packs the records once and, on the
device, uploads them once; it hands out pointers that are valid on the side that was chosen, result buffers of named fields
(`alloc`) that come back in one copy, and `call`, which runs s2s_<name> or s2s_<name>_host on the same arguments.  What else the
three commands share lives here too: the limits, `open_records`, the record calibration with the event level formula, and
`batches`, the budget loop -- DESIGN.md section 4, "The batch layer"."""
import math
import os
from typing import Callable, Iterable, Iterator, Sequence

import click
import numpy as np

SCALE = 64                       # S2S_DTW_SCALE: one MAD is 64 units
MAX_SAMPLES = 1 << 22            # S2S_DTW_MAX_SAMPLES per record


def max_band() -> int:
    from ._lib import lib
    return int(lib().s2s_dtw_max_band())


def host_threads() -> int:
    from .signal_io import cpu_share
    return cpu_share()


def check(rc: int, what: str) -> None:
    if rc != 0:
        from ._lib import lib
        raise RuntimeError(f"{what} failed ({rc}): {lib().s2s_last_error(None).decode()}")


def check_band(band: int) -> int:
    band = int(band)
    if not 1 <= band <= max_band():
        raise ValueError(f"band must be 1..{max_band()}")
    return band


def pack(records: Sequence[np.ndarray]):
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


def slots(need) -> np.ndarray:
    """Sizes -> int64 [len + 1] offsets of consecutive slots of these sizes."""
    return np.concatenate([[0], np.cumsum(need)]).astype(np.int64)


def _layout(sizes):
    """Byte sizes -> (the start of every part, each a multiple of 8 bytes: aligned for every item size in use; bytes in all)."""
    starts, at = [], 0
    for n in sizes:
        starts.append(at)
        at += (int(n) + 7) // 8 * 8
    return starts, at


def sample_at(pool: int, i: int) -> int:
    """The pointer of int16 sample i of the pool at `pool`."""
    return pool + 2 * int(i)


class device_only:
    """An argument of `Batch.call` that only the device entry point has (decision scratch and its slot offsets)."""

    def __init__(self, value):
        self.value = value


class Fields:
    """One result buffer of named, typed fields (`Batch.alloc`), zeroed.  Every field starts at a multiple of 8 bytes; a field of
    no items still owns one, so that its pointer is a valid one.  `buf`: the buffer, numpy or torch uint8.  zero=False: the buffer
    is left uninitialised (outputs of which only a prefix is ever read: `prefix`)."""

    def __init__(self, batch: "Batch", fields: dict, zero: bool = True):
        self.fields = {name: (np.dtype(dt), int(count)) for name, (dt, count) in fields.items()}
        starts, nbytes = _layout([dt.itemsize * max(count, 1) for dt, count in self.fields.values()])
        self._at = dict(zip(self.fields, starts))
        if batch.cpu:
            self.buf = (np.zeros if zero else np.empty)(nbytes, np.uint8)
            self._base = self.buf.ctypes.data
        else:
            self.buf = (batch.torch.zeros if zero else batch.torch.empty)(nbytes, dtype=batch.torch.uint8, device=batch.where)
            self._base = self.buf.data_ptr()

    def ptr(self, name: str) -> int:
        return self._base + self._at[name]

    def fetch(self) -> dict:
        """-> {name: numpy array}: views of the host buffer, or of the ONE device-to-host copy of the whole buffer."""
        raw = self.buf if isinstance(self.buf, np.ndarray) else self.buf.cpu().numpy()
        return {name: raw[self._at[name]:self._at[name] + dt.itemsize * count].view(dt) for name, (dt, count) in self.fields.items()}

    def prefix(self, name: str, count: int) -> np.ndarray:
        """The first `count` items of one field on the host: a copy down of these bytes alone."""
        dt, have = self.fields[name]
        part = self.buf[self._at[name]:self._at[name] + dt.itemsize * min(int(count), have)]
        return (part.copy() if isinstance(part, np.ndarray) else part.cpu().numpy()).view(dt)


class Batch:
    """One batch of int16 records with the tables that travel with them (problem tables, slot offsets, event offsets: integer arrays,
    or a function of the packed offsets [n_rec + 1] that returns them; `tables` keeps them, `table(i)` is the pointer of table i).
    A table only the device entry point reads is given as device_only(function that returns it): the host never forms it (None in
    `tables`) and its `table(i)` is a device_only argument.  Host: the packed arrays as they are, `threads` host threads.  Device: ONE uint8 buffer up -- offsets, then the tables, then the
    samples, each part at a multiple of 8 bytes -- and the current stream of `device`."""

    def __init__(self, records: Sequence[np.ndarray], tables=(), cpu: bool = False, device: int = 0,
                 threads: int = None):
        self.flat, self.host_offs = pack(records)
        self.n_rec, self.total = len(self.host_offs) - 1, int(self.host_offs[-1])
        self.cpu, self.device = bool(cpu), int(device)
        given = list(tables(self.host_offs) if callable(tables) else tables)
        self._device_tables = {i for i, t in enumerate(given) if isinstance(t, device_only)}
        self.tables = [None if self.cpu and i in self._device_tables else
                       np.ascontiguousarray(t.value() if i in self._device_tables else t).reshape(-1) for i, t in enumerate(given)]
        parts = [self.host_offs] + [np.zeros(0, np.int64) if t is None else t for t in self.tables] + [self.flat]
        self._pool = None                               # the normalised / marked copy of the samples, once there is one
        self._keep = []                                 # device scratch, alive as long as the batch
        if self.cpu:
            self.threads = threads or host_threads()
            ptrs = [p.ctypes.data for p in parts]
        else:
            import torch
            self.torch, self.where = torch, f"cuda:{self.device}"
            starts, nbytes = _layout([p.nbytes for p in parts])
            host = np.empty(nbytes, np.uint8)           # (the padding behind a part goes up as it is: no entry point reads it)
            for s, p in zip(starts, parts):
                host[s:s + p.nbytes] = p.view(np.uint8)
            self.up = torch.from_numpy(host).to(self.where)
            ptrs = [self.up.data_ptr() + s for s in starts]
            self.stream = torch.cuda.current_stream(self.device).cuda_stream
        self._offs, *self._tables, self.samples = ptrs

    def offs(self, i: int = 0) -> int:
        """The pointer of the record offsets from record i on."""
        return self._offs + 8 * int(i)

    def table(self, i: int):
        return device_only(self._tables[i]) if i in self._device_tables else self._tables[i]

    def alloc(self, **fields) -> Fields:
        """field=(dtype, count), ... -> one zeroed result buffer on the batch's side."""
        return Fields(self, fields)

    def alloc_raw(self, **fields) -> Fields:
        """`alloc` without the zeroing."""
        return Fields(self, fields, zero=False)

    def scratch(self, nbytes) -> device_only:
        """Uninitialised device scratch of nbytes (at least 16; a number, or a function that returns it); nothing on the host, whose
        twins keep their own: the function is not called there."""
        if self.cpu:
            return device_only(None)
        nbytes = nbytes() if callable(nbytes) else nbytes
        self._keep.append(self.torch.empty(max(int(nbytes), 16), dtype=self.torch.uint8, device=self.where))
        return device_only(self._keep[-1].data_ptr())

    def call(self, name: str, *args) -> None:
        """s2s_<name>_host(*args, threads) or s2s_<name>(device, stream, *args); `device_only` arguments are dropped on the host.  A
        return code other than 0 is a RuntimeError with the library's message."""
        from ._lib import lib
        if self.cpu:
            fn, full = f"s2s_{name}_host", [a for a in args if not isinstance(a, device_only)] + [self.threads]
        else:
            fn, full = f"s2s_{name}", [self.device, self.stream] + [a.value if isinstance(a, device_only) else a for a in args]
        check(getattr(lib(), fn)(*full), fn)

    def _copy(self, zero: bool, raw: bool = False) -> int:
        """A second pool of the samples' size (at least one sample): zeroed, uninitialised or the raw samples -> its pointer."""
        if self.cpu:
            self._pool = self.flat.copy() if raw else (np.zeros if zero else np.empty)(len(self.flat), np.int16)
            return self._pool.ctypes.data
        torch, n = self.torch, max(self.total, 1)
        if raw and self.total:
            at = self.samples - self.up.data_ptr()
            self._pool = self.up[at:at + 2 * self.total].view(torch.int16).clone()
        else:
            self._pool = (torch.zeros if zero or raw else torch.empty)(n, dtype=torch.int16, device=self.where)
        return self._pool.data_ptr()

    def measure(self, med: int, mad: int, n: int = None) -> None:
        """s2s_signal_median_mad of the first n records (default: all) into med / mad, int32 pointers of one value per record."""
        self.call("signal_median_mad", self.samples, self.offs(), self.n_rec if n is None else n, med, mad)

    def normalised(self, med: int, mad: int, norm: bool = True, given: bool = False, halves: int = 0, scale: int = SCALE) -> int:
        """Median / MAD, then normalise: `measure` into med / mad (unless they are `given`), then s2s_signal_normalise by these values
        at `scale` into a second pool -> its pointer.  With norm off nothing runs and the raw samples' pointer comes back.  halves=P
        is the pool of `resquiggle`, 3 P records: P of samples, P of known levels that are only measured, P of all levels that are
        normalised by the values of the known ones; the rest of the second pool is 0."""
        if not norm:
            return self.samples
        P = int(halves)
        if not given:
            self.measure(med, mad, 2 * P if P else None)
        q = self._copy(zero=bool(P))
        for rec, stat, n in ([(0, 0, P), (2 * P, P, P)] if P else [(0, 0, self.n_rec)]):
            self.call("signal_normalise", self.samples, self.offs(rec), n, med + 4 * stat, mad + 4 * stat, int(scale), q)
        return q

    def marked(self, q: int, at: int, mask: np.ndarray, value: int) -> int:
        """-> the pointer of a pool like q with `value` in the samples at + i where mask[i] (a fill, no arithmetic): q itself if it is
        the second pool, else a copy of the raw samples, which are never written.  On the device the mask is one more upload."""
        if q == self.samples:
            q = self._copy(False, raw=True)
        if self.cpu:
            self._pool[at:at + len(mask)][mask] = value
        elif len(mask):
            self._pool[at:at + len(mask)].masked_fill_(self.torch.from_numpy(mask).to(self.where), value)
        return q

    def pool(self) -> np.ndarray:
        """The second pool on the host, int16 [total] (device: one copy down)."""
        return self._pool[:self.total] if self.cpu else self._pool.cpu().numpy()[:self.total]


def batches(items: Iterable, cost: Callable, limits: Sequence[int]) -> Iterator[list]:
    """Greedy batches of `items`, lazily: cost(item) -> a tuple as long as `limits`; a batch ends before the first item that would
    carry any running sum past its limit, and never ends empty (an item beyond a limit on its own gets a batch to itself)."""
    batch, held = [], [0] * len(limits)
    for item in items:
        c = cost(item)
        if batch and any(h + x > l for h, x, l in zip(held, c, limits)):
            yield batch
            batch, held = [], [0] * len(limits)
        batch.append(item)
        held = [h + x for h, x in zip(held, c)]
    if batch:
        yield batch


def calibration(rec: dict):
    """-> (digitisation, offset, range) of a stored record: pA = (x + offset) * range / digitisation."""
    return float(rec["digitisation"]), float(rec["offset"]), float(rec["range"])


def event_level(S: int, Q: int, n: int, cal):
    """Sum S and sum of squares Q of the n > 0 stored samples of an event -> (level, deviation) in pA by the formulas of the event
    table (include/s2s_hip.h, s2s_events_format), in double."""
    digitisation, offset, signal_range = cal
    mean = (float(S) / n + offset) * signal_range / digitisation
    stdv = math.sqrt(float(max(n * Q - S * S, 0))) / n * signal_range / digitisation
    return mean, stdv


def open_records(path: str) -> Iterable[dict]:
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
