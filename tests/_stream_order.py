"""The late-input harness of tests/test_gpu_stream_order.py ("Tests of stream order").

include/s2s_hip.h promises that every device entry orders all its work on the stream it is given and does not wait for it.  A test
whose inputs are complete before the call cannot see a launch, memset or copy that went to another stream: it reads finished inputs
there too.  Here the inputs are LATE: the input tensors hold a decoy, the side stream is held back by a device-side delay, the real
inputs are copied in behind the delay, and the entry is called behind that copy.  Work that escaped the stream runs at once, reads
the decoy and gives the decoy's answer.

  delay            torch.cuda._sleep where torch has it, else a chain of matmuls; cycles (or matmuls) per millisecond are measured
                   once per session with two events on an idle stream.  A case's delay is 10 x t_solo (the entry timed alone on the
                   default stream), at least 20 ms, at most 500 ms; two events around it show afterwards that it really lasted 10 x
                   t_solo.
  decoy            a well formed input of the same shapes (other bases, samples, targets): a misordered kernel reads wrong data, never
                   a bad address.  Everything that carries addresses or sizes (offsets, chunk_start, lengths, capacities) is the same in
                   both and in place before the delay.  Every case shows that the decoy alone gives other bytes.
  early            right behind the call, on the same stream: the decoys are copied back over the inputs and the outputs are cloned,
                   before any host synchronisation -- an entry that returns with work still to be queued, or reads its inputs later,
                   shows.
  returned_before  right behind the call stream.query() is false: the delay still runs, so the entry did not wait for the stream.

Two forms.  `run_case` drives an entry that takes device tensors (Engine, Trainer).  `Late` drives the handle-free signal entries
through the package's own batch layer: inside it seq2squiggle_amd.signal_batch.Batch is `LateBatch`, whose upload is late in the sense
above, whose `call` notes every entry and whether it returned before the delay ended, and whose result buffers do `early` before they
come down.  Every result is compared with the same call on the default stream bit for bit, and with the host twin where there is one."""
import contextlib
import time

import numpy as np

MIN_MS, MAX_MS, FACTOR = 20.0, 500.0, 10.0
RECORDS = []                 # (case, t_solo ms, delay asked ms, delay measured ms): printed, and copied into LABNOTES.md
_RATE = {}


def _torch():
    import torch
    return torch


def rate():
    """-> ("sleep", cycles per ms) or ("matmul", products of two 2048^2 matrices per ms), measured once on an idle stream."""
    if _RATE:
        return _RATE["kind"], _RATE["per_ms"]
    torch = _torch()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        kind, n = "sleep", 20_000_000
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)                              # (the first launch of the kernel is not what is measured)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
    else:
        kind, n = "matmul", 20
        with torch.cuda.stream(s):
            a = torch.ones(2048, 2048, device="cuda")
            b = a @ a
            e0.record()
            for _ in range(n):
                b = a @ a
            e1.record()
    s.synchronize()
    _RATE.update(kind=kind, per_ms=n / e0.elapsed_time(e1))
    print(f"\nSTREAM-ORDER rate: {kind}, {_RATE['per_ms']:.1f} per ms")
    return kind, _RATE["per_ms"]


def delay(stream, ms):
    """Queue a device-side wait of about `ms` milliseconds on `stream` -> the two events around it."""
    torch = _torch()
    kind, per_ms = rate()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        if kind == "sleep":
            torch.cuda._sleep(int(ms * per_ms))
        else:
            a = torch.ones(2048, 2048, device="cuda")
            for _ in range(int(ms * per_ms) + 1):
                a @ a
        e1.record()
    return e0, e1


_SIDE = []


def runs_beside(stream, others):
    """True if work on each of `others` completes while a delay holds `stream`: they do not share a hardware queue with it (streams
    that do are served one after the other, and a launch that escaped to such a stream would wait for the delay like a right one)."""
    torch = _torch()
    torch.cuda.synchronize()
    x = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    delay(stream, 2 * MIN_MS)
    t0 = time.perf_counter()
    for o in others:
        with torch.cuda.stream(o):
            x.add_(1)
        o.synchronize()
    beside = not stream.query() and time.perf_counter() - t0 < 1e-3 * MIN_MS
    stream.synchronize()
    return beside


def side_stream(i=0):
    """Side stream i of the session (0 or 1): at most two live beside the default stream, so that each has a hardware queue of its
    own (the runtime opens four) -- which is measured here, not assumed: a candidate is taken only if work on the default stream (and
    on side stream 0) runs to its end while a delay holds the candidate."""
    torch = _torch()
    assert i in (0, 1)
    tried = 0
    while len(_SIDE) <= i:
        c = torch.cuda.Stream()
        tried += 1
        assert tried <= 64, "no stream with a hardware queue of its own beside the default stream"
        others = [torch.cuda.default_stream()] + _SIDE
        if runs_beside(c, others) and all(runs_beside(o, [c]) for o in others[1:]):
            _SIDE.append(c)
            print(f"\nSTREAM-ORDER side stream {len(_SIDE)}: candidate {tried} runs beside the default stream")
    return _SIDE[i]


def delay_for(t_solo_ms):
    """The delay to ask for: 10 x t_solo, at least 20 ms, plus a fifth (the calibrated rate is a mean; what is asserted afterwards is
    the measured length); at most 500 ms."""
    want = 1.2 * max(FACTOR * t_solo_ms, MIN_MS)
    assert want <= MAX_MS, f"the case runs {t_solo_ms:.2f} ms alone: too large for a delay of at most {MAX_MS} ms"
    return want


def lasted(case, events, t_solo_ms, asked_ms):
    """After the stream was synchronised: the delay really lasted 10 x t_solo."""
    got = events[0].elapsed_time(events[1])
    RECORDS.append((case, t_solo_ms, asked_ms, got))
    print(f"\nSTREAM-ORDER case {case}: t_solo {t_solo_ms:.3f} ms, delay asked {asked_ms:.1f} ms, measured {got:.1f} ms")
    assert got >= FACTOR * t_solo_ms and MIN_MS <= got <= MAX_MS, (case, got, t_solo_ms)


def timed(fn):
    """fn() on the current (default) stream between two events -> (its result, milliseconds)."""
    torch = _torch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


# ------------------------------------------------------------------ results as bytes
class Flat(list):
    """What flat() returns (flat() of it is itself)."""


def flat(x, out=None, path=""):
    """Any nesting of dicts, lists, tuples, tensors, arrays and numbers -> [(path, the bytes as a numpy array, or the value)]."""
    if isinstance(x, Flat):
        return x
    out = Flat() if out is None else out
    torch = _torch()
    if isinstance(x, dict):
        for k in sorted(x):
            flat(x[k], out, f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            flat(v, out, f"{path}[{i}]")
    elif isinstance(x, torch.Tensor):
        t = x.detach().cpu().contiguous()
        out.append((path, t.view(torch.uint8).numpy().copy() if t.numel() else np.zeros(0, np.uint8)))
    elif isinstance(x, np.ndarray):
        out.append((path, np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()))
    else:
        out.append((path, x))
    return out


def same(a, b):
    """Bit equality of two flattened results -> the first path that differs, or None."""
    a, b = flat(a), flat(b)
    if [p for p, _ in a] != [p for p, _ in b]:
        return "structure"
    for (p, x), (_, y) in zip(a, b):
        if isinstance(x, np.ndarray) != isinstance(y, np.ndarray):
            return p
        if isinstance(x, np.ndarray):
            if x.shape != y.shape or not np.array_equal(x, y):
                return p
        elif x != y:
            return p
    return None


# ------------------------------------------------------------------ entries that take device tensors
def decoys(decoy):
    """Step 1 of `late`: the input tensors, filled with the decoy (the caller synchronises once all of them exist)."""
    return {k: v.clone() for k, v in decoy.items()}


def hold(stream, ins, real, ms):
    """Steps 2 and 3 of `late`: the delay on `stream`, then the copies of the real inputs into `ins` -> the delay's events."""
    torch = _torch()
    ev = delay(stream, ms)
    with torch.cuda.stream(stream):
        for k in ins:
            ins[k].copy_(real[k])
    return ev


def late(stream, real, decoy, ms, between=None):
    """real / decoy: {name: device tensor}, complete.  -> (the input tensors, the delay's events[, between()'s result]): the inputs hold
    the decoy, the device is idle, and `stream` holds the delay and, behind it, the copies of the real inputs.  between(): runs on
    `stream` after the synchronisation and before the delay (a handle created there meets no synchronisation before its first launch)."""
    torch = _torch()
    ins = decoys(decoy)
    torch.cuda.synchronize()
    made = None
    if between is not None:
        with torch.cuda.stream(stream):
            made = between()
    ev = hold(stream, ins, real, ms)
    return (ins, ev) if between is None else (ins, ev, made)


def early(stream, ins, decoy, outs):
    """Behind the call, before any host synchronisation: decoys back over the inputs, clones of the output tensors."""
    torch = _torch()
    with torch.cuda.stream(stream):
        for k in ins:
            ins[k].copy_(decoy[k])
        return [(p, v.clone()) for p, v in _tensors(outs)]


def _tensors(x, path=""):
    torch = _torch()
    if isinstance(x, dict):
        for k in sorted(x):
            yield from _tensors(x[k], f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _tensors(v, f"{path}[{i}]")
    elif isinstance(x, torch.Tensor) and x.is_cuda:
        yield path, x


def returned_before(stream):
    """The delay still holds the stream: the entry that just returned did not synchronise the host with it."""
    return not stream.query()


def up(arrays):
    torch = _torch()
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in arrays.items()}


def run_case(name, fresh, call, real, decoy, fixed=None, synchronises=None, side=None, warm=True, fresh_on_side=False, host_after=None):
    """One late-input case of an entry that takes device tensors.
    fresh()           -> the object the entry runs on (a shared engine, or a new trainer: anything with state of its own is new);
    call(obj, ins)    runs the entry (or sequence of entries) on the CURRENT stream -> its outputs, any nesting of device tensors and
                      host values; `ins` holds the late inputs and the fixed ones by name;
    real, decoy       {name: array}: the late inputs (decoy None: the entry takes no input tensor); fixed: {name: array}: what carries addresses and sizes, the same in both;
    synchronises      None, or the header line that says the entry waits for the stream: returned_before is not asserted;
    warm              run the call once on the default stream first (workspaces grow there, not inside the delay);
    fresh_on_side     the side stream's object is made inside the side stream's context, right before the delay is queued;
    host_after(obj)   behind the call: an entry that hands values to the host (and so waits for the stream) -> those values.
    -> (the side stream's result, the default stream's), equal bit for bit."""
    torch = _torch()
    real_d, decoy_d, fixed_d = up(real), up(decoy or {}), up(fixed or {})
    assert sorted(real_d) == sorted(decoy_d) and all(real_d[k].shape == decoy_d[k].shape and real_d[k].dtype == decoy_d[k].dtype for k in real_d)
    torch.cuda.synchronize()
    clone = lambda d: {k: v.clone() for k, v in d.items()}      # noqa: E731
    if warm:
        call(fresh(), {**fixed_d, **clone(real_d)})
    obj = fresh()
    ins0 = {**fixed_d, **clone(real_d)}
    want, t_solo = timed(lambda: call(obj, ins0))
    want = flat(want)
    want_host = flat(host_after(obj)) if host_after else None
    if decoy is not None:                                       # (None: an entry without input tensors)
        of_decoy = flat(call(fresh(), {**fixed_d, **clone(decoy_d)}))
        assert same(want, of_decoy) is not None, f"{name}: the decoy gives the real input's bytes: the case proves nothing"
    side = side or side_stream(0)
    ms = delay_for(t_solo)
    if fresh_on_side:
        ins, ev, obj = late(side, real_d, decoy_d, ms, between=fresh)
    else:
        obj = fresh()
        ins, ev = late(side, real_d, decoy_d, ms)
    with torch.cuda.stream(side):
        got = call(obj, {**fixed_d, **ins})
    before = returned_before(side)
    snaps = early(side, ins, decoy_d, got)
    if host_after:
        with torch.cuda.stream(side):
            got_host = flat(host_after(obj))
        assert same(got_host, want_host) is None, f"{name}: the values handed to the host are not those of the real inputs: {same(got_host, want_host)}"
    side.synchronize()
    lasted(name, ev, t_solo, ms)
    if synchronises is None:
        assert before, f"{name}: the entry returned only after the stream had drained: it synchronised the host"
    bad = same(got, want)
    assert bad is None, f"{name}: {bad} on the side stream differs from the default stream's"
    want_t = dict((p, v) for p, v in want if isinstance(v, np.ndarray))
    for p, v in snaps:
        assert np.array_equal(flat(v)[0][1], want_t[p]), f"{name}: {p} was not complete in stream order behind the call"
    torch.cuda.synchronize()
    return got, want


# ------------------------------------------------------------------ the handle-free entries, through the batch layer
def other_samples(records, seed=12345):
    """The decoy of int16 records: other samples of the same lengths and range."""
    rng = np.random.default_rng(seed)
    out = []
    for r in records:
        r = np.asarray(r, np.int16).reshape(-1)
        lo, hi = (int(r.min()), int(r.max()) + 1) if len(r) else (0, 1)
        out.append(rng.integers(lo, hi, len(r)).astype(np.int16))
    return out


class Late:
    """with Late(name, modules, t_solo, ...) as h: the wrappers of `modules` (those of seq2squiggle_amd that import Batch) run on a side
    stream with late uploads.  decoy_records(i, records) / decoy_tables(i, tables) -> the decoy of batch i's records / evaluated tables
    (default: other_samples / the tables as they are).  mode "late" (above) or "decoy" (the decoy alone on the current stream: what a
    stray kernel would compute).  After the block: h.calls = [(entry, returned before the delay ended)]."""

    def __init__(self, name, modules, t_solo=0.0, decoy_records=None, decoy_tables=None, mode="late", side=None):
        torch = _torch()
        self.name, self.modules, self.t_solo, self.mode = name, modules, t_solo, mode
        self.decoy_records = decoy_records or (lambda i, recs: other_samples(recs, 12345 + i))
        self.decoy_tables = decoy_tables or (lambda i, tabs: tabs)
        self.side = side or (side_stream(0) if mode == "late" else None)
        self.calls, self.batches, self.events, self.done, self.snaps = [], [], None, False, []

    def __enter__(self):
        from seq2squiggle_amd import signal_batch
        torch, h = _torch(), self
        Real = signal_batch.Batch

        class LateFields(signal_batch.Fields):
            def fetch(self):
                if h.mode == "late" and not h.done:            # early: decoys back, a clone of the results, then the copy down
                    h.done = True
                    for b in h.batches:
                        b.up.copy_(b.decoy_up)
                    snap = self.buf.clone()
                    raw = super().fetch()
                    h.snaps.append((snap, self.buf))
                    return raw
                return super().fetch()

        class LateBatch(Real):
            def __init__(self, records, tables=(), cpu=False, device=0, threads=None):
                assert not cpu
                i = len(h.batches)
                recs = [np.ascontiguousarray(r, np.int16).reshape(-1) for r in records]
                decoy_recs = h.decoy_records(i, recs)
                assert [len(r) for r in decoy_recs] == [len(r) for r in recs]
                with torch.cuda.stream(torch.cuda.default_stream()):
                    Real.__init__(self, recs, tables, cpu, device, threads)
                    given = [signal_batch.device_only(lambda t=t: t) if j in self._device_tables else t for j, t in enumerate(self.tables)]
                    d = Real(decoy_recs, h.decoy_tables(i, given), cpu, device, threads)
                    assert d.up.shape == self.up.shape and np.array_equal(d.host_offs, self.host_offs)
                    self.decoy_up = d.up
                    if h.mode == "decoy":
                        self.up.copy_(self.decoy_up)
                    else:
                        self.real_up = self.up.clone()
                        self.up.copy_(self.decoy_up)
                    torch.cuda.default_stream().synchronize()
                h.batches.append(self)
                if h.mode == "late":
                    self.stream = h.side.cuda_stream
                    if h.events is None:
                        torch.cuda.synchronize()
                        h.ms = delay_for(h.t_solo)
                        h.events = delay(h.side, h.ms)
                    self.up.copy_(self.real_up)                # (the current stream is the side stream)

            def alloc(self, **fields):
                return LateFields(self, fields)

            def marked(self, q, at, mask, value):
                """Batch.marked with the mask (which k-mers have no level: the same in real and decoy) uploaded on the default
                stream: a pageable upload on the held stream would wait for the delay, and every later entry would run behind it."""
                if q == self.samples:
                    q = self._copy(False, raw=True)
                if len(mask):
                    with torch.cuda.stream(torch.cuda.default_stream()):
                        m = torch.from_numpy(np.ascontiguousarray(mask)).to(self.where)
                        torch.cuda.default_stream().synchronize()
                    self._pool[at:at + len(mask)].masked_fill_(m, value)
                return q

            def call(self, name, *args):
                assert not h.done, "an entry was called after the results came down"
                Real.call(self, name, *args)
                h.calls.append((name, h.mode != "late" or returned_before(h.side)))

        self._saved = [(m, m.Batch) for m in self.modules]
        for m in self.modules:
            m.Batch = LateBatch
        self._ctx = torch.cuda.stream(self.side) if self.mode == "late" else contextlib.nullcontext()
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self._ctx.__exit__(*exc)
        for m, b in self._saved:
            m.Batch = b
        if exc[0] is None and self.mode == "late":
            self.side.synchronize()
            assert self.events is not None, f"{self.name}: no batch was made"
            lasted(self.name, self.events, self.t_solo, self.ms)
            for snap, buf in self.snaps:
                assert bool((snap == buf).all()), f"{self.name}: the results were not complete in stream order behind the last call"
        return False


def run_wrapped(name, modules, fn, entries, twin=None, decoy_records=None, decoy_tables=None, synchronises=()):
    """One late-input case through the batch layer.  fn(cpu) -> the wrapper's result; entries: the set of entries the case must run;
    twin: fn(True) is the host twins' answer and must be equal too.  -> the result."""
    fn(False)                                                   # warm: the first launch of every kernel is not what is timed
    want, t_solo = timed(lambda: fn(False))
    with Late(name, modules, decoy_records=decoy_records, decoy_tables=decoy_tables, mode="decoy") as d:
        of_decoy = fn(False)
    assert {c for c, _ in d.calls} == set(entries), (name, sorted({c for c, _ in d.calls}))
    assert same(want, of_decoy) is not None, f"{name}: the decoy gives the real input's bytes: the case proves nothing"
    t0 = time.perf_counter()
    with Late(name, modules, t_solo, decoy_records, decoy_tables) as h:
        got = fn(False)
    assert {c for c, _ in h.calls} == set(entries), (name, h.calls)
    for entry, before in h.calls:
        assert before or entry in synchronises, f"{name}: s2s_{entry} returned only after the stream had drained (host part {time.perf_counter() - t0:.3f} s)"
    bad = same(got, want)
    assert bad is None, f"{name}: {bad} on the side stream differs from the default stream's"
    if twin is not None:
        bad = same(got, twin if not callable(twin) else twin())
        assert bad is None, f"{name}: {bad} differs from the host twin's"
    return got
