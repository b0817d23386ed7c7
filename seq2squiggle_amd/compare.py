"""`compare A B -o OUT.tsv`: how far the signals of two files are apart -- per pair of records the banded dynamic-time-warping (DTW)
distance between their median / MAD normalised int16 samples.  Everything is defined in integers (include/s2s_hip.h, next to
s2s_dtw_banded, states the definitions; tests/_dtw_ref.py restates them): the GPU kernels (csrc/s2s_dtw.h), their host twins
(`--cpu`) and any batching give the same bytes.  Per batch of pairs (signal_batch.Batch): one host-to-device copy (offsets, tables
and samples of both sides), the three kernels, one device-to-host copy (cost, med, mad; with --path steps and ops as well).  The
reference has no such command and no DTW tool was at hand to compare against: what is pinned is that every number is the stated
integer function of exactly the int16 samples the two files store -- DESIGN.md section 6.

`--path` adds the warping path behind every distance (s2s_dtw_path: the sweep in an instance that stores one 2-bit decision per
in-band cell into a device scratch, then a walk back), written run-length encoded, and `--events-a / --events-out` carry the
k-mer boundaries of an event table of file A (`predict --events`) through the path onto B's samples (`boundary_map`,
`transfer_events`: plain numpy on the host).

`--open-ends` is for a B that carries samples A lacks in front and behind (a real read against a simulated one): per batch the
first and the last samples of A are located in the head and the tail of B by subsequence DTW (s2s_sdtw, csrc/s2s_sdtw.h: free
start, free end, exact integers like the rest; `sdtw`, `_anchors`), and the batch path above then runs on that interval of B."""
import logging
import os
from typing import Sequence

import click
import numpy as np

from .signal_batch import (MAX_SAMPLES, SCALE, Batch, batches, calibration, check_band, device_only, event_level, max_band,
                           open_records, slots)

logger = logging.getLogger("seq2squiggle")

DEFAULT_BAND = 512
DEFAULT_MAX_SAMPLES = 1 << 27    # samples of both sides per batch: 256 MiB of int16 on the device, twice with the normalised copy
COLUMNS = ("read_id", "n_a", "n_b", "med_a", "mad_a", "med_b", "mad_b", "band", "dtw", "dtw_per_sample")
DEFAULT_PATH_MEMORY = 8 << 30    # bytes of decision scratch per batch with --path
PATH_COLUMNS = ("read_id", "n_a", "n_b", "band", "dtw", "steps", "path")
EVENT_COLUMNS = ("read_name", "position", "model_kmer", "start_idx", "end_idx", "event_level_mean", "event_stdv")
OPS = "MAB"                      # S2S_DTW_OP_M, _A, _B
DEFAULT_ANCHOR = 1024            # --open-ends: samples of A's head and tail that are located in B (a choice, not a measurement)
DEFAULT_ANCHOR_WINDOW = 16384    # ... inside this many samples of B's head and tail (a choice as well)
OPEN_COLUMNS = ("b_start", "b_end", "head_cost", "tail_cost")


def median_mad(records: Sequence[np.ndarray], cpu: bool = False, device: int = 0):
    """-> (med int32 [n], mad int32 [n]): the lower median of every int16 record and the lower median of its |x - med|."""
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    B = Batch(records, cpu=cpu, device=device)
    res = B.alloc(med=(np.int32, B.n_rec), mad=(np.int32, B.n_rec))
    B.measure(res.ptr("med"), res.ptr("mad"))
    r = res.fetch()
    return r["med"], r["mad"]


def normalise(records: Sequence[np.ndarray], med=None, mad=None, scale: int = SCALE, cpu: bool = False, device: int = 0):
    """-> list of int16 arrays: q = clamp(floor((2 (x - med) scale + d) / (2 d)), -32767, 32767), d = max(mad, 1); med / mad default
    to the records' own (median_mad)."""
    if not cpu:
        import torch  # noqa: F401
    if med is None or mad is None:
        med, mad = median_mad(records, cpu=cpu, device=device)

    def given(offs):                                    # med, mad travel with the samples as two int32 tables
        tab = np.ascontiguousarray(med, dtype=np.int32), np.ascontiguousarray(mad, dtype=np.int32)
        if tab[0].shape != (len(offs) - 1,) or tab[1].shape != (len(offs) - 1,):
            raise ValueError("med and mad must hold one value per record")
        return tab
    B = Batch(records, given, cpu=cpu, device=device)
    B.normalised(B.table(0), B.table(1), given=True, scale=scale)
    out, offs = B.pool(), B.host_offs
    return [out[offs[i]:offs[i + 1]] for i in range(B.n_rec)]


def path_scratch_bytes(n: int, m: int, band: int) -> int:
    """Bytes of decision scratch s2s_dtw_path needs for a pair of n against m samples (0 for a pair without path)."""
    from ._lib import lib
    r = int(lib().s2s_dtw_path_scratch_bytes(int(n), int(m), int(band)))
    if r < 0:
        raise ValueError(f"band must be 1..{max_band()}")
    return r


def _split_ops(ops: np.ndarray, path_offs: np.ndarray, steps: np.ndarray):
    """The right-aligned paths of a batch -> one uint8 array per pair."""
    return [ops[int(e) - int(k):int(e)].copy() for e, k in zip(path_offs[1:], steps)]


def _run_batch(a_list, b_list, band: int, norm: bool, cpu: bool, device: int = 0, threads: int = None, path: bool = False):
    """One batch of pairs -> (cost int64 [P], med int32 [2 P], mad int32 [2 P]); records 0..P-1 are A's, P..2P-1 B's.  path=True:
    s2s_dtw_path instead of s2s_dtw_banded, and a fourth result: the ops of every pair (uint8 arrays, empty without a path)."""
    P = len(a_list)

    def path_tables(offs):
        """-> path_offs int64 [P + 1]: the pairs' slots of ops, n + m - 2 bytes for a pair with two non-empty members, else none;
        scratch_offs int64 [P + 1]: their slots of decision scratch, formed for the device only."""
        n, m = np.diff(offs[:P + 1]), np.diff(offs[P:])
        return (slots(np.where((n > 0) & (m > 0), n + m - 2, 0)),
                device_only(lambda: slots([path_scratch_bytes(n[i], m[i], band) for i in range(P)])))
    B = Batch(list(a_list) + list(b_list), path_tables if path else (), cpu, device, threads)
    fields = dict(cost=(np.int64, P), med=(np.int32, 2 * P), mad=(np.int32, 2 * P))
    if path:
        path_offs = B.tables[0]
        fields.update(steps=(np.int64, P), ops=(np.uint8, path_offs[-1]))
    res = B.alloc(**fields)
    q = B.normalised(res.ptr("med"), res.ptr("mad"), norm)
    if not norm:
        B.measure(res.ptr("med"), res.ptr("mad"))       # (med / mad are results either way)
    if path:
        B.call("dtw_path", q, B.offs(), q, B.offs(P), P, band, res.ptr("cost"), B.scratch(lambda: B.tables[1][-1]), B.table(1),
               res.ptr("ops"), B.table(0), res.ptr("steps"))
    else:
        B.call("dtw_banded", q, B.offs(), q, B.offs(P), P, band, res.ptr("cost"))
    r = res.fetch()
    if path:
        return r["cost"], r["med"], r["mad"], _split_ops(r["ops"], path_offs, r["steps"])
    return r["cost"], r["med"], r["mad"]


def dtw_banded(a_list: Sequence[np.ndarray], b_list: Sequence[np.ndarray], band: int, cpu: bool = False, device: int = 0) -> np.ndarray:
    """The banded DTW cost (int64 [P]) of the int16 records a_list[p] against b_list[p] AS THEY ARE (no normalisation); -1 for a
    pair with an empty member."""
    if len(a_list) != len(b_list):
        raise ValueError("a_list and b_list must pair up")
    band = check_band(band)
    if not cpu:
        import torch  # noqa: F401
    if not len(a_list):
        return np.zeros(0, np.int64)
    return _run_batch(a_list, b_list, band, False, cpu, device)[0]


# ------------------------------------------------------------------ open ends: subsequence DTW anchors
def max_query() -> int:
    from ._lib import lib
    return int(lib().s2s_sdtw_max_query())


def _check_anchor(anchor: int, anchor_window: int):
    anchor, anchor_window = int(anchor), int(anchor_window)
    if not 1 <= anchor <= max_query():
        raise ValueError(f"anchor must be 1..{max_query()}")
    if not 1 <= anchor_window <= MAX_SAMPLES:
        raise ValueError(f"anchor_window must be 1..{MAX_SAMPLES}")
    return anchor, anchor_window


def _problem_tables(q_begin, q_len, t_begin, t_len, reverse):
    """The problems of one s2s_sdtw call as the five tables of a Batch: int64 q_begin, q_len, t_begin, t_len [N], reverse uint8 [N]."""
    return (*(np.asarray(x, np.int64) for x in (q_begin, q_len, t_begin, t_len)), np.asarray(reverse, np.uint8))


def _sdtw(B: Batch, N: int, norm: bool = False):
    """s2s_sdtw of the N problems in B's tables on B's samples, with `norm` on their normalised copy (whole-record median / MAD), then
    the one copy of its results -> (cost, start, end) int64 [N]."""
    n_stat = B.n_rec if norm else 0
    res = B.alloc(cost=(np.int64, N), start=(np.int64, N), end=(np.int64, N), med=(np.int32, n_stat), mad=(np.int32, n_stat))
    q = B.normalised(res.ptr("med"), res.ptr("mad"), norm)
    B.call("sdtw", q, B.table(0), B.table(1), q, B.table(2), B.table(3), B.table(4), N, res.ptr("cost"), res.ptr("start"), res.ptr("end"))
    r = res.fetch()
    return r["cost"], r["start"], r["end"]


def sdtw(queries: Sequence[np.ndarray], targets: Sequence[np.ndarray], reverse=False, cpu: bool = False, device: int = 0):
    """Subsequence DTW (include/s2s_hip.h, next to s2s_sdtw) of the int16 record queries[p] inside targets[p] AS THEY ARE (no
    normalisation) -> (cost, start, end), int64 [P] each: the query matched targets[p][start:end]; cost -1, start = end = 0 for an
    empty member.  `reverse`: a bool, or one per problem -- the same problem on both records read back to front, the interval in
    forward coordinates."""
    if len(queries) != len(targets):
        raise ValueError("queries and targets must pair up")
    P = len(queries)
    rev = np.broadcast_to(np.asarray(reverse, bool), (P,)) if np.ndim(reverse) == 0 else np.asarray(reverse, bool)
    if rev.shape != (P,):
        raise ValueError("reverse must be a bool or hold one per problem")
    if any(np.size(x) > max_query() for x in queries):
        raise ValueError(f"a query holds more than {max_query()} samples")
    if not cpu:
        import torch  # noqa: F401
    if not P:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    B = Batch(list(queries) + list(targets), lambda offs: _problem_tables(offs[:P], np.diff(offs)[:P], offs[P:2 * P], np.diff(offs)[P:], rev),
              cpu, device)
    return _sdtw(B, P)


def _anchors(a_list, b_list, norm: bool, cpu: bool, device: int, anchor: int, anchor_window: int, threads: int = None):
    """Stage 1 of `--open-ends` for one batch of pairs: pack and normalise A and B as _run_batch does (whole-record median / MAD),
    then ONE s2s_sdtw call of 2 P problems on the normalised pool -- problem p: the first La = min(anchor, n_a) samples of A inside
    the first Hb = min(anchor_window, n_b) of B; problem P + p: the last La of A inside the last Hb of B, reversed -- and one
    device-to-host copy.  -> (cost, start, end) int64 [2 P], start / end relative to the target's window, and Hb [P]."""
    P = len(a_list)

    def problems(offs):
        na, nb = np.diff(offs)[:P], np.diff(offs)[P:]
        la, hb = np.minimum(anchor, na), np.minimum(anchor_window, nb)
        return _problem_tables(np.concatenate([offs[:P], offs[:P] + na - la]), np.concatenate([la, la]),
                               np.concatenate([offs[P:2 * P], offs[P:2 * P] + nb - hb]), np.concatenate([hb, hb]), [0] * P + [1] * P)
    B = Batch(list(a_list) + list(b_list), problems, cpu, device, threads)
    return (*_sdtw(B, 2 * P, norm), B.tables[3][:P])        # (t_len of the head problems is Hb)


def _check_path_memory(path_memory: int) -> int:
    if int(path_memory) < 1:
        raise ValueError("path_memory must be >= 1")
    return int(path_memory)


def dtw_path(a_list: Sequence[np.ndarray], b_list: Sequence[np.ndarray], band: int, cpu: bool = False, device: int = 0,
             path_memory: int = DEFAULT_PATH_MEMORY):
    """dtw_banded with the warping path: -> (cost int64 [P], [ops uint8 array per pair]); ops[k] = 0 (M: both signals step), 1 (A:
    a steps) or 2 (B: b steps), forward from (0, 0); empty for a pair without path (an empty member, or n = m = 1).  The pairs
    run in batches whose decision scratch stays within path_memory bytes; a single pair beyond it is a ValueError."""
    if len(a_list) != len(b_list):
        raise ValueError("a_list and b_list must pair up")
    band = check_band(band)
    path_memory = _check_path_memory(path_memory)
    if not cpu:
        import torch  # noqa: F401
    need = [path_scratch_bytes(np.size(a), np.size(b), band) for a, b in zip(a_list, b_list)]
    for p, nb in enumerate(need):
        if nb > path_memory:
            raise ValueError(f"pair {p}: the path needs {nb} bytes of decision scratch, more than path_memory = {path_memory}")
    cost, ops = [np.zeros(0, np.int64)], []
    for run in batches(range(len(need)), lambda p: (need[p],), (path_memory,)):
        c, _, _, o = _run_batch(a_list[run[0]:run[-1] + 1], b_list[run[0]:run[-1] + 1], band, False, cpu, device, path=True)
        cost.append(c)
        ops += o
    return np.concatenate(cost), ops


def path_cells(ops):
    """-> (i, j), int64 arrays of length len(ops) + 1: the cells a path visits, from (0, 0)."""
    ops = np.asarray(ops, np.uint8).reshape(-1)
    if ops.size and int(ops.max()) > 2:
        raise ValueError("ops must be 0 (M), 1 (A) or 2 (B)")
    i = np.concatenate([[0], np.cumsum(ops != 2)]).astype(np.int64)
    j = np.concatenate([[0], np.cumsum(ops != 1)]).astype(np.int64)
    return i, j


def boundary_map(ops, n: int, m: int) -> np.ndarray:
    """-> g, int64 [n + 1]: g[0] = 0, g[n] = m, else the smallest j with (i, j) on the path; the samples [s, e) of a map to
    [g[s], g[e]) of b."""
    i, j = path_cells(ops)
    n, m = int(n), int(m)
    if n < 1 or m < 1 or int(i[-1]) != n - 1 or int(j[-1]) != m - 1:
        raise ValueError("ops is not a path from (0, 0) to (n - 1, m - 1)")
    g = np.empty(n + 1, np.int64)
    g[0], g[n] = 0, m
    g[1:n] = j[1:][np.asarray(ops).reshape(-1) != 2]           # the cell a step of i arrives at is the first of its row
    return g


def path_string(ops) -> str:
    """Run-length encoded ops, e.g. 12M3A1M2B; * for no ops."""
    ops = np.asarray(ops, np.uint8).reshape(-1)
    if not ops.size:
        return "*"
    cut = np.concatenate([[0], np.flatnonzero(np.diff(ops)) + 1, [ops.size]])
    return "".join(f"{int(e - s)}{OPS[int(ops[s])]}" for s, e in zip(cut[:-1], cut[1:]))


def read_events(path: str) -> dict:
    """An event table of `predict --events` -> {read_name: [(position, model_kmer, start_idx, end_idx)]} in the table's order; a
    `samples` column is ignored."""
    table = {}
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        if head[:len(EVENT_COLUMNS)] != list(EVENT_COLUMNS):
            raise click.ClickException(f"{path}: not an event table of predict --events (header {head[:len(EVENT_COLUMNS)]})")
        for no, line in enumerate(f, 2):
            v = line.rstrip("\n").split("\t")
            try:
                row = (v[1], v[2], int(v[3]), int(v[4]))
            except (IndexError, ValueError):
                raise click.ClickException(f"{path}: line {no} is not a row of an event table")
            table.setdefault(v[0], []).append(row)
    return table


def transfer_events(rid: str, rows, g: np.ndarray, b: np.ndarray, digitisation: float, offset: float, signal_range: float):
    """The rows of read `rid` (read_events) with [start_idx, end_idx) mapped through g onto b's stored int16 samples and the level
    and deviation of the event table (include/s2s_hip.h, s2s_events_format) formed from them with b's record calibration ->
    (text, dropped): rows that come out empty are dropped."""
    x = np.asarray(b, np.int64)
    cs = np.concatenate([[0], np.cumsum(x)])
    cq = np.concatenate([[0], np.cumsum(x * x)])
    n_a = len(g) - 1
    out, dropped = [], 0
    for pos, kmer, s, e in rows:
        if not 0 <= s <= e <= n_a:
            raise click.ClickException(f"read {rid}: event [{s}, {e}) lies outside its {n_a} samples")
        s2, e2 = int(g[s]), int(g[e])
        n = e2 - s2
        if n <= 0:
            dropped += 1
            continue
        S, Q = int(cs[e2] - cs[s2]), int(cq[e2] - cq[s2])
        mean, stdv = event_level(S, Q, n, (digitisation, offset, signal_range))
        out.append(f"{rid}\t{pos}\t{kmer}\t{s2}\t{e2}\t{'%.4f' % mean}\t{'%.4f' % stdv}\n")
    return "".join(out), dropped


# ------------------------------------------------------------------ files
def _pairs(a_path: str, b_path: str, by_order: bool):
    """-> generator of (read_id, signal a, signal b, (digitisation, offset, range) of b's record), counters {"unpaired_a",
    "unpaired_b", "records_a", "records_b"} (filled while the generator runs).  By id: B is held in memory by read id, A streams;
    A's order."""
    counts = dict(records_a=0, records_b=0, unpaired_a=0, unpaired_b=0)
    ia, ib = open_records(a_path), open_records(b_path)

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
                yield ra["read_id"], np.asarray(ra["signal"], np.int16), np.asarray(rb["signal"], np.int16), calibration(rb)
        else:
            b = {}
            for r in ib:
                counts["records_b"] += 1
                b.setdefault(r["read_id"], (np.array(r["signal"], np.int16), calibration(r)))
            used = set()
            for r in ia:
                counts["records_a"] += 1
                rid = r["read_id"]
                if rid not in b or rid in used:
                    counts["unpaired_a"] += 1
                    continue
                used.add(rid)
                yield rid, np.asarray(r["signal"], np.int16), *b[rid]
            counts["unpaired_b"] = counts["records_b"] - len(used)
    return gen(), counts


def _row(rid, n_a, n_b, med_a, mad_a, med_b, mad_b, band, cost, tail: str = "", m: int = None) -> str:
    """One row of OUT; `tail`: further columns (with their tabs), m: the samples of B the distance spans (default: all n_b)."""
    per = "nan" if cost < 0 else "%.6f" % (float(cost) / float(n_a + (n_b if m is None else m)) / float(SCALE))
    return f"{rid}\t{n_a}\t{n_b}\t{med_a}\t{mad_a}\t{med_b}\t{mad_b}\t{band}\t{cost if cost >= 0 else 'nan'}\t{per}{tail}\n"


def compare_files(a_path, b_path, out, band: int = DEFAULT_BAND, normalise: str = "mad", by_order: bool = False,
                  max_samples: int = DEFAULT_MAX_SAMPLES, cpu: bool = False, device: int = 0, path_out=None, events_a=None,
                  events_out=None, path_memory: int = DEFAULT_PATH_MEMORY, open_ends: bool = False, anchor: int = DEFAULT_ANCHOR,
                  anchor_window: int = DEFAULT_ANCHOR_WINDOW) -> dict:
    """Write OUT.tsv (COLUMNS; one row per pair, A's order) and return the summary: pairs, records and unpaired records per file,
    mean and median of dtw_per_sample over the pairs that have one.  `normalise` = "mad" | "none" (`none`: the stored samples as they
    are, in units of 1 / 64 ADC count per sample in the last column).  A batch holds pairs until the samples of both sides pass
    max_samples (at least one pair).
    path_out: also write PATH_COLUMNS, one row per pair: the warping path of the pair, run-length encoded (path_string).  events_a
    with events_out: carry the rows of A's event table (read_events) through the path onto B (transfer_events) and write
    EVENT_COLUMNS; the summary then counts events_written, events_dropped (mapped to no sample of B) and events_unpaired (rows of
    reads without a pair).  With either, a batch also ends before its decision scratch would pass path_memory bytes, and a pair
    that needs more on its own is refused by its read id in a first pass over the lengths, before anything is computed.
    open_ends: B may carry samples in front of and behind what A holds (adapter, stall, open pore, trailing samples).  Per batch,
    stage 1 (_anchors) locates the first and the last min(anchor, n_a) samples of A inside the first and the last
    min(anchor_window, n_b) of B by subsequence DTW on the records normalised as a whole: b_start = the head anchor's start, b_end
    = the tail anchor's end; anchors that cross (b_end - b_start < 1) fall back to all of B and are counted in anchors_crossed, a
    pair with an empty record gets no anchors.  Stage 2 is the batch path above on A against B[b_start:b_end) (median / MAD of that
    interval).  OUT gains OPEN_COLUMNS (n_b stays the stored length, dtw_per_sample = dtw / (n_a + b_end - b_start) / 64), the path
    rows gain b_start and b_end, and the carried events come out in B's own coordinates.  The trimmed lengths are known only after
    stage 1, so no first pass runs: a pair whose path needs more than path_memory is refused by its read id in front of its
    batch's stage 2, when earlier batches' rows are already written."""
    if (events_a is None) != (events_out is None):
        raise ValueError("events_a and events_out go together")
    want_path = path_out is not None or events_out is not None
    path_memory = _check_path_memory(path_memory)
    if normalise not in ("mad", "none"):
        raise ValueError("normalise must be 'mad' or 'none'")
    if int(max_samples) < 1:
        raise ValueError("max_samples must be >= 1")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    band = check_band(band)
    if open_ends:
        anchor, anchor_window = _check_anchor(anchor, anchor_window)
    events = read_events(str(events_a)) if events_a is not None else None
    if want_path and not open_ends:
        for rid, a, b, _ in _pairs(str(a_path), str(b_path), by_order)[0]:
            if len(a) <= MAX_SAMPLES and len(b) <= MAX_SAMPLES and path_scratch_bytes(len(a), len(b), band) > path_memory:
                raise click.ClickException(f"read {rid}: the path of {len(a)} against {len(b)} samples at band {band} needs "
                                           f"{path_scratch_bytes(len(a), len(b), band)} bytes of decision scratch, more than "
                                           f"--path-memory {path_memory}")
    pairs, counts = _pairs(str(a_path), str(b_path), by_order)
    per_sample = []
    n_pairs = 0
    ev = dict(written=0, dropped=0, paired=0)
    crossed = [0]
    with open(out, "w") as f, open(path_out or os.devnull, "w") as fp, open(events_out or os.devnull, "w") as fe:
        f.write("\t".join(COLUMNS + (OPEN_COLUMNS if open_ends else ())) + "\n")
        fp.write("\t".join(PATH_COLUMNS + (OPEN_COLUMNS[:2] if open_ends else ())) + "\n")
        fe.write("\t".join(EVENT_COLUMNS) + "\n")

        def stage2(al, bl):
            """_run_batch; with open ends and a path, in runs of pairs whose decision scratch stays within path_memory (the batches
            were formed before the trimmed lengths were known)."""
            if not (open_ends and want_path):
                return _run_batch(al, bl, band, normalise == "mad", cpu, device, path=want_path)
            P = len(al)
            need = [path_scratch_bytes(len(x), len(y), band) for x, y in zip(al, bl)]
            cost, med, mad, ops = np.zeros(P, np.int64), np.zeros(2 * P, np.int32), np.zeros(2 * P, np.int32), []
            for run in batches(range(P), lambda p: (need[p],), (path_memory,)):
                s, p = run[0], run[-1] + 1
                c, md, dv, o = _run_batch(al[s:p], bl[s:p], band, normalise == "mad", cpu, device, path=True)
                cost[s:p], ops = c, ops + o
                med[s:p], med[P + s:P + p], mad[s:p], mad[P + s:P + p] = md[:p - s], md[p - s:], dv[:p - s], dv[p - s:]
            return cost, med, mad, ops

        def flush(batch):
            P = len(batch)
            al, bl = [p[1] for p in batch], [p[2] for p in batch]
            iv = None                                   # per pair (b_start, b_end, head_cost, tail_cost)
            if open_ends:
                c1, s1, e1, hb = _anchors(al, bl, normalise == "mad", cpu, device, anchor, anchor_window)
                iv = []
                for i, (a, b) in enumerate(zip(al, bl)):
                    if not len(a) or not len(b):        # an empty record: no anchors
                        iv.append((0, len(b), "nan", "nan"))
                        continue
                    bs, be = int(s1[i]), len(b) - int(hb[i]) + int(e1[P + i])
                    if be - bs < 1:                     # the anchors crossed: all of B
                        bs, be = 0, len(b)
                        crossed[0] += 1
                    iv.append((bs, be, int(c1[i]), int(c1[P + i])))
                bl = [b[v[0]:v[1]] for b, v in zip(bl, iv)]
                if want_path:
                    for (rid, a, _, _), b in zip(batch, bl):
                        if path_scratch_bytes(len(a), len(b), band) > path_memory:
                            raise click.ClickException(f"read {rid}: the path of {len(a)} against {len(b)} samples at band {band} needs "
                                                       f"{path_scratch_bytes(len(a), len(b), band)} bytes of decision scratch, more than "
                                                       f"--path-memory {path_memory}")
            cost, med, mad, *ops = stage2(al, bl)
            for i, (rid, a, b, cal) in enumerate(batch):
                c, m = int(cost[i]), len(bl[i])         # m: the samples of B the distance spans (n_b without open ends)
                tail = "" if iv is None else "\t%d\t%d\t%s\t%s" % iv[i]
                f.write(_row(rid, len(a), len(b), int(med[i]), int(mad[i]), int(med[P + i]), int(mad[P + i]), band, c, tail, m))
                if c >= 0:
                    per_sample.append(float(c) / float(len(a) + m) / float(SCALE))
                if not want_path:
                    continue
                o = ops[0][i]
                ptail = "" if iv is None else "\t%d\t%d" % iv[i][:2]
                fp.write(f"{rid}\t{len(a)}\t{len(b)}\t{band}\t{c if c >= 0 else 'nan'}\t{len(o)}\t{path_string(o)}{ptail}\n")
                if events is not None and rid in events:
                    rows = events[rid]
                    ev["paired"] += len(rows)
                    if len(o) == 0 and (len(a) != 1 or m != 1):                      # no path (an empty record): nothing to map through
                        ev["dropped"] += len(rows)
                        continue
                    g = boundary_map(o, len(a), m)
                    if iv is not None:
                        g = g + iv[i][0]                # B's own coordinates
                    text, dropped = transfer_events(rid, rows, g, b, *cal)
                    fe.write(text)
                    ev["dropped"] += dropped
                    ev["written"] += len(rows) - dropped

        def cost(pair):
            rid, a, b, _ = pair
            if len(a) > MAX_SAMPLES or len(b) > MAX_SAMPLES:
                raise click.ClickException(f"read {rid}: more than {MAX_SAMPLES} samples")
            return len(a) + len(b), path_scratch_bytes(len(a), len(b), band) if want_path and not open_ends else 0

        for batch in batches(pairs, cost, (max_samples, path_memory)):
            flush(batch)
            n_pairs += len(batch)
    summary = dict(a=str(a_path), b=str(b_path), out=str(out), band=band, normalise=normalise, pairs=n_pairs,
                   records_a=counts["records_a"], records_b=counts["records_b"], unpaired_a=counts["unpaired_a"],
                   unpaired_b=counts["unpaired_b"],
                   mean_dtw_per_sample=float(np.mean(per_sample)) if per_sample else None,
                   median_dtw_per_sample=float(np.median(per_sample)) if per_sample else None)
    if open_ends:
        summary.update(open_ends=True, anchor=anchor, anchor_window=anchor_window, anchors_crossed=crossed[0])
    if path_out is not None:
        summary["path_out"] = str(path_out)
    if events is not None:
        unpaired = sum(len(r) for r in events.values()) - ev["paired"]
        summary.update(events_out=str(events_out), events_written=ev["written"], events_dropped=ev["dropped"], events_unpaired=unpaired)
        logger.info("compare: %d event(s) carried onto %s, %d dropped (no sample of B), %d of reads without a pair", ev["written"],
                    b_path, ev["dropped"], unpaired)
    if counts["unpaired_a"] or counts["unpaired_b"]:
        logger.warning("compare: %d record(s) of %s and %d of %s have no partner", counts["unpaired_a"], a_path, counts["unpaired_b"], b_path)
    return summary
