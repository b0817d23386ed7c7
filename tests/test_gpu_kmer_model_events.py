"""s2s_kmer_model_events on the GPU against its host twin and against the definition in Python integers
(tests/_kmer_model_events_ref.py): all three equal in every field of the table and every `dropped` counter.  The shapes are the
smallest at which the kernel can go wrong -- slot counts around a wave and a workgroup's round with record boundaries inside a wave
and empty records; one workgroup walking past its flush interval, and the same inputs on 0, 1, 2 and 768 workgroups; one code in
every slot (the wave merge and the hot cache slot), equal codes that are not neighbours; on the hashed path codes that share a home
slot beyond the probe limit, also at the cache's last slot where the probe wraps; the direct path at its last k, the first hashed k
and the largest; every drop rule of the CPU list.  Then the table is held to s2s_kmer_model_accumulate's on the same events, the two
commands to the bytes --cpu writes, and one and two rounds of re-estimation are MEASURED AND PRINTED, not asserted: the synthetic
checkpoints are untrained and no nanopolish / f5c / uncalled4 is at hand, so no direction is claimed."""
import json
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import _kmer_model_events_ref as REF
import seq2squiggle_amd as S
from _kmer_model_ref import header_constants
from _kmer_table_ref import kmer_codes as chunk_codes
from conftest import ROOT, load_ckpt
from seq2squiggle_amd import _lib, cli
from seq2squiggle_amd import resquiggle as RSQ
from seq2squiggle_amd import signal_batch as SB
from seq2squiggle_amd import utils as U
from test_compare_cpu import write_file
from test_gpu_events import make_inputs
from test_gpu_kmer_model import CKPT, LAMBDA, PROFILE, SEED
from test_gpu_kmer_table import dev_, make_letters
from test_kmer_model_events_cpu import ONE, edge_records, host, pooled, slot

pytestmark = pytest.mark.gpu

K = header_constants(open(os.path.join(ROOT, "include", "s2s_hip.h")).read())
ROUND = 256                                                     # slots of a workgroup's round: four waves of 64
NAMES = ("codes", "ev_len", "S", "Q", "l_offs", "gain", "shift")


def device(a, k, workgroups=0, table=None, dropped=None):
    """One call of the device entry on the arrays of `pooled` -> (rc, table, dropped) as numpy."""
    dev = torch.device("cuda:0")
    t = torch.zeros((4 ** k + 1, REF.FIELDS), dtype=torch.int64, device=dev) if table is None else torch.from_numpy(table).to(dev)
    d = torch.zeros(4, dtype=torch.int64, device=dev) if dropped is None else torch.from_numpy(dropped).to(dev)
    # (an array without items still gets a pointer: the slot count is on the device, so the entry cannot tell that none is read)
    up = {n: torch.from_numpy(np.ascontiguousarray(a[n] if len(a[n]) else np.zeros(1, a[n].dtype))).to(dev) for n in NAMES}
    ptr = lambda x: x.data_ptr()                                # noqa: E731
    rc = _lib.lib().s2s_kmer_model_events(0, torch.cuda.current_stream(0).cuda_stream, ptr(up["codes"]), ptr(up["ev_len"]), ptr(up["S"]),
                                          ptr(up["Q"]), up["l_offs"].data_ptr(), len(a["l_offs"]) - 1, up["gain"].data_ptr(),
                                          up["shift"].data_ptr(), k, workgroups, t.data_ptr(), d.data_ptr())
    torch.cuda.synchronize()
    return rc, t.cpu().numpy(), d.cpu().numpy()


def reference(a, k):
    """The definition and the host twin, which must agree -> (table, dropped)."""
    want_t, want_d = REF.ref_events(*[a[n] for n in NAMES], k)
    rc, t, d = host(a, k)
    assert rc == 0 and np.array_equal(t, want_t) and d.tolist() == want_d.tolist()
    return want_t, want_d


def same(a, k, want=None, grids=(0,)):
    want_t, want_d = reference(a, k) if want is None else want
    for workgroups in grids:
        rc, t, d = device(a, k, workgroups)
        assert rc == 0
        assert np.array_equal(t, want_t), (workgroups, np.argwhere(t != want_t)[:5])
        assert d.tolist() == want_d.tolist(), (workgroups, d, want_d)
    return want_t, want_d


def random_slots(rng, n, k, codes=None, drops=True):
    """n slots of 1 .. 40 noisy samples; with `drops` a few of every kind that adds nothing."""
    out = []
    for i in range(n):
        c = int(rng.integers(0, 4 ** k + 1)) if codes is None else int(codes[i])
        kind = rng.random() if drops else 1.0
        if kind < 0.03:
            out.append((0, 0, 0, c))
        elif kind < 0.05:
            out.append((1025 + int(rng.integers(0, 50)), 4000, 90000, c))
        elif kind < 0.07:
            out.append(slot(rng.integers(-500, 1500, 4), int(rng.choice([-1, 4 ** k + 1, -7]))))
        elif kind < 0.09:
            out.append(slot([-32768] * 8, c))                   # out of range under the shifts below
        else:
            out.append(slot(rng.integers(-500, 1500, int(rng.integers(1, 41))), c))
    return out


def deal(rng, slots, n_records):
    """The slots cut into n_records records at random places (so a boundary falls inside a wave), some of them empty, each record with
    a calibration of its own; one of seven contributes nothing."""
    cuts = np.sort(rng.integers(0, len(slots) + 1, n_records - 1)) if n_records > 1 else np.zeros(0, np.int64)
    if n_records >= 3:
        cuts[1] = cuts[0]                                       # an empty record between full ones
    edges = [0, *cuts.tolist(), len(slots)]
    cal = lambda p: (0, 0) if n_records == 7 and p == 4 else (int(rng.integers(1 << 20, 1 << 25)), int(rng.integers(-30000, 30000)))  # noqa: E731
    return [(*cal(p), slots[edges[p]:edges[p + 1]]) for p in range(n_records)]


@pytest.mark.parametrize("n_records", [1, 2, 7])
def test_slot_counts_around_a_wave_and_a_round(n_records):
    rng = np.random.default_rng(n_records)
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        a = pooled(deal(rng, random_slots(rng, n, 3), n_records))
        assert a["l_offs"][-1] == n and len(a["gain"]) == n_records
        want_t, want_d = same(a, 3, grids=(0, 1))
        assert n < 63 or want_d[3] > 0


@pytest.mark.parametrize("k", [5, 9])
@pytest.mark.parametrize("n", [8 * ROUND + 1, 3 * 8 * ROUND + 5])
def test_one_workgroup_walks_past_its_flush_and_the_grid_does_not_matter(n, k):
    assert K["FLUSH_ROUNDS"] == 8 and K["MAX_WORKGROUPS"] == 768 and K["SLOTS"] == 1025 and K["PROBES"] == 4
    rng = np.random.default_rng(n + k)
    a = pooled(deal(rng, random_slots(rng, n, k), 5))
    want_t, want_d = same(a, k, grids=(0, 1, 2, 768))
    # (at k = 9 a flush interval of one workgroup holds about 2,000 distinct codes for 1,025 slots: the overflow to the table runs)
    assert want_d[3] > 0.8 * n and (k == 5 or (want_t[:, 0] > 0).sum() > K["SLOTS"])
    # ADDED to: a second call on the same table doubles it
    rc, t, d = device(a, k, 1, want_t.copy(), want_d.copy())
    assert rc == 0 and np.array_equal(t, 2 * want_t) and d.tolist() == (2 * want_d).tolist()


@pytest.mark.parametrize("k", [3, 9])
def test_one_code_in_every_slot(k):
    rng = np.random.default_rng(k)
    n = 8 * ROUND + 70
    a = pooled(deal(rng, random_slots(rng, n, k, codes=[4 ** k - 2] * n, drops=False), 2))
    want_t, want_d = same(a, k, grids=(0, 1, 3))
    assert want_d.tolist() == [0, 0, 0, n] and want_t[4 ** k - 2, 0] == n and (want_t[:, 0] > 0).sum() == 1


@pytest.mark.parametrize("k", [4, 9])
def test_equal_codes_that_are_not_neighbours(k):
    rng = np.random.default_rng(k)
    few = rng.integers(0, 4 ** k, 5)
    n = 5 * 64 + 9
    codes = np.concatenate([np.tile(few[:2], 64)[:64], np.tile(few, 64)[:64 * 3], few[rng.integers(0, 5, n - 256)]])
    a = pooled(deal(rng, random_slots(rng, n, k, codes=codes, drops=False), 2))
    want_t, _ = same(a, k, grids=(0, 1))
    assert (want_t[:, 0] > 0).sum() == len(set(few.tolist()))


@pytest.mark.parametrize("home", [300, 1024])
def test_codes_that_share_a_home_slot_beyond_the_probe_limit(home):
    """Six codes with one home slot inside one flush interval of one workgroup: the probes 1 to 4 are used and two codes go straight to
    the table; at home slot 1,024 the probe wraps to slot 0.  The codes are found by the hash the header states."""
    k = 9
    assert K["DIRECT_MAX_K"] < k and K["SLOTS"] == 1025
    six = REF.codes_with_home(home, K["PROBES"] + 2, k, K)
    assert len(set(six)) == 6 and all(REF.cache_slot(c, K) == home for c in six)
    rng = np.random.default_rng(home)
    n = 2 * ROUND + 40                                          # three rounds of one workgroup: no flush in between
    codes = np.array(six)[rng.integers(0, 6, n)]
    codes[:12] = six + six[::-1]                                # (every one of them in the first wave)
    a = pooled(deal(rng, random_slots(rng, n, k, codes=codes, drops=False), 2))
    want_t, want_d = same(a, k, grids=(1, 0))
    assert (want_t[:, 0] > 0).sum() == 6 and want_d[3] == n


@pytest.mark.parametrize("k", [1, 5, 6, 10])
def test_every_k_with_every_drop_rule(k):
    """k = 5: the last direct k, 1,025 rows = the slot count; k = 6: the first hashed; k = 10: the largest table.  The records are the
    CPU test's: every rule at its edges."""
    rng = np.random.default_rng(k)
    records = edge_records(k, rng) + deal(rng, random_slots(rng, 700, k), 7)
    want_t, want_d = same(pooled(records), k, grids=(0, 1))
    assert all(want_d > 0)


def test_argument_checks():
    a = pooled([(ONE, 0, [slot([5, 6], 1)])])
    assert device(a, 2)[0] == 0
    for k in (0, 11):
        dev = torch.device("cuda:0")
        t = torch.zeros(8, dtype=torch.int64, device=dev)
        assert _lib.lib().s2s_kmer_model_events(0, None, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 1,
                                                t.data_ptr(), t.data_ptr(), k, 0, t.data_ptr(), t.data_ptr()) == -1
    L = _lib.lib()
    t = torch.zeros(4 ** 2 * 5 + 5, dtype=torch.int64, device="cuda:0")
    p = t.data_ptr()
    assert L.s2s_kmer_model_events(0, None, p, p, p, p, p, 1, p, p, 2, -1, p, p) == -1
    assert L.s2s_kmer_model_events(0, None, p, p, p, p, p, 1, p, p, 2, K["MAX_WORKGROUPS"] + 1, p, p) == -1
    assert L.s2s_kmer_model_events(0, None, p, p, p, p, p, -1, p, p, 2, 0, p, p) == -1
    for i in range(9):
        args = [p] * 9
        args[i] = None
        assert L.s2s_kmer_model_events(0, None, *args[:5], 1, *args[5:7], 2, 0, *args[7:]) == -1
    assert L.s2s_kmer_model_events(0, None, None, None, None, None, None, 0, None, None, 2, 0, None, None) == 0       # P = 0: nothing runs
    torch.cuda.synchronize()
    assert not t.any()
    empty = pooled([(ONE, 0, []), (ONE, 0, [])])
    rc, tab, d = device(empty, 2)
    assert rc == 0 and not tab.any() and not d.any()


@pytest.mark.parametrize("tag", ["k9", "k6"])
def test_held_to_the_table_of_kmer_model_accumulate(tag):
    """Sixteen chunks (the first of make_inputs, its crafted dwell rows among them) through Engine: Engine.event_stats gives (n, S, Q) per slot, the codes come from the read letters; with gain = 2^24
    and shift = 0 the table equals Engine.kmer_model_accumulate's on the same chunks, row for row."""
    from test_gpu_events import CAL
    eng = S.Engine(*load_ckpt(tag))
    te, ts, k = eng.t_enc, eng.t_dec, eng.k
    sig, dur = (x[:16] for x in make_inputs(te, ts)[:2])
    flat, start, nv = make_letters(16, te, k, seed=5)
    s_d, d_d, f_d, c_d, n_d = dev_(eng, sig, dur, flat, start, nv)
    st = eng.event_stats(s_d, d_d, *CAL)
    table = eng.kmer_model_accumulate(s_d, d_d, f_d, c_d, n_d, *CAL, eng.kmer_model_new()).cpu().numpy()
    codes = chunk_codes(flat, start, nv, k, te)                 # [16, te]: -1 for a pad slot, 4^k for a k-mer with an N
    n = np.where(codes >= 0, st["seg"].cpu().numpy()[:, :te].astype(np.int64), 0)
    a = dict(codes=np.maximum(codes, 0).astype(np.int32).reshape(-1), ev_len=n.astype(np.int32).reshape(-1),
             S=st["sum"].cpu().numpy()[:, :te].astype(np.int64).reshape(-1), Q=st["sumsq"].cpu().numpy()[:, :te].astype(np.int64).reshape(-1),
             l_offs=np.arange(17, dtype=np.int64) * te, gain=np.full(16, ONE, np.int64), shift=np.zeros(16, np.int64))
    want_t, want_d = same(a, k)
    assert table[:, 0].sum() == want_d[3] > 0 and want_d[:3].tolist() == [0, 0, 0]
    assert np.array_equal(want_t, table)


# ------------------------------------------------------------------ the commands
def run(command, *args):
    r = CliRunner().invoke(cli.main, [command, *[str(a) for a in args], "--json"], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    return json.loads(r.output.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def predicted(tmp_path_factory):
    """The six lambda reads of tests/test_gpu_predict_resquiggle.py, simulated with --kmer-model; j.blow5: the same records untrimmed."""
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    d = tmp_path_factory.mktemp("kmer_model_events")
    genome = next(iter(U.read_fasta(LAMBDA)))[0].upper()
    (d / "reads.fasta").write_text("".join(f">lambda_{i}\n{genome[3000 * i + 100:3000 * i + 320 + 40 * i]}\n" for i in range(6)))
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=str(d / "reads.fasta"), read_input=True, n=-1, r=400, c=-1,
                  out=str(d / "p.blow5"), profile=PROFILE, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True,
                  duration_sampling=True, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None,
                  digitisation=None, range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None,
                  min_noise=0.0, min_duration=3, min_read_len=30, preserve_read_ids=True, seed=SEED, events=None,
                  events_samples=False, kmer_table=None, kmer_model=str(d / "p.model"))
    recs = [(r["read_id"], np.asarray(r["signal"], np.int16)) for r in SB.open_records(str(d / "p.blow5"))]
    write_file(d / "j.blow5", [rid for rid, _ in recs], [np.concatenate([recs[(i + 1) % len(recs)][1][-400:], sig]) for i, (_, sig) in enumerate(recs)])
    return d


@pytest.mark.parametrize("command,signals", [("resquiggle", "p.blow5"), ("eventalign", "j.blow5")])
def test_commands_write_the_bytes_cpu_writes(predicted, command, signals):
    d = predicted
    got = {}
    for side, extra in (("gpu", ()), ("cpu", ("--cpu",))):
        got[side] = run(command, d / "reads.fasta", d / signals, "--kmer-model", d / "p.model", "-o", d / f"{command}.{side}.tsv", "--summary",
                        d / f"{command}.{side}.sum", "--kmer-model-out", d / f"{command}.{side}.model", "--max-samples", 20000, *extra)
    for ext in ("tsv", "sum", "model"):
        assert (d / f"{command}.gpu.{ext}").read_bytes() == (d / f"{command}.cpu.{ext}").read_bytes(), ext
    g, c = got["gpu"]["kmer_model"], got["cpu"]["kmer_model"]
    assert {k: v for k, v in g.items() if k not in ("out", "seconds")} == {k: v for k, v in c.items() if k not in ("out", "seconds")}
    assert g["counted"] > 0 and g["rows"] > 0 and got["gpu"]["solved"] >= 1
    assert RSQ.read_model(str(d / f"{command}.gpu.model"))[0] == 9


def test_measure_one_and_two_rounds_of_re_estimation(predicted):
    """MEASURED AND PRINTED, no bar: from the run's own model with every level shifted by a fixed pattern, the mean |level - truth| over
    the truth's k-mers before and after one and two rounds of `resquiggle --kmer-model-out`."""
    d = predicted
    k, truth = RSQ.read_model(str(d / "p.model"))
    have = np.flatnonzero(np.isfinite(truth))
    shifted = truth.copy()
    shifted[have] += 1.5 * ((have % 5) - 2)                      # -3, -1.5, 0, 1.5, 3 pA by the k-mer's row
    name = lambda c: "".join("ACGT"[(int(c) >> (2 * (k - 1 - t))) & 3] for t in range(k))      # noqa: E731
    (d / "round0.model").write_text("kmer\tlevel_mean\n" + "".join(f"{name(c)}\t{shifted[c]:.4f}\n" for c in have))
    err = lambda lv: (float(np.nanmean(np.abs(lv[have] - truth[have]))), int(np.isfinite(lv[have]).sum()))      # noqa: E731
    line = [f"round 0 (shifted): mean |level - truth| {err(shifted)[0]:.4f} pA over {len(have)} k-mers"]
    for r in (1, 2):
        s = run("resquiggle", d / "reads.fasta", d / "p.blow5", "--kmer-model", d / f"round{r - 1}.model", "-o", d / f"round{r}.tsv",
                "--kmer-model-out", d / f"round{r}.model")
        e, n = err(RSQ.read_model(str(d / f"round{r}.model"))[1])
        cost = s["mean_cost_per_sample"]
        line.append(f"round {r}: {e:.4f} pA over {n} k-mers ({s['kmer_model']['counted']} events, {s['skipped_kmers']} skipped k-mers, mean "
                    f"cost {'nan' if cost is None else '%.4f' % cost} MAD per sample)")
        assert s["kmer_model"]["counted"] > 0
    print("\nre-estimation of the pore model from resquiggle's alignments (6 reads, untrained checkpoint): " + "; ".join(line))
