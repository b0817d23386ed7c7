"""Every exported function of include/s2s_hip.h that takes a `void* stream`, held to the header's promise -- all work is ordered on that
stream and the call does not wait for it -- with LATE inputs on a side stream (tests/_stream_order.py: the delay, the decoy, early,
returned_before).  ENTRIES names every such function and the tests that run it; tests/test_stream_order_cpu.py holds that table to
the header, so an entry cannot arrive without a case.  Every side-stream result equals the same call on the default stream with
complete inputs bit for bit, and the host twin's where the existing tests have one (two equal GPU runs could both be wrong).

Shapes are the smallest of the entries' own tests; nothing needs the workload's size.  At most two side streams live beside the default
stream at any time: the suite runs with the runtime's four hardware queues, and every stream is to have one of its own.  No handle ever
runs on two streams at once (the header forbids it), nothing is captured into a graph, and no case asserts a speed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _lib, chunker
from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import eventalign as EA
from seq2squiggle_amd import preprocess as PP
from seq2squiggle_amd import resquiggle as RSQ
from seq2squiggle_amd import segment as SEG
from seq2squiggle_amd import train as T
from seq2squiggle_amd.checkpoint import load_checkpoint
from seq2squiggle_amd.kmer_model import ModelBuilder
import _eval_data as ED
import _eventalign_ref as EREF
import _preprocess_cases as PC
import _resquiggle_ref as RREF
import _stream_order as SO
import _train_ref as R
from conftest import load_ckpt

pytestmark = pytest.mark.gpu

# entry -> the tests below that run it with late inputs
ENTRIES = {
    "s2s_predict_chunks": ["test_tuned_predict", "test_first_launch_of_an_engine_made_on_the_side_stream", "test_back_to_back_dynamic_launches",
                           "test_generic_predict_grows_its_workspace_behind_queued_kernels", "test_two_engines_on_two_streams",
                           "test_an_engine_changes_stream"],
    "s2s_predict_packed": ["test_tuned_predict"],
    "s2s_evaluate_chunks": ["test_evaluate", "test_a_trainer_and_an_engine_on_two_streams"],
    "s2s_export_reads": ["test_per_chunk_entries"],
    "s2s_align_chunks": ["test_per_chunk_entries"],
    "s2s_event_stats": ["test_per_chunk_entries"],
    "s2s_kmer_table_accumulate": ["test_kmer_accumulators"],
    "s2s_kmer_model_accumulate": ["test_kmer_accumulators"],
    "s2s_svb_encode": ["test_svb_encode"],
    "s2s_philox_u32": ["test_philox"],
    "s2s_signal_median_mad": ["test_compare", "test_resquiggle", "test_eventalign_chain_into_the_model_table"],
    "s2s_signal_normalise": ["test_compare", "test_resquiggle", "test_eventalign_chain_into_the_model_table"],
    "s2s_dtw_banded": ["test_compare"],
    "s2s_dtw_path": ["test_compare", "test_two_scratch_taking_calls_on_two_streams"],
    "s2s_sdtw": ["test_sdtw"],
    "s2s_resquiggle": ["test_resquiggle"],
    "s2s_event_sums": ["test_resquiggle", "test_segment", "test_eventalign_chain_into_the_model_table"],
    "s2s_segment": ["test_segment", "test_eventalign_chain_into_the_model_table", "test_two_scratch_taking_calls_on_two_streams"],
    "s2s_event_means": ["test_eventalign_chain_into_the_model_table"],
    "s2s_eventalign": ["test_eventalign_chain_into_the_model_table"],
    "s2s_kmer_model_events": ["test_eventalign_chain_into_the_model_table"],
    "s2s_chunk_pack": ["test_chunk_pack"],
    "s2s_trainer_gradients": ["test_trainer", "test_a_trainer_and_an_engine_on_two_streams", "test_a_trainer_changes_stream"],
    "s2s_trainer_step": ["test_trainer", "test_a_trainer_and_an_engine_on_two_streams", "test_a_trainer_changes_stream"],
    "s2s_trainer_weights": ["test_trainer", "test_a_trainer_changes_stream"],
}
# Where a case does NOT assert returned_before: (entry, test) -> the words of include/s2s_hip.h that say the call waits for the stream.
SYNCHRONISES = {
    ("s2s_predict_chunks", "test_generic_predict_grows_its_workspace_behind_queued_kernels"):
        "the workspace grows on demand (the first launch of a larger batch synchronises the stream) and is reused",
    ("s2s_trainer_weights", "test_trainer"): "a host copy synchronises the stream",
}

FIRST = 123456789012
PARAMS = dict(dwell_mean=12.5, dwell_std=0.0, noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, min_duration=3.0,
              seed=77)
CAL = (8192.0, 1024.0, 10.0)
_KEEP = []                                       # handles of the session (closed with the process)


# ------------------------------------------------------------------ tuned predict
@functools.lru_cache(maxsize=None)
def chunks_of_reads(n, seed):
    """n chunks (k = 9) of ragged reads, as windows and packed.  The reads' lengths do not depend on the seed: another seed is a decoy
    of the same shapes, with the same chunk_start and n_valid."""
    k = 9
    lens_rng, rng = np.random.default_rng(20263), np.random.default_rng(seed)
    lens = [k, k + 15, k + 16, 30]                   # short reads first: ragged n_valid in the smallest launch too
    while sum(chunker.n_chunks(x, k) for x in lens) < n:
        lens.append(int(lens_rng.integers(k, 900)))
    reads = ["".join(rng.choice(list("ACGTN"), x, p=[.2475, .2475, .2475, .2475, .01])) for x in lens]
    bases, nv, _ = S.encode_reads(reads, k)
    flat, cs, nv2, _ = chunker.pack_reads(reads, k)
    assert np.array_equal(nv, nv2) and int(nv[:n].min()) < 16
    return dict(bases=bases[:n].copy(), nv=nv[:n].copy(), flat=flat, cs=cs[:n].copy())


@functools.lru_cache(maxsize=None)
def tuned(mode):
    e = S.Engine(*load_ckpt("k9"), mode=mode.split("-")[0])
    if mode.endswith("-exact"):
        e.attention_path = "exact"
    _KEEP.append(e)
    return e


def predict(e, ins, form, schedule, n=None, first=FIRST):
    e.schedule = schedule
    pp = S.PredictParams(**PARAMS)
    n = ins["nv"].shape[0] if n is None else n
    if form == "chunks":
        return e.predict_chunks(ins["bases"][:n], ins["nv"][:n], pp, first_global_chunk=first)
    return e.predict_packed(ins["flat"], ins["cs"][:n], ins["nv"][:n], pp, first_global_chunk=first)


def predict_inputs(n, form):
    a, b = chunks_of_reads(n, 1), chunks_of_reads(n, 2)
    late = ["bases"] if form == "chunks" else ["flat"]
    fixed = dict(nv=a["nv"]) if form == "chunks" else dict(nv=a["nv"], cs=a["cs"])
    assert np.array_equal(a["nv"], b["nv"]) and np.array_equal(a["cs"], b["cs"]) and a["flat"].shape == b["flat"].shape
    return {k: a[k] for k in late}, {k: b[k] for k in late}, fixed


TUNED = ([(m, "chunks", 17, "static") for m in ("f32", "f16x3", "f16")] + [(m, "packed", 257, "static") for m in ("f32", "f16x3", "f16")]
         + [(m, "chunks", 4097, "dynamic") for m in ("f32", "f16x3", "f16")]
         + [("f16x3-exact", "packed", 17, "static"), ("f16x3-exact", "chunks", 257, "static"), ("f16x3", "packed", 4097, "dynamic")])


@pytest.mark.parametrize("mode,form,n,schedule", TUNED)
def test_tuned_predict(mode, form, n, schedule):
    real, decoy, fixed = predict_inputs(n, form)
    e = tuned(mode)
    e.stats()
    SO.run_case(f"tuned predict {mode} {form} {n} {schedule}", lambda: e, lambda e, ins: predict(e, ins, form, schedule), real, decoy, fixed)
    st = e.stats()                                       # warm, default, decoy, side: four launches of n
    assert st["chunks"] == 4 * n and st["chunks_on_dynamic_schedule"] == (4 * n if schedule == "dynamic" else 0)


def test_first_launch_of_an_engine_made_on_the_side_stream():
    """s2s_create clears the claim counter; the engine's first launch claims from it, on a side stream, with no synchronisation in
    between (the engine is made inside the side stream's context right before the delay is queued)."""
    real, decoy, fixed = predict_inputs(4097, "chunks")

    def fresh():
        e = S.Engine(*load_ckpt("k9"), mode="f16x3")
        _KEEP.append(e)
        return e
    made = len(_KEEP)
    SO.run_case("first launch dynamic, engine made on the side stream", fresh, lambda e, ins: predict(e, ins, "chunks", "dynamic"), real, decoy,
                fixed, warm=False, fresh_on_side=True)
    st = _KEEP[-1].stats()
    assert len(_KEEP) == made + 3 and st["chunks"] == 4097 == st["chunks_on_dynamic_schedule"] and st["workgroups"] == 256


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_back_to_back_dynamic_launches(mode):
    """4,097, 17 and 4,097 chunks behind ONE delay: every launch starts from claim 0 because the last workgroup of the one before put
    the counter back -- in a queue that is really full."""
    real, decoy, fixed = predict_inputs(4097, "chunks")
    e = tuned(mode)

    def call(e, ins):
        return [predict(e, ins, "chunks", "dynamic", n, first) for n, first in ((4097, FIRST), (17, 5), (4097, 0))]
    e.stats()
    got, _ = SO.run_case(f"back to back dynamic {mode}", lambda: e, call, real, decoy, fixed)
    st = e.stats()
    assert st["chunks"] == 4 * (4097 + 17 + 4097) == st["chunks_on_dynamic_schedule"] and st["workgroups"] == 4 * (256 + 17 + 256)
    assert not torch.equal(got[0]["signal"], got[2]["signal"])


# ------------------------------------------------------------------ generic predict, evaluate
@functools.lru_cache(maxsize=None)
def golden_rows(tag, B, seed):
    sd, cfg = load_checkpoint(ED.checkpoint(tag))
    g = ED.load(tag)
    _, rows = ED.draw_rows(g, B, seed)
    target, stdev = ED.scaled(rows, float(cfg["scaling_max_value"]))
    bases, nv = chunker.codes_to_bases(rows["codes"])
    return dict(sd=sd, cfg=cfg, bases=bases, nv=nv, kmers=np.ascontiguousarray(R.kmers_of(rows["codes"])), dwell=rows["lengths"].astype(np.int32),
                target=np.ascontiguousarray(target * np.float32(1.3)), stdev=np.ascontiguousarray(stdev))


@pytest.mark.parametrize("tag,mode", [("d32", "generic"), ("d32", "generic-f16"), ("g5x37", "generic-geometry"), ("g5x37", "generic-geometry-f16")])
def test_generic_predict_grows_its_workspace_behind_queued_kernels(tag, mode):
    """B = 5, then B = 40 behind it with no synchronisation of the caller's: the second call frees and reallocates the slice workspace
    while the first call's kernels still wait behind the delay (grow_device drains the stream it is given first)."""
    a, b = golden_rows(tag, 40, 1), golden_rows(tag, 40, 2)
    warm5 = torch.from_numpy(a["bases"][:5]).cuda(), torch.from_numpy(a["nv"][:5]).cuda()
    queried = []

    def fresh():                                         # a workspace of 5 chunks, grown on the default stream
        e = S.Engine(a["sd"], a["cfg"], mode=mode)
        e.predict_chunks(*warm5, S.PredictParams(**PARAMS))
        torch.cuda.synchronize()
        _KEEP.append(e)
        return e

    def call(e, ins):
        pp = S.PredictParams(**PARAMS)
        small = e.predict_chunks(ins["bases"][:5], ins["nv"][:5], pp, first_global_chunk=FIRST)
        queried.append(torch.cuda.current_stream().query())
        return [small, e.predict_chunks(ins["bases"], ins["nv"], pp, first_global_chunk=FIRST + 5)]
    name = "test_generic_predict_grows_its_workspace_behind_queued_kernels"
    SO.run_case(f"generic predict {tag} {mode} B 5 then 40", fresh, call, dict(bases=a["bases"]), dict(bases=b["bases"]), dict(nv=a["nv"]),
                warm=False, synchronises=SYNCHRONISES["s2s_predict_chunks", name])
    assert queried[-1] is False, "the call of B = 5 (no growth) waited for the stream"


@pytest.mark.parametrize("tag,mode", [("k9", "f16x3"), ("g5x37", "generic-geometry")])
def test_evaluate(tag, mode):
    a, b = golden_rows(tag, 7, 1), golden_rows(tag, 7, 2)
    e = S.Engine(a["sd"], a["cfg"], mode=mode)
    names = ("kmers", "dwell", "target", "stdev")
    SO.run_case(f"evaluate {tag} {mode} B 7", lambda: e, lambda e, ins: e.evaluate_chunks(*(ins[k] for k in names), want_y=True, debug=True),
                {k: a[k] for k in names}, {k: b[k] for k in names})
    e.close()


# ------------------------------------------------------------------ the per-chunk entries of a handle
@pytest.mark.parametrize("tag", ["tuned", "e5x37"])
def test_per_chunk_entries(tag):
    """s2s_export_reads, s2s_align_chunks and s2s_event_stats on the crafted chunks of tests/test_gpu_events.py (another seed is the decoy)."""
    from test_gpu_events import engine, make_inputs
    e = engine(tag)
    B = 257
    (sig, dur, _), (sig2, dur2, _) = make_inputs(e.t_enc, e.t_dec, B), make_inputs(e.t_enc, e.t_dec, B, seed=5)
    read_first = np.unique(np.concatenate([[0, B], np.random.default_rng(3).integers(0, B, 40)])).astype(np.int32)
    cap = B * e.t_dec

    def call(e, ins):
        ex = e.export_reads(ins["signal"], ins["read_first"], *CAL, rna=True, want_pa=True, want_dac=True)
        kept = torch.arange(cap, device=e.device) < ex["offsets"][-1]                 # (what lies behind the samples is not written)
        return dict(offsets=ex["offsets"], pa=torch.where(kept, ex["pa"], 0), dac=torch.where(kept, ex["dac"], 0),
                    seg=e.align_chunks(ins["signal"], ins["dur"]), stats=e.event_stats(ins["signal"], ins["dur"], *CAL))
    got, _ = SO.run_case(f"export_reads, align_chunks, event_stats {tag}", lambda: e, call, dict(signal=sig, dur=dur),
                         dict(signal=sig2, dur=dur2), dict(read_first=read_first))
    from _events_ref import ref_event_stats
    seg, s, ss = ref_event_stats(sig, dur, *CAL)                                         # the numpy restatement of the definition
    assert np.array_equal(got["seg"].cpu().numpy(), seg) and np.array_equal(got["stats"]["sum"].cpu().numpy(), s)
    assert np.array_equal(got["stats"]["sumsq"].cpu().numpy(), ss) and int(got["offsets"][-1]) == int(seg.sum())


@pytest.mark.parametrize("k", [5, 6])
def test_kmer_accumulators(k):
    """k = 5: the table per workgroup in LDS / the direct slots of the model's cache; k = 6: straight to the table / hashed slots."""
    from test_gpu_events import make_inputs
    from test_gpu_kmer_model import expected as model_expected
    from test_gpu_kmer_table import engine, expected, make_letters
    e = engine(16, 250, k)
    B = 257
    (sig, dur, _), (sig2, dur2, _) = make_inputs(16, 250, B), make_inputs(16, 250, B, seed=5)
    (flat, start, nv), (flat2, start2, nv2) = make_letters(B, 16, k, 1), make_letters(B, 16, k, 1)
    flat2 = np.concatenate([np.random.default_rng(9).choice(np.frombuffer(b"ACGT", np.uint8), len(flat) - 1), flat[-1:]])
    assert np.array_equal(start, start2) and np.array_equal(nv, nv2)

    def call(e, ins):
        a = (ins["signal"], ins["dur"], ins["flat"], ins["start"], ins["nv"])
        return dict(table=e.kmer_table_accumulate(*a, *CAL, e.kmer_table_new()), model=e.kmer_model_accumulate(*a, *CAL, e.kmer_model_new()))
    got, _ = SO.run_case(f"kmer_table_accumulate, kmer_model_accumulate k {k}", lambda: e, call, dict(signal=sig, dur=dur, flat=flat),
                         dict(signal=sig2, dur=dur2, flat=flat2), dict(start=start, nv=nv))
    assert np.array_equal(got["table"].cpu().numpy(), expected(sig, dur, flat, start, nv, k, CAL))
    assert np.array_equal(got["model"].cpu().numpy(), model_expected(sig, dur, flat, start, nv, k, CAL))


def test_svb_encode():
    e = tuned("f16x3")
    lens = [1000, 1, 0, 4097, 250, 64]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.default_rng(4)
    dac, dac2 = (np.cumsum(rng.integers(-300, 300, int(offs[-1]))).astype(np.int16) for _ in range(2))
    R_ = len(lens)
    rows = dict(read_offsets=offs, row_read=np.arange(R_, dtype=np.int32), row_index=np.zeros(R_, np.int32))

    def call(e, ins):
        out = []
        for variant in (32, 16):
            buf = torch.zeros(e.svb_capacity(int(offs[-1]), R_, variant), dtype=torch.uint8, device=e.device)
            out.append(e.svb_encode(ins["dac"], ins["read_offsets"], ins["row_read"], ins["row_index"], 1 << 40, variant, int(offs[-1]), out=buf))
        return out
    got, _ = SO.run_case("svb_encode 32 and 16", lambda: e, call, dict(dac=dac), dict(dac=dac2), rows)
    assert int(got[0]["offsets"][-1]) > int(offs[-1]) and int(got[1]["offsets"][-1]) > int(offs[-1])


def test_philox():
    """No input tensor to come late: the output is preset to a sentinel ON the stream right before the call, behind the delay -- words
    written by a launch that escaped the stream are overwritten by the sentinel."""
    from _philox_ref import philox4x32_10
    e = tuned("f16x3")
    n = 4097

    def call(e, ins):
        out = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device=e.device)
        with torch.cuda.device(e.device):
            rc = _lib.lib().s2s_philox_u32(e._h, e._stream(), 77, 5, 6, 7, 8, n, C.c_void_p(out.data_ptr()))
        assert rc == 0
        return out
    got, _ = SO.run_case("philox_u32", lambda: e, call, {}, None)
    words = got.cpu().numpy().view(np.uint32)
    want = np.stack(philox4x32_10(5 + np.arange(n), 6, 7, 8, 77, 0), axis=1)
    assert np.array_equal(words.astype(np.uint64), want)


# ------------------------------------------------------------------ the handle-free entries, through the batch layer
def test_compare():
    """median / MAD, normalise and the banded DTW of 40 mixed pairs, then the same with the warping path."""
    from test_compare_cpu import mixed_pairs
    al, bl = (v[:40] for v in mixed_pairs())
    for path, dtw in ((False, "dtw_banded"), (True, "dtw_path")):
        SO.run_wrapped(f"compare {dtw}", [CMP], lambda cpu: CMP._run_batch(al, bl, 5, True, cpu, path=path),
                       {"signal_median_mad", "signal_normalise", dtw}, twin=lambda: CMP._run_batch(al, bl, 5, True, True, path=path))


def test_sdtw():
    from test_compare_open_ends_cpu import KINDS, SHAPES, make
    probs = [(k, L_, H_, rev) for k in KINDS for L_, H_ in SHAPES for rev in (False, True)]
    qs, ts = [make(k, L_, H_)[0] for k, L_, H_, _ in probs], [make(k, L_, H_)[1] for k, L_, H_, _ in probs]
    rv = [p[3] for p in probs]
    SO.run_wrapped("sdtw", [CMP], lambda cpu: CMP.sdtw(qs, ts, reverse=rv, cpu=cpu), {"sdtw"}, twin=lambda: CMP.sdtw(qs, ts, reverse=rv, cpu=True))


def test_resquiggle():
    """Five reads at band 64 (two chunks of the band a wave), normalised: median / MAD, normalise, the solver, then the k-mer sums."""
    band = 64
    reads = [RREF.case(n, K, band, kind)[:2] for n, K, kind in ((500, 70, "noisy"), (129, 64, "planted"), (1200, 150, "noisy"), (65, 9, "unknown"),
                                                                (2600, 300, "noisy"))]
    sigs, levs = [r[0] for r in reads], [r[1] for r in reads]
    known = [l != RREF.UNKNOWN for l in levs]
    fn = lambda cpu: RSQ._run_batch(sigs, levs, known, band, RREF.SKIP, RREF.UNK, True, cpu)      # noqa: E731
    got = SO.run_wrapped("resquiggle", [RSQ], fn, {"signal_median_mad", "signal_normalise", "resquiggle", "event_sums"}, twin=lambda: fn(True))
    assert min(int(c) for c in got["cost"]) >= 0 and sum(int(x.sum()) for x in got["len"]) > 1000


def test_segment():
    """Three records across seven tiles of 2,048 samples: the events, then their sums."""
    from test_gpu_segment import noisy
    from test_segment_cpu import T_DEFAULT
    recs = [noisy(21, 5000), noisy(22, 100), noisy(23, 9000)]
    fn = lambda cpu: SEG._run_batch(recs, 3, 6, *T_DEFAULT, cpu)                                  # noqa: E731
    got = SO.run_wrapped("segment", [SEG], fn, {"segment", "event_sums"}, twin=lambda: fn(True))
    assert min(got["n_events"]) > 5


def test_eventalign_chain_into_the_model_table():
    """The whole chain of `eventalign --kmer-model-out` on the planted reads: segment, event sums, event means, median / MAD,
    normalise, the aligner, the k-mer sums and s2s_kmer_model_events, which reads the (ev_len, S, Q) slots that s2s_event_sums left on
    the device one call before, on the same stream."""
    k = 3
    rng = np.random.default_rng(8)
    reads = [EREF.planted_read(K, head, tail) for K, head, tail in EREF.PLANTED[:4]]
    sigs = [r[0] for r in reads]
    ints_known = [RSQ.level_ints(r[1]) for r in reads]
    levs, known = [x[0] for x in ints_known], [x[1] for x in ints_known]
    cleans = ["".join(rng.choice(list("ACGT"), len(l) + k - 1)) for l in levs]
    cals = [(8192.0, 200.0, 1400.0)] * len(reads)
    from test_eventalign_cpu import SEG as SEG_DEFAULT

    def fn(cpu):
        mb = ModelBuilder(k)
        r = EA._run_batch(sigs, levs, known, 64, EREF.SKIP_PENALTY, EREF.TRIM_PENALTY, EREF.UNKNOWN_COST, SEG_DEFAULT, cpu,
                          model_out=(mb, cals, cleans))
        table, dropped = mb.counts()
        return dict(r, table=table, dropped=dropped)
    entries = {"segment", "event_sums", "event_means", "signal_median_mad", "signal_normalise", "eventalign", "kmer_model_events"}
    got = SO.run_wrapped("eventalign chain and kmer_model_events", [EA], fn, entries, twin=lambda: fn(True))
    assert int(got["dropped"][3]) > 100 and int(got["table"][:, 0].sum()) == int(got["dropped"][3]) and min(int(c) for c in got["cost"]) >= 0


def test_chunk_pack():
    """The six row counts of tests/_preprocess_cases.py at 5 / 37 / 6, raw source.  Offsets, event starts and lengths are the same in
    the decoy; its samples, their sums and the k-mers' letters are another batch's."""
    import _preprocess_ref as PR
    te, ts, k = 5, 37, 6
    case = PC.standard(te, ts, k)
    decoy = dict(case, records=SO.other_samples(case["records"], 77), kmers=np.roll(case["kmers"], 1, axis=0))
    PC.sums(decoy)

    def decoy_tables(i, tabs):                           # (l_offs, ev_start, ev_len, S, Q, cal, letters) of preprocess.pack
        return tabs[:3] + [decoy["S"], decoy["Q"], tabs[5], decoy["kmers"].reshape(-1)]
    fn = lambda cpu: PC.run(case, PR.RAW, te, ts, cpu=cpu)                                         # noqa: E731
    got = SO.run_wrapped("chunk_pack", [PP], fn, {"chunk_pack"}, twin=lambda: fn(True), decoy_records=lambda i, recs: decoy["records"],
                         decoy_tables=decoy_tables)
    PC.same(got, PC.ref(case, PR.RAW, te, ts))
    assert int(got["counters"][1]) > 5


# ------------------------------------------------------------------ the trainer
LR, CLIP = 5e-4, 1.0
NAMES = ("kmers", "dwell", "target", "stdev")


def train_sequence(tr, ins):
    """gradients, three steps, the weights: everything on the device, nothing waits."""
    a = tuple(ins[k] for k in NAMES)
    g = tr.gradients(*a)
    stats = [tr.step(*a, lr=LR, step=s + 1, optimizer="Adam", weight_decay=0.0, clip=CLIP) for s in range(3)]
    return dict(loss=g["loss"], grad=g["grad"], stats=stats, weights=tr.weights())


def weights_on_the_host(tr):
    """s2s_trainer_weights into (pinned) host memory: the entry waits for the stream, so the values are there when it returns; then
    state_dict().  The buffer lives on in the result."""
    out = torch.full((tr.n_floats,), float("nan"), dtype=torch.float32).pin_memory()
    with torch.cuda.device(tr.device):
        rc = _lib.lib().s2s_trainer_weights(tr._t, tr._stream(), C.c_void_p(out.data_ptr()))
    at_return = out.numpy().copy()
    assert rc == 0
    _KEEP.append(out)                                    # (a copy that was still in flight must find its buffer)
    return dict(blob=at_return, sd={k: v.numpy() for k, v in tr.state_dict().items()})


def new_trainer(a, B):
    """A trainer whose tape holds B chunks already (gradients() changes no weight): the calls under test grow nothing."""
    tr = T.Trainer(a["sd"], a["cfg"], 0)
    tr.gradients(*(torch.from_numpy(a[k][:B]).cuda() for k in NAMES))
    torch.cuda.synchronize()
    _KEEP.append(tr)
    return tr


@pytest.mark.parametrize("tag", ["k6", "g5x37"])
@pytest.mark.parametrize("made_on", ["default", "side"])
def test_trainer(tag, made_on):
    import _train_classes as TC
    B = TC.default_batch(load_checkpoint(ED.checkpoint(tag))[1])
    a, b = golden_rows(tag, B, 1), golden_rows(tag, B, 2)
    got, _ = SO.run_case(f"trainer {tag} B {B}, made on the {made_on} stream", lambda: new_trainer(a, B), train_sequence, {k: a[k] for k in NAMES},
                         {k: b[k] for k in NAMES}, warm=False, fresh_on_side=made_on == "side", host_after=weights_on_the_host)
    assert not np.array_equal(got["weights"].cpu().numpy(), S.checkpoint.state_dict_to_blob(a["sd"], a["cfg"]))     # the steps moved the weights


# ------------------------------------------------------------------ two handles at once, and a handle that changes stream
def interleaved(name, jobs):
    """jobs: [(fresh, call, real, decoy, fixed, rounds)].  Each job alone on the default stream gives what is wanted; then every job
    gets a side stream and a delay of its own, the calls are issued in turn from this one thread, and nothing is waited for until the
    end.  -> [(the objects, the results)] of the interleaved run."""
    assert len(jobs) == 2                                 # two side streams beside the default one: a hardware queue each
    want, t_solo, dev = [], [], []
    for fresh, call, real, decoy, fixed, rounds in jobs:
        real_d, decoy_d, fixed_d = SO.up(real), SO.up(decoy), SO.up(fixed)
        obj = fresh()
        call(obj, {**fixed_d, **{k: v.clone() for k, v in real_d.items()}})               # warm (a job's object keeps what it must)
        obj = fresh()
        ins = {**fixed_d, **{k: v.clone() for k, v in real_d.items()}}
        w, t = SO.timed(lambda: [call(obj, ins) for _ in range(rounds)])
        want.append(SO.flat(w))
        t_solo.append(t)
        dev.append((real_d, decoy_d, fixed_d))
    t_all = sum(t_solo)                                   # a stream's delay covers the other's calls too
    objs = [job[0]() for job in jobs]
    sides = [SO.side_stream(0), SO.side_stream(1)]
    ins = [SO.decoys(d[1]) for d in dev]
    torch.cuda.synchronize()                              # once, before either delay: both streams are held from here on
    held = [(i, SO.hold(side, i, d[0], SO.delay_for(t_all))) for side, i, d in zip(sides, ins, dev)]
    got, before = [[], []], []
    for r in range(max(job[5] for job in jobs)):
        for j, (fresh, call, real, decoy, fixed, rounds) in enumerate(jobs):
            if r < rounds:
                with torch.cuda.stream(sides[j]):
                    got[j].append(call(objs[j], {**dev[j][2], **held[j][0]}))
    before = [SO.returned_before(side) for side in sides]
    snaps = [SO.early(side, h[0], d[1], g) for side, h, d, g in zip(sides, held, dev, got)]
    for j, side in enumerate(sides):
        side.synchronize()
        SO.lasted(f"{name}, stream {j + 1}", held[j][1], t_all, SO.delay_for(t_all))
    assert all(before), f"{name}: a call waited for its stream"
    for j in range(2):
        bad = SO.same(got[j], want[j])
        assert bad is None, f"{name}: job {j + 1}: {bad} differs from its solo run"
        flat_want = dict(want[j])
        for p, v in snaps[j]:
            assert np.array_equal(SO.flat(v)[0][1], flat_want[p]), (name, j, p)
    return objs, got


def test_two_engines_on_two_streams():
    """Engine A (k9, f16x3, dynamic) on stream 1, engine B (k6, f32) on stream 2, three calls each, interleaved: each engine's bytes are
    its solo run's, and A's counters count A's chunks only."""
    real, decoy, fixed = predict_inputs(4097, "chunks")
    b_real, b_decoy = golden_rows("k6", 40, 1), golden_rows("k6", 40, 2)
    eng_b = S.Engine(*load_ckpt("k6"), mode="f32")
    a = tuned("f16x3")
    call_b = lambda e, ins: e.predict_chunks(ins["bases"], ins["nv"], S.PredictParams(**PARAMS), first_global_chunk=FIRST)     # noqa: E731
    a.stats()
    eng_b.stats()
    _, _ = interleaved("two engines", [(lambda: a, lambda e, ins: predict(e, ins, "chunks", "dynamic"), real, decoy, fixed, 3),
                                               (lambda: eng_b, call_b, dict(bases=b_real["bases"]), dict(bases=b_decoy["bases"]),
                                                dict(nv=b_real["nv"]), 3)])
    st = a.stats()                                        # warm + three solo + three interleaved launches of A's 4,097 chunks
    assert st["chunks"] == 7 * 4097 == st["chunks_on_dynamic_schedule"]
    assert eng_b.stats()["chunks"] == 7 * 40
    eng_b.close()


def test_a_trainer_and_an_engine_on_two_streams():
    """The same checkpoint twice: a trainer stepping on stream 1, an engine evaluating on stream 2."""
    tag, B = "g5x37", 7
    a, b = golden_rows(tag, B, 1), golden_rows(tag, B, 2)
    eng = S.Engine(a["sd"], a["cfg"], mode="generic-geometry")
    ev = lambda e, ins: e.evaluate_chunks(*(ins[k] for k in NAMES), want_y=True)                  # noqa: E731
    real, decoy = {k: a[k] for k in NAMES}, {k: b[k] for k in NAMES}
    objs, got = interleaved("a trainer and an engine", [(lambda: new_trainer(a, B), train_sequence, real, decoy, {}, 1),
                                                       (lambda: eng, ev, real, decoy, {}, 3)])
    assert torch.equal(got[1][0]["loss"], got[1][2]["loss"]) and torch.equal(got[0][0]["loss"], got[1][0]["loss"])       # one model
    eng.close()


def test_two_scratch_taking_calls_on_two_streams():
    """s2s_segment and s2s_dtw_path take their scratch from the caller: one raw call each on device pointers, on two streams at the
    same time, each equal to its solo run and to its host twin."""
    from test_compare_cpu import mixed_pairs
    from test_gpu_segment import noisy, pool
    from test_segment_cpu import T_DEFAULT
    L = _lib.lib()
    recs = [noisy(21, 5000), noisy(22, 100), noisy(23, 9000)]
    flat, offs = pool(recs)
    eo = np.concatenate([[0], np.cumsum(SEG.capacity(np.diff(offs), 3))]).astype(np.int64)
    n_rec, total, slots = len(recs), int(offs[-1]), int(eo[-1])
    seg_scratch = int(L.s2s_segment_scratch_bytes(total, n_rec))
    ptr = lambda t: C.c_void_p(t.data_ptr())                                                    # noqa: E731
    now = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                           # noqa: E731

    def seg_call(_, ins):
        st, ln = (torch.zeros(slots, dtype=torch.int32, device="cuda") for _ in range(2))
        ne, scratch = torch.zeros(n_rec, dtype=torch.int32, device="cuda"), torch.empty(max(seg_scratch, 16), dtype=torch.uint8, device="cuda")
        assert L.s2s_segment(0, now(), ptr(ins["x"]), ptr(ins["offs"]), n_rec, total, 3, 6, *T_DEFAULT, ptr(scratch), ptr(ins["eo"]), ptr(st),
                             ptr(ln), ptr(ne)) == 0
        return dict(start=st, len=ln, n_events=ne)
    band = 5
    al, bl = (v[:40] for v in mixed_pairs())
    P = len(al)
    pooled = lambda v: np.concatenate([np.asarray(r, np.int16) for r in v] + [np.zeros(1, np.int16)])      # noqa: E731
    lens = lambda v: np.concatenate([[0], np.cumsum([len(r) for r in v])]).astype(np.int64)              # noqa: E731
    so = lens([np.zeros(CMP.path_scratch_bytes(len(a), len(b), band), np.uint8) for a, b in zip(al, bl)])
    po = lens([np.zeros(len(a) + len(b) - 2 if len(a) and len(b) else 0, np.uint8) for a, b in zip(al, bl)])

    def dtw_call(_, ins):
        out = torch.zeros(2 * P, dtype=torch.int64, device="cuda")
        ops, scratch = torch.zeros(int(po[-1]) + 16, dtype=torch.uint8, device="cuda"), torch.empty(int(so[-1]) + 16, dtype=torch.uint8, device="cuda")
        assert L.s2s_dtw_path(0, now(), ptr(ins["a"]), ptr(ins["ao"]), ptr(ins["b"]), ptr(ins["bo"]), P, band, ptr(out), ptr(scratch), ptr(ins["so"]),
                              ptr(ops), ptr(ins["po"]), C.c_void_p(out.data_ptr() + 8 * P)) == 0
        return dict(out=out, ops=ops)
    decoy_recs = SO.other_samples(recs, 5)
    jobs = [(lambda: None, seg_call, dict(x=flat), dict(x=pool(decoy_recs)[0]), dict(offs=offs, eo=eo), 1),
            (lambda: None, dtw_call, dict(a=pooled(al), b=pooled(bl)), dict(a=pooled(SO.other_samples(al, 6)), b=pooled(SO.other_samples(bl, 7))),
             dict(ao=lens(al), bo=lens(bl), so=so, po=po), 1)]
    _, got = interleaved("two scratch-taking calls", jobs)
    host = SEG._run_batch(recs, 3, 6, *T_DEFAULT, True, sums=False)
    for key in ("start", "len", "n_events"):
        assert np.array_equal(got[0][0][key].cpu().numpy(), host[key]), key
    hcost, hops = CMP.dtw_path(al, bl, band, cpu=True)
    out, ops = got[1][0]["out"].cpu().numpy(), got[1][0]["ops"].cpu().numpy()
    assert out[:P].tolist() == hcost.tolist() and out[P:].tolist() == [len(o) for o in hops]
    for i in range(P):
        assert np.array_equal(ops[po[i + 1] - len(hops[i]):po[i + 1]], hops[i]), i


def changes_stream(name, fresh, call, real, decoy, fixed=None):
    """default stream, synchronize, a side stream with late inputs, synchronize, the default stream again: the third result is the
    first (run_case makes the first two on one object when fresh() returns the same one)."""
    obj = fresh()
    got, want = SO.run_case(name, lambda: obj, call, real, decoy, fixed, warm=False)
    torch.cuda.synchronize()
    d = {**SO.up(fixed or {}), **SO.up(real)}
    torch.cuda.synchronize()
    third = call(obj, d)
    torch.cuda.synchronize()
    return want, got, third


def test_an_engine_changes_stream():
    real, decoy, fixed = predict_inputs(4097, "chunks")
    e = tuned("f16x3")
    want, got, third = changes_stream("an engine changes stream", lambda: e, lambda e, ins: predict(e, ins, "chunks", "dynamic"), real, decoy, fixed)
    assert SO.same(third, want) is None and SO.same(third, got) is None


def test_a_trainer_changes_stream():
    """gradients() changes no weight: the same trainer gives the same loss rows and gradient on the default stream, on a side stream
    with late inputs, and on the default stream again; then the three steps of test_trainer from there."""
    tag, B = "g5x37", 7
    a, b = golden_rows(tag, B, 1), golden_rows(tag, B, 2)
    tr = new_trainer(a, B)
    grads = lambda tr, ins: tr.gradients(*(ins[k] for k in NAMES))                                # noqa: E731
    want, got, third = changes_stream("a trainer changes stream", lambda: tr, grads, {k: a[k] for k in NAMES}, {k: b[k] for k in NAMES})
    assert SO.same(third, want) is None and SO.same(third, got) is None
    after = train_sequence(tr, SO.up({k: a[k] for k in NAMES}))
    alone = train_sequence(new_trainer(a, B), SO.up({k: a[k] for k in NAMES}))
    torch.cuda.synchronize()
    assert SO.same(after, alone) is None
