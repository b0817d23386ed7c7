"""The predict kernel's dynamic schedule (claims from the handle's counter, include/s2s_hip.h: s2s_set_schedule) against its static
split on the same handle: a chunk's output depends on its global index and the seed alone, so the two must give the same bytes --
at every launch size that takes another way through the claim list, in every mode, on both attention paths, through both input
forms, on the production and on the test instance; the counter must be back at zero behind every launch; the workgroup-span
counters must be consistent with the launch's event time."""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import _lib, chunker
from conftest import load_ckpt, load_npz
from test_gpu_parity import MAE_TOL, MAX_TOL, P

pytestmark = pytest.mark.gpu

N_MAX = 5003                 # the ragged size of test_production_instance_equals_test_instance
# fewer chunks than workgroups (1, 7, 16, 17, 255), one more than workgroups (257), the taper zone plus one chunk (4,097: one
# ragged single behind the full zone of 256 x 16), whole groups in front of the zone and a ragged remainder (5,003)
SIZES = [1, 7, 16, 17, 255, 257, 4097, 5003]
FIRST = 123456789012


@pytest.fixture(scope="module", autouse=True)
def _no_schedule_override():
    import os
    saved = os.environ.pop("S2S_SCHEDULE", None)
    yield
    if saved is not None:
        os.environ["S2S_SCHEDULE"] = saved


@pytest.fixture(scope="module")
def batch():
    """5,003 chunks of ragged reads with N bases (k = 9), as windows and packed; shared, never written."""
    sd, cfg = load_ckpt("k9")
    k = cfg["seq_kmer"]
    rng = np.random.default_rng(20263)
    lens = list(rng.integers(k, 900, size=170)) + [k, k + 15, k + 16, 5000]
    reads = ["".join(rng.choice(list("ACGTN"), int(n), p=[.2475, .2475, .2475, .2475, .01])) for n in lens]
    while sum(chunker.n_chunks(len(r), k) for r in reads) < N_MAX:
        reads.append("".join(rng.choice(list("ACGT"), int(rng.integers(k, 900)))))
    bases, nv, _ = S.encode_reads(reads, k)
    flat, cs, nv2, _ = chunker.pack_reads(reads, k)
    assert np.array_equal(nv, nv2) and int(nv[:N_MAX].min()) < 16
    return dict(sd=sd, cfg=cfg, bases=torch.from_numpy(bases[:N_MAX]).cuda(), nv=torch.from_numpy(nv[:N_MAX]).cuda(),
                flat=torch.from_numpy(flat).cuda(), cs=torch.from_numpy(cs[:N_MAX]).cuda())


@pytest.fixture(scope="module", params=["f32", "f16x3", "f16x3-exact", "f16", "f16-exact"])
def eng(request, batch):
    mode = request.param
    e = S.Engine(batch["sd"], batch["cfg"], mode=mode.split("-")[0])
    assert e.schedule == "auto"
    if mode.endswith("-exact"):
        e.attention_path = "exact"
    yield e
    e.close()


def run(e, batch, n, schedule, first=FIRST, **kw):
    """One launch of the first n chunks into buffers filled with a sentinel: a chunk no claim covered would show."""
    e.schedule = schedule
    sig = torch.full((n, 250), float("nan"), dtype=torch.float32, device="cuda")
    dur = torch.full((n, 16), -7, dtype=torch.int32, device="cuda")
    out = e.predict_chunks(batch["bases"][:n].contiguous(), batch["nv"][:n].contiguous(), S.PredictParams(**P(seed=77)),
                           first_global_chunk=first, out_signal=sig, out_dur=dur, **kw)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_dynamic_equals_static(eng, batch, n):
    e = eng
    e.stats()
    ref = run(e, batch, n, "static")
    st = e.stats()
    assert st["chunks"] == n and st["chunks_on_dynamic_schedule"] == 0 and st["workgroups"] == min(256, n)
    got = run(e, batch, n, "dynamic")
    st = e.stats()
    assert st["chunks"] == n and st["chunks_on_dynamic_schedule"] == n and st["workgroups"] == min(256, n)
    assert bool(torch.isfinite(ref["signal"]).all()) and int(ref["dur"].min()) >= 0
    assert torch.equal(got["dur"], ref["dur"]) and torch.equal(got["signal"], ref["signal"])
    assert int((ref["signal"] != 0).sum()) > 50 * n
    # the packed input form (chunk_start), global chunk 0 onward
    pp = S.PredictParams(**P(seed=77))
    cs, nv = batch["cs"][:n].contiguous(), batch["nv"][:n].contiguous()
    e.schedule = "static"
    a = e.predict_packed(batch["flat"], cs, nv, pp)
    e.schedule = "dynamic"
    b = e.predict_packed(batch["flat"], cs, nv, pp)
    assert torch.equal(a["dur"], b["dur"]) and torch.equal(a["signal"], b["signal"])
    again = run(e, batch, n, "dynamic", first=0)
    assert torch.equal(again["dur"], a["dur"]) and torch.equal(again["signal"], a["signal"])


@pytest.mark.parametrize("n", [17, 5003])
def test_test_instance_on_the_dynamic_schedule(eng, batch, n):
    """`s2s_fused_kernel<MODE, true>` (stage outputs asked for) under claims == the production instance under the static split."""
    ref = run(eng, batch, n, "static")
    got = run(eng, batch, n, "dynamic", debug=True)
    assert torch.equal(got["dur"], ref["dur"]) and torch.equal(got["signal"], ref["signal"])


@pytest.mark.parametrize("tag", ["k9", "k6"])
@pytest.mark.parametrize("mode", ["f32", "f16x3", "f16x3-exact"])
def test_dynamic_against_the_reference_goldens(tag, mode):
    """Injected g / z01 (the test instance) on the golden chunks, forced to claims: the bound of test_gpu_parity.py."""
    sd, cfg = load_ckpt(tag)
    e = S.Engine(sd, cfg, mode=mode.split("-")[0])
    if mode.endswith("-exact"):
        e.attention_path = "exact"
    e.schedule = "dynamic"
    for name in (f"stages_{tag}.npz", f"wide_{tag}.npz"):
        g = load_npz(name)
        bases, nv = chunker.codes_to_bases(g["codes"])
        e.stats()
        out = e.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), S.PredictParams(**P()),
                               inject_g=torch.from_numpy(np.ascontiguousarray(g["g"])).cuda(),
                               inject_z01=torch.from_numpy(np.ascontiguousarray(g["z01"]).astype(np.float32)).cuda())
        assert e.stats()["chunks_on_dynamic_schedule"] == bases.shape[0]
        assert np.array_equal(out["dur"].cpu().numpy(), g["dur_gamma"])
        y, ref = out["signal"].cpu().numpy(), g["y_gamma_nsamp"]
        assert np.array_equal(y == 0, ref == 0)
        d = np.abs(y - ref)
        print(f"GOLDEN {name} {mode} dynamic: {y.shape[0]} chunks, MAE {d.mean():.2e} max {d.max():.2e}")
        assert d.mean() < MAE_TOL and d.max() < MAX_TOL, (d.mean(), d.max())
    e.close()


def test_counter_is_back_at_zero_behind_every_launch(eng, batch):
    """Launches of other sizes back to back, nothing waited for in between: each starts from claim 0 (the last workgroup of the one
    before reset the counter) -- a counter left anywhere else would skip chunks (the sentinels stay) or run them twice."""
    sizes = [5003, 17, 4097, 1, 5003]
    want = {n: run(eng, batch, n, "static") for n in set(sizes)}
    torch.cuda.synchronize()
    eng.stats()
    eng.schedule = "dynamic"
    pp = S.PredictParams(**P(seed=77))
    ins = {n: (batch["bases"][:n].contiguous(), batch["nv"][:n].contiguous()) for n in set(sizes)}
    outs = [(torch.full((n, 250), float("nan"), dtype=torch.float32, device="cuda"), torch.full((n, 16), -7, dtype=torch.int32, device="cuda"))
            for n in sizes]
    torch.cuda.synchronize()
    for n, (sig, dur) in zip(sizes, outs):
        eng.predict_chunks(*ins[n], pp, first_global_chunk=FIRST, out_signal=sig, out_dur=dur)
    st = eng.stats()
    for n, (sig, dur) in zip(sizes, outs):
        assert torch.equal(dur, want[n]["dur"]) and torch.equal(sig, want[n]["signal"]), n
    assert st["chunks"] == sum(sizes) == st["chunks_on_dynamic_schedule"]
    assert st["workgroups"] == sum(min(256, n) for n in sizes)


def test_workgroup_spans(eng, batch):
    eng.stats()
    for schedule in ("static", "dynamic"):
        eng.schedule = schedule
        run(eng, batch, 4097, schedule)              # warm
        torch.cuda.synchronize()
        eng.stats()
        eng.kernel_ms()
        eng.set_profiling(True)
        run(eng, batch, 4097, schedule)
        ms, nl, nc = eng.kernel_ms()
        eng.set_profiling(False)
        st = eng.stats()
        assert nl == 1 and nc == 4097 and st["workgroups"] == 256
        print(f"SPANS {eng.mode} {schedule}: kernel {ms:.3f} ms, span mean {st['wg_span_ms_mean']:.3f} max {st['wg_span_ms_max']:.3f} "
              f"min {st['wg_span_ms_min']:.3f}")
        assert 0.0 < st["wg_span_ms_min"] <= st["wg_span_ms_mean"] <= st["wg_span_ms_max"] < ms + 1.0
        again = eng.stats()                            # read-and-reset
        assert again["chunks"] == 0 and again["workgroups"] == 0 and again["chunks_on_dynamic_schedule"] == 0
        assert again["wg_span_ms_mean"] == again["wg_span_ms_max"] == again["wg_span_ms_min"] == 0.0


def test_override_and_auto(monkeypatch, batch):
    sd, cfg = batch["sd"], batch["cfg"]
    for env in ("bogus", "dyn", "1"):
        monkeypatch.setenv("S2S_SCHEDULE", env)
        with pytest.raises(ValueError, match="S2S_SCHEDULE must be auto, static or dynamic"):
            S.Engine(sd, cfg, mode="f16x3")
    for env, want in (("dynamic", "dynamic"), ("Static", "static"), ("AUTO", "auto"), ("", "auto")):
        monkeypatch.setenv("S2S_SCHEDULE", env)
        e = S.Engine(sd, cfg, mode="f16x3")
        assert e.schedule == want
        if want != "auto":
            e.stats()
            run_n = 257
            e.predict_chunks(batch["bases"][:run_n].contiguous(), batch["nv"][:run_n].contiguous(), S.PredictParams(**P(seed=1)))
            assert e.stats()["chunks_on_dynamic_schedule"] == (run_n if want == "dynamic" else 0)
        e.close()
    monkeypatch.delenv("S2S_SCHEDULE")
    e = S.Engine(sd, cfg, mode="f16x3")
    with pytest.raises(ValueError):
        e.schedule = "sideways"
    # auto consults the decision function: every test shape is below its threshold, i.e. on the static split (the function itself,
    # threshold included, is walked in test_schedule_cpu.py)
    assert e.schedule == "auto"
    for n in (257, 5003):
        assert not _lib.lib().s2s_schedule_is_dynamic(n, 256, 16)
        e.stats()
        e.predict_chunks(batch["bases"][:n].contiguous(), batch["nv"][:n].contiguous(), S.PredictParams(**P(seed=1)))
        st = e.stats()
        assert st["chunks"] == n and st["chunks_on_dynamic_schedule"] == 0
    e.close()
