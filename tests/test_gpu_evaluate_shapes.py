"""s2s_evaluate_chunks past one chunk per workgroup, one slice and the goldens' dwell range (tests/test_gpu_evaluate.py runs every
launch at one chunk per workgroup, inside one slice).

Datasets are built out of golden rows (ED.draw_rows: chained permutations, no two adjacent rows from the same golden chunk), so that
every row of a large batch has the reference's own answer: a row swapped with its neighbour, a stale prefetched slot or a filler chunk
leaking into a live one shows up as a row that disagrees with the reference.

Batch shapes (the tuned instances, s2s_eval_kernel): workgroup i of min(B, CUs) owns chunks [i * B / grid, (i + 1) * B / grid) and
walks them in groups of GROUP (16 for f16x3 / f16, whose frontend takes two chunks per wave once a group holds more than DEC_WAVES,
8 for f32).  `walks` restates that split; the batch sizes are multiples of the CU count torch reports, and the test fails if they
stop reaching one of WALKS.  Bounds per row: tests/test_gpu_evaluate.py's (y MAE < 1e-4 pA for the fp32 class, the reference's own
16-mixed MAE / max for f16; heads 1e-4 relative; loss rows 1e-5 relative + 1e-7 against float64 sums of the GPU's own stage outputs;
finalized losses 1e-4 relative of logged_bs32, or within the 16-mixed run's per-chunk distance), tests/test_gpu_parity.py's rule (no
further from the fp64 oracle than 5 x the fp32 oracle is), and bit-equality of loss / y / sigma / conc / rate with the same chunk's row
of a 96-chunk launch (Engine.evaluate_chunks: "independent of B and of its neighbours").  The exact attention path is held to the
same bounds, and to bit-equality with its own 96-chunk launch.

Slices: S2S_EVAL_SLICE + 300 chunks with and without the optional outputs (scratch or caller's buffers, the two branches of `pick`),
the generic pipeline's inner slice (slice_max + 13), a smaller batch in between (the kept workspace).

Stalled k-mers: rows no golden holds (a dwell of 32767, the top of the preprocess files' int16 range, at k-mer 0, te / 2, te - 1 and
everywhere; all-zero dwell) against the CPU oracle, which tests/test_evaluate_cpu.py anchors to the reference.  fp32 class: the
predict bounds (tests/test_gpu_geometry.py's MAE_TOL / MAX_TOL) and the 5 x rule.  f16 class: a row whose oracle y is bit-equal to a
golden row's (the stall lies behind the crop) takes that golden's 16-mixed bar; the others, which no golden of these weights holds,
take the loosest 16-mixed bar of the goldens that hold a stalled chunk (STALLED_TAGS: 0.0069 - 0.051 pA MAE over seven other weight
sets -- what the reference's own reduced precision does to such chunks).

Every test prints its measured distances (EVAL-SHAPES ...) before it asserts."""
import numpy as np
import pytest
import torch

import seq2squiggle_amd as S
from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd.checkpoint import load_checkpoint
from oracle import s2s_oracle as O
import _eval_data as ED
from test_gpu_evaluate import FP32_CLASS, host_sums
from _bounds import MAE_TOL, MAX_TOL

pytestmark = pytest.mark.gpu

DEC_WAVES = 8                                        # s2s_hip.hip
GROUP = {"f16x3": 2 * DEC_WAVES, "f16": 2 * DEC_WAVES, "f32": DEC_WAVES}     # Fused<MODE>::GROUP = DEC_WAVES * FNQ
EVAL_SLICE = 32768                                   # S2S_EVAL_SLICE
SIZE_FACTORS = (1.5, 3.5, 8.5, 16.5, 37.5)           # chunks per workgroup, on average
WALKS = {"1 and 2", "3 and 4", "DEC_WAVES and DEC_WAVES + 1", "GROUP and GROUP + 1", "> 2 * GROUP with a partial tail"}
TUNED = [("f16x3", "fast"), ("f16x3", "exact"), ("f16", "fast"), ("f16", "exact"), ("f32", None)]
HEADS = ("sigma", "conc", "rate")
STALLED_TAGS = ("hd1", "g5x37", "hd24", "hd64", "hd96s", "g64x1024", "hd208")
STALL = 32767


def cu_count() -> int:
    """What the library sizes its grid by (hipDeviceProp_t::multiProcessorCount)."""
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def per_workgroup(B: int, n_wg: int) -> set:
    """s2s_eval_kernel's split: the chunk counts of the workgroups of a launch of B chunks."""
    grid = min(B, n_wg)
    return {(i + 1) * B // grid - i * B // grid for i in range(grid)}


def walks(B: int, n_wg: int, group: int) -> set:
    """The labels of WALKS a launch of B chunks reaches."""
    c = per_workgroup(B, n_wg)
    out = set()
    for label, pair in (("1 and 2", {1, 2}), ("3 and 4", {3, 4}), ("DEC_WAVES and DEC_WAVES + 1", {DEC_WAVES, DEC_WAVES + 1}),
                        ("GROUP and GROUP + 1", {group, group + 1})):
        if pair <= c:
            out.add(label)
    if any(n > 2 * group and n % group for n in c):
        out.add("> 2 * GROUP with a partial tail")
    return out


def sizes(n_wg: int) -> list:
    return [int(f * n_wg) for f in SIZE_FACTORS]


_REF = {}


def reference(tag):
    """-> dict(g, sd, cfg, scale, o32 / o64: the fp32 / fp64 oracle's y for the golden's rows)."""
    if tag not in _REF:
        torch.set_float32_matmul_precision("highest")
        g = ED.load(tag)
        sd, cfg = load_checkpoint(ED.checkpoint(tag))
        scale = float(cfg["scaling_max_value"])
        tg, sv = ED.scaled(g, scale)
        o32 = O.evaluate_chunks(sd, cfg, g["codes"], g["lengths"], tg, sv)["y"].double().numpy()
        o64 = O.evaluate_chunks(sd, cfg, g["codes"], g["lengths"], tg, sv, dtype=torch.float64)["y"].numpy()
        _REF[tag] = dict(g=g, sd=sd, cfg=cfg, scale=scale, o32=o32, o64=o64)
    return _REF[tag]


def make_engine(tag, mode, path=None):
    r = reference(tag)
    eng = S.Engine(r["sd"], r["cfg"], device=0, mode=mode)
    if path is not None:
        eng.attention_path = path                    # s2s_set_attention_path
        assert eng.attention_path == path
    return eng


def run(eng, rows, **kw):
    a = ED.arrays(rows)
    scale = float(eng.config["scaling_max_value"])
    out = EV.evaluate_batch(eng, a["chunks"], a["chunks_lengths"], (a["targets"] / scale).astype(np.float32),
                            (a["stdevs"] / scale).astype(np.float32), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def five_x(y, o32, o64):
    """tests/test_gpu_parity.py's rule -> (mode's mean distance to the fp64 oracle, the fp32 oracle's), zero-pattern flips aside."""
    agree = (o32 == 0) == (o64 == 0)
    same = (y == 0) == (o32 == 0)
    return float(np.abs(y - o64)[same & agree].mean()), float(np.abs(o32 - o64)[agree].mean())


def check_rows(label, mode, out, rows, idx, r, base=None, fin_rows=None):
    """Every bound of the module docstring on one launch's rows -> the list of failures (empty: all hold)."""
    g, scale = r["g"], r["scale"]
    bad = []
    y = out["y"].astype(np.float64)
    d = np.abs(y - rows["prediction_ref"]) * scale
    e_gpu, e_ref = five_x(y, r["o32"][idx], r["o64"][idx])
    rel = {n: float((np.abs(out[n] - rows[n].astype(np.float64)) / np.abs(rows[n].astype(np.float64))).max()) for n in HEADS}
    mine = host_sums({k: torch.from_numpy(v) for k, v in out.items()}, rows, scale)
    loss = out["loss"].astype(np.float64)
    lerr = np.abs(loss - mine) - (1e-5 * np.abs(mine) + 1e-7)
    print(f"EVAL-SHAPES {label}: y MAE {d.mean():.3e} max {d.max():.3e} pA (worst row MAE {d.mean(1).max():.3e}) | to fp64: mode "
          f"{e_gpu:.3e} fp32 oracle {e_ref:.3e} | heads rel {max(rel.values()):.2e} | loss rows over the bound {int((lerr > 0).sum())}")
    if mode in FP32_CLASS:
        if not d.mean() < 1e-4:
            bad.append(f"{label}: y MAE {d.mean():.3e} pA")
        if not e_gpu <= 5 * e_ref:
            bad.append(f"{label}: to fp64 {e_gpu:.3e} > 5 x {e_ref:.3e}")
    else:
        if not (d.mean() <= float(g["y16_mae_pa"]) and d.max() <= float(g["y16_max_pa"])):
            bad.append(f"{label}: y MAE {d.mean():.3e} max {d.max():.3e} pA over the 16-mixed bar")
    if not max(rel.values()) < 1e-4:
        bad.append(f"{label}: heads {rel}")
    if (lerr > 0).any():
        bad.append(f"{label}: {int((lerr > 0).any(1).sum())} loss rows off their float64 sums, first {int(np.argwhere(lerr > 0)[0][0])}")
    if fin_rows is not None:
        te, ts = g["lengths"].shape[1], g["targets"].shape[1]
        assert np.array_equal(np.sort(idx[fin_rows]), np.arange(g["codes"].shape[0]))        # the golden exactly once
        fin = EV.finalize(loss[fin_rows], te, ts)
        d16 = EV.finalize(np.abs(g["per_chunk16"] - g["per_chunk"]), te, ts)
        for i, name in enumerate(ED.LOSSES):
            ref = float(g["logged_bs32"][i])
            dist = abs(fin[name] - ref)
            print(f"EVAL-SHAPES {label} {name}: rel {dist / abs(ref):.2e}")
            if not (dist <= 1e-4 * abs(ref) if mode in FP32_CLASS else dist <= d16[name]):
                bad.append(f"{label}: {name} {fin[name]:.9g} ref {ref:.9g}")
    if base is not None:
        for n in ("loss", "y") + HEADS:
            if n in out and not np.array_equal(out[n], base[n][idx]):
                rows_off = np.argwhere((out[n] != base[n][idx]).reshape(len(idx), -1).any(1))[:, 0]
                bad.append(f"{label}: {n} differs from the 96-chunk launch in {len(rows_off)} rows, first {rows_off[:8].tolist()}")
    return bad


@pytest.mark.parametrize("mode", sorted(GROUP))
def test_sizes_reach_every_walk(mode):
    n_wg = cu_count()
    reached = {B: walks(B, n_wg, GROUP[mode]) for B in sizes(n_wg)}
    for B, w in reached.items():
        print(f"EVAL-SHAPES walks {mode} CUs {n_wg} B {B}: chunks per workgroup {sorted(per_workgroup(B, n_wg))} -> {sorted(w)}")
    assert set().union(*reached.values()) == WALKS, WALKS - set().union(*reached.values())
    # the restatement itself, at a size every existing test uses: one chunk per workgroup
    assert per_workgroup(96, n_wg) == {1} or n_wg < 96


@pytest.mark.parametrize("mode,path", TUNED)
@pytest.mark.parametrize("tag", ["k9", "k6"])
def test_batch_shapes(tag, mode, path):
    r = reference(tag)
    g, N = r["g"], r["g"]["codes"].shape[0]
    n_wg = cu_count()
    eng = make_engine(tag, mode, path)
    base = run(eng, g, want_y=True, debug=True)
    name = f"{tag} {mode}" + (f" {path}" if path else "")
    bad = check_rows(f"{name} B {N}", mode, base, g, np.arange(N), r, fin_rows=slice(0, N))
    reached = set()
    for B in sizes(n_wg):
        reached |= walks(B, n_wg, GROUP[mode])
        idx, rows = ED.draw_rows(g, B, seed=B)
        out = run(eng, rows, want_y=True, debug=True)
        bad += check_rows(f"{name} B {B}", mode, out, rows, idx, r, base=base, fin_rows=slice(0, N))
    eng.close()
    assert reached == WALKS, WALKS - reached
    assert not bad, "\n".join(bad)


def generic_slice_max(cfg) -> int:
    """G.slice_max (pack_generic, s2s_hip.hip), as tests/test_gpu_envelope.py restates it."""
    te, ts, d, f = (cfg[n] for n in ("max_dna_len", "max_signal_len", "dmodel", "dff"))
    n = (512 << 20) // (4 * (te * d + te + ts * d + ts + max(te, ts) * max(3 * d, f)))
    return max(1, min(n, (2 ** 32 - 1) // (max(cfg["encoder_heads"], cfg["decoder_heads"]) * max(1024, 256 * -(-ts // 64)))))


def boundary_check(label, mode, out, rows, idx, r, at):
    """The 64 rows on either side of row `at` against the reference (two equal GPU runs could both be wrong)."""
    sl = slice(at - 64, at + 64)
    return check_rows(label, mode, {k: v[sl] for k, v in out.items()}, {k: v[sl] for k, v in rows.items()}, idx[sl], r)


@pytest.mark.parametrize("tag,mode", [("k9", "f16x3"), ("k9", "f32"), ("k9", "generic"), ("r16x500", "generic-geometry")])
def test_slices(tag, mode):
    r = reference(tag)
    g, N = r["g"], r["g"]["codes"].shape[0]
    eng = make_engine(tag, mode)
    base = run(eng, g, want_y=True, debug=True)
    B = EVAL_SLICE + 300
    idx, rows = ED.draw_rows(g, B, seed=77)
    variants = {"a": dict(), "b": dict(want_y=True), "c": dict(debug=True), "d": dict(want_y=True, debug=True)}
    outs = {v: run(eng, rows, **kw) for v, kw in variants.items()}
    bad = []
    for v, out in outs.items():
        if not np.array_equal(out["loss"], base["loss"][idx]):
            off = np.argwhere((out["loss"] != base["loss"][idx]).any(1))[:, 0]
            bad.append(f"({v}) loss differs from the 96-chunk rows in {len(off)} rows, first {off[:8].tolist()} (slice boundary {EVAL_SLICE})")
        for n in ("y",) + HEADS:
            if n in out and not np.array_equal(out[n], base[n][idx]):
                off = np.argwhere((out[n] != base[n][idx]).any(1))[:, 0]
                bad.append(f"({v}) {n} differs from the 96-chunk rows in {len(off)} rows, first {off[:8].tolist()}")
    bad += boundary_check(f"slice {tag} {mode} rows {EVAL_SLICE - 64}..{EVAL_SLICE + 63}", mode, outs["d"], rows, idx, r, EVAL_SLICE)
    # a smaller batch, then the large one again: the kept workspace
    small_idx, small = ED.draw_rows(g, 1000, seed=78)
    s = run(eng, small)
    if not np.array_equal(s["loss"], base["loss"][small_idx]):
        bad.append("the smaller batch after the large one differs from the 96-chunk rows")
    again = run(eng, rows)
    if not np.array_equal(again["loss"], outs["a"]["loss"]):
        bad.append("the large batch differs on its second run")
    eng.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", ["generic", "generic-f16"])
def test_generic_inner_slice(mode):
    """slice_max + 13 chunks: evaluate_generic's own slice loop (s2s_generic_host.h) entered twice (its offsets into the caller's y /
    sigma / conc / rate)."""
    r = reference("k9")
    g = r["g"]
    eng = make_engine("k9", mode)
    base = run(eng, g, want_y=True, debug=True)
    S_ = generic_slice_max(r["cfg"])
    B = S_ + 13
    assert 64 < S_ < EVAL_SLICE
    idx, rows = ED.draw_rows(g, B, seed=79)
    out = run(eng, rows, want_y=True, debug=True)
    bad = check_rows(f"inner slice k9 {mode} B {B}", mode, out, rows, idx, r, base=base, fin_rows=slice(0, g["codes"].shape[0]))
    sl = slice(S_ - 64, B)
    bad += check_rows(f"inner slice k9 {mode} rows {S_ - 64}..{B - 1}", mode, {k: v[sl] for k, v in out.items()},
                      {k: v[sl] for k, v in rows.items()}, idx[sl], r)
    plain = run(eng, rows)
    if not np.array_equal(plain["loss"], out["loss"]):
        bad.append("loss through the scratch differs from loss through the caller's buffers")
    eng.close()
    assert not bad, "\n".join(bad)


def stalled_rows(g):
    """Rows no golden holds -> (rows, what each is).  From a fit chunk (row 0) and the cropped chunk (every dwell 3 * ts / te): one
    k-mer of dwell 32767 at k-mer 0, te / 2 and te - 1; from row 0 also every k-mer at 32767 and an all-zero dwell."""
    N, te = g["lengths"].shape
    crop = 2 * N // 3 + 2
    assert g["lengths"][crop].min() == g["lengths"][crop].max() and int(g["lengths"][crop].sum()) > g["targets"].shape[1]
    src, what = [], []
    edits = []
    for b in (0, crop):
        for pos in sorted({0, te // 2, te - 1}):
            src.append(b); what.append(f"row {b} stalled at {pos}"); edits.append((pos, STALL))
    src += [0, 0]
    what += ["row 0 stalled everywhere", "row 0 all-zero dwell"]
    edits += [(slice(None), STALL), (slice(None), 0)]
    rows = {k: g[k][np.array(src)].copy() for k in ("codes", "lengths", "targets", "stdevs")}
    for i, (pos, v) in enumerate(edits):
        rows["lengths"][i, pos] = v
    return rows, what


@pytest.mark.parametrize("tag,mode", [("k9", m) for m in ("f16x3", "f32", "f16", "generic", "generic-f16", "generic-geometry",
                                                          "generic-geometry-f16")]
                         + [("r16x500", "generic-geometry"), ("hd96s", "generic-geometry")])
def test_stalled_kmers(tag, mode):
    r = reference(tag)
    g, sd, cfg, scale = r["g"], r["sd"], r["cfg"], r["scale"]
    rows, what = stalled_rows(g)
    tg, sv = ED.scaled(rows, scale)
    torch.set_float32_matmul_precision("highest")
    o32 = O.evaluate_chunks(sd, cfg, rows["codes"], rows["lengths"], tg, sv)
    o64 = O.evaluate_chunks(sd, cfg, rows["codes"], rows["lengths"], tg, sv, dtype=torch.float64)
    y32, y64 = o32["y"].double().numpy(), o64["y"].numpy()
    eng = make_engine(tag, mode)
    out = run(eng, rows, want_y=True, debug=True)
    eng.close()
    y = out["y"].astype(np.float64)
    d = np.abs(y - y32) * scale
    bad = []
    rel = {n: float((np.abs(out[n] - o32[n].double().numpy()) / np.abs(o32[n].double().numpy())).max()) for n in HEADS}
    mine = host_sums({k: torch.from_numpy(v) for k, v in out.items()}, rows, scale)
    lerr = np.abs(out["loss"].astype(np.float64) - mine) - (1e-5 * np.abs(mine) + 1e-7)
    # the sums themselves against the fp32 oracle's float64 sums, at the bound of the logged losses
    osum = np.abs(out["loss"].astype(np.float64) - o32["per_chunk"]) / np.abs(o32["per_chunk"])
    print(f"EVAL-SHAPES stalled {tag} {mode}: heads rel {max(rel.values()):.2e} | loss rows over the bound {int((lerr > 0).sum())} | "
          f"sums to the oracle's rel {osum.max(0)}")
    if not max(rel.values()) < 1e-4:
        bad.append(f"heads {rel}")
    if (lerr > 0).any():
        bad.append(f"loss rows off their float64 sums: {np.argwhere(lerr > 0).tolist()}")
    if not (osum[:, 1:] <= 1e-4).all():
        bad.append(f"duration / noise sums off the oracle's: {osum[:, 1:].max(0)}")
    if mode in FP32_CLASS and not (osum[:, 0] <= 1e-4).all():           # (the f16 class's y is not the oracle's)
        bad.append(f"signal sums off the oracle's: {osum[:, 0].max()}")
    loose = (max(float(ED.load(t)["y16_mae_pa"]) for t in STALLED_TAGS), max(float(ED.load(t)["y16_max_pa"]) for t in STALLED_TAGS))
    for i, w in enumerate(what):
        twin = [j for j in range(g["codes"].shape[0]) if np.array_equal(r["o32"][j], y32[i])]
        if mode in FP32_CLASS:
            e_gpu, e_ref = five_x(y[i], y32[i], y64[i])
            print(f"EVAL-SHAPES stalled {tag} {mode} {w}: MAE {d[i].mean():.3e} max {d[i].max():.3e} pA | to fp64: mode {e_gpu:.3e} fp32 "
                  f"oracle {e_ref:.3e} | bit-equal golden rows {twin}")
            if not (d[i].mean() < MAE_TOL and d[i].max() < MAX_TOL):
                bad.append(f"{w}: MAE {d[i].mean():.3e} max {d[i].max():.3e} pA")
            if not e_gpu <= 5 * e_ref:
                bad.append(f"{w}: to fp64 {e_gpu:.3e} > 5 x {e_ref:.3e}")
        else:
            bar = (float(g["y16_mae_pa"]), float(g["y16_max_pa"])) if twin else loose
            print(f"EVAL-SHAPES stalled {tag} {mode} {w}: MAE {d[i].mean():.3e} max {d[i].max():.3e} pA | bar {bar[0]:.3e} / {bar[1]:.3e} "
                  f"({'the golden row ' + str(twin[0]) if twin else 'the goldens with a stalled chunk'})")
            if not (d[i].mean() <= bar[0] and d[i].max() <= bar[1]):
                bad.append(f"{w}: MAE {d[i].mean():.3e} max {d[i].max():.3e} pA over {bar}")
    assert not bad, "\n".join(bad)
