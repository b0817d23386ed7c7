"""The evaluate command without a GPU: preprocess-directory discovery and pairing (batched and single-file layouts), the one-hot ->
k-mer letter conversion, the reference's scaling, the loader's refusals, the finalisation of per-chunk sums into the reference's
four logged losses (tests/golden/eval_<tag>.npz, tools/make_eval_goldens.py), the CLI's argument errors, and the teacher-forced CPU
oracle (oracle.s2s_oracle.evaluate_chunks) against the reference's own tensors and logged losses at every golden -- the anchor that
lets the GPU tests use the oracle for rows no golden holds."""
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd import _lib
from seq2squiggle_amd.checkpoint import load_checkpoint
from seq2squiggle_amd.cli import main
from oracle import s2s_oracle as O
from conftest import GOLDEN
import _eval_data as ED
from _bounds import MAE_TOL, MAX_TOL


@pytest.fixture(scope="module")
def k9():
    sd, cfg = load_checkpoint(os.path.join(GOLDEN, "synthetic_k9.ckpt"))
    return cfg, ED.load("k9")


def test_batched_discovery_orders_and_pairs_by_number(tmp_path, k9):
    cfg, g = k9
    ED.write_dir(g, str(tmp_path), per_file=40, numbers=[9, 10, 2])      # 3 files; name order is not number order
    files = EV.discover(str(tmp_path))
    assert [os.path.basename(f["chunks"]) for f in files] == ["chunks-0002.npy", "chunks-0009.npy", "chunks-0010.npy"]
    for f in files:
        assert {os.path.basename(p).rsplit("-", 1)[1] for p in f.values()} == {os.path.basename(f["chunks"]).rsplit("-", 1)[1]}
        assert os.path.basename(f["chunks_lengths"]).startswith("chunks_lengths-")     # "chunks-" does not swallow "chunks_lengths-"
    data = EV.EvalData(str(tmp_path), cfg)
    assert data.n == g["codes"].shape[0]
    firsts = [b[0] for b in data.batches(1000)]
    assert firsts == [0, 16, 56]                                      # file 0002 holds chunks 80-95 (16), then 0009 (40), 0010 (40)
    lens = np.concatenate([b[2] for b in data.batches(7)])
    want = np.concatenate([g["lengths"][80:], g["lengths"][:80]])
    assert np.array_equal(lens, want)


def test_single_file_layout_and_scaling(tmp_path, k9):
    cfg, g = k9
    ED.write_dir(g, str(tmp_path))
    files = EV.discover(str(tmp_path))
    assert len(files) == 1 and os.path.basename(files[0]["stdevs"]) == "stdevs.npy"
    data = EV.EvalData(str(tmp_path), cfg, max_chunks=50)
    assert data.n == 50
    got = list(data.batches(32))
    assert [b[0] for b in got] == [0, 32] and sum(b[1].shape[0] for b in got) == 50
    scale = float(cfg["scaling_max_value"])
    tg = np.concatenate([b[3] for b in got])
    sd = np.concatenate([b[4] for b in got])
    # ChunkDataSetMemmap.__getitem__: / scaling_max_value, float32
    assert tg.dtype == np.float32 and np.array_equal(tg, (g["targets"][:50].astype(np.float32) / scale).astype(np.float32))
    assert np.array_equal(sd, (g["stdevs"][:50] / scale).astype(np.float32))


@pytest.mark.parametrize("layout", ["k5", "flat"])
def test_onehot_to_kmers(k9, layout):
    cfg, g = k9
    k = int(cfg["seq_kmer"])
    x = torch.from_numpy(ED.onehot(g["codes"]))
    if layout == "k5":
        x = x.reshape(x.shape[0], x.shape[1], k, 5)
    got = EV.onehot_to_kmers(x.float() if layout == "flat" else x, k).numpy()
    want = np.frombuffer(b"_ACGTN", np.uint8)[g["codes"]]
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert (got == ord("_")).all(-1).any() and (got == ord("N")).any()          # pads and the unknown rows are in the golden


def test_onehot_two_hot_row_is_refused(k9):
    cfg, g = k9
    k = int(cfg["seq_kmer"])
    x = torch.from_numpy(ED.onehot(g["codes"][:4])).reshape(4, 16, k, 5).clone()
    x[2, 5, 3, :2] = 1
    with pytest.raises(ValueError, match=r"chunks-0007.npy: chunk 12, k-mer 5, letter 3 has 2 hot entries"):
        EV.onehot_to_kmers(x, k, name="chunks-0007.npy", first_chunk=10)


def test_loader_refusals(tmp_path, k9):
    cfg, g = k9
    d = ED.write_dir(g, str(tmp_path / "ok"), per_file=48)
    EV.EvalData(d, cfg)
    for key, val, pat in (("max_signal_len", 300, r"targets-0000.npy: shape \[48, 250\], expected \[48, 300\].*max_signal_len 300"),
                          ("max_dna_len", 12, r"chunks-0000.npy: shape \[48, 16, 45\].*max_dna_len 12"),
                          ("seq_kmer", 6, r"chunks-0000.npy: shape \[48, 16, 45\], expected \[48, 16, 30\].*seq_kmer 6")):
        with pytest.raises(ValueError, match=pat):
            EV.EvalData(d, dict(cfg, **{key: val}))
    neg = dict(g)
    neg["lengths"] = g["lengths"].copy()
    neg["lengths"][50, 3] = -2
    d2 = ED.write_dir(neg, str(tmp_path / "neg"), per_file=48)
    with pytest.raises(ValueError, match=r"chunks_lengths-0001.npy: negative length -2 at chunk 2, k-mer 3"):
        EV.EvalData(d2, cfg)
    d3 = ED.write_dir(g, str(tmp_path / "missing"), per_file=48)
    os.remove(os.path.join(d3, "stdevs-0001.npy"))
    with pytest.raises(ValueError, match=r"same number of <kind>-NNNN.npy files.*stdevs 1"):
        EV.EvalData(d3, cfg)
    d4 = ED.write_dir(g, str(tmp_path / "single"))
    os.remove(os.path.join(d4, "stdevs.npy"))
    with pytest.raises(ValueError, match=r"missing stdevs.npy"):
        EV.discover(d4)
    d5 = ED.write_dir(g, str(tmp_path / "unpaired"), per_file=48)
    os.rename(os.path.join(d5, "targets-0001.npy"), os.path.join(d5, "targets-0005.npy"))
    with pytest.raises(ValueError, match=r"do not pair up"):
        EV.discover(d5)


@pytest.mark.parametrize("tag", ED.TAGS)
def test_finalize_reproduces_logged_losses(tag):
    """Per-chunk sums (the reference's own, float64) -> the reference's epoch-level logged losses at both batch sizes."""
    g = ED.load(tag)
    N, ts = g["targets"].shape
    te = g["lengths"].shape[1]
    fin = EV.finalize(g["per_chunk"], te, ts)
    for bs in (32, 96):
        ref = g[f"logged_bs{bs}"]
        for i, name in enumerate(ED.LOSSES):
            assert abs(fin[name] - ref[i]) <= 1e-6 * abs(ref[i]), (tag, bs, name, fin[name], ref[i])


@pytest.mark.parametrize("tag", ED.TAGS)
def test_oracle_reproduces_the_reference(tag):
    """oracle.evaluate_chunks against the reference's first-pass tensors and logged losses.  fp64: y within the project's predict
    bounds of prediction_ref (MAE_TOL / MAX_TOL, pA), heads within 1e-5 relative.  fp32 (the reference's own arithmetic, bit-equal
    where the BLAS sums in the same order): no further from prediction_ref than the fp64 oracle, its float64 per-chunk sums within
    1e-4 relative + 1e-7 of the golden's (the bound of the logged losses, chunk by chunk), its finalized losses within 1e-4 relative
    of logged_bs32.  The data hold a dwell of 32767, zero dwell, the crop, pad and unknown-letter rows (tools/make_eval_goldens.py)."""
    torch.set_float32_matmul_precision("highest")
    g = ED.load(tag)
    sd, cfg = load_checkpoint(ED.checkpoint(tag))
    scale = float(cfg["scaling_max_value"])
    te, ts = g["lengths"].shape[1], g["targets"].shape[1]
    assert (te, ts) == (cfg["max_dna_len"], cfg["max_signal_len"])
    tg, sv = ED.scaled(g, scale)
    o32 = O.evaluate_chunks(sd, cfg, g["codes"], g["lengths"], tg, sv)
    o64 = O.evaluate_chunks(sd, cfg, g["codes"], g["lengths"], tg, sv, dtype=torch.float64)
    ref = g["prediction_ref"].astype(np.float64)
    d32 = np.abs(o32["y"].double().numpy() - ref) * scale
    d64 = np.abs(o64["y"].numpy() - ref) * scale
    rel = {n: float((np.abs(o64[n].numpy() - g[n].astype(np.float64)) / np.abs(g[n].astype(np.float64))).max()) for n in ("sigma", "conc", "rate")}
    rel32 = {n: float((np.abs(o32[n].double().numpy() - g[n].astype(np.float64)) / np.abs(g[n].astype(np.float64))).max())
             for n in ("sigma", "conc", "rate")}
    pc = np.abs(o32["per_chunk"] - g["per_chunk"])
    print(f"EVAL oracle {tag}: y to prediction_ref fp64 MAE {d64.mean():.3e} max {d64.max():.3e} pA, fp32 MAE {d32.mean():.3e} max "
          f"{d32.max():.3e} pA | heads rel fp64 {max(rel.values()):.2e} fp32 {max(rel32.values()):.2e} | per-chunk sums rel "
          f"{(pc / (np.abs(g['per_chunk']) + 1e-300)).max():.2e}")
    assert o64["y"].shape == ref.shape and o32["y"].dtype == torch.float32
    assert d64.mean() < MAE_TOL and d64.max() < MAX_TOL, (d64.mean(), d64.max())
    assert max(rel.values()) < 1e-5, rel
    assert d32.mean() <= d64.mean() and d32.max() <= d64.max(), (d32.mean(), d64.mean(), d32.max(), d64.max())
    assert max(rel32.values()) <= max(rel.values()), (rel32, rel)
    assert np.all(pc <= 1e-4 * np.abs(g["per_chunk"]) + 1e-7), pc.max(0)
    fin = EV.finalize(o32["per_chunk"], te, ts)
    for i, name in enumerate(ED.LOSSES):
        r = float(g["logged_bs32"][i])
        assert abs(fin[name] - r) <= 1e-4 * abs(r), (name, fin[name], r)
    if tag not in ("k9", "k6", "d32", "r16x500"):
        assert (g["lengths"] == 32767).sum() == 1                      # the stalled k-mer is in the data


def test_draw_rows_chains_permutations():
    g = ED.load("k9")
    N = g["codes"].shape[0]
    for B in (1, N, 5 * N + 17):
        idx, rows = ED.draw_rows(g, B, seed=3)
        assert idx.shape == (B,) and rows["codes"].shape[0] == B and np.array_equal(rows["lengths"], g["lengths"][idx])
        assert (idx[1:] != idx[:-1]).all()
        for lo in range(0, B - N + 1, N):
            assert np.array_equal(np.sort(idx[lo:lo + N]), np.arange(N))
    assert np.array_equal(ED.draw_rows(g, 300, seed=3)[0], ED.draw_rows(g, 300, seed=3)[0])
    assert not np.array_equal(ED.draw_rows(g, 300, seed=3)[0], ED.draw_rows(g, 300, seed=4)[0])


def test_finalize_refuses_empty():
    with pytest.raises(ValueError):
        EV.finalize(np.zeros((0, 3)), 16, 250)


def test_c_abi_exports_evaluate():
    assert "s2s_evaluate_chunks" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "s2s_evaluate_chunks")


def test_cli_help_and_argument_errors(tmp_path):
    r = CliRunner().invoke(main, ["evaluate", "--help"])
    assert r.exit_code == 0 and "--per-chunk" in r.output and "--max-chunks" in r.output and "generic-geometry-f16" in r.output
    ck = os.path.join(GOLDEN, "synthetic_k9.ckpt")
    cases = [(["evaluate", str(tmp_path)], "Missing option '-m'"),
             (["evaluate", str(tmp_path / "nope"), "-m", ck], "is not a directory"),
             (["evaluate", str(tmp_path), "-m", str(tmp_path / "x.ckpt")], "does not exist"),
             (["evaluate", str(tmp_path), "-m", ck, "--batch-size", "0"], "must be >= 1"),
             (["evaluate", str(tmp_path), "-m", ck, "--max-chunks", "-1"], "must be >= 0"),
             (["evaluate", str(tmp_path), "-m", ck, "--compute-mode", "f64"], "Invalid value for '--compute-mode'")]
    for args, msg in cases:
        r = CliRunner().invoke(main, args)
        assert r.exit_code == 2 and msg in r.output, (args, r.output)
