"""`predict --alignment`: the host side without a GPU -- the native PAF formatter (s2s_paf_format) against the plain-Python
formatter of tests/_alignment_ref.py, the exports, the command line, the argument checks and the join of the rank files.
Every comparison is between bytes or integers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd.alignment import format_alignment, join_rank_files
from _alignment_ref import kmer_counts, parse_line, py_format
from conftest import GOLDEN, ROOT


def case(te, reads):
    """reads: [(rows [[te+1 counts] per chunk], K)] -> the formatter's arrays; the export's offsets are the row sums."""
    seg = np.array([row for rows, _ in reads for row in rows], np.uint16).reshape(-1, te + 1)
    first = np.concatenate([[0], np.cumsum([len(rows) for rows, _ in reads])]).astype(np.int32)
    per_chunk = seg.sum(axis=1, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum([per_chunk[first[r]:first[r + 1]].sum() for r in range(len(reads))])]).astype(np.int64)
    kmers = np.array([K for _, K in reads], np.int64)
    n_rec = int((np.diff(offs) > 0).sum())
    return seg, first, kmers, offs, n_rec


def both(te, reads, rna, ids=None, threads=3):
    seg, first, kmers, offs, n_rec = case(te, reads)
    ids = ids or [f"read-{i:04d}" for i in range(n_rec)]
    got = bytes(format_alignment(seg, te, first, kmers, offs, ids, rna, threads=threads))
    assert got == py_format(seg, te, first, kmers, offs, ids, rna)
    lines = got.decode().splitlines()
    assert len(lines) == n_rec
    return [parse_line(x) for x in lines]


@pytest.mark.parametrize("rna", [False, True])
@pytest.mark.parametrize("te", [1, 5, 16, 64])
def test_native_formatter_equals_the_python_formatter_on_random_rows(te, rna):
    rng = np.random.default_rng(100 * te + rna)
    reads = []
    for _ in range(40):
        C = int(rng.integers(1, 6))
        rows = rng.integers(0, 40, (C, te + 1))
        rows[rng.random((C, te + 1)) < 0.4] = 0                     # D runs, empty tails
        if rng.random() < 0.15:
            rows[:] = 0                                             # a read without samples: no line
        if rng.random() < 0.2:
            rows[:, :te] = 0                                        # samples in the tails only
        K = te * (C - 1) + int(rng.integers(1, te + 1))
        reads.append((rows.tolist(), K))
    reads.append((rng.integers(1000, 1025, (2, te + 1)).tolist(), 2 * te))     # the widest counts
    for threads in (1, 4):
        lines = both(te, reads, rna, threads=threads)
    for d in lines:
        assert (d["kmer_start"], d["kmer_end"]) == ((d["K"], 0) if rna else (0, d["K"]))


@pytest.mark.parametrize("rna", [False, True])
def test_hand_made_rows(rna):
    te = 4
    # K = 1: one chunk, three pad k-mers with samples and a tail -> trailing insertion, trimmed
    (d,) = both(te, [([[7, 2, 0, 1, 5]], 1)], rna)
    assert d["toks"] == [(7, ",")] and d["K"] == 1 and d["n"] == 15
    assert (d["sig_start"], d["sig_end"]) == ((8, 15) if rna else (0, 7))
    # every k-mer empty, samples in the tail only: D alone, nothing left between sig_start and sig_end
    (d,) = both(te, [([[0, 0, 0, 0, 9]], 4)], rna)
    assert d["toks"] == [(4, "D")] and d["mapped"] == 0 and d["sig_start"] == d["sig_end"] == (9 if rna else 0)
    # an insertion between two chunks is kept, the one behind the last k-mer is trimmed
    (d,) = both(te, [([[3, 3, 3, 3, 6], [2, 2, 2, 2, 5]], 8)], rna)
    fwd = [(3, ","), (3, ","), (3, ","), (3, ","), (6, "I"), (2, ","), (2, ","), (2, ","), (2, ",")]
    assert d["toks"] == (fwd[::-1] if rna else fwd)
    assert (d["sig_start"], d["sig_end"]) == ((5, 31) if rna else (0, 26))
    # a last chunk with n_valid = 1: its pad k-mers hold samples -> I (here at the end: trimmed together with the tail);
    # the first chunk's tail stays
    (d,) = both(te, [([[4, 0, 0, 1, 2], [5, 6, 7, 8, 9]], 5)], rna)
    fwd = [(4, ","), (2, "D"), (1, ","), (2, "I"), (5, ",")]
    assert d["toks"] == (fwd[::-1] if rna else fwd)
    assert (d["sig_start"], d["sig_end"]) == ((30, 42) if rna else (0, 12))
    # runs that must merge: D across a chunk border with an EMPTY tail between, I from a tail
    # ... and an empty k-mer on either side of an insertion stays two D runs
    (d,) = both(te, [([[1, 0, 0, 0, 0], [0, 0, 2, 0, 3], [0, 4, 0, 0, 0]], 12)], rna)
    fwd = [(1, ","), (5, "D"), (2, ","), (1, "D"), (3, "I"), (1, "D"), (4, ","), (2, "D")]
    assert d["toks"] == (fwd[::-1] if rna else fwd)
    assert kmer_counts(d) == ([1, 0, 0, 0, 0, 0, 2, 0, 0, 4, 0, 0][::-1] if rna else [1, 0, 0, 0, 0, 0, 2, 0, 0, 4, 0, 0])
    # a read with no samples between two that have some: two lines, the ids of the two RECORDS
    a, b = both(te, [([[1, 1, 1, 1, 0]], 4), ([[0, 0, 0, 0, 0]], 3), ([[2, 2, 2, 2, 2]], 2)], rna, ids=["first", "third"])
    assert (a["read_id"], b["read_id"]) == ("first", "third") and b["K"] == 2 and b["toks"] == [(2, ","), (2, ",")]


def test_formatter_refuses_what_does_not_fit_together():
    te = 2
    seg, first, kmers, offs, _ = case(te, [([[1, 2, 3]], 2)])
    with pytest.raises(RuntimeError):                               # one id too many
        format_alignment(seg, te, first, kmers, offs, ["a", "b"], False)
    with pytest.raises(RuntimeError):                               # the offsets hold another signal than the counts
        format_alignment(seg, te, first, kmers, offs + np.array([0, 1]), ["a"], False)
    with pytest.raises(RuntimeError):                               # more k-mers than the chunks hold
        format_alignment(seg, te, first, kmers + 5, offs, ["a"], False)
    with pytest.raises(ValueError):
        format_alignment(seg[:, :2], te, first, kmers, offs, ["a"], False)
    assert bytes(format_alignment(np.zeros((0, 3), np.uint16), te, np.zeros(1, np.int32), np.zeros(0), np.zeros(1), [], False)) == b""


def test_exports_load():
    L = _lib.lib()
    for name in ("s2s_align_chunks", "s2s_paf_format", "s2s_paf_format_bound"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.s2s_paf_format_bound(32768, 16, 100, 3600) >= 32768 * 17 * 5
    assert L.s2s_paf_format_bound(-1, 16, 0, 0) < 0


def test_cli_lists_the_option_and_hands_it_to_the_ranks(tmp_path):
    r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "predict", "--show-advanced-options"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--alignment" in r.stdout
    r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "predict", "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert "--alignment" not in r.stdout                            # an advanced option
    env = {k: v for k, v in dict(os.environ, S2S_DRY_LAUNCH="1").items() if k != "WORLD_SIZE"}
    r = subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "predict", "g.fa", "-o", str(tmp_path / "o.blow5"), "--gpus", "2",
                        "--alignment", "a.paf"], cwd=ROOT, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["dry_launch"]
    assert cmd[cmd.index("--alignment") + 1] == "a.paf" and "--gpus" not in cmd
    assert not os.path.exists(os.path.join(ROOT, "a.paf"))          # a dry launch joins nothing


def test_alignment_needs_the_streaming_path(tmp_path):
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    out = tmp_path / "o.blow5"
    with pytest.raises(ValueError, match="streaming"):
        inference_run(config=set_config(None), saved_weights=os.path.join(GOLDEN, "synthetic_k9.ckpt"),
                      fasta=os.path.join(GOLDEN, "example_test.fasta"), read_input=True, n=-1, r=1000, c=-1, out=str(out),
                      profile="dna-r10-prom", dwell_mean=None, dwell_std=0.0, noise_std=0.0, noise_sampling=False,
                      duration_sampling=False, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000,
                      sample_rate=None, bps=None, digitisation=None, range_val=None, offset_mean=None, offset_std=None,
                      median_before_mean=None, median_before_std=None, min_noise=0.0, min_duration=3, min_read_len=30,
                      preserve_read_ids=True, seed=1, streaming=False, alignment=str(tmp_path / "a.paf"))
    assert not out.exists() and not (tmp_path / "a.paf").exists()   # refused before anything is written


def test_rank_files_join_in_rank_order_and_are_removed(tmp_path):
    from seq2squiggle_amd.parallel import rank_output_path
    out = str(tmp_path / "a.paf")
    paths = [rank_output_path(out, r, 3) for r in range(3)]
    assert paths[1].endswith("a.rank1.paf")
    for p, text in zip(paths, (b"r0 line 1\nr0 line 2\n", b"", b"r2 line\n")):      # (a rank without reads leaves an empty file)
        with open(p, "wb") as f:
            f.write(text)
    assert join_rank_files(paths, out) == 28
    assert open(out, "rb").read() == b"r0 line 1\nr0 line 2\nr2 line\n"
    assert not any(os.path.exists(p) for p in paths)
    for p in paths:
        with open(p, "wb") as f:
            f.write(b"x\n")
    join_rank_files(paths, out, keep=True)
    assert open(out, "rb").read() == b"x\nx\nx\n" and all(os.path.exists(p) for p in paths)
