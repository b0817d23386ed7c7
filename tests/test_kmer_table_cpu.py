"""`predict --kmer-table`: the host side without a GPU -- the native table formatter (s2s_kmer_table_format) against the restatement
in Python integers of tests/_kmer_table_ref.py, its bound and error paths, the rank files and their join, the exports, the header
and the command line.  Every comparison is between bytes or integers."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd.kmer_table import format_table, join_rank_files, load_counts, rank_counts_path, save_counts
from _kmer_table_ref import HEADER, parse_table, py_table
from conftest import ROOT

CAL = (8192.0, 1437.976, 10.0)


def consistent_table(k, seed, fill=0.7):
    """Counters as an accumulation would leave them: per row a number of occurrences, some of them events of 1..1024 samples with
    int16 levels; about 1 - fill of the rows never occurred and some occurred without ever getting a sample."""
    rng = np.random.default_rng(seed)
    t = np.zeros((4 ** k + 1, 6), np.int64)
    for r in range(4 ** k + 1):
        if rng.random() > fill:
            continue
        occ = int(rng.integers(1, 40))
        ev = 0 if rng.random() < 0.1 else int(rng.integers(1, occ + 1))
        n = rng.integers(1, 1025, ev).astype(np.int64)
        q = [rng.integers(-32768, 32768, int(x)).astype(np.int64) for x in n]
        t[r] = [occ, ev, n.sum(), (n * n).sum(), sum(int(x.sum()) for x in q), sum(int((x * x).sum()) for x in q)]
    return t


def raw_format(table, k, cal, with_header, capacity, out):
    return _lib.lib().s2s_kmer_table_format(table.ctypes.data, k, *cal, int(with_header), out.ctypes.data, capacity)


@pytest.mark.parametrize("k", [1, 3, 6])
def test_format_equals_the_restatement(k):
    t = consistent_table(k, seed=k)
    t[0] = [5, 0, 0, 0, 0, 0]                                  # occurred, never got a sample: nan
    t[4 ** k] = [7, 3, 30, 302, -12345, 9 ** 8]                # the N..N row: printed last
    t[1] = [0, 0, 0, 0, 0, 0]                                  # never occurred: no row
    for cal in (CAL, (2048.0, 281.345551, -127.5655735), (1.0, -1e6, -3e4)):
        for header in (True, False):
            text = bytes(format_table(t, k, *cal, with_header=header))
            assert text == py_table(t, k, *cal, with_header=header)
        rows = parse_table(bytes(format_table(t, k, *cal)))
        names = list(rows)
        assert names[0] == "A" * k and names[-1] == "N" * k and "A" * (k - 1) + "C" not in rows
        assert names[:-1] == sorted(names[:-1]) and len(names) == int((t[:, 0] >= 1).sum())       # code order = lexicographic in ACGT
        assert [rows["A" * k][c] for c in HEADER[4:]] == ["nan"] * 4 and rows["A" * k]["n_occ"] == 5
    assert bytes(format_table(np.zeros((5, 6), np.int64), 1, *CAL)) == ("\t".join(HEADER) + "\n").encode()   # a run without reads
    assert bytes(format_table(np.zeros((5, 6), np.int64), 1, *CAL, with_header=False)) == b""


def test_products_that_need_128_bits_and_a_zero_variance():
    k = 1
    t = np.zeros((5, 6), np.int64)
    n = 2 ** 33
    # 2^33 samples around -23170: sumsq is near 2^62, n*Q near 2^95 and S*S too; their difference is small beside them
    S = -23170 * n + 12345
    Q = 23170 * 23170 * n - 2 * 23170 * 12345 + 98765432123
    assert 2 ** 61 < Q < 2 ** 63 and n * Q - S * S > 0 and n * Q > 2 ** 94
    t[0] = [n, 2 ** 23, n, 2 ** 43 + 999, S, Q]
    t[1] = [3, 3, 12, 48, 12 * 777, 12 * 777 * 777]            # every sample 777, every dwell 4: both variances exactly 0
    t[2] = [2 ** 22, 2 ** 22, 2 ** 32, 2 ** 42, 2 ** 32 * 32767, 2 ** 32 * 32767 ** 2]   # ... and where both products are 2^94 / 2^64
    t[3] = [1, 1, 2, 4, 3, 4]                                  # n*Q - S*S = -1 (no such samples): clamped to 0
    text = bytes(format_table(t, k, *CAL))
    assert text == py_table(t, k, *CAL)
    rows = parse_table(text)
    assert rows["C"]["level_stdv"] == rows["C"]["dwell_stdv"] == "0.0000" and rows["C"]["dwell_mean"] == "4.0000"
    assert rows["G"]["level_stdv"] == "0.0000" and rows["T"]["level_stdv"] == "0.0000"
    # what a 64-bit product would have printed differs: the case does test the width
    wrapped = ((n * Q - S * S + 2 ** 63) % 2 ** 64) - 2 ** 63
    assert wrapped != n * Q - S * S and float(rows["A"]["level_stdv"]) > 0.0


def test_bound_capacity_and_arguments():
    L = _lib.lib()
    k = 3
    t = consistent_table(k, seed=9)
    for header in (0, 1):
        need = L.s2s_kmer_table_format_bound(t.ctypes.data, k, *CAL, header)
        out = np.full(need + 64, 0xAB, np.uint8)
        got = raw_format(t, k, CAL, header, need, out)
        assert 0 < got <= need and (out[need:] == 0xAB).all() and out[:got].tobytes() == py_table(t, k, *CAL, with_header=bool(header))
        for cap in (0, need - 1):                               # one byte under the bound: an error, the buffer untouched
            out[:] = 0xAB
            assert raw_format(t, k, CAL, header, cap, out) == -1 and (out == 0xAB).all()
    # the widest numbers any int64 counters give fit the bound
    wide = np.zeros((4 ** k + 1, 6), np.int64)
    wide[:] = [2 ** 62, 1, 1, 2 ** 62, -2 ** 63, 2 ** 63 - 1]
    need = L.s2s_kmer_table_format_bound(wide.ctypes.data, k, 1.0, -1e6, -3e4, 1)
    out = np.full(need + 8, 0xAB, np.uint8)
    got = raw_format(wide, k, (1.0, -1e6, -3e4), 1, need, out)
    assert 0 < got <= need and out[:got].tobytes() == py_table(wide, k, 1.0, -1e6, -3e4)
    out = np.full(1 << 16, 0xAB, np.uint8)
    for bad_k in (0, 11, -1):
        assert L.s2s_kmer_table_format_bound(t.ctypes.data, bad_k, *CAL, 1) == -1
        assert raw_format(t, bad_k, CAL, 1, out.size, out) == -1
    for cal in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (float("nan"), 1.0, 0.0)):
        assert L.s2s_kmer_table_format_bound(t.ctypes.data, k, *cal, 1) == -1 and raw_format(t, k, cal, 1, out.size, out) == -1
    neg = t.copy()
    neg[5, 0] = -1
    assert raw_format(neg, k, CAL, 1, out.size, out) == -1
    assert L.s2s_kmer_table_format(None, k, *CAL, 1, out.ctypes.data, out.size) == -1
    assert L.s2s_kmer_table_format(t.ctypes.data, k, *CAL, 1, None, out.size) == -1
    assert (out == 0xAB).all()
    assert [L.s2s_kmer_table_rows(x) for x in (0, 1, 6, 10, 11)] == [-1, 5, 4097, 4 ** 10 + 1, -1]
    for bad in (lambda: format_table(t, 2, *CAL), lambda: format_table(t, 11, *CAL), lambda: format_table(t, k, 0.0, 1.0, 0.0),
                lambda: format_table(neg, k, *CAL)):
        with pytest.raises(ValueError):
            bad()


def test_rank_files_sum_to_the_whole(tmp_path):
    k = 3
    parts = [consistent_table(k, seed=s, fill=0.5) for s in (1, 2, 3)]
    parts[1][:] = 0                                             # (a rank without reads)
    whole = parts[0] + parts[1] + parts[2]
    out = str(tmp_path / "t.tsv")
    paths = [rank_counts_path(out, r) for r in range(3)]
    assert paths[2] == str(tmp_path / "t.rank2.npz")
    for p, t in zip(paths, parts):
        save_counts(p, t, k, *CAL)
    got = load_counts(paths[0])
    assert np.array_equal(got[0], parts[0]) and got[1] == k and got[2] == tuple(float(np.float32(x)) for x in CAL)
    want = bytes(format_table(whole, k, *CAL))
    assert join_rank_files(paths, out, keep=True) == len(want)
    assert open(out, "rb").read() == want and all(os.path.exists(p) for p in paths)
    assert join_rank_files(paths[::-1], out) == len(want)       # integer sums: any order
    assert open(out, "rb").read() == want and not any(os.path.exists(p) for p in paths)
    # differing k or calibration: refused, nothing removed
    save_counts(paths[0], parts[0], k, *CAL)
    save_counts(paths[1], consistent_table(1, seed=1), 1, *CAL)
    save_counts(paths[2], parts[2], k, CAL[0], CAL[1], 11.0)
    for pair in ([paths[0], paths[1]], [paths[0], paths[2]]):
        with pytest.raises(ValueError, match="differ"):
            join_rank_files(pair, out)
    assert all(os.path.exists(p) for p in paths)
    with pytest.raises(ValueError):
        save_counts(paths[0], parts[0][:-1], k, *CAL)


def test_exports_load_and_the_header_declares_them():
    """(fails before this feature: the library has none of the four)"""
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()
    for name in ("s2s_kmer_table_rows", "s2s_kmer_table_accumulate", "s2s_kmer_table_format", "s2s_kmer_table_format_bound"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"^int(64_t)? %s\(" % name, header, re.M), name
    assert re.search(r"#define S2S_KMER_TABLE_MAX_K\s+10\b", header) and re.search(r"#define S2S_KMER_TABLE_FIELDS\s+6\b", header)
    assert "\t".join(HEADER) in open(os.path.join(ROOT, "seq2squiggle_amd", "csrc", "s2s_host.cpp")).read().replace("\\t", "\t")


def test_cli_lists_the_option_and_names_the_rank_files(tmp_path):
    run = lambda *a, **kw: subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "predict", *a], cwd=ROOT, capture_output=True,
                                          text=True, timeout=120, **kw)
    r = run("--show-advanced-options")
    assert r.returncode == 0 and "--kmer-table " in r.stdout
    assert "--kmer-table" not in run("--help").stdout               # an advanced option
    env = {k: v for k, v in dict(os.environ, S2S_DRY_LAUNCH="1").items() if k != "WORLD_SIZE"}
    r = run("g.fa", "-o", str(tmp_path / "o.blow5"), "--gpus", "2", "--kmer-table", "t.tsv", env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.strip().splitlines()]
    assert lines[-2] == {"kmer_table_rank_files": ["t.rank0.npz", "t.rank1.npz"]}
    cmd = lines[-1]["dry_launch"]
    assert cmd[cmd.index("--kmer-table") + 1] == "t.tsv" and "--gpus" not in cmd
    assert not os.path.exists(os.path.join(ROOT, "t.tsv"))          # a dry launch joins nothing


def test_the_table_needs_the_streaming_path(tmp_path):
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    from conftest import GOLDEN
    kw = dict(config=set_config(None), saved_weights=os.path.join(GOLDEN, "synthetic_k9.ckpt"),
              fasta=os.path.join(GOLDEN, "example_test.fasta"), read_input=True, n=-1, r=1000, c=-1, out=str(tmp_path / "o.blow5"),
              profile="dna-r10-prom", dwell_mean=None, dwell_std=0.0, noise_std=0.0, noise_sampling=False, duration_sampling=False,
              distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None, digitisation=None,
              range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None, min_noise=0.0,
              min_duration=3, min_read_len=30, preserve_read_ids=True, seed=1)
    with pytest.raises(ValueError, match="kmer_table needs the streaming path"):
        inference_run(**kw, streaming=False, kmer_table=str(tmp_path / "t.tsv"))
    assert not (tmp_path / "o.blow5").exists() and not (tmp_path / "t.tsv").exists()   # refused before anything is written
