"""`predict --kmer-model`: the host side without a GPU -- the fixed-point event statistics (s2s_event_fixed) and the native model
formatter (s2s_kmer_model_format) against the restatements in Python integers of tests/_kmer_model_ref.py, the bound and error
paths, the rank files and their join, the exports, the header and the command line.  Every comparison is between bytes or
integers."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from seq2squiggle_amd import _lib
from seq2squiggle_amd.kmer_model import format_model, join_rank_files, load_counts, missing_kmers, rank_counts_path, save_counts
from _kmer_model_ref import COLUMNS, event_fixed, header_constants, parse_model, py_model
from conftest import ROOT

CAL = (8192.0, 1437.976, 10.0)


def lib_fixed(n, S, Q):
    M, D = C.c_int64(-1), C.c_int64(-1)
    assert _lib.lib().s2s_event_fixed(int(n), int(S), int(Q), C.byref(M), C.byref(D)) == 0
    return M.value, D.value


def nsq(q):
    q = np.asarray(q, np.int64)
    return len(q), int(q.sum()), int((q * q).sum())


def test_event_fixed_on_random_sample_vectors():
    rng = np.random.default_rng(0)
    for i in range(3000):
        n = int(rng.integers(1, 1025)) if i % 3 else int(rng.integers(1, 9))
        spread = int(rng.choice([1, 3, 50, 3000, 32768]))
        centre = int(rng.integers(-32768 + spread, 32768 - spread + 1)) if spread < 32768 else 0
        q = rng.integers(max(-32768, centre - spread), min(32767, centre + spread) + 1, n)
        args = nsq(q)
        M, D = lib_fixed(*args)
        assert (M, D) == event_fixed(*args), args
        assert abs(M) <= 2 ** 23 and 0 <= D <= 2 ** 23


def test_event_fixed_ties_bounds_and_squares():
    # exact ties: n even, 2r == n, both parities of q, both signs of S.  256 S / n with n = 512: S odd gives a remainder of n / 2
    for S in (1, 3, 5, 7, -1, -3, -5, -7, 32767 * 512 + 1, -(32767 * 512 + 3)):
        n = 512
        num = 256 * S
        q, r = divmod(num, n)
        assert 2 * r == n
        M, _ = lib_fixed(n, S, 2 ** 40)
        assert M == event_fixed(n, S, 2 ** 40)[0] == (q if q % 2 == 0 else q + 1) and M % 2 == 0
    assert {divmod(256 * S, 512)[0] % 2 for S in (1, 3, -1, -3)} == {0, 1}           # (both parities of q occur above)
    # just beside a tie
    for n, S in ((1024, 2), (1024, 6), (1024, -2), (1000, 125), (1000, -125), (6, 3), (6, -3), (3, 1), (3, -1), (7, 5)):
        Q = S * S + 5
        assert lib_fixed(n, S, Q) == event_fixed(n, S, Q)
    # n = 1: M = 256 q, D = 0
    for q in (-32768, -1, 0, 1, 32767):
        assert lib_fixed(1, q, q * q) == event_fixed(1, q, q * q) == (256 * q, 0)
    # all samples equal: D = 0
    for n, q in ((2, 5), (1024, -32768), (1024, 32767), (777, -123), (3, 1)):
        assert lib_fixed(*nsq([q] * n)) == (event_fixed(*nsq([q] * n))[0], 0)
    # the bounds: 1,024 samples of +-32767 / -32768, and alternating -32768 / 32767 (V = 2^50 less a little, D near 2^23)
    for q in ([32767] * 1024, [-32767] * 1024, [-32768] * 1024, [-32768, 32767] * 512, [32767, -32767] * 512, [-32768, 32767] * 1):
        args = nsq(q)
        assert lib_fixed(*args) == event_fixed(*args)
    M, D = lib_fixed(*nsq([-32768, 32767] * 512))
    assert M == -128 and 2 ** 23 - 256 <= D <= 2 ** 23
    assert lib_fixed(*nsq([-32768] * 1024))[0] == -2 ** 23
    # perfect squares x and x +- 1.  Two samples a, -a: S = 0, Q = 2 a^2, V = 4 a^2, x = a^2 * 2^16 = (256 a)^2 ...
    for a in (1, 2, 3, 1000, 32767):
        assert lib_fixed(2, 0, 2 * a * a) == event_fixed(2, 0, 2 * a * a) == (0, 256 * a)
    # ... and any x at n = 1024, where x = floor(V / 16): one of the 16 values of V is 7 mod 8, so -V is a square mod 1024 and
    # some S < 1024 makes V + S^2 a multiple of 1024: Q = (V + S^2) / 1024 then gives n Q - S^2 = V exactly
    hits = 0
    for d in (1, 2, 3, 255, 256, 257, 4095, 4097, 65535, 2 ** 20 + 1, 2 ** 22 + 3, 2 ** 23 - 1):
        for x in (d * d - 1, d * d, d * d + 1):
            V = next(v for v in range(16 * x, 16 * x + 16) if v % 8 == 7)
            S = next(s_ for s_ in range(1024) if (V + s_ * s_) % 1024 == 0)
            Q = (V + S * S) // 1024
            assert 1024 * Q - S * S == V and V // 16 == x and Q <= 2 ** 40
            got = lib_fixed(1024, S, Q)
            assert got == event_fixed(1024, S, Q) and got[1] == (d - 1 if x == d * d - 1 else d)
            hits += 1
    assert hits == 36


def test_event_fixed_argument_errors():
    L = _lib.lib()
    M, D = C.c_int64(7), C.c_int64(7)
    for n in (0, -1, 1025, 2 ** 31 - 1):
        assert L.s2s_event_fixed(n, 0, 0, C.byref(M), C.byref(D)) == -1
    assert L.s2s_event_fixed(1, 0, 0, None, C.byref(D)) == -1 and L.s2s_event_fixed(1, 0, 0, C.byref(M), None) == -1
    assert (M.value, D.value) == (7, 7)
    assert L.s2s_event_fixed(1024, 0, 0, C.byref(M), C.byref(D)) == 0 and (M.value, D.value) == (0, 0)


def consistent_model(k, seed, fill=0.7):
    """Counters as an accumulation would leave them: per row some events of 1..1024 int16 samples around a level of the row's own
    (negative for about half of the rows); about 1 - fill of the rows have no event."""
    rng = np.random.default_rng(seed)
    t = np.zeros((4 ** k + 1, 5), np.int64)
    for r in range(4 ** k + 1):
        if rng.random() > fill:
            continue
        level = int(rng.integers(-30000, 30000))
        row = [0, 0, 0, 0, 0]
        for _ in range(int(rng.integers(1, 30))):
            q = np.clip(level + rng.integers(-400, 400, int(rng.integers(1, 200))), -32768, 32767)
            M, D = event_fixed(*nsq(q))
            row = [row[0] + 1, row[1] + M, row[2] + M * M, row[3] + D, row[4] + D * D]
        t[r] = row
    return t


def raw_format(table, k, cal, with_header, capacity, out):
    return _lib.lib().s2s_kmer_model_format(table.ctypes.data, k, *cal, int(with_header), out.ctypes.data, capacity)


@pytest.mark.parametrize("k", [1, 3, 6])
def test_format_equals_the_restatement(k):
    t = consistent_model(k, seed=k)
    t[0] = [1, -256 * 777 - 3, (256 * 777 + 3) ** 2, 0, 0]      # one event: both deviations 0.0000, a negative sum_m
    t[1] = 0                                                     # no event: no row
    t[2] = [3, -3 * 5000, 3 * 5000 * 5000, 3 * 40, 3 * 40 * 40]  # three equal events
    t[4 ** k] = [9, 12345, 99999999, 77, 7777]                   # a populated N row: absent from the text
    assert (t[:, 1] < 0).any() and (t[:, 1] > 0).any()
    for cal in (CAL, (2048.0, 281.345551, -127.5655735), (1.0, -1e6, -3e4)):
        for header in (True, False):
            text = bytes(format_model(t, k, *cal, with_header=header))
            assert text == py_model(t, k, *cal, with_header=header)
        text = bytes(format_model(t, k, *cal))
        got_k, rows = parse_model(text)
        names = list(rows)
        assert got_k == k and names[0] == "A" * k and "N" * k not in rows and "A" * (k - 1) + "C" not in rows
        assert names == sorted(names) and len(names) == int((t[:4 ** k, 0] >= 1).sum()) == 4 ** k - missing_kmers(t, k)
        assert rows["A" * k]["level_stdv"] in ("0.0000", "-0.0000") and rows["A" * k]["sd_mean"] in ("0.0000", "-0.0000")
        assert rows["A" * k]["n_events"] == 1
        assert rows["A" * (k - 1) + "G"]["level_stdv"] in ("0.0000", "-0.0000") and rows["A" * (k - 1) + "G"]["sd_stdv"] in ("0.0000", "-0.0000")
    head = f"#k\t{k}\n#alphabet\tnucleotide\n".encode() + ("\t".join(COLUMNS) + "\n").encode()
    assert bytes(format_model(np.zeros((4 ** k + 1, 5), np.int64), k, *CAL)) == head          # a run without reads
    assert bytes(format_model(np.zeros((4 ** k + 1, 5), np.int64), k, *CAL, with_header=False)) == b""
    only_n = np.zeros((4 ** k + 1, 5), np.int64)
    only_n[4 ** k] = [5, 1, 1, 1, 1]
    assert bytes(format_model(only_n, k, *CAL)) == head


def test_products_that_need_128_bits():
    t = np.zeros((5, 5), np.int64)
    e = 2 ** 16
    M = -(2 ** 23) + 12345
    t[0] = [e, e * M + 999, e * M * M + 2 * 999 * M + 10 ** 9, e * 2 ** 22, e * 2 ** 44 + 10 ** 12]
    assert int(t[0, 0]) * int(t[0, 2]) > 2 ** 77 and int(t[0, 0]) * int(t[0, 2]) - int(t[0, 1]) ** 2 > 0     # (beyond 64 bits)
    t[1] = [1, 2, 3, 4, 5]                                      # e*A2 - A*A = -1, e*B2 - Bs*Bs = -11 (no such events): clamped to 0
    text = bytes(format_model(t, 1, *CAL))
    assert text == py_model(t, 1, *CAL)
    _, rows = parse_model(text)
    assert float(rows["A"]["level_stdv"]) > 0 and float(rows["A"]["sd_stdv"]) > 0
    assert rows["C"]["level_stdv"] == "0.0000" and rows["C"]["sd_stdv"] == "0.0000"


def test_bound_capacity_and_arguments():
    L = _lib.lib()
    k = 3
    t = consistent_model(k, seed=9)
    for header in (0, 1):
        need = L.s2s_kmer_model_format_bound(t.ctypes.data, k, *CAL, header)
        out = np.full(need + 64, 0xAB, np.uint8)
        got = raw_format(t, k, CAL, header, need, out)
        assert 0 < got <= need and (out[need:] == 0xAB).all() and out[:got].tobytes() == py_model(t, k, *CAL, with_header=bool(header))
        for cap in (0, need - 1):                               # one byte under the bound: an error, the buffer untouched
            out[:] = 0xAB
            assert raw_format(t, k, CAL, header, cap, out) == -1 and (out == 0xAB).all()
    # the widest numbers any int64 counters give fit the bound
    wide = np.zeros((4 ** k + 1, 5), np.int64)
    wide[:] = [1, -2 ** 63, 2 ** 63 - 1, 2 ** 63 - 1, 2 ** 63 - 1]
    wide[1] = [2 ** 63 - 1, 2 ** 63 - 1, 2 ** 63 - 1, 0, 2 ** 63 - 1]
    need = L.s2s_kmer_model_format_bound(wide.ctypes.data, k, 1.0, -1e6, -3e4, 1)
    out = np.full(need + 8, 0xAB, np.uint8)
    got = raw_format(wide, k, (1.0, -1e6, -3e4), 1, need, out)
    assert 0 < got <= need and out[:got].tobytes() == py_model(wide, k, 1.0, -1e6, -3e4)
    out = np.full(1 << 16, 0xAB, np.uint8)
    for bad_k in (0, 11, -1):
        assert L.s2s_kmer_model_format_bound(t.ctypes.data, bad_k, *CAL, 1) == -1
        assert raw_format(t, bad_k, CAL, 1, out.size, out) == -1
    for cal in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (float("nan"), 1.0, 0.0)):
        assert L.s2s_kmer_model_format_bound(t.ctypes.data, k, *cal, 1) == -1 and raw_format(t, k, cal, 1, out.size, out) == -1
    for col in (0, 2, 3, 4):                                    # a negative counter other than sum_m
        neg = t.copy()
        neg[5, col] = -1
        assert raw_format(neg, k, CAL, 1, out.size, out) == -1
    neg = t.copy()
    neg[5, 1] = -abs(neg[5, 1]) - 1                             # ... sum_m may be
    assert raw_format(neg, k, CAL, 1, out.size, out) > 0
    out[:] = 0xAB
    assert L.s2s_kmer_model_format(None, k, *CAL, 1, out.ctypes.data, out.size) == -1
    assert L.s2s_kmer_model_format(t.ctypes.data, k, *CAL, 1, None, out.size) == -1
    assert (out == 0xAB).all()
    neg[5, 0] = -1
    for bad in (lambda: format_model(t, 2, *CAL), lambda: format_model(t, 11, *CAL), lambda: format_model(t, k, 0.0, 1.0, 0.0),
                lambda: format_model(neg, k, *CAL), lambda: format_model(t[:, :4], k, *CAL)):
        with pytest.raises(ValueError):
            bad()


def test_rank_files_sum_to_the_whole(tmp_path):
    k = 3
    parts = [consistent_model(k, seed=s, fill=0.5) for s in (1, 2, 3)]
    parts[1][:] = 0                                             # (a rank without reads)
    whole = parts[0] + parts[1] + parts[2]
    out = str(tmp_path / "m.model")
    paths = [rank_counts_path(out, r) for r in range(3)]
    assert paths[2] == str(tmp_path / "m.rank2.npz")
    for p, t in zip(paths, parts):
        save_counts(p, t, k, *CAL)
    got = load_counts(paths[0])
    assert np.array_equal(got[0], parts[0]) and got[1] == k and got[2] == tuple(float(np.float32(x)) for x in CAL)
    want = bytes(format_model(whole, k, *CAL))
    assert want == py_model(whole, k, *CAL)
    assert join_rank_files(paths, out, keep=True) == len(want)
    assert open(out, "rb").read() == want and all(os.path.exists(p) for p in paths)
    assert join_rank_files(paths[::-1], out) == len(want)       # integer sums: any order
    assert open(out, "rb").read() == want and not any(os.path.exists(p) for p in paths)
    # differing k or calibration: refused, nothing removed
    save_counts(paths[0], parts[0], k, *CAL)
    save_counts(paths[1], consistent_model(1, seed=1), 1, *CAL)
    save_counts(paths[2], parts[2], k, CAL[0], CAL[1], 11.0)
    for pair in ([paths[0], paths[1]], [paths[0], paths[2]]):
        with pytest.raises(ValueError, match="differ"):
            join_rank_files(pair, out)
    assert all(os.path.exists(p) for p in paths)
    with pytest.raises(ValueError):
        save_counts(paths[0], parts[0][:-1], k, *CAL)
    # the counts of a k-mer TABLE (six columns) are not a model's
    from seq2squiggle_amd.kmer_table import save_counts as save_table_counts
    save_table_counts(paths[0], np.zeros((4 ** k + 1, 6), np.int64), k, *CAL)
    with pytest.raises(ValueError, match="not the counts of a k-mer model"):
        load_counts(paths[0])


def test_exports_load_and_the_header_declares_them():
    """(fails before this feature: the library has none of the four)"""
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()
    for name in ("s2s_event_fixed", "s2s_kmer_model_accumulate", "s2s_kmer_model_format", "s2s_kmer_model_format_bound"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"^int(64_t)? %s\(" % name, header, re.M), name
    assert re.search(r"#define S2S_KMER_MODEL_FIELDS\s+5\b", header)
    c = header_constants(header)
    assert c["FIELDS"] == 5 and c["SLOTS"] >= 4 ** c["DIRECT_MAX_K"] + 1 and c["PROBES"] >= 1 and c["FLUSH_ROUNDS"] >= 1
    assert c["MAX_WORKGROUPS"] >= 1 and c["HASH_MUL"] % 2 == 1
    # two workgroups per CU at least: a slot is a 4-byte key and five 8-byte counters, a CU has 160 KiB of LDS
    assert 2 * c["SLOTS"] * (4 + 8 * c["FIELDS"]) <= 160 * 1024
    # between two flushes a workgroup inserts at most 4 chunks x 16 k-mers per round: a random k = 9 genome cannot overfill the cache
    assert c["FLUSH_ROUNDS"] * 4 * 16 <= c["SLOTS"]
    assert "\t".join(COLUMNS) in open(os.path.join(ROOT, "seq2squiggle_amd", "csrc", "s2s_host.cpp")).read().replace("\\t", "\t")


def test_cli_lists_the_option_and_names_the_rank_files(tmp_path):
    run = lambda *a, **kw: subprocess.run([sys.executable, "-m", "seq2squiggle_amd", "predict", *a], cwd=ROOT, capture_output=True,
                                          text=True, timeout=120, **kw)
    r = run("--show-advanced-options")
    assert r.returncode == 0 and "--kmer-model " in r.stdout
    assert "--kmer-model" not in run("--help").stdout               # an advanced option
    env = {k: v for k, v in dict(os.environ, S2S_DRY_LAUNCH="1").items() if k != "WORLD_SIZE"}
    r = run("g.fa", "-o", str(tmp_path / "o.blow5"), "--gpus", "2", "--kmer-model", "m.model", "--kmer-table", "t.tsv", env=env)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.strip().splitlines()]
    assert lines[-3] == {"kmer_model_rank_files": ["m.rank0.npz", "m.rank1.npz"]}     # before the k-mer table's line
    assert lines[-2] == {"kmer_table_rank_files": ["t.rank0.npz", "t.rank1.npz"]}
    cmd = lines[-1]["dry_launch"]
    assert cmd[cmd.index("--kmer-model") + 1] == "m.model" and "--gpus" not in cmd
    assert not os.path.exists(os.path.join(ROOT, "m.model"))        # a dry launch joins nothing
    # without the option the dry-launch output has no such line
    r = run("g.fa", "-o", str(tmp_path / "o.blow5"), "--gpus", "2", "--kmer-table", "t.tsv", env=env)
    assert r.returncode == 0 and "kmer_model" not in r.stdout


def test_the_model_needs_the_streaming_path(tmp_path):
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    from conftest import GOLDEN
    kw = dict(config=set_config(None), saved_weights=os.path.join(GOLDEN, "synthetic_k9.ckpt"),
              fasta=os.path.join(GOLDEN, "example_test.fasta"), read_input=True, n=-1, r=1000, c=-1, out=str(tmp_path / "o.blow5"),
              profile="dna-r10-prom", dwell_mean=None, dwell_std=0.0, noise_std=0.0, noise_sampling=False, duration_sampling=False,
              distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None, digitisation=None,
              range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None, min_noise=0.0,
              min_duration=3, min_read_len=30, preserve_read_ids=True, seed=1)
    with pytest.raises(ValueError, match="kmer_model needs the streaming path"):
        inference_run(**kw, streaming=False, kmer_model=str(tmp_path / "m.model"))
    assert not (tmp_path / "o.blow5").exists() and not (tmp_path / "m.model").exists()   # refused before anything is written
