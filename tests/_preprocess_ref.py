"""The definition of the training chunks (include/s2s_hip.h, next to s2s_chunk_pack) restated in plain numpy, read by read: what
s2s_chunk_pack_host must equal byte for byte.  It follows the reference's preprocess.py (process_df -> get_chunks -> pad_lengths ->
typical_indices, per read) with the deviations the README lists; nothing here is shared with the package."""
import math

import numpy as np

RAW, PA = 0, 1
LETTERS = b"_ACGT"


def rows_of_read(ev_start, ev_len, n_samples, kmers, backwards):
    """The slots of one read -> (the row slots in position order, all-N rows).  kmers: uint8 [slots, k]."""
    rows, all_n = [], 0
    for j in range(len(ev_len)):
        st, ln = int(ev_start[j]), int(ev_len[j])
        if ln < 1 or st < 0 or st + ln > n_samples:
            continue
        if bytes(kmers[j]) == b"N" * kmers.shape[1]:
            all_n += 1
            continue
        rows.append(j)
    return (rows[::-1] if backwards else rows), all_n


def stdv_raw(n, S, Q, cal):
    if n > 1024:
        return np.float32(0.0)
    digitisation, _, rng = cal
    v = max(int(n) * int(Q) - int(S) * int(S), 0)
    return np.float32(np.float64(math.sqrt(v)) / np.float64(n) * np.float64(rng) / np.float64(digitisation))


def pa_raw(x, cal):
    digitisation, offset, rng = (np.float64(c) for c in cal)
    return ((x.astype(np.float64) + offset) * rng / digitisation).astype(np.float32)


def pack(pool, s_offs, source, l_offs, ev_start, ev_len, S, Q, cal, stdv, kmers, k, te, ts, reverse=False, backwards=False, capacity=None):
    """-> dict(chunks uint16 [N, te, k, 5] (fp16 bits), chunks_lengths int64 [N, te], targets float32 [N, ts], targets_lengths int64
    [N], stdevs float32 [N, te], n_rows int32 [P], counters int64 [3]: formed, kept, all-N rows).
    capacity (the header's rule for the device entry): "chunks beyond chunk_capacity are not formed (counters[0] still counts them)" --
    of the chunks in read order, then chunk order, only the first `capacity` exist; the kept ones among them come out and are what
    counters[1] counts; n_rows and counters[0] are those of the whole batch.
    Offsets (the header's definition of a row): a read has rows only if 0 <= l_offs[p] <= l_offs[p+1] <= slots and 0 <= s_offs[p] <=
    s_offs[p+1] <= total, with slots = len(ev_len) and total = len(pool)."""
    P = len(l_offs) - 1
    kmers = np.asarray(kmers, np.uint8).reshape(-1, k)
    out = {"chunks": [], "chunks_lengths": [], "targets": [], "targets_lengths": [], "stdevs": []}
    n_rows, formed, all_n_total = np.zeros(P, np.int32), 0, 0
    for p in range(P):
        lo, hi, s0 = int(l_offs[p]), int(l_offs[p + 1]), int(s_offs[p])
        n_samples = int(s_offs[p + 1]) - s0
        if not (0 <= lo <= hi <= len(ev_len) and 0 <= s0 <= s0 + n_samples <= len(pool)):
            continue
        rows, all_n = rows_of_read(ev_start[lo:hi], ev_len[lo:hi], n_samples, kmers[lo:hi], backwards)
        all_n_total += all_n
        n = n_rows[p] = len(rows)
        if n == 0:
            continue
        c = tuple(cal[3 * p:3 * p + 3]) if source == RAW else None
        letters, lengths, samples, devs = [], [], [], []
        for j in rows:
            g = lo + j
            st, ln = int(ev_start[g]), int(ev_len[g])
            x = pool[s0 + st:s0 + st + ln]
            x = pa_raw(x, c) if source == RAW else x.astype(np.float32)
            letters.append(bytes(kmers[g]))
            lengths.append(ln)
            samples.append(x[::-1] if reverse else x)
            devs.append(stdv_raw(ln, S[g], Q[g], c) if source == RAW else np.float32(stdv[g]))
        for _ in range(te - n % te):
            letters.append(b"_" * k)
            lengths.append(1)
            samples.append(np.zeros(1, np.float32))
            devs.append(np.float32(0.0))
        for a in range(0, len(letters), te):
            formed += 1
            tl = sum(lengths[a:a + te])
            if tl > ts or (capacity is not None and formed > capacity):
                continue
            hot = np.zeros((te, k, 5), np.uint16)
            for r, word in enumerate(letters[a:a + te]):
                for t, ch in enumerate(word):
                    if ch in LETTERS:
                        hot[r, t, LETTERS.index(ch)] = 0x3C00
            tg = np.zeros(ts, np.float32)
            tg[:tl] = np.concatenate(samples[a:a + te])
            out["chunks"].append(hot)
            out["chunks_lengths"].append(np.array(lengths[a:a + te], np.int64))
            out["targets"].append(tg)
            out["targets_lengths"].append(tl)
            out["stdevs"].append(np.array(devs[a:a + te], np.float32))
    N = len(out["targets_lengths"])
    return {"chunks": np.array(out["chunks"], np.uint16).reshape(N, te, k, 5),
            "chunks_lengths": np.array(out["chunks_lengths"], np.int64).reshape(N, te),
            "targets": np.array(out["targets"], np.float32).reshape(N, ts),
            "targets_lengths": np.array(out["targets_lengths"], np.int64).reshape(N),
            "stdevs": np.array(out["stdevs"], np.float32).reshape(N, te),
            "n_rows": n_rows, "counters": np.array([formed, N, all_n_total], np.int64)}
