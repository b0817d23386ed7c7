// `segment`: event detection by two windowed t-statistics (include/s2s_hip.h states the definition next to s2s_segment), in integers
// only.  A position's score depends on the 2 w samples around it and on nothing else, so the work is split over the POOLED positions:
// workgroup t owns [S2S_SEG_TILE t, S2S_SEG_TILE (t + 1)) whatever records lie there -- the inside of one long record, or thousands
// of empty ones.  The score and the layout of the scratch are one set of functions for the kernels, the host entry and the host twin
// (s2s_host.cpp); the two kernels follow under S2S_DTW_KERNELS, and the scan between them is s2s_prims.h's.
#pragma once
#include <stdint.h>

#include "../../include/s2s_hip.h"
#include "s2s_dtw.h"
#include "s2s_prims.h"

#define S2S_SEG_MAX_HALO (3 * S2S_SEG_MAX_WINDOW)   // max(2 w_l, 3 w_s) at the largest windows

// max(2 w_l, 3 w_s): a long peak at p needs the long scores of [p - w_l, p + w_l], i.e. the samples [p - 2 w_l, p + 2 w_l); the merge
// rule needs the short peaks of [p - w_s, p + w_s], those the short scores of [p - 2 w_s, p + 2 w_s], those the samples
// [p - 3 w_s, p + 3 w_s).
S2S_DTW_HD constexpr int32_t s2s_seg_halo(int32_t w_s, int32_t w_l) { return 2 * w_l > 3 * w_s ? 2 * w_l : 3 * w_s; }
S2S_DTW_HD constexpr int64_t s2s_seg_tiles(int64_t total) { return (total + S2S_SEG_TILE - 1) / S2S_SEG_TILE; }
// scratch: [tiles][32] flag words (uint64), [tiles][32] ranks of the words inside their tile (int32), [tiles + 1] ranks of the tiles
S2S_DTW_HD constexpr int64_t s2s_seg_scratch(int64_t total) { return s2s_seg_tiles(total) * (S2S_SEG_WORDS * 12) + (s2s_seg_tiles(total) + 1) * 8; }
S2S_DTW_HD constexpr bool s2s_seg_params_ok(int32_t w_s, int32_t w_l, int64_t t_s, int64_t t_l) {
    return w_s >= 1 && w_s <= w_l && w_l <= S2S_SEG_MAX_WINDOW && t_s >= 1 && t_s <= S2S_SEG_MAX_THRESHOLD && t_l >= 1 &&
           t_l <= S2S_SEG_MAX_THRESHOLD;
}

// floor(256 w d^2 / max(V, 1)) from the window sums: sl, sr the sums of L and R (|.| <= 32 * 32,768 = 2^20), qq = Q_L + Q_R (<= 2^36).
S2S_DTW_HD inline int64_t s2s_seg_score(int32_t sl, int32_t sr, int64_t qq, int32_t w) {
    const int64_t d = (int64_t)sr - sl;
    if (d == 0) return 0;                           // (no division)
    const int64_t v = (int64_t)w * qq - (int64_t)sl * sl - (int64_t)sr * sr;
    return (int64_t)((uint64_t)(256 * (int64_t)w * d * d) / (uint64_t)(v < 1 ? 1 : v));
}

#if defined(S2S_DTW_KERNELS)
#include <hip/hip_runtime.h>

#define S2S_SEG_THREADS 256
#define S2S_SEG_EXT (S2S_SEG_TILE + 2 * S2S_SEG_MAX_HALO)

struct S2SSegLds {
    long long sc_s[S2S_SEG_EXT], sc_l[S2S_SEG_EXT]; // the two detectors' scores of the tile and its halo
    unsigned long long words[S2S_SEG_WORDS];        // the tile's flags
    int16_t x[S2S_SEG_EXT];                          // the samples (0 where no record is)
    unsigned char dl[S2S_SEG_EXT], dr[S2S_SEG_EXT];  // min(255, samples between the position and its record's start / end); dr = 0: no record
    unsigned char pk[S2S_SEG_EXT];                   // short peaks
};
#define S2S_SEG_LDS_BYTES 47296                     // 2 x 2,240 x 8 + 32 x 8 + 2,240 x (2 + 1 + 1 + 1)
static_assert(sizeof(S2SSegLds) == S2S_SEG_LDS_BYTES && S2S_SEG_LDS_BYTES <= 65536, "include/s2s_hip.h states the LDS bytes of s2s_segment");
static_assert(S2S_SEG_TILE % (64 * (S2S_SEG_THREADS / 64)) == 0 && S2S_SEG_WORDS <= 64, "a wave's ballot is one whole flag word");

// Launch 1.  Every branch around a barrier depends on blockIdx and the arguments only.
__global__ __launch_bounds__(S2S_SEG_THREADS) void s2s_segment_flags_kernel(
    const int16_t* __restrict__ samples, const long long* __restrict__ offs, int R, long long total, int w_s, int w_l, long long t_s,
    long long t_l, unsigned long long* __restrict__ words, int* __restrict__ wrank, long long* __restrict__ trank) {
    __shared__ S2SSegLds s;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int H = s2s_seg_halo(w_s, w_l), ext = S2S_SEG_TILE + 2 * H;
    const long long g0 = (long long)blockIdx.x * S2S_SEG_TILE, gb = g0 - H;
    int ra, rb;
    {                                               // the records of the two ends of what this tile reads (the same for every thread)
        long long lo, hi;
        const long long ga = gb < 0 ? 0 : gb, ge = (gb + ext < total ? gb + ext : total) - 1;
        s2s_record_find(offs, 0, R - 1, total, ga, ra, lo, hi);
        s2s_record_find(offs, 0, R - 1, total, ge, rb, lo, hi);
        if (rb < ra) rb = ra;                       // (offsets that decrease)
    }
    for (int e = tid; e < ext; e += S2S_SEG_THREADS) {
        const long long g = gb + e;
        int r;
        long long lo = 0, hi = 0;
        const bool in = g >= 0 && g < total && s2s_record_find(offs, ra, rb, total, g, r, lo, hi) && hi - lo <= S2S_DTW_MAX_SAMPLES;
        const long long a = g - lo, b = hi - g;
        s.x[e] = in ? samples[g] : (int16_t)0;
        s.dl[e] = (unsigned char)(in ? (a > 255 ? 255 : a) : 0);
        s.dr[e] = (unsigned char)(in ? (b > 255 ? 255 : b) : 0);
    }
    __syncthreads();
    // score(e) needs x[e - w, e + w): for the short detector e in [H - 2 w_s, H + TILE + 2 w_s) reads x[H - 3 w_s ..] >= x[0], for the long
    // one e in [H - w_l, H + TILE + w_l) reads x[H - 2 w_l ..]; both end below ext.  w <= i <= n - w is dl >= w and dr >= w: then both
    // windows lie inside the record.
    for (int e = tid; e < ext; e += S2S_SEG_THREADS) {
        long long vs = 0, vl = 0;
        const int dl = s.dl[e], dr = s.dr[e];
        if (e >= H - 2 * w_s && e < H + S2S_SEG_TILE + 2 * w_s && dl >= w_s && dr >= w_s) {
            int sl = 0, sr = 0;
            long long qq = 0;
            for (int k = 1; k <= w_s; ++k) {
                const int a = s.x[e - k], b = s.x[e + k - 1];
                sl += a; sr += b;
                qq += (long long)(a * a) + (long long)(b * b);      // (|a| <= 32,768: a * a <= 2^30 fits int)
            }
            vs = s2s_seg_score(sl, sr, qq, w_s);
        }
        if (e >= H - w_l && e < H + S2S_SEG_TILE + w_l && dl >= w_l && dr >= w_l) {
            int sl = 0, sr = 0;
            long long qq = 0;
            for (int k = 1; k <= w_l; ++k) {
                const int a = s.x[e - k], b = s.x[e + k - 1];
                sl += a; sr += b;
                qq += (long long)(a * a) + (long long)(b * b);
            }
            vl = s2s_seg_score(sl, sr, qq, w_l);
        }
        s.sc_s[e] = vs;
        s.sc_l[e] = vl;
    }
    __syncthreads();
    // short peaks of [H - w_s, H + TILE + w_s): their neighbours' scores were formed above.  A peak has w <= i <= n - w, so every
    // neighbour lies in [0, n] of the same record, and position n -- sample 0 of the next record, or no sample -- has score 0.
    for (int e = tid; e < ext; e += S2S_SEG_THREADS) {
        bool p = false;
        if (e >= H - w_s && e < H + S2S_SEG_TILE + w_s) {
            const long long v = s.sc_s[e];
            p = v >= t_s;
            for (int k = 1; k <= w_s; ++k) p = p && v > s.sc_s[e - k] && v >= s.sc_s[e + k];
        }
        s.pk[e] = p ? 1 : 0;
    }
    __syncthreads();
    for (int j = 0; j < S2S_SEG_TILE / S2S_SEG_THREADS; ++j) {
        const int k = tid + S2S_SEG_THREADS * j, e = H + k;
        bool f = false;
        if (s.dr[e] > 0) {                          // a sample of a record that is not too long
            f = s.dl[e] == 0 || s.pk[e];
            if (!f) {
                const long long v = s.sc_l[e];
                bool p = v >= t_l;
                for (int q = 1; q <= w_l; ++q) p = p && v > s.sc_l[e - q] && v >= s.sc_l[e + q];
                for (int q = -w_s; q <= w_s; ++q) p = p && !s.pk[e + q];
                f = p;
            }
        }
        const unsigned long long word = __ballot(f);
        if (lane == 0) s.words[k >> 6] = word;
    }
    __syncthreads();
    s2s_bitmap_publish(s.words, tid, blockIdx.x, words, wrank, trank);       // trank[t + 1]: the tile's count; launch 2 scans it
}

// Launch 2 is s2s_scan_kernel<1, S2SScanNext> over trank: trank[t] = the flags of the tiles before t, trank[tiles] = all.

// Launch 3.  The flagged positions of tile blockIdx.x write their events; the records are dealt out over all threads of the grid for
// n_events.  The flag after a flagged position of rank k in a record whose end has rank > k + 1 is the flag of rank k + 1: in the
// same word, or the first bit of a word that two searches find -- the last tile with trank <= k + 1, the last word of it with
// wrank <= the rest (empty tiles and words share their rank with the one behind them, so the last is the one that holds it).
__global__ __launch_bounds__(S2S_SEG_THREADS) void s2s_segment_compact_kernel(
    const long long* __restrict__ offs, int R, long long total, long long tiles, const unsigned long long* __restrict__ words,
    const int* __restrict__ wrank, const long long* __restrict__ trank, const long long* __restrict__ ev_offs, int* __restrict__ ev_start,
    int* __restrict__ ev_len, int* __restrict__ n_events) {
    const int tid = (int)threadIdx.x;
    for (long long r = (long long)blockIdx.x * S2S_SEG_THREADS + tid; r < R; r += (long long)gridDim.x * S2S_SEG_THREADS) {
        const long long lo = offs[r], hi = offs[r + 1];
        int v = 0;
        if (lo >= 0 && hi >= lo && hi <= total) {
            if (hi - lo > S2S_DTW_MAX_SAMPLES) {
                v = S2S_DTW_COST_TOO_LONG;
            } else if (hi > lo) {
                const long long cnt = s2s_bitmap_rank(words, wrank, trank, hi) - s2s_bitmap_rank(words, wrank, trank, lo);
                const long long eo = ev_offs[r], cap = ev_offs[r + 1] - eo;
                v = (int)(eo >= 0 && cnt <= cap ? cnt : -cnt);
            }
        }
        n_events[r] = v;
    }
    const long long t = blockIdx.x, g0 = t * S2S_SEG_TILE;
    int ra, rb;
    {
        long long lo, hi;
        s2s_record_find(offs, 0, R - 1, total, g0, ra, lo, hi);
        s2s_record_find(offs, 0, R - 1, total, (g0 + S2S_SEG_TILE < total ? g0 + S2S_SEG_TILE : total) - 1, rb, lo, hi);
        if (rb < ra) rb = ra;
    }
    for (int j = 0; j < S2S_SEG_TILE / S2S_SEG_THREADS; ++j) {
        const long long g = g0 + tid + S2S_SEG_THREADS * j;
        const int bit = (int)(g & 63);
        const unsigned long long word = words[g >> 6];
        if (!((word >> bit) & 1ull)) continue;
        int r;
        long long lo, hi;
        if (!s2s_record_find(offs, ra, rb, total, g, r, lo, hi)) continue;      // (a flagged position has a record: not taken)
        const long long rk = s2s_bitmap_rank_in(trank[t], wrank, g, word);
        const long long r_lo = s2s_bitmap_rank(words, wrank, trank, lo), r_hi = s2s_bitmap_rank(words, wrank, trank, hi);
        const long long cnt = r_hi - r_lo, idx = rk - r_lo;
        const long long eo = ev_offs[r], cap = ev_offs[r + 1] - eo;
        if (eo < 0 || cnt > cap || idx < 0 || idx >= cnt) continue;          // the slot is too small: nothing is written to it
        long long next = hi;
        if (rk + 1 < r_hi) {
            const unsigned long long above = bit == 63 ? 0ull : (word >> (bit + 1)) << (bit + 1);
            if (above) {
                next = (g & ~63LL) + __ffsll((long long)above) - 1;
            } else {
                const long long a = s2s_last_le(t, tiles - 1, rk + 1, [&](long long m) { return trank[m]; });     // the last tile with trank <= rk + 1
                const int rest = (int)(rk + 1 - trank[a]);          // the last word of it with wrank <= rest
                const int qa = s2s_last_le(0, S2S_SEG_WORDS - 1, rest, [&](int m) { return wrank[a * S2S_SEG_WORDS + m]; });
                unsigned long long w2 = words[a * S2S_SEG_WORDS + qa];
                for (int c = rest - wrank[a * S2S_SEG_WORDS + qa]; c > 0 && w2; --c) w2 &= w2 - 1;     // (c = 0 here: the word's first flag)
                const long long found = (a * S2S_SEG_WORDS + qa) * 64 + (w2 ? __ffsll((long long)w2) - 1 : 0);
                next = found > g && found < hi ? found : hi;     // (always the former)
            }
        }
        ev_start[eo + idx] = (int)(g - lo);
        ev_len[eo + idx] = (int)(next - g);
    }
}
#endif  // S2S_DTW_KERNELS
