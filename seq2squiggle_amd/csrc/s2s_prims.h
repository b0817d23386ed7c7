// What the signal kernels share (s2s_hip.hip's export, s2s_segment.h, s2s_eventalign.h, s2s_chunk.h): the 64-lane prefix and sum, the
// search for the last entry <= x and the record lookup built on it, the ranked bitmap over tiles of S2S_SEG_TILE pooled positions,
// and the one single-workgroup scan.  Only what has more than one user is here (but s2s_wave_sum, which only s2s_chunk_lengths_kernel
// calls: it stands beside the prefix as the other wave primitive); the device part follows under S2S_DTW_KERNELS.
#pragma once
#include <stdint.h>

#include "../../include/s2s_hip.h"
#include "s2s_dtw.h"

#define S2S_SEG_WORDS (S2S_SEG_TILE / 64)           // flag words of a tile
#define S2S_SEG_MAX_TOTAL ((int64_t)1 << 40)        // pooled samples of one call: 2^29 tiles, a grid the runtime takes

#if defined(S2S_DTW_KERNELS)
#include <hip/hip_runtime.h>

// ---- a wave.  All 64 lanes call these: the control flow around a call is uniform over the wave.
template <class T>
__device__ inline T s2s_wave_prefix(T v, int lane) {          // the sum of the lanes 0 .. lane
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}
template <class T>
__device__ inline T s2s_wave_sum(T v) {                         // the sum of all lanes, in every lane
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- the largest i in [a, b] with key(i) <= x; a where there is none (b < a included).  Equal keys: the last of them.
template <class I, class K>
__device__ inline I s2s_last_le(I a, I b, long long x, K key) {
    while (a < b) {
        const I m = a + (b - a + 1) / 2;
        if (key(m) <= x) a = m; else b = m - 1;
    }
    return a;
}

// The record of pooled position g: the largest r in [ra, rb] with offs[r] <= g, then the check that makes any content of offs safe:
// 0 <= offs[r] <= g < offs[r+1] <= total.  (Empty records share their offset with the record behind them: the largest r is the one
// that holds g.)  ra, rb: 0 .. R - 1, or what the same search gave for the ends of a range that holds g.
__device__ inline bool s2s_record_find(const long long* __restrict__ offs, int ra, int rb, long long total, long long g, int& r, long long& lo,
                                       long long& hi) {
    r = s2s_last_le(ra, rb, g, [&](int m) { return offs[m]; });
    lo = offs[r];
    hi = offs[r + 1];
    return lo >= 0 && lo <= g && g < hi && hi <= total;
}

// ---- the ranked bitmap: [tiles][S2S_SEG_WORDS] flag words, wrank the flags of a tile before each of its words, trank[t] the flags
// before tile t ([tiles + 1]; a flag kernel leaves the tile's own count in trank[t + 1] and a scan makes the ranks of them).
// Publishing tile `tile` from its words in LDS, after the barrier behind their last write; every thread of the workgroup may call it.
__device__ inline void s2s_bitmap_publish(const unsigned long long* s_words, int tid, long long tile, unsigned long long* __restrict__ words,
                                          int* __restrict__ wrank, long long* __restrict__ trank) {
    if (tid >= S2S_SEG_WORDS) return;
    int before = 0;
    for (int q = 0; q < tid; ++q) before += __popcll(s_words[q]);
    const long long at = tile * S2S_SEG_WORDS + tid;
    words[at] = s_words[tid];
    wrank[at] = before;
    if (tid == S2S_SEG_WORDS - 1) trank[tile + 1] = before + __popcll(s_words[tid]);
}
// The rank of pooled position g, whose word is `word` and whose tile has rank `tile_rank` (trank[g / S2S_SEG_TILE], which a
// workgroup that owns a tile reads once for all its threads): the tile's rank, the word's rank in the tile, the bits below.
__device__ inline long long s2s_bitmap_rank_in(long long tile_rank, const int* __restrict__ wrank, long long g, unsigned long long word) {
    return tile_rank + wrank[g >> 6] + __popcll(word & ((1ull << (g & 63)) - 1ull));
}
// Flags before pooled position pos (0 <= pos <= tiles * S2S_SEG_TILE).
__device__ inline long long s2s_bitmap_rank(const unsigned long long* __restrict__ words, const int* __restrict__ wrank,
                                            const long long* __restrict__ trank, long long pos) {
    if ((pos & (S2S_SEG_TILE - 1)) == 0) return trank[pos / S2S_SEG_TILE];          // (also pos = tiles * S2S_SEG_TILE, which has no word)
    return s2s_bitmap_rank_in(trank[pos / S2S_SEG_TILE], wrank, pos, words[pos >> 6]);
}

// ---- the scan: out[i] = the sum of value(j) over j < i, for i = 0 .. n; out[n] is the total.  One workgroup of 1,024 threads walks
// the array, ITEMS consecutive elements per thread and step: a 64-lane prefix, the 16 wave sums through LDS (its only 128 B), their
// prefix over a row of 16 lanes in every wave, and the carry in a register.  `out` may be the array that `value`
// reads one entry ahead of (S2SScanNext).  THE RULE that makes this sound, for any ITEMS: every read of a step happens before that
// step's first barrier and every write after it, and step s + 1 reads only entries that step s did not write -- a step reads the
// entries base + 1 .. base + 1024 ITEMS of such an array and writes base .. base + 1024 ITEMS - 1; out[n] is written after the
// last step.  Hence no __restrict__ on `out`.
struct S2SScanInts {                                // value(i) = c[i]; c 16-byte aligned
    const int* c;
    __device__ long long operator()(long long i) const { return c[i]; }
};
struct S2SScanNext {                                // value(i) = a[i + 1], out = a: a[i + 1] holds element i, a[0] anything
    const long long* a;
    __device__ long long operator()(long long i) const { return a[i + 1]; }
};

// The ITEMS elements from i0 on, 0 beyond n.
template <int ITEMS, class V>
__device__ inline void s2s_scan_load(const V& value, long long i0, long long n, long long (&c)[ITEMS]) {
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) c[k] = i0 + k < n ? value(i0 + k) : 0;
}
__device__ inline void s2s_scan_load(const S2SScanInts& value, long long i0, long long n, long long (&c)[8]) {
    if (i0 + 8 <= n) {                              // (i0 a multiple of 8)
        const int4 a = *reinterpret_cast<const int4*>(value.c + i0), b = *reinterpret_cast<const int4*>(value.c + i0 + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
        s2s_scan_load<8, S2SScanInts>(value, i0, n, c);
    }
}

// v of the lane SHIFT lanes below in the same row of 16 lanes, 0 from beyond the row's start: a DPP row shift of either half, no LDS.
template <int SHIFT>
__device__ inline long long s2s_row_below(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + SHIFT, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(v >> 32), 0x110 + SHIFT, 0xF, 0xF, true);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// v of lane `from`, the same for the whole wave, as a scalar.
__device__ inline long long s2s_lane_value(long long v, int from) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, from), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), from);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

template <int ITEMS, class V>
__global__ __launch_bounds__(1024) void s2s_scan_kernel(V value, long long n, long long* out) {
    __shared__ long long wsum[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    long long carry = 0;
    for (long long base = 0; base < n; base += 1024 * ITEMS) {       // (uniform)
        const long long i0 = base + (long long)ITEMS * tid;
        long long c[ITEMS], own = 0;
        s2s_scan_load(value, i0, n, c);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) own += c[k];
        const long long v = s2s_wave_prefix(own, lane);
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        // the 16 wave sums in the lanes 0 .. 15 of every wave and their inclusive prefix over that row: lane 15 holds the step's total,
        // lane wave - 1 the sums of the waves before this one.  (All 64 lanes run this; the rows above read nothing and hold 0.)
        long long p = lane < 16 ? wsum[lane] : 0;
        p += s2s_row_below<1>(p);
        p += s2s_row_below<2>(p);
        p += s2s_row_below<4>(p);
        p += s2s_row_below<8>(p);
        const long long all = s2s_lane_value(p, 15), before = wave > 0 ? s2s_lane_value(p, wave > 0 ? wave - 1 : 0) : 0;
        long long run = carry + before + v - own;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (i0 + k < n) out[i0 + k] = run;
            run += c[k];
        }
        carry += all;
        __syncthreads();
    }
    if (tid == 0) out[n] = carry;
}
#endif  // S2S_DTW_KERNELS
