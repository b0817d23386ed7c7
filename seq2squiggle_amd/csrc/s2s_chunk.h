// `preprocess`: training chunks from alignments (include/s2s_hip.h states the definition next to s2s_chunk_pack).  The rows of a read
// are the slots that pass s2s_chunk_row; they are compacted by ranks over the POOLED slots (tiles of S2S_SEG_TILE slots, the flag
// words, ranks and scan of s2s_prims.h), the reads' chunk counts are scanned, and from there on a wave owns one of the POOLED
// chunks: it finds its read by a search in the chunk offsets, whatever that read's length.  The row test, the sample and deviation
// formulas and the layout of the scratch are one set of functions for the kernels, the host entry and the host twin (s2s_host.cpp);
// the four kernels follow under S2S_DTW_KERNELS.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/s2s_hip.h"
#include "s2s_dtw.h"
#include "s2s_prims.h"

#define S2S_CHK_ONE 0x3C00                          // 1.0 in fp16
#define S2S_CHK_STDV_MAX_LEN 1024                   // n Q < 2^10 2^10 2^30 = 2^50 and S^2 <= 2^50: both fit int64

S2S_DTW_HD constexpr int64_t s2s_chk_tiles(int64_t slots) { return (slots + S2S_SEG_TILE - 1) / S2S_SEG_TILE; }
S2S_DTW_HD constexpr bool s2s_chk_params_ok(int32_t source, int32_t k, int32_t te, int32_t ts) {
    return (source == S2S_CHUNK_RAW || source == S2S_CHUNK_PA) && k >= 1 && k <= S2S_CHUNK_MAX_K && te >= 1 && te <= S2S_CHUNK_MAX_TE &&
           ts >= 1 && ts <= S2S_CHUNK_MAX_TS;
}
S2S_DTW_HD constexpr bool s2s_chk_counts_ok(int32_t P, int64_t total, int64_t slots, int64_t capacity) {
    return P >= 0 && P <= S2S_DTW_MAX_SAMPLES && total >= 0 && total <= S2S_SEG_MAX_TOTAL && slots >= 0 && slots <= S2S_CHUNK_MAX_SLOTS &&
           capacity >= 0 && capacity <= S2S_CHUNK_MAX_SLOTS;
}

// The scratch, every part at a multiple of 8 bytes: [tiles][32] flag words, [tiles + 1] ranks of the tiles, [tiles + 1] all-N rows
// before the tiles, [P] the rank of every read's first slot, [P + 1] the chunks before every read, [capacity + 1] the kept chunks
// before every chunk, [tiles][32] int32 ranks of the words inside their tile, [slots] int32: the slot of every row, by rank.
struct S2SChkScratch {
    int64_t words, trank, nrank, r_offs, c_offs, krank, wrank, rows, bytes;
};
S2S_DTW_HD inline S2SChkScratch s2s_chk_layout(int64_t slots, int32_t P, int64_t capacity) {
    const int64_t t = s2s_chk_tiles(slots);
    S2SChkScratch s;
    s.words = 0;
    s.trank = s.words + t * S2S_SEG_WORDS * 8;
    s.nrank = s.trank + (t + 1) * 8;
    s.r_offs = s.nrank + (t + 1) * 8;
    s.c_offs = s.r_offs + (int64_t)P * 8;
    s.krank = s.c_offs + ((int64_t)P + 1) * 8;
    s.wrank = s.krank + (capacity + 1) * 8;
    s.rows = s.wrank + t * S2S_SEG_WORDS * 4;
    s.bytes = (s.rows + slots * 4 + 15) / 16 * 16;
    return s;
}

// Slot g of a read whose record is samples [lo, hi) of a pool of `total`: 0 no row, 1 a row, 2 a row but for its k letters, all N.
S2S_DTW_HD inline int s2s_chunk_row(int64_t st, int64_t len, int64_t lo, int64_t hi, int64_t total, const uint8_t* letters, int32_t k) {
    if (len < 1 || st < 0 || lo < 0 || hi < lo || hi > total || st + len > hi - lo) return 0;
    for (int32_t t = 0; t < k; ++t)
        if (letters[t] != 'N') return 1;
    return 2;
}

// No a * b + c anywhere below: the device contracts, the host does not.
S2S_DTW_HD inline float s2s_chunk_pa(int32_t x, double digitisation, double offset, double range) {
    return (float)(((double)x + offset) * range / digitisation);
}
S2S_DTW_HD inline float s2s_chunk_stdv(int64_t n, int64_t S, int64_t Q, double digitisation, double range) {
    if (n < 1 || n > S2S_CHK_STDV_MAX_LEN) return 0.0f;
    const int64_t v = (int64_t)((uint64_t)n * (uint64_t)Q - (uint64_t)S * (uint64_t)S);      // (sums of a row: exact, never negative)
    return (float)(sqrt((double)(v < 0 ? 0 : v)) / (double)n * range / digitisation);
}
S2S_DTW_HD inline int32_t s2s_chunk_column(uint8_t letter) {
    return letter == '_' ? 0 : letter == 'A' ? 1 : letter == 'C' ? 2 : letter == 'G' ? 3 : letter == 'T' ? 4 : -1;
}

#if defined(S2S_DTW_KERNELS)
#include <hip/hip_runtime.h>

#define S2S_CHK_THREADS 256
#define S2S_CHK_WAVES (S2S_CHK_THREADS / 64)
#define S2S_CHK_LDS_BYTES (S2S_SEG_WORDS * 8 + S2S_CHK_WAVES * 4)          // the flag kernel: a tile's words and the waves' all-N counts
static_assert(S2S_SEG_TILE % S2S_CHK_THREADS == 0 && S2S_SEG_WORDS <= 64 && S2S_CHUNK_MAX_TE <= 64, "a wave's ballot is a flag word; a wave holds a chunk's rows");

struct S2SChkIn {
    const void* pool;                               // int16 (raw) or float (pa)
    const long long* s_offs;
    const long long* l_offs;
    const int* ev_start;
    const int* ev_len;
    const long long* S;
    const long long* Q;
    const double* cal;
    const float* stdv;
    const uint8_t* kmers;
    long long total, slots, capacity;
    int P, source, k, te, ts, reverse, backwards;
};

// Launch 1: one flag per slot that is a row, one count of all-N rows per tile.  Every branch around a barrier is uniform.
__global__ __launch_bounds__(S2S_CHK_THREADS) void s2s_chunk_flags_kernel(S2SChkIn in, unsigned long long* __restrict__ words,
                                                                          int* __restrict__ wrank, long long* __restrict__ trank,
                                                                          long long* __restrict__ nrank) {
    __shared__ unsigned long long s_words[S2S_SEG_WORDS];
    __shared__ int s_n[S2S_CHK_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long g0 = (long long)blockIdx.x * S2S_SEG_TILE;
    int ra, rb;
    {
        long long lo, hi;
        s2s_record_find(in.l_offs, 0, in.P - 1, in.slots, g0, ra, lo, hi);
        s2s_record_find(in.l_offs, 0, in.P - 1, in.slots, (g0 + S2S_SEG_TILE < in.slots ? g0 + S2S_SEG_TILE : in.slots) - 1, rb, lo, hi);
        if (rb < ra) rb = ra;
    }
    int all_n = 0;
    for (int j = 0; j < S2S_SEG_TILE / S2S_CHK_THREADS; ++j) {
        const int e = tid + S2S_CHK_THREADS * j;
        const long long g = g0 + e;
        int p, row = 0;
        long long lo, hi;
        if (g < in.slots && s2s_record_find(in.l_offs, ra, rb, in.slots, g, p, lo, hi))
            row = s2s_chunk_row(in.ev_start[g], in.ev_len[g], in.s_offs[p], in.s_offs[p + 1], in.total, in.kmers + g * in.k, in.k);
        const unsigned long long word = __ballot(row == 1);
        all_n += __popcll(__ballot(row == 2));
        if (lane == 0) s_words[e >> 6] = word;
    }
    if (lane == 0) s_n[wave] = all_n;
    __syncthreads();
    s2s_bitmap_publish(s_words, tid, blockIdx.x, words, wrank, trank);
    if (tid == 0) {                                 // the tile's other count; launch 2 scans the two
        int n = 0;
        for (int q = 0; q < S2S_CHK_WAVES; ++q) n += s_n[q];
        nrank[blockIdx.x + 1] = n;
    }
}

// Launch 3: the flagged slots of tile blockIdx.x write themselves at their rank; the reads are dealt out over all threads of the grid
// for their row counts and chunk counts (c_offs[p + 1]: launch 4 scans it).
__global__ __launch_bounds__(S2S_CHK_THREADS) void s2s_chunk_compact_kernel(S2SChkIn in, const unsigned long long* __restrict__ words,
                                                                            const int* __restrict__ wrank, const long long* __restrict__ trank,
                                                                            int* __restrict__ rows, long long* __restrict__ r_offs,
                                                                            long long* __restrict__ c_offs, int* __restrict__ n_rows) {
    const int tid = (int)threadIdx.x;
    for (long long p = (long long)blockIdx.x * S2S_CHK_THREADS + tid; p < in.P; p += (long long)gridDim.x * S2S_CHK_THREADS) {
        const long long lo = in.l_offs[p], hi = in.l_offs[p + 1];
        long long at = 0, n = 0;
        if (lo >= 0 && hi >= lo && hi <= in.slots) {
            at = s2s_bitmap_rank(words, wrank, trank, lo);
            n = s2s_bitmap_rank(words, wrank, trank, hi) - at;
        }
        r_offs[p] = at;
        n_rows[p] = (int)n;
        c_offs[p + 1] = n > 0 ? n / in.te + 1 : 0;
    }
    const long long t = blockIdx.x, g0 = t * S2S_SEG_TILE;
    for (int j = 0; j < S2S_SEG_TILE / S2S_CHK_THREADS; ++j) {
        const long long g = g0 + tid + S2S_CHK_THREADS * j;
        const int bit = (int)(g & 63);
        const unsigned long long word = words[g >> 6];
        if ((word >> bit) & 1ull) rows[s2s_bitmap_rank_in(trank[t], wrank, g, word)] = (int)g;
    }
}

// What lane j of the wave that owns chunk c knows of row j of the chunk.
struct S2SChkRow {
    long long first;                                // the row's first sample in the pool
    int len, slot;                                  // len 0: no row (j >= te); slot -1: a pad row
    bool ok;
    int p;
    long long lo;
};

// formed = min(c_offs[P], capacity); c < formed.  The read: the largest p with c_offs[p] <= c (reads without chunks share their offset
// with the read behind them).
__device__ inline S2SChkRow s2s_chunk_load(const S2SChkIn& in, const int* __restrict__ rows, const long long* __restrict__ r_offs,
                                           const long long* __restrict__ c_offs, const int* __restrict__ n_rows, long long c, int lane) {
    const int a = s2s_last_le(0, in.P - 1, c, [&](int m) { return c_offs[m]; });
    S2SChkRow r;
    r.p = a;
    r.lo = in.s_offs[a];
    r.first = 0; r.len = 0; r.slot = -1; r.ok = true;
    const long long n = n_rows[a], i = (c - c_offs[a]) * in.te + lane;
    if (lane >= in.te) return r;
    r.len = 1;
    if (i >= n) return r;                           // a pad row
    const long long g = rows[r_offs[a] + (in.backwards ? n - 1 - i : i)];
    const long long st = in.ev_start[g], len = in.ev_len[g], hi = in.s_offs[a + 1];
    r.slot = (int)g;
    r.ok = !(len < 1 || st < 0 || r.lo < 0 || hi < r.lo || hi > in.total || st + len > hi - r.lo);      // (always: launch 1 tested it)
    r.len = r.ok ? (int)len : 1;
    r.first = r.lo + st;
    return r;
}

// Launch 5: krank[c + 1] = 1 for a chunk that is kept, else 0 -- over the whole capacity, which launch 6 scans.
__global__ __launch_bounds__(S2S_CHK_THREADS) void s2s_chunk_lengths_kernel(S2SChkIn in, const int* __restrict__ rows,
                                                                            const long long* __restrict__ r_offs,
                                                                            const long long* __restrict__ c_offs, const int* __restrict__ n_rows,
                                                                            long long* __restrict__ krank) {
    const int lane = (int)threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * S2S_CHK_WAVES + ((int)threadIdx.x >> 6);      // (the same for the whole wave)
    if (c >= in.capacity) return;
    const long long formed = c_offs[in.P] < in.capacity ? c_offs[in.P] : in.capacity;
    long long keep = 0;
    if (c < formed) {
        const S2SChkRow r = s2s_chunk_load(in, rows, r_offs, c_offs, n_rows, c, lane);
        const long long tl = s2s_wave_sum<long long>(r.len), bad = s2s_wave_sum<long long>(r.ok ? 0 : 1);
        keep = tl <= in.ts && bad == 0 ? 1 : 0;
    }
    if (lane == 0) krank[c + 1] = keep;
}

// Launch 7: the kept chunk c writes row krank[c] of the five outputs.  Every shuffle runs with all 64 lanes: the loops around them
// are uniform, only the stores are predicated.
__global__ __launch_bounds__(S2S_CHK_THREADS) void s2s_chunk_write_kernel(S2SChkIn in, const int* __restrict__ rows,
                                                                          const long long* __restrict__ r_offs,
                                                                          const long long* __restrict__ c_offs, const int* __restrict__ n_rows,
                                                                          const long long* __restrict__ krank, const long long* __restrict__ nrank,
                                                                          long long tiles, uint16_t* __restrict__ chunks,
                                                                          long long* __restrict__ chunks_lengths, float* __restrict__ targets,
                                                                          long long* __restrict__ targets_lengths, float* __restrict__ stdevs,
                                                                          long long* __restrict__ counters) {
    const int lane = (int)threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * S2S_CHK_WAVES + ((int)threadIdx.x >> 6);
    if (c == 0 && lane == 0) {
        counters[0] = c_offs[in.P];
        counters[1] = krank[in.capacity];
        counters[2] = nrank[tiles];
    }
    if (c >= in.capacity) return;
    const long long formed = c_offs[in.P] < in.capacity ? c_offs[in.P] : in.capacity;
    if (c >= formed || krank[c + 1] == krank[c]) return;                     // (the same for the whole wave)
    const long long at = krank[c];
    const int te = in.te, k = in.k, ts = in.ts;
    const S2SChkRow r = s2s_chunk_load(in, rows, r_offs, c_offs, n_rows, c, lane);
    const int incl = s2s_wave_prefix(r.len, lane);  // the rows' lengths: inclusive prefix over the lanes, <= ts here
    const int excl = incl - r.len, tl = __shfl(incl, 63);
    const double dig = in.cal ? in.cal[3 * r.p] : 1.0, off = in.cal ? in.cal[3 * r.p + 1] : 0.0, rng = in.cal ? in.cal[3 * r.p + 2] : 1.0;
    if (lane < te) {
        float dev = 0.0f;
        if (r.slot >= 0) dev = in.source == S2S_CHUNK_RAW ? s2s_chunk_stdv(r.len, in.S[r.slot], in.Q[r.slot], dig, rng) : in.stdv[r.slot];
        chunks_lengths[at * te + lane] = r.len;
        stdevs[at * te + lane] = dev;
    }
    if (lane == 0) targets_lengths[at] = tl;
    const int cells = te * k * 5;
    for (int base = 0; base < cells; base += 64) {
        const int e = base + lane, j = e / (k * 5), rest = e - j * (k * 5), t = rest / 5, col = rest - t * 5;
        const int slot = __shfl(r.slot, j & 63);
        if (e < cells) {
            const int hot = slot < 0 ? 0 : s2s_chunk_column(in.kmers[(long long)slot * k + t]);
            chunks[at * cells + e] = (uint16_t)(hot == col ? S2S_CHK_ONE : 0);
        }
    }
    for (int base = 0; base < ts; base += 64) {
        const int t = base + lane;
        int a = 0, b = te - 1;                      // the row of sample t: the last j < te with excl[j] <= t (every row holds a sample)
        for (int step = 0; step < 6; ++step) {      // (64 rows at most)
            const int m = a + (b - a + 1) / 2;
            const int v = __shfl(excl, m & 63);
            if (a < b) { if (v <= t) a = m; else b = m - 1; }
        }
        const int j_excl = __shfl(excl, a), j_len = __shfl(r.len, a), j_slot = __shfl(r.slot, a);
        const long long j_first = __shfl(r.first, a);
        if (t < ts) {
            float v = 0.0f;
            if (t < tl && j_slot >= 0) {
                const int o = t - j_excl;
                const long long idx = j_first + (in.reverse ? j_len - 1 - o : o);
                v = in.source == S2S_CHUNK_RAW ? s2s_chunk_pa(reinterpret_cast<const int16_t*>(in.pool)[idx], dig, off, rng)
                                               : reinterpret_cast<const float*>(in.pool)[idx];
            }
            targets[at * ts + t] = v;
        }
    }
}
#endif  // S2S_DTW_KERNELS
