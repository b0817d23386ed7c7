// `resquiggle`: the alignment of a stored signal to the levels of its k-mers (include/s2s_hip.h states the definition next to
// s2s_resquiggle), in integers only.  Every sample belongs to one k-mer and the k-mer index never falls, so a cell depends on the
// previous sample row alone -- (i - 1, j - 1), (i - 1, j), (i - 1, j - 2) -- and a whole row is computed in parallel: no
// anti-diagonal skew.  The layout of the decision scratch is one set of functions for the kernels, the host entry and the host twin
// (s2s_host.cpp); the three kernels follow under S2S_DTW_KERNELS.
#pragma once
#include <stdint.h>

#include "../../include/s2s_hip.h"
#include "s2s_dtw.h"

#define S2S_RSQ_ADV 0                               // from (i - 1, j - 1): the sample opens k-mer j
#define S2S_RSQ_STAY 1                              // from (i - 1, j)
#define S2S_RSQ_SKIP 2                              // from (i - 1, j - 2): k-mer j - 1 gets no sample
#define S2S_RSQ_NONE 3                              // row 0, cells outside the band and unreached cells

// The decision scratch of a read: row i holds at most 2 R + 1 in-band cells; they are packed by SLOT, slot(j) = j mod ring with
// ring = 64 chunks(R) > 2 R + 1 (2 R + 1 is odd), 64 slots to a 16-byte word pair (bit 0 of the 64 codes, then bit 1): cell
// (i, j) is bit slot(j) mod 64 of pair i chunks + slot(j) / 64.  The walk back needs no band arithmetic at all.
S2S_DTW_HD constexpr int32_t s2s_rsq_chunks(int64_t R) { return (int32_t)((2 * R + 1 + 63) / 64); }
S2S_DTW_HD inline bool s2s_rsq_solvable(int64_t n, int64_t K) {
    return n >= 1 && K >= 1 && n <= S2S_DTW_MAX_SAMPLES && K <= S2S_DTW_MAX_SAMPLES && K <= 2 * n;
}
S2S_DTW_HD inline int64_t s2s_rsq_bytes(int64_t n, int64_t K, int64_t R) { return s2s_rsq_solvable(n, K) ? n * s2s_rsq_chunks(R) * 16 : 0; }

#if defined(S2S_DTW_KERNELS)
#include <hip/hip_runtime.h>

#define S2S_RSQ_MAX_WAVES 16
#define S2S_RSQ_PER_WAVE 3                          // ceil(chunks(S2S_DTW_MAX_BAND) / S2S_RSQ_MAX_WAVES) = ceil(33 / 16)
#define S2S_RSQ_BLOCK 64                            // rows per refill of the level window and of the wave's sample register
#define S2S_RSQ_LEVEL_RING(R) (64 * (size_t)s2s_rsq_chunks(R) + 2 * S2S_RSQ_BLOCK)
#define S2S_RSQ_LDS_BYTES(R) (2 * 64 * (size_t)s2s_rsq_chunks(R) * 8 + S2S_RSQ_LEVEL_RING(R) * 2)
static_assert(S2S_RSQ_MAX_WAVES * S2S_RSQ_PER_WAVE >= (2 * S2S_DTW_MAX_BAND + 1 + 63) / 64, "every chunk of the widest band has a wave");

// Waves of the sweep's workgroup for a band: the chunks are dealt out evenly, ceil(chunks / 16) to a wave.
inline int s2s_rsq_waves(int R) {
    const int chunks = s2s_rsq_chunks(R), per = (chunks + S2S_RSQ_MAX_WAVES - 1) / S2S_RSQ_MAX_WAVES;
    return (chunks + per - 1) / per;
}

// One workgroup per read; rows i = 0 .. n - 1, one barrier each.  Row i holds the columns
//   jlo(i) = max(0, ceil(i K / n) - R)  ...  jhi(i) = min(K - 1, floor(i K / n) + R),
// floor(i K / n) carried with its remainder (i K grows by K <= 2 n: the quotient by at most 2 -- no division in the loop).  D lives in
// two rows of `ring` int64 in LDS (read row i - 1, write row i: one barrier per row is enough), slot(j) = j mod ring.  A thread
// owns up to S2S_RSQ_PER_WAVE slots (chunk = wave + u waves, slot = 64 chunk + lane) and for each its present column j: when
// j + ring <= jhi the slot moves on to column j + ring (the old one left the band: ring > the row width).  EVERY owned slot is
// written in every row -- D, or "unreached" for a slot whose column is outside [jlo, jhi] -- so a slot never shows a stale row:
// the slot of j - 1 (j - 2) holds D(i - 1, j - 1) exactly when that cell is in the band and reached, because K <= 2 n lets a row's
// window move by at most two columns, fewer than would bring column j - 1 - ring back into it.  D(i - 1, j) is the thread's own
// register.  The sample of a row is the same for every lane: lane t of every wave holds sample i0 + t of the current block of 64
// rows (the next block's is in flight meanwhile) and the row's is read from lane i mod 64.  The levels come from a window in LDS,
// level(j) at j mod (ring + 128), topped up every 64 rows with the columns the next 64 rows can reach; a lane reads its level when
// its slot's column becomes active, not per row.  Per 64 slots: two ballots and one 16-byte store of the decisions by lane 0 (only
// into a slot of `scratch` that is aligned and large enough: s2s_rsq_bytes).  n, K, R and the loop counters are the only inputs of
// every branch around a barrier.  LDS: S2S_RSQ_LDS_BYTES(R) = 1024 chunks + 2 (64 chunks + 128), 38,272 B at S2S_DTW_MAX_BAND.
__global__ __launch_bounds__(64 * S2S_RSQ_MAX_WAVES) void s2s_resquiggle_kernel(
    const int16_t* __restrict__ q, const long long* __restrict__ q_offs, const int16_t* __restrict__ l, const long long* __restrict__ l_offs,
    int R, int skip_penalty, int unknown_cost, long long* __restrict__ cost, unsigned char* __restrict__ scratch,
    const long long* __restrict__ scratch_offs) {
    extern __shared__ long long s2s_rsq_lds[];      // [2][ring] int64, then the level window [ring + 128] int16
    const int p = blockIdx.x;
    const long long qo = q_offs[p], lo_ = l_offs[p];
    const long long n64 = q_offs[p + 1] - qo, K64 = l_offs[p + 1] - lo_;
    if (!s2s_rsq_solvable(n64, K64)) {              // (uniform over the workgroup: before any barrier)
        if (threadIdx.x == 0)
            cost[p] = (n64 > S2S_DTW_MAX_SAMPLES || K64 > S2S_DTW_MAX_SAMPLES) ? S2S_DTW_COST_TOO_LONG
                      : (n64 <= 0 || K64 <= 0)                                 ? S2S_DTW_COST_EMPTY
                                                                               : S2S_RSQ_UNREACHED;
        return;
    }
    const int n = (int)n64, K = (int)K64;
    const int chunks = s2s_rsq_chunks(R), ring = 64 * chunks, lring = ring + 2 * S2S_RSQ_BLOCK;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
    const int16_t* pq = q + qo;
    const int16_t* pl = l + lo_;
    int16_t* lev = reinterpret_cast<int16_t*>(s2s_rsq_lds + 2 * ring);
    ulonglong2* dec = nullptr;
    {
        const long long so = scratch_offs[p], sz = scratch_offs[p + 1] - so;
        if (so >= 0 && (so & 15) == 0 && sz >= (long long)n * chunks * 16) dec = reinterpret_cast<ulonglong2*>(scratch + so);
    }
    int col[S2S_RSQ_PER_WAVE], lslot[S2S_RSQ_PER_WAVE], have[S2S_RSQ_PER_WAVE], level[S2S_RSQ_PER_WAVE];
    long long own[S2S_RSQ_PER_WAVE];
#pragma unroll
    for (int u = 0; u < S2S_RSQ_PER_WAVE; ++u) {
        col[u] = lslot[u] = 64 * (wave + u * waves) + lane;      // (slot < ring < lring while the chunk exists)
        have[u] = -1;                                           // the column whose level is in level[u]
        level[u] = 0;
        own[u] = S2S_DTW_UNREACHED;
    }
    int f = 0, r = 0;                               // floor(i K / n) and i K mod n
    int filled = -1;                                // the level window holds the columns <= filled that a row can still reach
    int xs = 0, xn = lane < n ? pq[lane] : 0;       // the samples of this block of rows and of the next
    for (int i = 0; i < n; ++i) {
        if ((i & (S2S_RSQ_BLOCK - 1)) == 0) {       // (uniform: i is)
            // the rows i .. i + 63 reach no column beyond floor(i K / n) + R + ceil(63 K / n) <= f + R + 127, and need none below
            // ceil(i K / n) - R >= f - R: at most 2 R + 128 < lring columns, all distinct in the window
            int target = f + R + 2 * S2S_RSQ_BLOCK - 1;
            target = target > K - 1 ? K - 1 : target;
            for (int c = filled + 1 + (int)threadIdx.x; c <= target; c += (int)blockDim.x) lev[(unsigned)c % (unsigned)lring] = pl[c];
            filled = target > filled ? target : filled;
            xs = xn;
            const int nx = i + S2S_RSQ_BLOCK + lane;
            xn = nx < n ? pq[nx] : 0;
            __syncthreads();
        }
        const int x = __shfl(xs, i & (S2S_RSQ_BLOCK - 1));
        int jlo = f + (r != 0) - R, jhi = f + R;
        jlo = jlo < 0 ? 0 : jlo;
        jhi = jhi > K - 1 ? K - 1 : jhi;
        const long long* rd = s2s_rsq_lds + ((i & 1) ? 0 : ring);
        long long* wr = s2s_rsq_lds + ((i & 1) ? ring : 0);
#pragma unroll
        for (int u = 0; u < S2S_RSQ_PER_WAVE; ++u) {
            const int chunk = wave + u * waves;
            if (chunk < chunks) {                   // (the same for a wave's lanes; no barrier inside)
                const int s = 64 * chunk + lane;
                if (col[u] + ring <= jhi) {         // the slot moves on to its next column
                    col[u] += ring;
                    lslot[u] += ring;
                    lslot[u] = lslot[u] >= lring ? lslot[u] - lring : lslot[u];
                    own[u] = S2S_DTW_UNREACHED;     // (ring == 2 R + 2 and a window that moves by two: the old column was active a row ago)
                }
                const int j = col[u];
                const bool active = j >= jlo && j <= jhi;
                if (active && have[u] != j) { level[u] = lev[lslot[u]]; have[u] = j; }
                const long long p1 = rd[s == 0 ? ring - 1 : s - 1], p2 = rd[s < 2 ? s + ring - 2 : s - 2];
                long long best = S2S_DTW_UNREACHED;
                unsigned code = S2S_RSQ_NONE;       // the tie rule: advance, then stay, then skip ('<' keeps the earlier one)
                if (j >= 1 && p1 < best) { best = p1; code = S2S_RSQ_ADV; }
                if (own[u] < best) { best = own[u]; code = S2S_RSQ_STAY; }
                const long long t2 = p2 >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : p2 + skip_penalty;
                if (j >= 2 && t2 < best) { best = t2; code = S2S_RSQ_SKIP; }
                if (i == 0) { best = j == 0 ? 0 : S2S_DTW_UNREACHED; code = S2S_RSQ_NONE; }
                const int lv = level[u];
                const int dx = x - lv;               // (no branch: |x - lv| <= 65,535)
                const int c = lv == S2S_RSQ_UNKNOWN ? unknown_cost : (dx < 0 ? -dx : dx);
                const bool reached = active && best < S2S_DTW_UNREACHED;
                const long long v = reached ? best + c : S2S_DTW_UNREACHED;
                code = reached ? code : (unsigned)S2S_RSQ_NONE;
                own[u] = v;
                wr[s] = v;
                const unsigned long long b0 = __ballot(code & 1u), b1 = __ballot(code & 2u);
                if (lane == 0 && dec) dec[(long long)i * chunks + chunk] = make_ulonglong2(b0, b1);
            }
        }
        __syncthreads();
        r += K;
        if (r >= n) { r -= n; f += 1; }
        if (r >= n) { r -= n; f += 1; }
    }
    if (threadIdx.x == 0) {                         // D(n - 1, K - 1): row n - 1 was written last (the barrier above)
        const long long v = s2s_rsq_lds[(((n - 1) & 1) ? ring : 0) + (K - 1) % ring];
        cost[p] = v < S2S_DTW_UNREACHED ? v : (long long)S2S_RSQ_UNREACHED;
    }
}

// The walk back through the decisions of s2s_resquiggle_kernel: one wave per read, from (n - 1, K - 1).  Every lane runs the same walk
// on the same values (the loads are wave-uniform); lane 0 stores ev_start / ev_len of a k-mer when the walk leaves its column.  The
// wave first writes start = -1, len = 0 to all K k-mers of a read that is not too long -- what a skipped k-mer, an unsolved read and a
// read whose slot of scratch is too small or misaligned keep.  The row falls by one per step, so the walk takes at most n steps
// whatever the scratch holds; the slot index stays inside the row's words, and a walk that does not end in (0, 0) (no sweep writes
// such decisions) takes its stores back.
__global__ __launch_bounds__(64) void s2s_resquiggle_trace_kernel(const long long* __restrict__ q_offs, const long long* __restrict__ l_offs,
                                                                  int R, const long long* __restrict__ cost,
                                                                  const unsigned char* __restrict__ scratch,
                                                                  const long long* __restrict__ scratch_offs, int* __restrict__ ev_start,
                                                                  int* __restrict__ ev_len) {
    const int p = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const long long lo_ = l_offs[p];
    const long long n64 = q_offs[p + 1] - q_offs[p], K64 = l_offs[p + 1] - lo_;
    if (lo_ < 0 || K64 <= 0 || K64 > S2S_DTW_MAX_SAMPLES || n64 > S2S_DTW_MAX_SAMPLES) return;
    const int K = (int)K64;
    int* st = ev_start + lo_;
    int* ln = ev_len + lo_;
    for (int j = lane; j < K; j += 64) { st[j] = -1; ln[j] = 0; }
    const int chunks = s2s_rsq_chunks(R), ring = 64 * chunks;
    const long long so = scratch_offs[p], sz = scratch_offs[p + 1] - so;
    if (!s2s_rsq_solvable(n64, K64) || cost[p] < 0 || so < 0 || (so & 15) != 0 || sz < n64 * chunks * 16) return;
    __threadfence();                                // the fill is complete before lane 0 stores into it
    const ulonglong2* dec = reinterpret_cast<const ulonglong2*>(scratch + so);
    int i = (int)n64 - 1, j = K - 1, s = j % ring, len = 0;
    bool arrived = false;
    for (;;) {
        ++len;
        if (i == 0) {
            arrived = j == 0;
            if (arrived && lane == 0) { st[0] = 0; ln[0] = len; }
            break;
        }
        const ulonglong2 w = dec[(long long)i * chunks + (s >> 6)];
        const unsigned code = (unsigned)((w.x >> (s & 63)) & 1ull) | ((unsigned)((w.y >> (s & 63)) & 1ull) << 1);
        if (code == S2S_RSQ_NONE) break;
        if (code != S2S_RSQ_STAY) {
            const int dj = code == S2S_RSQ_ADV ? 1 : 2;
            if (j < dj) break;
            if (lane == 0) { st[j] = i; ln[j] = len; }
            len = 0;
            j -= dj;
            s -= dj;
            s = s < 0 ? s + ring : s;
        }
        --i;
    }
    if (!arrived) {
        __threadfence();
        for (int t = lane; t < K; t += 64) { st[t] = -1; ln[t] = 0; }
    }
}

// S = sum x, Q = sum x^2 (int64) of every k-mer's raw stored samples [start, start + len): a quarter wave (16 lanes) per k-mer strides
// its samples and adds up by four shuffles -- no atomics.  A k-mer is shared by its 16 lanes whatever its length: the usual event holds
// about ten samples (one stride), and a stalled k-mer of 30,000 costs its quarter wave 1,875 strides of one coalesced 32-byte load
// while the other k-mers of the read go to other quarter waves -- far below the sweep of such a read.  An interval that does not lie
// inside the read's samples counts as empty: nothing is read outside a record whatever ev_start / ev_len hold.
#define S2S_RSQ_SUM_SLICES 8                        // workgroups per read (blockIdx.y), striding over its k-mers
__global__ __launch_bounds__(256) void s2s_event_sums_kernel(const int16_t* __restrict__ samples, const long long* __restrict__ s_offs,
                                                             const int* __restrict__ ev_start, const int* __restrict__ ev_len,
                                                             const long long* __restrict__ l_offs, long long* __restrict__ S,
                                                             long long* __restrict__ Q) {
    const int p = blockIdx.x;
    const long long so = s_offs[p], n = s_offs[p + 1] - so, lo_ = l_offs[p], K = l_offs[p + 1] - lo_;
    const int sub = (int)threadIdx.x & 15;
    for (long long j = (long long)blockIdx.y * 16 + ((int)threadIdx.x >> 4); j < K; j += 16LL * S2S_RSQ_SUM_SLICES) {
        const long long b = ev_start[lo_ + j], len = ev_len[lo_ + j];
        const bool ok = b >= 0 && len > 0 && b + len <= n;
        long long s1 = 0, s2 = 0;
        for (long long t = sub; ok && t < len; t += 16) {
            const long long x = samples[so + b + t];
            s1 += x;
            s2 += x * x;
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
            s1 += __shfl_xor(s1, d);
            s2 += __shfl_xor(s2, d);
        }
        if (sub == 0) { S[lo_ + j] = s1; Q[lo_ + j] = s2; }
    }
}
#endif  // S2S_DTW_KERNELS
