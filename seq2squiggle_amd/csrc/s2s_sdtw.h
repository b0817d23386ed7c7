// `compare --open-ends`: subsequence DTW of a short query inside a target, in integers only (include/s2s_hip.h states the
// definition next to s2s_sdtw; s2s_sdtw_host in s2s_host.cpp is its host twin).  Included by s2s_hip.hip behind s2s_dtw.h.
#pragma once
#include <stdint.h>

#include "../../include/s2s_hip.h"

#if defined(S2S_DTW_KERNELS)
#include <hip/hip_runtime.h>

#ifndef S2S_SDTW_THREADS
#define S2S_SDTW_THREADS 1024                       // one cell per thread at the largest default anchor (a build may set another count)
#endif
#define S2S_SDTW_WINDOW 256                         // diagonals per refill of the target window (a power of two)
#define S2S_SDTW_RING (S2S_SDTW_MAX_QUERY + 2)      // slots of one diagonal: row i at slot i + 1 (slot 0 is "row -1": read, never used)
#define S2S_SDTW_LDS_BYTES (3 * S2S_SDTW_RING * 8 + S2S_SDTW_MAX_QUERY * 2 + (S2S_SDTW_MAX_QUERY + S2S_SDTW_WINDOW) * 2)   // 57,904
#define S2S_SDTW_NONE 0x7fffffff                    // E of a predecessor outside the matrix (never added to: (i - 1, j) always exists)

// One workgroup per problem; anti-diagonals d = i + j, one barrier each.  The matrix is dense: diagonal d holds the rows
// lo(d) = max(0, d - (H - 1)) .. hi(d) = min(L - 1, d), every one of them computed, so a predecessor exists exactly when its row and
// column are >= 0 and no range has to be kept.  Three diagonals of (E, S) live in LDS, row i at slot i + 1; a slot that still holds
// an older diagonal's value is never read as a predecessor (row i - 1 of diagonal d - 1 and d - 2 and row i of d - 1 were all
// written on exactly those diagonals when the cell exists).  Thread x keeps the rows i = x mod blockDim.x: r = (x - lo(d)) mod
// blockDim.x is carried (lo grows by at most 1 per diagonal), so the loop holds no division, and row L - 1 belongs to one thread,
// which keeps the running (min E, smallest j, S) in registers -- j grows with d, so '<' keeps the smallest j.  The query sits in
// LDS whole (read back to front for reverse); the target samples come from a window that is refilled every S2S_SDTW_WINDOW
// diagonals: d - hi(d) never decreases, so the columns of the next S2S_SDTW_WINDOW diagonals lie in j0 = d0 - hi(d0) ..
// j0 + (hi(d0) - lo(d0)) + S2S_SDTW_WINDOW - 1 < j0 + L + S2S_SDTW_WINDOW.  L, H and the loop counter are the only inputs of every
// loop bound and of every branch around a barrier: the control flow is uniform over the workgroup, and the sweep takes L + H - 1
// diagonals whatever memory holds.  Any number of threads gives the same integers.
__global__ __launch_bounds__(S2S_SDTW_THREADS) void s2s_sdtw_kernel(const int16_t* __restrict__ q, const long long* __restrict__ q_begin,
                                                                   const long long* __restrict__ q_len, const int16_t* __restrict__ t,
                                                                   const long long* __restrict__ t_begin, const long long* __restrict__ t_len,
                                                                   const unsigned char* __restrict__ reverse, long long* __restrict__ cost,
                                                                   long long* __restrict__ start, long long* __restrict__ end) {
    __shared__ int2 ring[3 * S2S_SDTW_RING];        // (E, S) of diagonal d, d - 1, d - 2
    __shared__ int16_t qs[S2S_SDTW_MAX_QUERY];
    __shared__ int16_t wt[S2S_SDTW_MAX_QUERY + S2S_SDTW_WINDOW];
    const int p = blockIdx.x;
    const int x = (int)threadIdx.x, bd = (int)blockDim.x;
    const long long qb = q_begin[p], L64 = q_len[p], tb = t_begin[p], H64 = t_len[p];
    const bool refused = qb < 0 || tb < 0 || L64 < 0 || H64 < 0 || L64 > S2S_SDTW_MAX_QUERY || H64 > S2S_DTW_MAX_SAMPLES;
    if (refused || L64 == 0 || H64 == 0) {          // (uniform over the workgroup: before any barrier)
        if (x == 0) {
            cost[p] = refused ? S2S_DTW_COST_TOO_LONG : S2S_DTW_COST_EMPTY;
            start[p] = 0;
            end[p] = 0;
        }
        return;
    }
    const int L = (int)L64, H = (int)H64;
    const bool rev = reverse[p] != 0;
    const int16_t* pq = q + qb;
    const int16_t* pt = t + tb;
    for (int i = x; i < L; i += bd) qs[i] = rev ? pq[L - 1 - i] : pq[i];     // (visible behind the barrier of the first refill)
    int oc = 0, o1 = S2S_SDTW_RING, o2 = 2 * S2S_SDTW_RING;
    int r = x, lo1 = 0;                             // (x - lo(d)) mod bd, and lo of the diagonal before
    int j0 = 0;                                     // first column of the window
    int best_e = S2S_SDTW_NONE, best_j = 0, best_s = 0;
    const int last = L + H - 2, win = L + S2S_SDTW_WINDOW;
    for (int d = 0; d <= last; ++d) {
        int lo = d - (H - 1);
        lo = lo < 0 ? 0 : lo;
        const int hi = d < L - 1 ? d : L - 1;
        if (lo > lo1) r = r == 0 ? bd - 1 : r - 1;
        lo1 = lo;
        if ((d & (S2S_SDTW_WINDOW - 1)) == 0) {     // (uniform: d is) the target samples of the next S2S_SDTW_WINDOW diagonals, once
            j0 = d - hi;
            for (int k = x; k < win; k += bd) {
                const int j = j0 + k;
                wt[k] = j < H ? (rev ? pt[H - 1 - j] : pt[j]) : (int16_t)0;
            }
            __syncthreads();
        }
        // the three predecessors are read whatever they hold (every slot lies inside the ring) and chosen by i > 0 and j > 0; the
        // tie rule: diagonal, then up, then left ('<' keeps the earlier one)
        auto cell = [&](int i) -> int2 {
            const int j = d - i;
            const int xa = qs[i], xb = wt[j - j0];
            const int c = xa < xb ? xb - xa : xa - xb;
            const int2 up = ring[o1 + i], left = ring[o1 + i + 1], diag = ring[o2 + i];
            int2 b = j > 0 ? diag : make_int2(S2S_SDTW_NONE, 0);
            b = up.x < b.x ? up : b;
            b = (j > 0 && left.x < b.x) ? left : b;
            return i == 0 ? make_int2(c, j) : make_int2(b.x + c, b.y);
        };
        auto keep = [&](int i, int2 v) {
            ring[oc + i + 1] = v;
            if (i == L - 1 && v.x < best_e) { best_e = v.x; best_j = d - i; best_s = v.y; }
        };
        int i = lo + r;
        for (; i + bd <= hi; i += 2 * bd) {          // two cells per step while two strides fit: their LDS reads issue together
            const int2 v0 = cell(i), v1 = cell(i + bd);
            keep(i, v0);
            keep(i + bd, v1);
        }
        if (i <= hi) keep(i, cell(i));
        __syncthreads();
        const int o = o2; o2 = o1; o1 = oc; oc = o;
    }
    if (x == (L - 1) % bd) {                        // the owner of row L - 1
        cost[p] = best_e;
        start[p] = rev ? H - (best_j + 1) : best_s;
        end[p] = rev ? H - best_s : best_j + 1;
    }
}
#endif  // S2S_DTW_KERNELS
