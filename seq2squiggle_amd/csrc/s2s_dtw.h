// `compare`: median / MAD, normalisation and banded DTW of stored int16 signals, in integers only (include/s2s_hip.h states the
// definitions next to s2s_dtw_banded).  The normalisation of one sample is one function for the kernel and for the host entry
// (s2s_host.cpp), so both sides compute the same integers by construction; the three kernels follow under S2S_DTW_KERNELS.
#pragma once
#include <stdint.h>

#include "../../include/s2s_hip.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define S2S_DTW_HD __host__ __device__
#else
#define S2S_DTW_HD
#endif

#define S2S_DTW_MAX_SCALE 8192                      // 2 * 65,535 * scale + 65,535 stays below 2^31
#define S2S_DTW_UNREACHED ((int64_t)1 << 62)        // "+infinity" of the recurrence (a real cost stays below 2^40)

// q = clamp(floor((2 (x - med) scale + d) / (2 d)), -32767, 32767), d = max(mad, 1): round-half-up on a true floor division.
// med and mad are clamped to what a record of int16 samples can give, so that no argument overflows the 32-bit numerator.
S2S_DTW_HD inline int16_t s2s_dtw_normalise_one(int32_t x, int32_t med, int32_t mad, int32_t scale) {
    med = med < -32768 ? -32768 : med > 32767 ? 32767 : med;
    const int32_t d = mad < 1 ? 1 : mad > 65535 ? 65535 : mad;
    const int32_t num = 2 * (x - med) * scale + d, den = 2 * d;
    int32_t q = num / den;                          // (C++ truncates towards zero)
    if (num - q * den < 0) q -= 1;
    return (int16_t)(q < -32767 ? -32767 : q > 32767 ? 32767 : q);
}

// The decision scratch of a pair's warping path (s2s_dtw_path): diagonal d = i + j holds at most floor(2 T / (n + m)) + 1 in-band
// cells, T = R max(n, m) (the rows i with |i (n + m) - d n| <= T), packed 64 cells to a 16-byte word pair (bit 0 of the 64 codes,
// then bit 1), cell i at bit (i - lo(d)) of pair (i - lo(d)) / 64: a fixed number of pairs per diagonal, n + m - 1 diagonals.
S2S_DTW_HD inline int32_t s2s_dtw_path_chunks(int64_t n, int64_t m, int64_t R) {
    const int64_t T = R * (n > m ? n : m);
    return (int32_t)((2 * T / (n + m) + 1 + 63) / 64);
}
S2S_DTW_HD inline int64_t s2s_dtw_path_bytes(int64_t n, int64_t m, int64_t R) {
    if (n <= 0 || m <= 0 || n > S2S_DTW_MAX_SAMPLES || m > S2S_DTW_MAX_SAMPLES) return 0;
    return (n + m - 1) * s2s_dtw_path_chunks(n, m, R) * 16;
}

#if defined(S2S_DTW_KERNELS)           // s2s_hip.hip alone defines it: s2s_host.cpp passes through the same compiler
#include <hip/hip_runtime.h>

#define S2S_DTW_SELECT_THREADS 256                  // = the bins of one histogram pass: thread t clears bin t

// The key of rank k (0-based) among the n 16-bit keys of a record, by two 256-bin histogram passes: the high byte, then the low byte
// among the keys of the selected high byte.  ABS = false: key = x + 32768 (order of x); ABS = true: key = |x - med| (0 .. 65,535).
// Called by all 256 threads of the workgroup with the same p, n, k, med (every barrier in uniform control flow).
template <bool ABS>
__device__ __forceinline__ unsigned s2s_dtw_key(int x, int med) { return ABS ? (unsigned)(x < med ? med - x : x - med) : (unsigned)(x + 32768); }

template <bool ABS>
__device__ unsigned s2s_dtw_select(const int16_t* __restrict__ p, int n, unsigned k, int med, unsigned* hist, unsigned* sel) {
    const int t = threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += S2S_DTW_SELECT_THREADS) atomicAdd(&hist[s2s_dtw_key<ABS>(p[i], med) >> 8], 1u);
    __syncthreads();
    if (t == 0) {
        unsigned acc = 0;
        int b = 0;
        for (; b < 255 && acc + hist[b] <= k; ++b) acc += hist[b];
        sel[0] = (unsigned)b;
        sel[1] = k - acc;
    }
    __syncthreads();
    const unsigned hi = sel[0], k2 = sel[1];
    hist[t] = 0;                                    // (every thread has its own bin: nobody reads hist between the barriers)
    __syncthreads();
    for (int i = t; i < n; i += S2S_DTW_SELECT_THREADS) {
        const unsigned key = s2s_dtw_key<ABS>(p[i], med);
        if ((key >> 8) == hi) atomicAdd(&hist[key & 255u], 1u);
    }
    __syncthreads();
    if (t == 0) {
        unsigned acc = 0;
        int b = 0;
        for (; b < 255 && acc + hist[b] <= k2; ++b) acc += hist[b];
        sel[0] = (unsigned)b;
    }
    __syncthreads();
    const unsigned lo = sel[0];
    __syncthreads();                                // sel and hist are free again for the next call
    return (hi << 8) | lo;
}

// One workgroup of 256 threads per record: four coalesced sweeps, no sort, no float.
__global__ __launch_bounds__(S2S_DTW_SELECT_THREADS) void s2s_median_mad_kernel(const int16_t* __restrict__ samples,
                                                                               const long long* __restrict__ offs,
                                                                               int* __restrict__ med_out, int* __restrict__ mad_out) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[2];
    const int r = blockIdx.x;
    const long long o0 = offs[r], len = offs[r + 1] - o0;
    if (len <= 0 || len > S2S_DTW_MAX_SAMPLES) {    // (uniform over the workgroup: before any barrier)
        if (threadIdx.x == 0) { med_out[r] = 0; mad_out[r] = 0; }
        return;
    }
    const int n = (int)len;
    const int16_t* p = samples + o0;
    const unsigned k = (unsigned)(n - 1) >> 1;
    const int med = (int)s2s_dtw_select<false>(p, n, k, 0, hist, sel) - 32768;
    const int mad = (int)s2s_dtw_select<true>(p, n, k, med, hist, sel);
    if (threadIdx.x == 0) { med_out[r] = med; mad_out[r] = mad; }
}

#define S2S_DTW_NORM_SLICES 8                       // workgroups per record (blockIdx.y), striding over its samples

__global__ __launch_bounds__(256) void s2s_normalise_kernel(const int16_t* __restrict__ samples, const long long* __restrict__ offs,
                                                            const int* __restrict__ med, const int* __restrict__ mad, int scale,
                                                            int16_t* __restrict__ out) {
    const int r = blockIdx.x;
    const long long o0 = offs[r], n = offs[r + 1] - o0;
    const int m = med[r], d = mad[r];
    for (long long i = (long long)blockIdx.y * 256 + threadIdx.x; i < n; i += 256LL * S2S_DTW_NORM_SLICES)
        out[o0 + i] = s2s_dtw_normalise_one(samples[o0 + i], m, d, scale);
}

#ifndef S2S_DTW_CELLS
#define S2S_DTW_CELLS 2                             // cells per thread whose LDS reads are in flight together
#endif
#define S2S_DTW_WINDOW 256                          // diagonals per refill of the sample windows (a power of two)
#define S2S_DTW_LDS_BYTES(R) (3 * (2 * (size_t)(R) + 2) * 8 + 2 * (2 * (size_t)(R) + S2S_DTW_WINDOW) * 2)

// One workgroup per pair; anti-diagonals d = i + j, one barrier each.  On diagonal d the in-band rows are
//   lo(d) = max(0, d - (m - 1), ceil((d n - T) / (n + m)))  ...  hi(d) = min(n - 1, d, floor((d n + T) / (n + m))),  T = R max(n, m),
// at most 2 R + 1 of them.  The two quotients are carried from diagonal to diagonal with their remainders (d n grows by n < n + m:
// each quotient by 0 or 1), so the loop holds no division.  Three diagonals of int64 live in LDS, each a ring of W = 2 R + 2 slots
// indexed by i mod W; the slot of lo(d) is carried as well.  A predecessor is read only when its row lies in [lo, hi] of ITS
// diagonal (kept for the last two diagonals): a cell that has left the band, or a slot that still holds an older diagonal's value,
// never counts, so nothing has to be cleared.  The samples come from two LDS windows that are refilled every S2S_DTW_WINDOW
// diagonals (a global load per cell would sit on the critical path of every diagonal): lo(d) and hi(d) never decrease and grow by at
// most 1 per diagonal, so the rows of the next S2S_DTW_WINDOW diagonals lie in lo(d0) .. lo(d0) + 2 R + S2S_DTW_WINDOW - 1 and their
// columns in d0 - hi(d0) .. d0 - hi(d0) + 2 R + S2S_DTW_WINDOW - 1.  n, m, R and the two offsets are the only inputs of every loop bound and of
// every branch around a barrier: the control flow is uniform over the workgroup.  Any number of threads gives the same integers.
//   PATH = true (s2s_dtw_path) also records, per in-band cell, which predecessor its D came from -- S2S_DTW_OP_M / _A / _B for
// (i - 1, j - 1) / (i - 1, j) / (i, j - 1), the smallest D, on equal D in this order; S2S_DTW_OP_NONE for (0, 0) and for a cell no
// reached predecessor leads to -- as 2 bits in the pair's slot of `scratch` (layout: s2s_dtw_path_chunks above).  A wave's lanes
// hold 64 consecutive rows of the diagonal: two ballots and one 16-byte store by lane 0.  The strides are walked per wave here
// (the ballots need all 64 lanes in the same step); lanes past hi(d) repeat row hi(d), store nothing and vote NONE.  A slot that is
// misaligned or smaller than s2s_dtw_path_bytes gets no store at all (s2s_dtw_trace_kernel applies the same test and reports no
// path).  PATH = false is the cost-only kernel of s2s_dtw_banded, statement for statement what it was before the flag.
template <bool PATH>
__global__ __launch_bounds__(256) void s2s_dtw_kernel(const int16_t* __restrict__ a, const long long* __restrict__ a_offs,
                                                      const int16_t* __restrict__ b, const long long* __restrict__ b_offs, int R,
                                                      long long* __restrict__ cost, unsigned char* __restrict__ scratch,
                                                      const long long* __restrict__ scratch_offs) {
    extern __shared__ long long s2s_dtw_ring[];     // [3][W] int64, then the two sample windows [2][2 R + S2S_DTW_WINDOW] int16
    const int p = blockIdx.x;
    const long long ao = a_offs[p], bo = b_offs[p];
    const long long n64 = a_offs[p + 1] - ao, m64 = b_offs[p + 1] - bo;
    if (n64 <= 0 || m64 <= 0 || n64 > S2S_DTW_MAX_SAMPLES || m64 > S2S_DTW_MAX_SAMPLES) {
        if (threadIdx.x == 0) cost[p] = (n64 > S2S_DTW_MAX_SAMPLES || m64 > S2S_DTW_MAX_SAMPLES) ? S2S_DTW_COST_TOO_LONG : S2S_DTW_COST_EMPTY;
        return;
    }
    const int n = (int)n64, m = (int)m64, nm = n + m;
    const int W = 2 * R + 2;
    const int16_t* pa = a + ao;
    const int16_t* pb = b + bo;
    const long long T = (long long)R * (n > m ? n : m);
    // floor(T / nm) and ceil(-T / nm) = floor((-T + nm - 1) / nm): |quotient| <= R + 1
    int qh = (int)(T / nm), rh = (int)(T - (long long)qh * nm);
    const long long numl = nm - 1 - T;
    long long ql64 = numl / nm;
    if (numl - ql64 * nm < 0) ql64 -= 1;
    int ql = (int)ql64, rl = (int)(numl - ql64 * nm);
    int oc = 0, o1 = W, o2 = 2 * W;                 // ring of diagonal d, d - 1, d - 2
    int lo1 = 0, lo2 = 0;                           // the row ranges of the last two diagonals: first row and
    unsigned cnt1 = 0, cnt2 = 0;                    // number of rows (0 in front of the first diagonal)
    int slo = 0;                                    // lo(d) mod W
    const int last = nm - 2;
    const int win = 2 * R + S2S_DTW_WINDOW;
    int16_t* wa = reinterpret_cast<int16_t*>(s2s_dtw_ring + 3 * W);
    int16_t* wb = wa + win;
    int a0 = 0, b0 = 0;                             // first row / column of the windows
    int chunks = 0;                                 // (PATH) word pairs per diagonal, and the pair's slot (nullptr: record nothing)
    ulonglong2* dec = nullptr;
    if constexpr (PATH) {
        chunks = s2s_dtw_path_chunks(n, m, R);
        const long long so = scratch_offs[p], sz = scratch_offs[p + 1] - so;
        if (so >= 0 && (so & 15) == 0 && sz >= (long long)(nm - 1) * chunks * 16) dec = reinterpret_cast<ulonglong2*>(scratch + so);
    }
    for (int d = 0; d <= last; ++d) {
        int lo = d - (m - 1);
        lo = lo < 0 ? 0 : lo;
        lo = lo < ql ? ql : lo;
        int hi = d < n - 1 ? d : n - 1;
        hi = hi > qh ? qh : hi;
        hi = hi > lo + 2 * R ? lo + 2 * R : hi;      // (never binds: hi - lo <= 2 T / nm < 2 R; keeps every slot inside the ring whatever happens)
        if constexpr (PATH) hi = hi > lo + 64 * chunks - 1 ? lo + 64 * chunks - 1 : hi;   // (never binds either: keeps every store inside the slot)
        slo += lo - lo1;                            // lo never decreases and grows by at most 1
        while (slo >= W) slo -= W;
        if ((d & (S2S_DTW_WINDOW - 1)) == 0) {      // (uniform: d is) the samples of the next S2S_DTW_WINDOW diagonals, once
            a0 = lo;
            b0 = d - hi;
            for (int t = threadIdx.x; t < win; t += (int)blockDim.x) {
                wa[t] = a0 + t < n ? pa[a0 + t] : (int16_t)0;
                wb[t] = b0 + t < m ? pb[b0 + t] : (int16_t)0;
            }
            __syncthreads();
        }
        // S2S_DTW_CELLS cells per thread and step while that many strides fit: all their LDS reads first (no branch in between, so they
        // issue back to back), then the stores; the rest of the diagonal one cell per thread and step.  The three predecessors are
        // read whatever they hold (every slot lies inside the ring) and chosen by their row ranges.
        const long long first = d == 0 ? 0 : S2S_DTW_UNREACHED;
        auto cell = [&](int i, int& slot, unsigned& code) -> long long {
            int s = slo + (i - lo);
            s = s >= W ? s - W : s;
            const int sm = s == 0 ? W - 1 : s - 1;       // slot of row i - 1
            const int xa = wa[i - a0], xb = wb[d - i - b0];
            const int c = xa < xb ? xb - xa : xa - xb;
            const long long up = s2s_dtw_ring[o1 + sm], left = s2s_dtw_ring[o1 + s], diag = s2s_dtw_ring[o2 + sm];
            const bool has_up = (unsigned)(i - 1 - lo1) < cnt1;         // (i - 1, j)
            const bool has_left = (unsigned)(i - lo1) < cnt1;           // (i, j - 1)
            const bool has_diag = (unsigned)(i - 1 - lo2) < cnt2;       // (i - 1, j - 1)
            slot = s;
            if constexpr (PATH) {                   // the tie rule of the path: diagonal, then up, then left ('<' keeps the earlier one)
                long long best = S2S_DTW_UNREACHED;
                code = S2S_DTW_OP_NONE;
                if (has_diag && diag < best) { best = diag; code = S2S_DTW_OP_M; }
                if (has_up && up < best) { best = up; code = S2S_DTW_OP_A; }
                if (has_left && left < best) { best = left; code = S2S_DTW_OP_B; }
                best = d == 0 ? 0 : best;           // (0, 0) has no predecessor: NONE
                return best >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : best + c;
            }
            long long best = first;
            best = has_up && up < best ? up : best;
            best = has_left && left < best ? left : best;
            best = has_diag && diag < best ? diag : best;
            return best >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : best + c;
        };
        const int bd = (int)blockDim.x;
        if constexpr (PATH) {
            const int lane = (int)threadIdx.x & 63;
            for (int base = lo + (int)threadIdx.x - lane; base <= hi; base += S2S_DTW_CELLS * bd) {      // (base: the same for a wave's lanes)
                long long v[S2S_DTW_CELLS];
                int slot[S2S_DTW_CELLS];
                unsigned code[S2S_DTW_CELLS];
#pragma unroll
                for (int u = 0; u < S2S_DTW_CELLS; ++u) {
                    const int i = base + u * bd + lane;
                    v[u] = cell(i <= hi ? i : hi, slot[u], code[u]);
                    code[u] = i <= hi ? code[u] : (unsigned)S2S_DTW_OP_NONE;
                }
#pragma unroll
                for (int u = 0; u < S2S_DTW_CELLS; ++u)
                    if (base + u * bd + lane <= hi) s2s_dtw_ring[oc + slot[u]] = v[u];
#pragma unroll
                for (int u = 0; u < S2S_DTW_CELLS; ++u) {
                    if (base + u * bd <= hi) {
                        const unsigned long long b0 = __ballot(code[u] & 1u), b1 = __ballot(code[u] & 2u);
                        if (lane == 0 && dec) dec[(long long)d * chunks + ((base + u * bd - lo) >> 6)] = make_ulonglong2(b0, b1);
                    }
                }
            }
        } else {
            int i0 = lo + (int)threadIdx.x;
            for (; i0 + (S2S_DTW_CELLS - 1) * bd <= hi; i0 += S2S_DTW_CELLS * bd) {
                long long v[S2S_DTW_CELLS];
                int slot[S2S_DTW_CELLS];
                unsigned code;
#pragma unroll
                for (int u = 0; u < S2S_DTW_CELLS; ++u) v[u] = cell(i0 + u * bd, slot[u], code);
#pragma unroll
                for (int u = 0; u < S2S_DTW_CELLS; ++u) s2s_dtw_ring[oc + slot[u]] = v[u];
            }
            for (; i0 <= hi; i0 += bd) {
                int slot;
                unsigned code;
                const long long v = cell(i0, slot, code);
                s2s_dtw_ring[oc + slot] = v;
            }
        }
        __syncthreads();
        const int o = o2; o2 = o1; o1 = oc; oc = o;
        lo2 = lo1; cnt2 = cnt1; lo1 = lo; cnt1 = hi < lo ? 0u : (unsigned)(hi - lo + 1);
        rh += n; if (rh >= nm) { rh -= nm; qh += 1; }
        rl += n; if (rl >= nm) { rl -= nm; ql += 1; }
    }
    // D(n - 1, m - 1) sits on the last diagonal (now o1), row n - 1 (inside its range: the corner is always in the band)
    if (threadIdx.x == 0) {
        int s = slo + (n - 1 - lo1);
        s = s >= W ? s - W : s;
        cost[p] = (unsigned)(n - 1 - lo1) < cnt1 ? s2s_dtw_ring[o1 + s] : S2S_DTW_UNREACHED;
    }
}

// The walk back through the decisions of s2s_dtw_kernel<true>: one wave per pair, from (n - 1, m - 1) on diagonal n + m - 2.  Every
// lane runs the same walk on the same values (the loads are wave-uniform); lane k mod 64 keeps the k-th op and the wave stores 64
// of them at a time, right-aligned in the pair's slot of `ops`: the k-th op of the walk is byte path_offs[p + 1] - 1 - k.  lo(d) is
// carried downwards the way the sweep carries it upwards (one 64-bit division in front of the loop).  The walk ends at (0, 0), on
// a NONE code, on a step that would leave the matrix, or after n + m - 2 steps, and the cell index is clamped to the diagonal's
// words: whatever the scratch holds, the loop is bounded and every address lies inside the pair's slots.  steps[p] = the ops
// written if the walk arrived at (0, 0), else 0 (also for a pair without cost, or whose slots are too small).
__global__ __launch_bounds__(64) void s2s_dtw_trace_kernel(const long long* __restrict__ a_offs, const long long* __restrict__ b_offs, int R,
                                                           const long long* __restrict__ cost, const unsigned char* __restrict__ scratch,
                                                           const long long* __restrict__ scratch_offs, unsigned char* __restrict__ ops,
                                                           const long long* __restrict__ path_offs, long long* __restrict__ steps) {
    const int p = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const long long n64 = a_offs[p + 1] - a_offs[p], m64 = b_offs[p + 1] - b_offs[p];
    const long long so = scratch_offs[p], sz = scratch_offs[p + 1] - so;
    const long long pend = path_offs[p + 1], cap = pend - path_offs[p];
    const long long c = cost[p];
    bool ok = n64 > 0 && m64 > 0 && n64 <= S2S_DTW_MAX_SAMPLES && m64 <= S2S_DTW_MAX_SAMPLES && c >= 0 && c < S2S_DTW_UNREACHED;
    const int n = ok ? (int)n64 : 1, m = ok ? (int)m64 : 1, nm = n + m;
    const int chunks = s2s_dtw_path_chunks(n, m, R);
    const int bound = nm - 2;
    ok = ok && so >= 0 && (so & 15) == 0 && sz >= (long long)(nm - 1) * chunks * 16 && path_offs[p] >= 0 && cap >= bound;
    if (!ok) {
        if (lane == 0) steps[p] = 0;
        return;
    }
    const ulonglong2* dec = reinterpret_cast<const ulonglong2*>(scratch + so);
    const long long T = (long long)R * (n > m ? n : m);
    int i = n - 1, j = m - 1, d = nm - 2;
    const long long numl = nm - 1 - T + (long long)d * n;        // ceil((d n - T) / nm) = floor(numl / nm)
    long long ql64 = numl / nm;
    if (numl - ql64 * nm < 0) ql64 -= 1;
    int ql = (int)ql64, rl = (int)(numl - ql64 * nm);
    int k = 0;
    unsigned mine = 0;
    while ((i | j) != 0 && k < bound) {
        int lo = d - (m - 1);
        lo = lo < 0 ? 0 : lo;
        lo = lo < ql ? ql : lo;
        int x = i - lo;
        x = x < 0 ? 0 : x > 64 * chunks - 1 ? 64 * chunks - 1 : x;
        const ulonglong2 w = dec[(long long)d * chunks + (x >> 6)];
        const unsigned code = (unsigned)((w.x >> (x & 63)) & 1ull) | ((unsigned)((w.y >> (x & 63)) & 1ull) << 1);
        const int di = code != S2S_DTW_OP_B, dj = code != S2S_DTW_OP_A;
        if (code == S2S_DTW_OP_NONE || i < di || j < dj) break;
        mine = (k & 63) == lane ? code : mine;
        ++k;
        if ((k & 63) == 0) ops[pend - 1 - (k - 64 + lane)] = (unsigned char)mine;
        i -= di;
        j -= dj;
        for (int s = di + dj; s > 0; --s) {          // one or two diagonals down
            --d;
            rl -= n; if (rl < 0) { rl += nm; ql -= 1; }
        }
    }
    if (lane < (k & 63)) ops[pend - 1 - ((k & ~63) + lane)] = (unsigned char)mine;
    if (lane == 0) steps[p] = (i | j) == 0 ? k : 0;
}
#endif  // S2S_DTW_KERNELS
