// `eventalign`: the means of detected events aligned to the levels of a read's k-mers inside a narrow band that follows the path
// (include/s2s_hip.h states the definitions next to s2s_event_means and s2s_eventalign), in integers only.  Band b holds the W cells
// of anti-diagonal e + j = b from k-mer lk(b) on; a band moves right or down by comparing the costs at its two ends, so a cell's
// three predecessors sit at one offset for the whole workgroup.  The layout of the decision scratch and the rounding of a mean are
// one set of functions for the kernels, the host entries and the host twins (s2s_host.cpp); the kernels follow under S2S_DTW_KERNELS.
#pragma once
#include <stdint.h>

#include "../../include/s2s_hip.h"
#include "s2s_dtw.h"

#define S2S_EVA_DIAG 0                              // from (e - 1, j - 1): event e opens k-mer j
#define S2S_EVA_STAY 1                              // from (e - 1, j): one more event of k-mer j
#define S2S_EVA_SKIP 2                              // from (e, j - 1): k-mer j gets no event from this move
#define S2S_EVA_START 3                             // the path begins here (j = 0); also the code of an unreached cell, which no walk visits

S2S_DTW_HD constexpr bool s2s_eva_params_ok(int32_t W, int32_t skip, int32_t trim, int32_t unknown) {
    return W >= 64 && W <= S2S_EVA_MAX_WIDTH && W % 64 == 0 && skip >= 0 && skip <= S2S_RSQ_MAX_SKIP_PENALTY && trim >= 0 &&
           trim <= S2S_EVA_MAX_TRIM_PENALTY && unknown >= 0 && unknown <= S2S_RSQ_MAX_UNKNOWN_COST;
}
S2S_DTW_HD inline bool s2s_eva_solvable(int64_t E, int64_t K) { return E >= 1 && K >= 1 && E <= S2S_DTW_MAX_SAMPLES && K <= S2S_DTW_MAX_SAMPLES; }
// The decision scratch of a read: E + K - 1 bands of W / 64 16-byte word pairs (bit 0 of the 64 codes, then bit 1; cell o of band b is
// bit o mod 64 of pair b W / 64 + o / 64), then one int32 lk per band; the whole rounded up to 16 bytes.
S2S_DTW_HD inline int64_t s2s_eva_dec_bytes(int64_t E, int64_t K, int64_t W) { return (E + K - 1) * (W / 64) * 16; }
S2S_DTW_HD inline int64_t s2s_eva_bytes(int64_t E, int64_t K, int64_t W) {
    return s2s_eva_solvable(E, K) ? (s2s_eva_dec_bytes(E, K, W) + (E + K - 1) * 4 + 15) / 16 * 16 : 0;
}

// x = round-half-even(S / n) clamped to int16; 0 for n < 1.
S2S_DTW_HD inline int16_t s2s_eva_mean(int64_t S, int64_t n) {
    if (n < 1) return 0;
    int64_t q = S / n, r = S - q * n;                // (C++ truncates towards zero)
    if (r < 0) { q -= 1; r += n; }
    if (2 * r > n || (2 * r == n && (q & 1))) q += 1;
    return (int16_t)(q < -32768 ? -32768 : q > 32767 ? 32767 : q);
}
// The means a record contributes: its n_events when they are positive and fit its slot, else none.
S2S_DTW_HD inline int64_t s2s_eva_count(int64_t n_events, int64_t eo, int64_t eo_next) {
    return n_events > 0 && eo >= 0 && n_events <= eo_next - eo ? n_events : 0;
}

#if defined(S2S_DTW_KERNELS)
#include <hip/hip_runtime.h>

#define S2S_EVA_REFILL 256                          // bands per refill of the two staged windows (a power of two)
#define S2S_EVA_LDS_BYTES(W) (3 * ((size_t)(W) + 2) * 8 + 2 * ((size_t)(W) + S2S_EVA_REFILL) * 2)

// Launch 1 of s2s_event_means is s2s_scan_kernel<1, S2SEvaCounts> (s2s_prims.h): m_offs[r] = the means of the records before r,
// m_offs[R] = all.
struct S2SEvaCounts {
    const int* n_events;
    const long long* ev_offs;
    __device__ long long operator()(long long r) const { return s2s_eva_count(n_events[r], ev_offs[r], ev_offs[r + 1]); }
};

// Launch 2: the means of record blockIdx.x, its events strided over the workgroups of blockIdx.y.  A record whose means would end
// beyond `capacity` writes none.
#define S2S_EVA_MEAN_SLICES 8
__global__ __launch_bounds__(256) void s2s_event_means_fill_kernel(const long long* __restrict__ S, const int* __restrict__ ev_len,
                                                                    const long long* __restrict__ ev_offs, const int* __restrict__ n_events,
                                                                    long long capacity, const long long* __restrict__ m_offs,
                                                                    int16_t* __restrict__ means) {
    const int r = blockIdx.x;
    const long long eo = ev_offs[r], cnt = s2s_eva_count(n_events[r], eo, ev_offs[r + 1]), mo = m_offs[r];
    if (mo < 0 || mo + cnt > capacity) return;
    for (long long e = (long long)blockIdx.y * 256 + threadIdx.x; e < cnt; e += 256LL * S2S_EVA_MEAN_SLICES)
        means[mo + e] = s2s_eva_mean(S[eo + e], ev_len[eo + e]);
}

// One workgroup of W threads per read; bands b = 0 .. E + K - 2, one barrier each.  Thread o owns cell o of every band: k-mer
// j = lk(b) + o, event e = b - j.  D of the last three bands lives in LDS, each band W + 2 int64 with an `unreached` sentinel at
// either end, so a predecessor beyond the band's ends is read like any other; a cell outside the matrix is written as unreached.
// After the barrier of band b - 1 every thread reads that band's two end cells and forms the same r_b (right: 1, down: 0); then
//   stay is cell o + r_b of band b - 1, skip cell o + r_b - 1 of band b - 1, diag cell o + r_b + r_(b-1) - 1 of band b - 2.
// A thread keeps its own m[e] and l[j] in registers; per band exactly one of e and j grows by one and only that one is read again,
// from two windows in LDS that are refilled every S2S_EVA_REFILL bands: in 256 bands lk and b - lk each grow by at most 255, so the
// k-mers lk0 .. lk0 + W + 254 and the events e0 .. e0 + W + 254 (e0 = b0 - lk0 - W + 1) cover them.  Per wave and band: two ballots; lane
// b mod 64 keeps the two words and lk(b), and after every 64th band (and the last) each lane stores the 16 bytes of its band and wave
// 0 the lk -- no barrier waits for a store of its own band (measured against a store per band: 3 % of the call at W = 128; the band's
// chain of LDS reads is what a band costs).  Both go only into a slot of `scratch` that is aligned and large enough (s2s_eva_bytes).  A thread keeps the best D(e, K - 1) + (E - 1 - e) trim of its own cells (its e ascend with b, so
// '<' keeps the smallest); one reduction over (value, e) at the end.  E, K, W and the loop counters are the only inputs of every
// branch around a barrier.  The winner's e + 1 goes to end_event for the walk back.  LDS: S2S_EVA_LDS_BYTES(W) = 3 (W + 2) 8 +
// 2 (W + 256) 2: 29,744 B at W = 1024, 4,656 B at W = 128.
__global__ __launch_bounds__(S2S_EVA_MAX_WIDTH) void s2s_eventalign_kernel(
    const int16_t* __restrict__ m, const long long* __restrict__ m_offs, const int16_t* __restrict__ l, const long long* __restrict__ l_offs,
    int W, int skip_penalty, int trim_penalty, int unknown_cost, long long* __restrict__ cost, unsigned char* __restrict__ scratch,
    const long long* __restrict__ scratch_offs, int* __restrict__ end_event) {
    extern __shared__ long long s2s_eva_lds[];      // [3][W + 2] int64, then the windows of l and of m, [W + 256] int16 each
    const int p = blockIdx.x;
    const long long mo = m_offs[p], lo_ = l_offs[p];
    const long long E64 = m_offs[p + 1] - mo, K64 = l_offs[p + 1] - lo_;
    if (!s2s_eva_solvable(E64, K64) || mo < 0 || lo_ < 0) {     // (uniform over the workgroup: before any barrier)
        if (threadIdx.x == 0)
            cost[p] = (E64 > S2S_DTW_MAX_SAMPLES || K64 > S2S_DTW_MAX_SAMPLES) ? S2S_DTW_COST_TOO_LONG : S2S_DTW_COST_EMPTY;
        return;
    }
    const int E = (int)E64, K = (int)K64;
    const int o = (int)threadIdx.x, lane = o & 63, wave = o >> 6, chunks = W >> 6;
    const int stride = W + 2, win = W + S2S_EVA_REFILL;
    const int16_t* pm = m + mo;
    const int16_t* pl = l + lo_;
    int16_t* wl = reinterpret_cast<int16_t*>(s2s_eva_lds + 3 * stride);
    int16_t* wm = wl + win;
    const int bands = E + K - 1;
    ulonglong2* dec = nullptr;
    int* lks = nullptr;
    {
        const long long so = scratch_offs[p], sz = scratch_offs[p + 1] - so;
        if (so >= 0 && (so & 15) == 0 && sz >= s2s_eva_bytes(E, K, W)) {
            dec = reinterpret_cast<ulonglong2*>(scratch + so);
            lks = reinterpret_cast<int*>(scratch + so + s2s_eva_dec_bytes(E, K, W));
        }
    }
    for (int t = o; t < 3 * stride; t += W) s2s_eva_lds[t] = S2S_DTW_UNREACHED;      // the sentinels, and no band before band 0
    int lk = -(W >> 1), r1 = 0;                     // lk(b), r_(b-1)
    int lk0 = 0, e0 = 0;                            // the windows' first k-mer and first event
    int xm = 0, xl = 0;
    long long best = S2S_DTW_UNREACHED;
    int best_e = 0;
    unsigned long long k0 = 0, k1 = 0;              // the decisions and lk of band (b & ~63) + lane, until they are stored
    int klk = 0;
    int cur = 0, b1 = 2, b2 = 1;                   // which of the three arrays holds band b, b - 1, b - 2
    __syncthreads();
    for (int b = 0; b < bands; ++b) {
        int r = 0;
        if (b > 0) {
            const long long ll = s2s_eva_lds[b1 * stride + 1], ur = s2s_eva_lds[b1 * stride + W];
            r = (ll >= S2S_DTW_UNREACHED && ur >= S2S_DTW_UNREACHED) ? (b & 1) : (ll > ur ? 1 : 0);
        }
        lk += r;
        const int j = lk + o, e = b - j;
        if ((b & (S2S_EVA_REFILL - 1)) == 0) {      // (uniform: b is)
            lk0 = lk;
            e0 = b - lk - (W - 1);
            for (int t = o; t < win; t += W) {
                const int jj = lk0 + t, ee = e0 + t;
                wl[t] = jj >= 0 && jj < K ? pl[jj] : (int16_t)0;
                wm[t] = ee >= 0 && ee < E ? pm[ee] : (int16_t)0;
            }
            __syncthreads();
            xl = wl[j - lk0];
            xm = wm[e - e0];
        } else if (r) {
            xl = wl[j - lk0];
        } else {
            xm = wm[e - e0];
        }
        const long long pstay = s2s_eva_lds[b1 * stride + 1 + o + r], pskip = s2s_eva_lds[b1 * stride + o + r],
                        pdiag = s2s_eva_lds[b2 * stride + o + r + r1];
        const int dx = xm - xl;
        const long long c = xl == S2S_RSQ_UNKNOWN ? unknown_cost : (dx < 0 ? -dx : dx);
        long long v = S2S_DTW_UNREACHED;
        unsigned code = S2S_EVA_START;              // the tie rule: diag, stay, skip, start ('<' keeps the earlier one)
        if (j >= 1 && pdiag < v) { v = pdiag + c; code = S2S_EVA_DIAG; }
        const long long ts = pstay >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : pstay + c;
        if (ts < v) { v = ts; code = S2S_EVA_STAY; }
        const long long tk = pskip >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : pskip + skip_penalty;
        if (j >= 1 && tk < v) { v = tk; code = S2S_EVA_SKIP; }
        const long long t0 = (long long)e * trim_penalty + c;
        if (j == 0 && t0 < v) { v = t0; code = S2S_EVA_START; }
        const bool inside = j >= 0 && j < K && e >= 0 && e < E;
        v = inside ? v : S2S_DTW_UNREACHED;
        code = v < S2S_DTW_UNREACHED ? code : (unsigned)S2S_EVA_START;
        s2s_eva_lds[cur * stride + 1 + o] = v;
        if (j == K - 1 && v < S2S_DTW_UNREACHED) {
            const long long f = v + (long long)(E - 1 - e) * trim_penalty;
            if (f < best) { best = f; best_e = e; }
        }
        const unsigned long long w0 = __ballot(code & 1u), w1 = __ballot(code & 2u);
        if (lane == (b & 63)) { k0 = w0; k1 = w1; klk = lk; }
        if ((b & 63) == 63 || b == bands - 1) {     // (uniform) the wave's last up to 64 bands go out together
            const int bb = (b & ~63) + lane;
            if (dec && bb <= b) {
                dec[(long long)bb * chunks + wave] = make_ulonglong2(k0, k1);
                if (wave == 0) lks[bb] = klk;
            }
        }
        __syncthreads();
        r1 = r;
        const int t = b2;
        b2 = b1; b1 = cur; cur = t;
    }
    // (value, e) of every thread -> the smallest value, on equal values the smallest e: inside the wave by shuffles, then over the waves
    for (int d = 32; d >= 1; d >>= 1) {
        const long long ov = __shfl_xor(best, d);
        const int oe = __shfl_xor(best_e, d);
        if (ov < best || (ov == best && oe < best_e)) { best = ov; best_e = oe; }
    }
    int* wes = reinterpret_cast<int*>(s2s_eva_lds + 16);        // (the loop's last barrier is behind every read of the bands)
    if (lane == 0) { s2s_eva_lds[wave] = best; wes[wave] = best_e; }
    __syncthreads();
    if (o == 0) {
        for (int q = 1; q < chunks; ++q) {
            const long long ov = s2s_eva_lds[q];
            const int oe = wes[q];
            if (ov < best || (ov == best && oe < best_e)) { best = ov; best_e = oe; }
        }
        const bool solved = best < S2S_DTW_UNREACHED;
        cost[p] = solved ? best : (long long)S2S_RSQ_UNREACHED;
        end_event[p] = solved ? best_e + 1 : 0;
    }
}

// The walk back through the decisions of s2s_eventalign_kernel: one wave per read, from (end_event - 1, K - 1) until a start.  Every
// lane runs the same walk on the same values (the loads are wave-uniform); lane 0 stores.  The wave first writes "no path" to a read
// that is not too long: kmer -1 for its E events, -1 / 0 / 0 for its K k-mers, first_event = end_event = 0 -- what an unsolved read
// and a read whose slot of scratch is too small or misaligned, or whose slot of events is smaller than E, keep.  Every step lowers
// e or j, so the walk takes at most E + K steps whatever the scratch holds; a cell index outside the band, a move out of the matrix,
// a skip into a k-mer that already has events or a start off k-mer 0 (no sweep writes such decisions) end it, and a walk that did
// not arrive takes its stores back.
__global__ __launch_bounds__(64) void s2s_eventalign_trace_kernel(
    const long long* __restrict__ m_offs, const long long* __restrict__ l_offs, const int* __restrict__ ev_start,
    const int* __restrict__ ev_len, const long long* __restrict__ ev_offs, int W, const long long* __restrict__ cost,
    const unsigned char* __restrict__ scratch, const long long* __restrict__ scratch_offs, int* __restrict__ first_event,
    int* __restrict__ end_event, int* __restrict__ ev_kmer, int* __restrict__ k_start, int* __restrict__ k_len, int* __restrict__ k_events) {
    const int p = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const long long mo = m_offs[p], lo_ = l_offs[p];
    const long long E64 = m_offs[p + 1] - mo, K64 = l_offs[p + 1] - lo_;
    if (mo < 0 || lo_ < 0 || E64 < 0 || K64 < 0 || E64 > S2S_DTW_MAX_SAMPLES || K64 > S2S_DTW_MAX_SAMPLES) return;
    const int E = (int)E64, K = (int)K64;
    const int end = end_event[p];                   // (the sweep's, read before it is reset)
    int* km = ev_kmer + mo;
    int* ks = k_start + lo_;
    int* kl = k_len + lo_;
    int* ke = k_events + lo_;
    auto clear = [&]() {
        for (int t = lane; t < E; t += 64) km[t] = -1;
        for (int t = lane; t < K; t += 64) { ks[t] = -1; kl[t] = 0; ke[t] = 0; }
        if (lane == 0) { first_event[p] = 0; end_event[p] = 0; }
    };
    clear();
    const long long so = scratch_offs[p], sz = scratch_offs[p + 1] - so, eo = ev_offs[p];
    if (!s2s_eva_solvable(E64, K64) || cost[p] < 0 || so < 0 || (so & 15) != 0 || sz < s2s_eva_bytes(E, K, W) || eo < 0 ||
        ev_offs[p + 1] - eo < E || end < 1 || end > E)
        return;
    __threadfence();                                // the fill is complete before lane 0 stores into it
    const int chunks = W >> 6;
    const ulonglong2* dec = reinterpret_cast<const ulonglong2*>(scratch + so);
    const int* lks = reinterpret_cast<const int*>(scratch + so + s2s_eva_dec_bytes(E, K, W));
    const int* st = ev_start + eo;
    const int* ln = ev_len + eo;
    int e = end - 1, j = K - 1, run = 0, hi = 0;
    bool arrived = false;
    for (int step = 0; step < E + K; ++step) {
        const int b = e + j;
        const long long oo = (long long)j - lks[b];
        if (oo < 0 || oo >= W) break;
        const int o = (int)oo;
        const ulonglong2 w = dec[(long long)b * chunks + (o >> 6)];
        const unsigned code = (unsigned)((w.x >> (o & 63)) & 1ull) | ((unsigned)((w.y >> (o & 63)) & 1ull) << 1);
        if (code == S2S_EVA_SKIP) {
            if (run != 0 || j == 0) break;
            --j;
            continue;
        }
        if (lane == 0) km[e] = j;
        if (run == 0) hi = e;
        ++run;
        if (code == S2S_EVA_STAY) {
            if (e == 0) break;
            --e;
            continue;
        }
        if (lane == 0) { ks[j] = st[e]; kl[j] = st[hi] + ln[hi] - st[e]; ke[j] = run; }
        run = 0;
        if (code == S2S_EVA_START) {
            arrived = j == 0;
            break;
        }
        if (e == 0 || j == 0) break;
        --e;
        --j;
    }
    if (arrived) {
        if (lane == 0) { first_event[p] = e; end_event[p] = end; }
    } else {
        __threadfence();
        clear();
    }
}
#endif  // S2S_DTW_KERNELS
