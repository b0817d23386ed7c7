// The pore model from alignments (`resquiggle / eventalign --kmer-model-out`; include/s2s_hip.h states the definition next to
// s2s_kmer_model_events): the k-mer slots (ev_len, S, Q) a batch's last s2s_event_sums left, each converted to the fixed-point event
// of s2s_event_fixed and from there to 2^-8 pA by its own record's calibration, summed per k-mer into the table s2s_kmer_model_format
// prints.  Three parts: the conversion and the rule of one slot, one set of functions for the kernel, the host entry and the host
// twin (s2s_host.cpp); the workgroup's write-combining cache, by the rules of s2s_kmer_model_kernel (s2s_hip.hip); the kernel.
#pragma once
#include <stdint.h>

#include "../../include/s2s_hip.h"
#include "s2s_event_fixed.h"

#define S2S_KME_MAX_LEN 1024                        // the longest event s2s_event_fixed is defined for
#define S2S_KME_GAIN_ONE ((int64_t)1 << 24)         // gain is range / digitisation in units of 2^-24
#define S2S_KME_LIMIT ((int64_t)1 << 23)            // |Mp|, Dp: squares <= 2^46, the exactness statement of the table

// (M, D) in 2^-8 ADC counts -> (Mp, Dp) in 2^-8 pA; false: out of range.  1 <= gain <= 2^30, |shift| <= 2^30, |M|, D <= 2^23: the
// products stay below 2^62.  (They are formed unsigned: arguments outside the contract give some number, not undefined behaviour.)
S2S_FIXED_HD inline bool s2s_event_fixed_pa(int64_t M, int64_t D, int64_t gain, int64_t shift, int64_t& Mp, int64_t& Dp) {
    // Mp = round-half-even((M + shift) * gain / 2^24): floor division, then the remainder decides
    const int64_t num = (int64_t)((uint64_t)(M + shift) * (uint64_t)gain);
    int64_t q = num / S2S_KME_GAIN_ONE, r = num - q * S2S_KME_GAIN_ONE;      // (C++ truncates towards zero)
    if (r < 0) { q -= 1; r += S2S_KME_GAIN_ONE; }
    if (2 * r > S2S_KME_GAIN_ONE || (2 * r == S2S_KME_GAIN_ONE && (q & 1))) q += 1;
    Mp = q;
    Dp = (int64_t)(((uint64_t)D * (uint64_t)gain) >> 24);                    // D >= 0: the shift is the floor
    return Mp >= -S2S_KME_LIMIT && Mp <= S2S_KME_LIMIT && Dp >= 0 && Dp <= S2S_KME_LIMIT;
}

// One slot of a record with gain != 0 -> what it is: nothing, one of the three drops, or an event with its (Mp, Dp).
enum { S2S_KME_NONE = 0, S2S_KME_OVERLONG = 1, S2S_KME_OUT_OF_RANGE = 2, S2S_KME_BAD_CODE = 3, S2S_KME_EVENT = 4 };
S2S_FIXED_HD inline int s2s_kme_slot(int32_t n, int64_t S, int64_t Q, int32_t code, int32_t rows, int64_t gain, int64_t shift, int64_t& Mp,
                                     int64_t& Dp) {
    if (n < 1) return S2S_KME_NONE;
    if (n > S2S_KME_MAX_LEN) return S2S_KME_OVERLONG;
    if (code < 0 || code >= rows) return S2S_KME_BAD_CODE;                  // rows = 4^k + 1: the pooled row 4^k is a row
    int64_t M, D;
    s2s_event_fixed_point(n, (int32_t)S, Q, M, D);
    return s2s_event_fixed_pa(M, D, gain, shift, Mp, Dp) ? S2S_KME_EVENT : S2S_KME_OUT_OF_RANGE;
}

#if defined(S2S_DTW_KERNELS)
#include <hip/hip_runtime.h>

#include "s2s_prims.h"

// ---- the write-combining cache of a workgroup: S2S_KMER_MODEL_SLOTS slots, each a key (the code, or EMPTY) and five counters
// (field-major: one bank pattern per field) -- the constants and the rules of s2s_kmer_model_kernel, which s2s_hip.hip states above
// it.  This kernel's own copy of the insertion and the flush: calling one pair from both kernels changed the register count of
// s2s_kmer_model_kernel<0> (68 -> 70 VGPRs), so that kernel stays as it was.
#define S2S_KME_EMPTY (-1)
#define S2S_KME_LDS_BYTES (S2S_KMER_MODEL_SLOTS * 4 + S2S_KMER_MODEL_FIELDS * S2S_KMER_MODEL_SLOTS * 8)
static_assert(S2S_KME_LDS_BYTES == 45100, "include/s2s_hip.h states the LDS bytes of s2s_kmer_model_events");

__device__ __forceinline__ void s2s_kme_flush(int* keys, unsigned long long (*cnt)[S2S_KMER_MODEL_SLOTS],
                                                     unsigned long long* __restrict__ table) {
    for (int i = threadIdx.x; i < S2S_KMER_MODEL_SLOTS; i += 256) {
        const int key = keys[i];
        if (key == S2S_KME_EMPTY) continue;
        unsigned long long* row = table + (size_t)key * S2S_KMER_MODEL_FIELDS;
#pragma unroll
        for (int f = 0; f < S2S_KMER_MODEL_FIELDS; ++f) {
            const unsigned long long v = cnt[f][i];
            if (v) __hip_atomic_fetch_add(row + f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cnt[f][i] = 0ull;
        }
        keys[i] = S2S_KME_EMPTY;
    }
}

// The five sums f of `code` (0 <= code <= 4^k) into the cache, or past it into the table when S2S_KMER_MODEL_PROBES slots are held
// by other codes.
__device__ __forceinline__ void s2s_kme_insert(int* keys, unsigned long long (*cnt)[S2S_KMER_MODEL_SLOTS],
                                                      unsigned long long* __restrict__ table, bool direct, int code,
                                                      const unsigned long long (&f)[S2S_KMER_MODEL_FIELDS]) {
    unsigned slot = direct ? (unsigned)code
                           : (unsigned)(((unsigned long long)((unsigned)code * S2S_KMER_MODEL_HASH_MUL) * S2S_KMER_MODEL_SLOTS) >> 32);
    bool placed = false;
#pragma unroll
    for (int probe = 0; probe < S2S_KMER_MODEL_PROBES; ++probe) {
        if (!placed) {
            const int old = atomicCAS(&keys[slot], S2S_KME_EMPTY, code);
            if (old == S2S_KME_EMPTY || old == code) placed = true;
            else slot = slot + 1 == S2S_KMER_MODEL_SLOTS ? 0u : slot + 1;
        }
    }
    if (placed) {
#pragma unroll
        for (int i = 0; i < S2S_KMER_MODEL_FIELDS; ++i)
            atomicAdd(&cnt[i][slot], f[i]);
    } else {
        unsigned long long* row = table + (size_t)code * S2S_KMER_MODEL_FIELDS;
#pragma unroll
        for (int i = 0; i < S2S_KMER_MODEL_FIELDS; ++i)
            if (f[i]) __hip_atomic_fetch_add(row + i, f[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the kernel.  Persistent workgroups of four waves walk the POOLED slots, 256 per round and 64 consecutive ones per wave, so a
// lone long read runs at the rate of many short ones.  A lane finds its record by a search in l_offs (any content of l_offs is safe:
// a slot that no record holds adds nothing), takes that record's gain and shift, and classifies its slot (s2s_kme_slot).  Lanes of a
// wave with equal codes -- neighbours, in a homopolymer or a repeat -- are merged by ballots and shuffles, and the first lane of every
// code inserts into the cache.  The cache is flushed every S2S_KMER_MODEL_FLUSH_ROUNDS rounds and after the walk; whether a round
// flushes depends on the round number, the grid and the slot count alone: uniform over the workgroup, with a barrier before and
// after.  The three drop counts and `counted` are ballots summed in a register of the wave: one atomic per wave and non-zero counter.
// Static LDS: the cache, S2S_KME_LDS_BYTES = 45,100 B (three workgroups per CU); the counts need none.
struct S2SKmeIn {
    const int* codes;
    const int* ev_len;
    const long long* S;
    const long long* Q;
    const long long* l_offs;
    const long long* gain;
    const long long* shift;
    int P, k;
};

__global__ __launch_bounds__(256) void s2s_kmer_model_events_kernel(S2SKmeIn in, unsigned long long* __restrict__ table,
                                                                    unsigned long long* __restrict__ dropped) {
    __shared__ __attribute__((aligned(8))) int lds[S2S_KME_LDS_BYTES / 4];  // the counters, 8-byte words, in front of the keys
    static_assert(sizeof(lds) == S2S_KME_LDS_BYTES, "the cache and nothing else");
    unsigned long long (*cnt)[S2S_KMER_MODEL_SLOTS] = reinterpret_cast<unsigned long long (*)[S2S_KMER_MODEL_SLOTS]>(lds);
    int* keys = lds + S2S_KMER_MODEL_FIELDS * S2S_KMER_MODEL_SLOTS * 2;
    const long long slots = in.l_offs[in.P], step = (long long)gridDim.x * 256;
    if ((long long)blockIdx.x * 256 >= slots) return;                       // (the whole workgroup: it has no round)
    const int lane = threadIdx.x & 63, rows = (1 << (2 * in.k)) + 1;
    const bool direct = in.k <= S2S_KMER_MODEL_DIRECT_MAX_K;
    for (int i = threadIdx.x; i < S2S_KMER_MODEL_SLOTS; i += 256) {
        keys[i] = S2S_KME_EMPTY;
#pragma unroll
        for (int f = 0; f < S2S_KMER_MODEL_FIELDS; ++f) cnt[f][i] = 0ull;
    }
    __syncthreads();
    int round = 0, n_over = 0, n_range = 0, n_code = 0, n_counted = 0;      // (the same in every lane of a wave)
    // (every wave of a workgroup runs the same rounds; a wave without a slot skips the body -- wave-uniformly -- not the barriers)
    for (long long g0 = (long long)blockIdx.x * 256; g0 < slots; g0 += step) {
        const long long gw = g0 + (threadIdx.x >> 6) * 64;
        if (gw < slots) {
            const long long g = gw + lane;
            int what = S2S_KME_NONE, code = 0, p;
            long long lo, hi, m = 0, d = 0;
            if (g < slots && s2s_record_find(in.l_offs, 0, in.P - 1, slots, g, p, lo, hi)) {
                const long long gain = in.gain[p];
                if (gain != 0) {
                    code = in.codes[g];
                    int64_t Mp = 0, Dp = 0;
                    what = s2s_kme_slot(in.ev_len[g], in.S[g], in.Q[g], code, rows, gain, in.shift[p], Mp, Dp);
                    m = Mp; d = Dp;
                }
            }
            const bool real = what == S2S_KME_EVENT;
            n_over += __popcll(__ballot(what == S2S_KME_OVERLONG));
            n_range += __popcll(__ballot(what == S2S_KME_OUT_OF_RANGE));
            n_code += __popcll(__ballot(what == S2S_KME_BAD_CODE));
            n_counted += __popcll(__ballot(real));
            if (!real) { m = 0; d = 0; }
            long long ev = real ? 1 : 0, m2 = m * m, d2 = d * d;
            bool issue = real;
            unsigned long long todo = __ballot(real);
            while (todo) {                                          // wave-uniform: one round per distinct code of the wave's slots
                const int first = __ffsll((long long)todo) - 1;
                const int lc = __shfl(code, first, 64);
                const bool mine = real && code == lc;
                const unsigned long long same = __ballot(mine);
                todo &= ~same;
                if (__popcll(same) < 2) continue;
                long long r_m = mine ? m : 0, r_m2 = mine ? m2 : 0, r_d = mine ? d : 0, r_d2 = mine ? d2 : 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    r_m += __shfl_xor(r_m, o, 64);
                    r_m2 += __shfl_xor(r_m2, o, 64);
                    r_d += __shfl_xor(r_d, o, 64);
                    r_d2 += __shfl_xor(r_d2, o, 64);
                }
                if (lane == first) { ev = __popcll(same); m = r_m; m2 = r_m2; d = r_d; d2 = r_d2; }
                else if (mine) issue = false;
            }
            if (issue) {
                const unsigned long long f[S2S_KMER_MODEL_FIELDS] = {(unsigned long long)ev, (unsigned long long)m, (unsigned long long)m2,
                                                                     (unsigned long long)d, (unsigned long long)d2};
                s2s_kme_insert(keys, cnt, table, direct, code, f);
            }
        }
        ++round;
        if (round % S2S_KMER_MODEL_FLUSH_ROUNDS == 0 && g0 + step < slots) {                // (the last round's flush is the one below)
            __syncthreads();
            s2s_kme_flush(keys, cnt, table);
            __syncthreads();
        }
    }
    __syncthreads();
    s2s_kme_flush(keys, cnt, table);
    if (lane == 0) {
        if (n_over) __hip_atomic_fetch_add(dropped + 0, (unsigned long long)n_over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_range) __hip_atomic_fetch_add(dropped + 1, (unsigned long long)n_range, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_code) __hip_atomic_fetch_add(dropped + 2, (unsigned long long)n_code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_counted) __hip_atomic_fetch_add(dropped + 3, (unsigned long long)n_counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#endif  // S2S_DTW_KERNELS
