// Do two spellings of the same value give the same BITS on gfx950?  A stand-alone check (tests/test_gpu_split_residual.py builds and
// runs it) of three pieces of the attention loop's vector stream against the alternative each was priced against (LABNOTES round 35):
//   split   the hi/lo split of two pairs of values.  A: split2x2<true> of the library (and split2<true>, its single-pair form, which
//           has to agree with it bit for bit or the value counts as a mismatch) (s2s_device_h.h: v_cvt_pk_f16_f32, the residual
//           x * 1 - hi taken in fp32 by v_fma_mix_f32 -- exact: x and f16(x) are multiples of ulp32(x) and differ by at most half an f16
//           ulp -- then one more v_cvt_pk_f16_f32); B: the split of rounds 1-34 (v_cvt_pk_f16_f32, then v_fma_mix{lo,hi}_f16 -- x * 1 - hi
//           rounded ONCE, straight to f16).  Over every fp32 bit pattern of the exponent classes below, both signs, each value in the
//           low and in the high half of a pair.
//   mask    the phantom-key mask of a score tile.  A: att32_mask_tile of the library (a select per register); B: a bit-field select
//           with a per-lane keep mask.  Tiles 5 and 6 (dealt-out key order) and tile 7 (natural order), both lane halves.
//   max     the row maximum of a pass's two score tiles.  A: the 32-deep fmaxf chain of softmax_pv32; B: a tree of three-input maxima.
// mask and max run on score tiles filled with +0, -0, -inf, the largest finite value of either sign and ordinary scores.
// Build with the library's own flags:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -I seq2squiggle_amd/csrc
//                                       -o tools/probes/split_residual_check tools/probes/split_residual_check.hip
// Prints one line per check, "<name> ... mismatches N"; exit status 0 when every N is 0.
#include "s2s_device_h.h"
#include <cstdio>
#include <cstdlib>

// the exponent FIELDS whose 2^23 mantissas are all run, both signs: unbiased -25 (hi a subnormal f16 that rounds to 0 or to the smallest
// one), -15 (hi subnormal), -14 (the smallest normal hi; lo subnormal), -4 (lo subnormal, below 2^-3), -3, 0, 1 (normal hi and lo), 15
// (the top binade: hi turns inf from 65520), then 16 (hi = inf throughout), 0 (fp32 subnormals and the zeros) and 255 (inf and the NaNs)
__constant__ int EXP_FIELDS[11] = {127 - 25, 127 - 15, 127 - 14, 127 - 4, 127 - 3, 127, 128, 127 + 15, 127 + 16, 0, 255};
#define N_FIELDS 11

// B: one pair as rounds 1-34 split it (fma + conversion fold into v_fma_mixlo_f16 / v_fma_mixhi_f16)
__device__ __forceinline__ void split2_mix_f16(const float a, const float b, const float one, unsigned& hi, unsigned& lo) {
    unsigned hb = __builtin_bit_cast(unsigned, (h2v{(_Float16)a, (_Float16)b}));
    asm("" : "+v"(hb));
    const h2v h = __builtin_bit_cast(h2v, hb);
    const h2v l = {(_Float16)__builtin_fmaf(a, one, -(float)h[0]), (_Float16)__builtin_fmaf(b, one, -(float)h[1])};
    hi = hb;
    lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ bool is_nan16(const unsigned h) { return (h & 0x7fffu) > 0x7c00u; }

// counters: [0] finite inputs whose hi or lo differ, [1] infinite inputs whose hi or lo differ, [2] NaN inputs without a NaN hi and lo
// on either side, [3] values run; first[]: the bit pattern of the first few offenders
__global__ __launch_bounds__(256) void split_check(const float one, unsigned long long* cnt, unsigned* first) {
    const long long n = (long long)N_FIELDS << 23;
    unsigned long long bad[3] = {0, 0, 0}, ran = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned bits = ((unsigned)EXP_FIELDS[i >> 23] << 23) | (unsigned)(i & 0x7fffff);
        const float p = __uint_as_float(bits), q = __uint_as_float(bits | 0x80000000u);
        unsigned ha2[2], la2[2], hb2[2], lb2[2];
        split2x2<true>(p, q, q, p, one, ha2[0], ha2[1], la2[0], la2[1]);
        split2_mix_f16(p, q, one, hb2[0], lb2[0]);
        split2_mix_f16(q, p, one, hb2[1], lb2[1]);
#pragma unroll
        for (int swap = 0; swap < 2; ++swap) {
            const float a = swap ? q : p, b = swap ? p : q;
            unsigned hs, ls;
            split2<true>(a, b, one, hs, ls);                  // the library's single-pair form (the GEMM operands): must equal split2x2's pair
            const bool pair_forms_agree = hs == ha2[swap] && ls == la2[swap];
            const unsigned ha = pair_forms_agree ? ha2[swap] : ~hb2[swap], la = la2[swap], hb = hb2[swap], lb = lb2[swap];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const unsigned x = __float_as_uint(half ? b : a) & 0x7fffffffu;
                const unsigned h0 = (ha >> (16 * half)) & 0xffffu, l0 = (la >> (16 * half)) & 0xffffu;
                const unsigned h1 = (hb >> (16 * half)) & 0xffffu, l1 = (lb >> (16 * half)) & 0xffffu;
                int k = -1;
                if (x > 0x7f800000u) { if (!(is_nan16(h0) && is_nan16(l0) && is_nan16(h1) && is_nan16(l1))) k = 2; }
                else if (h0 != h1 || l0 != l1) k = x == 0x7f800000u ? 1 : 0;
                if (k >= 0 && bad[k]++ == 0) {
                    const unsigned slot = atomicAdd(&first[0], 1u);
                    if (slot < 15) first[1 + slot] = __float_as_uint(half ? b : a);
                }
                ++ran;
            }
        }
    }
    for (int k = 0; k < 3; ++k) if (bad[k]) atomicAdd(&cnt[k], bad[k]);
    atomicAdd(&cnt[3], ran);
}

// B: the phantom-key mask as a bit-field select -- keep[half] is all ones where the lane half keeps its score (v_bfi_b32)
template <int TV, bool NATURAL>
__device__ __forceinline__ void mask_tile_bfi(f32x16& t, const int tile, const int h) {
    unsigned keep_lo = h ? ~0u : 0u, keep_hi = h ? 0u : ~0u;             // keeps the score where lane half 0 / lane half 1 holds the phantom key
    asm("" : "+v"(keep_lo), "+v"(keep_hi));
    const unsigned ninf = 0xff800000u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2);
        const bool p0 = att32_key_at<NATURAL>(32 * tile + row) >= TV, p1 = att32_key_at<NATURAL>(32 * tile + row + 4) >= TV;
        const unsigned u = __float_as_uint(t[r]);
        if (p0 && p1) t[r] = -__builtin_inff();
        else if (p1) t[r] = __uint_as_float((u & keep_hi) | (ninf & ~keep_hi));
        else if (p0) t[r] = __uint_as_float((u & keep_lo) | (ninf & ~keep_lo));
    }
}
__device__ __forceinline__ float max_chain(const f32x16 (&sc)[2]) {       // A: as in softmax_pv32, pass 0
    float mh = sc[0][0];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) mh = fmaxf(mh, sc[i][r]);
    return mh;
}
__device__ __forceinline__ float max3f(const float a, const float b, const float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float max_tree(const f32x16 (&sc)[2]) {        // B: three-input maxima, 27 -> 9 -> 3 -> 1 and the five left over
    float m9[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { const int e = 3 * j + k; v[k] = sc[e >> 4][e & 15]; }
        m9[j] = max3f(v[0], v[1], v[2]);
    }
    const float a = max3f(m9[0], m9[1], m9[2]), b = max3f(m9[3], m9[4], m9[5]), c = max3f(m9[6], m9[7], m9[8]);
    const float d = max3f(sc[1][11], sc[1][12], sc[1][13]), e = fmaxf(sc[1][14], sc[1][15]);
    return max3f(max3f(a, b, c), d, e);
}
// score tiles: every register one of eight special values or an ordinary score, drawn by a hash of (case, lane, register)
__device__ __forceinline__ float tile_value(const unsigned c, const unsigned lane, const unsigned r) {
    unsigned x = c * 0x9E3779B1u + lane * 0x85EBCA77u + r * 0xC2B2AE3Du;
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    switch (x & 7u) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return -__builtin_inff();
        case 3: return 3.4028234663852886e38f;
        case 4: return -3.4028234663852886e38f;
        default: return (float)(int)((x >> 8) & 0xffffu) * (1.0f / 256.0f) - 128.0f;
    }
}
template <int TILE, bool NATURAL>
__device__ __forceinline__ unsigned mask_case(const f32x16& t0, const int h) {
    f32x16 a = t0, b = t0;
    att32_mask_tile<250, NATURAL>(a, TILE, h);
    mask_tile_bfi<250, NATURAL>(b, TILE, h);
    unsigned bad = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) bad += __float_as_uint(a[r]) != __float_as_uint(b[r]);
    return bad;
}
// counters: [4] mask registers that differ, [5] row maxima that differ, [6] cases run (per lane)
__global__ __launch_bounds__(256) void mask_max_check(const int cases, unsigned long long* cnt) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    unsigned long long bad_mask = 0, bad_max = 0, ran = 0;
    for (int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < cases; c += gridDim.x * (blockDim.x >> 6)) {
        f32x16 sc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[i][r] = tile_value(c, lane, 16 * i + r);
        bad_mask += mask_case<5, false>(sc[0], h) + mask_case<6, false>(sc[1], h) + mask_case<7, true>(sc[0], h) + mask_case<0, false>(sc[1], h);
        bad_max += __float_as_uint(max_chain(sc)) != __float_as_uint(max_tree(sc));
        // ... and behind the masks, as the loop has them (a tile may then be -inf throughout)
        att32_mask_tile<250, true>(sc[1], 7, h);
        bad_max += __float_as_uint(max_chain(sc)) != __float_as_uint(max_tree(sc));
        ++ran;
    }
    if (bad_mask) atomicAdd(&cnt[4], bad_mask);
    if (bad_max) atomicAdd(&cnt[5], bad_max);
    atomicAdd(&cnt[6], ran);
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } } while (0)
int main() {
    unsigned long long* cnt; unsigned* first;
    CHECK(hipMalloc(&cnt, 8 * sizeof(unsigned long long)));
    CHECK(hipMalloc(&first, 16 * sizeof(unsigned)));
    CHECK(hipMemset(cnt, 0, 8 * sizeof(unsigned long long)));
    CHECK(hipMemset(first, 0, 16 * sizeof(unsigned)));
    split_check<<<4096, 256>>>(1.0f, cnt, first);
    CHECK(hipGetLastError());
    const int cases = 1 << 16;
    mask_max_check<<<1024, 256>>>(cases, cnt);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    unsigned long long h[8]; unsigned f[16];
    CHECK(hipMemcpy(h, cnt, sizeof h, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(f, first, sizeof f, hipMemcpyDeviceToHost));
    const unsigned long long want = ((unsigned long long)N_FIELDS << 23) * 4;
    printf("split finite inputs: values %llu (expected %llu) mismatches %llu\n", h[3], want, h[0]);
    printf("split infinite inputs: mismatches %llu\n", h[1]);
    printf("split NaN inputs without NaN hi and lo: mismatches %llu\n", h[2]);
    for (unsigned i = 0; i < f[0] && i < 15; ++i) printf("  offending input 0x%08x\n", f[1 + i]);
    printf("mask select: lane-cases %llu (expected %llu) mismatches %llu\n", h[6], (unsigned long long)cases * 64, h[4]);
    printf("row maximum: mismatches %llu\n", h[5]);
    const bool ok = h[3] == want && h[6] == (unsigned long long)cases * 64 && !h[0] && !h[1] && !h[2] && !h[4] && !h[5];
    printf(ok ? "ALL EQUAL\n" : "DIFFERENT\n");
    return ok ? 0 : 1;
}
