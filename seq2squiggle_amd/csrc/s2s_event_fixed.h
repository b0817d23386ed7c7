// The fixed-point statistics of ONE event (`predict --kmer-model`; include/s2s_hip.h: s2s_event_fixed states the definition): the
// event mean M and the event's population deviation D in units of 2^-8 ADC counts, from the slot's n / S / Q in 64-bit integers
// only, so that they can be summed per k-mer with integer adds.  One function for the kernel (s2s_kmer_model_kernel) and for the
// host entry (s2s_event_fixed): both sides compute the same integers by construction.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define S2S_FIXED_HD __host__ __device__
#else
#define S2S_FIXED_HD
#endif

// 1 <= n <= 1024, |S| <= 2^25, 0 <= Q <= 2^40 with n*Q >= S*S (what s2s_event_stats gives; a negative n*Q - S*S counts as 0).
S2S_FIXED_HD inline void s2s_event_fixed_point(int32_t n, int32_t S, int64_t Q, int64_t& M, int64_t& D) {
    // M = round-half-even(256 * S / n): floor division, then the remainder decides
    const int64_t num = 256 * (int64_t)S;
    int64_t q = num / n, r = num - q * n;                       // (C++ truncates towards zero)
    if (r < 0) { q -= 1; r += n; }
    if (2 * r > n || (2 * r == n && (q & 1))) q += 1;
    M = q;
    // D = floor(sqrt(floor(V * 2^16 / n^2))), V = n*Q - S*S <= 2^50: the quotient in two parts so that nothing passes 2^63.
    // (The products that only arguments outside the contract can overflow are formed unsigned and x is capped: such arguments
    // give some number, not undefined behaviour.)
    int64_t V = (int64_t)((uint64_t)n * (uint64_t)Q - (uint64_t)((int64_t)S * (int64_t)S));
    if (V < 0) V = 0;
    const int64_t n2 = (int64_t)n * n;
    const int64_t a = V / n2, b = V - a * n2;                   // b < n^2 <= 2^20: b << 16 < 2^36
    uint64_t xu = ((uint64_t)a << 16) + (((uint64_t)b << 16) / (uint64_t)n2);
    if (xu > ((uint64_t)1 << 60)) xu = (uint64_t)1 << 60;
    const int64_t x = (int64_t)xu;                              // <= 2^46 inside the contract
    int64_t d = (int64_t)sqrt((double)x);                       // exact to within one; the comparisons settle it
    while (d * d > x) --d;
    while ((d + 1) * (d + 1) <= x) ++d;
    D = d;
}
