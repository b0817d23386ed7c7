// s2s_generic_h.h -- the decoder FFT blocks of the reduced-precision generic instances (S2S_MODE_GENERIC_F16 and, at any chunk
// geometry, S2S_MODE_GENERIC_GEOMETRY_F16), included by s2s_hip.hip after s2s_generic.h.
//
// Everything else of those instances -- embedding, pre-net, the encoder FFT blocks, the heads, dwell, the length regulator and
// out_linear / noise / clamp -- is S2S_MODE_GENERIC's fp32 code (s2s_generic.h), launched the same way.  In the decoder every matrix
// product takes its two operands rounded to f16 once (round to nearest even) and accumulates in fp32 on v_mfma_f32_16x16x32_f16:
//   gen_gemm_h_kernel<EPI>         QKV, fc, w_1, w_2: the epilogues of gen_gemm_kernel<EPI> (bias, ReLU, residual) in fp32
//   gen_attention_h_kernel         Q.K^T and P.V of one (chunk, head) over the 250 decoder keys, fp32 softmax with its exact row
//                                  maximum; gen_attention_h_any_kernel the same over T <= 256 keys, T at run time
//   gen_attention_long_h_kernel<NT>  the same over 257..1024 keys: one workgroup per (chunk, head, 64 queries), two passes over K
// The LayerNorms stay gen_layernorm_kernel (fp32).
//
// 16x16x32 f16 operand layout (lane l = 16g + c): A[row c][k 8g + j], B[k 8g + j][col c] in element j = 0..7; the result
// D[row 4g + r][col c] in register r.  Any permutation of k that both operands share gives the same product.
#pragma once
#include "s2s_generic.h"

typedef _Float16 gen_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 gen_h4 __attribute__((ext_vector_type(4)));
// float offsets into the arena of one decoder FFT block's f16 weights (host: pack_generic): wqkv [3d][ld_d], wfc [d][ld_d],
// w1 [dff][ld_d], w2 [d][ld_f] halves, ld_d / ld_f = dmodel / dff rounded up to 32; the biases and LayerNorms are GenLayer's fp32 ones
struct GenLayerH { long long wqkv, wfc, w1, w2; };

#define GEN_MFMA_H(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ gen_h8 gen_to_h8(const f32x4 a, const f32x4 b) {
    return gen_h8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3], (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
}

// ---- C[m][n] = epilogue(sum_k f16(A[m][k]) Wh[n][k] + bias[n]) for M x N x K.  A fp32 (the workspace rows), Wh f16 in nn.Linear's
//      [out][in] layout with its rows zero-padded to ldw = K rounded up to 32 (s2s_create converts the decoder weights once).
//      EPI as gen_gemm_kernel: 0: + bias; 1: + bias, ReLU; 2: + bias + R[m][n] (R may alias C: each element is read, then written,
//      by the same lane).  A 64 x 64 output tile per 4-wave workgroup, 32 x 32 per wave (2 x 2 MFMA tiles), K in steps of 32: each
//      thread loads 8 consecutive k of one A row (two float4, converted to f16 on the way into LDS) and 8 of one Wh row (16 bytes)
//      for the next step while the MFMAs of this one run.  LDS rows of 40 halves (80 bytes), so the 16-byte operand reads of the
//      16 lanes of a row group start on different banks.  Requires K % 8 == 0 (an octet is all inside K or all outside), lda a
//      multiple of 4 and 16-byte aligned bases: every dmodel and dff of the generic limits qualifies.  LDS 10,240 bytes.
#define GENH_BK 32
#define GENH_LDK (GENH_BK + 8)
template <int EPI>
__global__ void __launch_bounds__(256) gen_gemm_h_kernel(const float* __restrict__ A, int lda, const _Float16* __restrict__ Wh, int ldw,
                                                         const float* __restrict__ bias, float* C, int ldc, const float* R, int ldr,
                                                         int M, int N, int K) {
    __shared__ __attribute__((aligned(16))) _Float16 As[GEN_BM * GENH_LDK];
    __shared__ __attribute__((aligned(16))) _Float16 Ws[GEN_BN * GENH_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int m0 = blockIdx.x * GEN_BM, n0 = blockIdx.y * GEN_BN;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int lr = tid >> 2, lk = (tid & 3) * 8;              // staging: row lr of the tile, k-octet lk
    const long long am = m0 + lr, wr = n0 + lr;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    f32x4 a0, a1;
    gen_h8 wv;
    auto load = [&](int k0) {
        const int kk = k0 + lk;
        const bool in = am < M && kk < K;
        a0 = in ? ldg4(A + am * lda + kk) : f32x4{0, 0, 0, 0};
        a1 = in ? ldg4(A + am * lda + kk + 4) : f32x4{0, 0, 0, 0};
        // kk < ldw always (k0 < K <= ldw, ldw % 32 == 0); the padding k are zeros
        wv = wr < N ? *reinterpret_cast<const gen_h8*>(Wh + wr * ldw + kk) : gen_h8{};
    };
    load(0);
    for (int k0 = 0; k0 < K; k0 += GENH_BK) {
        __syncthreads();                                      // the previous step's reads are done
        *reinterpret_cast<gen_h8*>(As + lr * GENH_LDK + lk) = gen_to_h8(a0, a1);
        *reinterpret_cast<gen_h8*>(Ws + lr * GENH_LDK + lk) = wv;
        __syncthreads();
        if (k0 + GENH_BK < K) load(k0 + GENH_BK);
        gen_h8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const gen_h8*>(As + (wm + 16 * i + c) * GENH_LDK + 8 * g);
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const gen_h8*>(Ws + (wn + 16 * j + c) * GENH_LDK + 8 * g);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = GEN_MFMA_H(a[i], b[j], acc[i][j]);
    }
    // D[4g + r][c] of tile (i, j) = C[m0 + wm + 16i + 4g + r][n0 + wn + 16j + c]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + 16 * j + c;
        if (n >= N) continue;
        const float bn = bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = m0 + wm + 16 * i + 4 * g + r;
                if (m >= M) continue;
                float v = acc[i][j][r] + bn;
                if (EPI == 1) v = relu1(v);
                if (EPI == 2) v += R[m * ldr + n];
                C[m * ldc + n] = v;
            }
    }
}

// ---- scaled dot-product attention of one decoder (chunk, head) on the matrix cores (layers.py:19-41, 64-88; no mask in predict),
//      on the QKV rows [row][3d] = q | k | v as gen_attention_kernel reads them; O overwrites Q in place.  T <= 256 keys and queries
//      per chunk: the constant 250 in gen_attention_h_kernel (S2S_MODE_GENERIC_F16's instance, whose code a run-time T would
//      change: the select of a run-time mask keeps the compiler from contracting s * sc - max into one fma), max_signal_len at run
//      time in gen_attention_h_any_kernel (S2S_MODE_GENERIC_GEOMETRY_F16 at other lengths up to 256).
//      16 waves, wave w the queries 16w .. 16w+15 (queries T..255 are computed on zero rows and never stored); the T keys padded to
//      256.  Scores are computed transposed, S^T = K Q^T (A = K, B = Q^T): lane (g, c) then holds query 16w + c against keys
//      16jt + 4g + r in register r of tile jt = 0..15, 64 fp32 scores, so a query's whole row sits in the 4 lanes c, c+16, c+32, c+48
//      and no online rescale is needed.  Padding keys are masked to -inf; softmax in fp32 with the exact row maximum
//      (exp(s - max) / sum, as torch.softmax), P rounded to f16 after the normalisation.  P.V (A = P, B = V) takes those registers
//      as they are: element j of k-block kb is key 32kb + 16(j>>2) + 4g + (j&3), and the V^T rows in LDS supply the same keys as two
//      8-byte reads.  K and Q are staged in steps of 32 head dims and V^T in steps of 64, so every head_dim up to 512 fits:
//        LDS   Q.K^T step: K [256][40] + Q [256][40] halves = 40,960 bytes; P.V step: V^T [64][264] halves = 33,792 bytes in the same
//              bytes (the steps are separated by barriers): 40,960 bytes per workgroup, 3 workgroups fit a CU's 160 KiB.
//        VGPR  64 fp32 scores (then 32 for P in f16) + 4 accumulators of P.V + 8 operand and 16 staging registers: within the 128 of
//              a 1024-thread workgroup, no spills (tests/test_generic_f16_cpu.py).
#define GENH_TP 256
#define GENH_EK 32
#define GENH_LDQ (GENH_EK + 8)
#define GENH_EV 64
#define GENH_LDV (GENH_TP + 8)
template <int TD>
__device__ __forceinline__ void gen_attention_h_body(float* __restrict__ QKV, int d, int H, int T_) {
    const int T = TD ? TD : T_;
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * GENH_TP * GENH_LDQ];
    _Float16* Ks = lds;
    _Float16* Qs = lds + GENH_TP * GENH_LDQ;
    _Float16* Vt = lds;
    const int hd = d / H, ld = 3 * d;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    float* base = QKV + (long long)b * T * ld + h * hd;
    f32x4 s[16];
#pragma unroll
    for (int jt = 0; jt < 16; ++jt) s[jt] = f32x4{0, 0, 0, 0};
    const int sr = tid >> 2, se = (tid & 3) * 8;              // staging: key and query sr, head dims se .. se+7 of the step
    const float* krow = base + (long long)sr * ld + d;
    const float* qrow = base + (long long)sr * ld;
    for (int e0 = 0; e0 < hd; e0 += GENH_EK) {
        f32x4 k4[2], q4[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = e0 + se + i;
            const bool in = sr < T && e < hd;
            k4[i >> 2][i & 3] = in ? krow[e] : 0.0f;
            q4[i >> 2][i & 3] = in ? qrow[e] : 0.0f;
        }
        __syncthreads();                                      // the previous step's reads are done
        *reinterpret_cast<gen_h8*>(Ks + sr * GENH_LDQ + se) = gen_to_h8(k4[0], k4[1]);
        *reinterpret_cast<gen_h8*>(Qs + sr * GENH_LDQ + se) = gen_to_h8(q4[0], q4[1]);
        __syncthreads();
        const gen_h8 qf = *reinterpret_cast<const gen_h8*>(Qs + (16 * wave + c) * GENH_LDQ + 8 * g);
#pragma unroll
        for (int jt = 0; jt < 16; ++jt)
            s[jt] = GEN_MFMA_H(*reinterpret_cast<const gen_h8*>(Ks + (16 * jt + c) * GENH_LDQ + 8 * g), qf, s[jt]);
    }
    // softmax over the keys of query 16w + c: s / temperature (d_k ** 0.5, layers.py:58) as exp2 of log2(e)-scaled scores
    const float sc = 1.4426950408889634f / sqrtf((float)hd);
    float mx = -__builtin_inff();
#pragma unroll
    for (int jt = 0; jt < 16; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = 16 * jt + 4 * g + r < T ? s[jt][r] * sc : -__builtin_inff();
            s[jt][r] = v;
            mx = fmaxf(mx, v);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.0f;
#pragma unroll
    for (int jt = 0; jt < 16; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[jt][r] = exp2f(s[jt][r] - mx);
            sum += s[jt][r];
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    gen_h8 p[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) p[kb][j] = (_Float16)(s[2 * kb + (j >> 2)][j & 3] * inv);
    // O = P V in steps of 64 head dims; V^T staged with one head dim and 16 consecutive keys per thread
    const int ve = tid & 63, vk = 16 * (tid >> 6);
    for (int e0 = 0; e0 < hd; e0 += GENH_EV) {
        gen_h8 v0, v1;
        const int e = e0 + ve;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k0 = vk + i, k1 = vk + 8 + i;
            v0[i] = (_Float16)(k0 < T && e < hd ? base[(long long)k0 * ld + 2 * d + e] : 0.0f);
            v1[i] = (_Float16)(k1 < T && e < hd ? base[(long long)k1 * ld + 2 * d + e] : 0.0f);
        }
        __syncthreads();                                      // Q.K^T's (or the previous step's) reads of these bytes are done
        *reinterpret_cast<gen_h8*>(Vt + ve * GENH_LDV + vk) = v0;
        *reinterpret_cast<gen_h8*>(Vt + ve * GENH_LDV + vk + 8) = v1;
        __syncthreads();
        const int net = (hd - e0 + 15) / 16 < GENH_EV / 16 ? (hd - e0 + 15) / 16 : GENH_EV / 16;
        for (int et = 0; et < net; ++et) {
            const _Float16* vr = Vt + (16 * et + c) * GENH_LDV + 4 * g;
            f32x4 o = {0, 0, 0, 0};
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                const gen_h4 lo = *reinterpret_cast<const gen_h4*>(vr + 32 * kb);
                const gen_h4 hi = *reinterpret_cast<const gen_h4*>(vr + 32 * kb + 16);
                o = GEN_MFMA_H(p[kb], (gen_h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}), o);
            }
            // o[r] = O[query 16w + 4g + r][head dim e0 + 16et + c]
            const int eo = e0 + 16 * et + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * wave + 4 * g + r;
                if (q < T && eo < hd) base[(long long)q * ld + eo] = o[r];
            }
        }
    }
}


// S2S_MODE_GENERIC_F16 (and S2S_MODE_GENERIC_GEOMETRY_F16 at 250 samples): the 250-key instance, T a constant
__global__ void __launch_bounds__(1024) gen_attention_h_kernel(float* __restrict__ QKV, int d, int H) {
    gen_attention_h_body<GEN_T_DEC>(QKV, d, H, GEN_T_DEC);
}
// S2S_MODE_GENERIC_GEOMETRY_F16 at any other max_signal_len <= 256: T at run time
__global__ void __launch_bounds__(1024) gen_attention_h_any_kernel(float* __restrict__ QKV, int d, int H, int T) {
    gen_attention_h_body<0>(QKV, d, H, T);
}
// ---- scaled dot-product attention of one decoder (chunk, head) over T = 257..1024 keys on the matrix cores
//      (S2S_MODE_GENERIC_GEOMETRY_F16 beyond 256 samples, where gen_attention_h_kernel's 64 score registers per lane no longer hold a
//      query's row); O overwrites Q in place.  One workgroup per (chunk, head, 64 queries), gen_attention_long_kernel's layout: wave w
//      owns queries 16w .. 16w+15 of the tile, scores transposed, S^T = K Q^T (A = 16 keys x 32 head dims of K from LDS, B = the
//      wave's Q^T fragment), so lane (g, c) holds query c against keys 16kt + 4g + r in register r of key tile kt.
//      Keys go in blocks of 64: K [64][32 head dims] (and V^T [64 head dims][64]) are staged through LDS as f16, shared by the four
//      waves.  Two passes over the blocks:
//        1. S^T, the exact row maximum (of the unscaled scores; the scale 1/sqrt(d_k) > 0 keeps the argmax).
//        2. S^T again, p = exp2(s log2(e)/sqrt(d_k) - max log2(e)/sqrt(d_k)) in fp32 (one v_fma + one v_exp per score: every exp is
//           computed once), the fp32 row sum, p rounded to f16 once -- p lies in [0, 1], unnormalised -- and O^T += V^T P^T
//           (A = V^T from LDS, B = P as it sits in the score registers: element j of k-block kb is key 32kb + 16(j>>2) + 4g + (j&3),
//           as in gen_attention_h_kernel); at the end O = O^T^T / sum in fp32.
//      Dividing at the end, not normalising P before its rounding as gen_attention_h_kernel and the reference's autocast do: the sum
//      is only known after the last block, and normalising first would take a third pass (or a second exp) per score.  Both round
//      one value of [0, 1] per score to f16; the two conventions differ by that rounding, within the 16-mixed bar.  No online
//      rescaling of O.  The price of the exact maximum is the score product done twice -- at small head_dim the exp, not the matrix
//      pipe, bounds the kernel (4 scores per lane per MFMA), so the second product is nearly free there.
//      NT output tiles of 16 head dims, 16 NT >= hd (NT 1 | 8 | 32 for hd <= 16 | 128 | 512); Q in registers as QS = 1 | 4 fragments
//      of 32 head dims for NT = 1 | 8; for NT = 32 read again for every step from the L1 / L2 (held, its 64 registers made the
//      instance spill).
//      Q, K and V are read through a buffer resource over the chunk's rows (no load leaves them): keys past T are zero rows in LDS
//      with p = 0, queries past T compute on zero rows and are not stored.
//        LDS   K [64][40] + V^T [64][72] halves = 5,120 + 9,216 = 14,336 bytes per workgroup (rows padded by 8 halves: the 16-byte
//              and 8-byte operand reads of 16 lanes start on different banks).
//        VGPR  4 NT accumulators + 4 QS for Q + 16 scores + 8 for P + 8 K / 16 V staging registers: 57 + 20 AGPRs (NT = 1),
//              108 + 48 (NT = 8), 139 + 144 (NT = 32); no scratch, no spills (tests/test_geometry_f16_cpu.py).  At most 6 | 3 | 1
//              waves per SIMD by registers; by LDS 11 workgroups fit a CU.
#define GENHL_KB 64
#define GENHL_LDV (GENHL_KB + 8)
template <int NT>
__global__ void __launch_bounds__(256) gen_attention_long_h_kernel(float* __restrict__ QKV, int d, int H, int T) {
    constexpr int QS = NT == 1 ? 1 : NT == 8 ? 4 : 0;          // Q fragments held in registers
    __shared__ __attribute__((aligned(16))) _Float16 Ks[GENHL_KB * GENH_LDQ];
    __shared__ __attribute__((aligned(16))) _Float16 Vt[GENH_EV * GENHL_LDV];
    const int nqt = (T + 63) / 64;
    const int b = blockIdx.x / (H * nqt), h = (blockIdx.x / nqt) % H, qt = blockIdx.x % nqt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int hd = d / H, ld = 3 * d;
    float* base = QKV + (long long)b * T * ld + h * hd;
    // The chunk's rows as a buffer resource: a load past their end returns 0, so the rows of keys and queries past T read as zeros.
    // Columns past the head's hd are other data of the same rows: zeroed for Q and K (bitwise, no branch), left as they are for V
    // (V^T row e >= hd only feeds output rows that are not stored).
    const __amdgpu_buffer_rsrc_t rows = __builtin_amdgcn_make_buffer_rsrc(QKV + (long long)b * T * ld, 0, T * ld * 4, 0x00020000);
    auto ldb = [&](int row, int part, int e) {                // QKV[chunk b][row][part + h * hd + e], 0 for row >= T
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rows, (unsigned)((row * ld + part + h * hd + e) * 4), 0, 0));
    };
    auto in_head = [&](float x, int e) { return __uint_as_float(__float_as_uint(x) & (unsigned)((e - hd) >> 31)); };   // e < hd ? x : 0
    const int q = qt * 64 + wave * 16 + c;                     // this lane's query: B-operand column c
    const bool qin = q < T;
    auto q_frag = [&](int e0) {                                // Q^T fragment of head dims e0 .. e0+31: B[k 8g + j][col c] = Q[q][e0 + 8g + j]
        gen_h8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (_Float16)in_head(ldb(q, 0, e0 + 8 * g + j), e0 + 8 * g + j);
        return f;
    };
    gen_h8 qf[QS > 0 ? QS : 1];                                // (QS = 0: read for every step instead, from the L1 / L2)
#pragma unroll
    for (int i = 0; i < QS; ++i) qf[i] = q_frag(32 * i);
    const int sr = tid >> 2, se = (tid & 3) * 8;              // staging: key sr of the block, head dims se .. se+7 of a K step
                                                              // (16 (tid & 3) .. +15 of a V step)
    f32x4 s[4];
    auto k_step = [&](int key, int e0, const gen_h8 qv) {     // s += K[keys of the block][e0 .. e0+31] Q^T
        f32x4 k4[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) k4[i >> 2][i & 3] = in_head(ldb(key, d, e0 + se + i), e0 + se + i);
        __syncthreads();                                      // the previous reads of Ks are done
        *reinterpret_cast<gen_h8*>(Ks + sr * GENH_LDQ + se) = gen_to_h8(k4[0], k4[1]);
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
            s[kt] = GEN_MFMA_H(*reinterpret_cast<const gen_h8*>(Ks + (16 * kt + c) * GENH_LDQ + 8 * g), qv, s[kt]);
    };
    auto scores = [&](int j0) {                                // s[kt][r] = S[query c][key j0 + 16kt + 4g + r] (unscaled)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) s[kt] = f32x4{0, 0, 0, 0};
        if (QS > 0) {
#pragma unroll
            for (int i = 0; i < QS; ++i) {
                if (32 * i >= hd) break;
                k_step(j0 + sr, 32 * i, qf[i]);
            }
        } else {
            for (int e0 = 0; e0 < hd; e0 += 32) k_step(j0 + sr, e0, q_frag(e0));
        }
    };
    float mx = -__builtin_inff();
    for (int j0 = 0; j0 < T; j0 += GENHL_KB) {
        scores(j0);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (j0 + 16 * kt + 4 * g + r < T) mx = fmaxf(mx, s[kt][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));                    // the four lanes of query c: c, c + 16, c + 32, c + 48
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float sc = 1.4426950408889634f / sqrtf((float)hd);   // log2(e) / temperature (d_k ** 0.5, layers.py:58)
    const float nms = -(mx * sc);
    f32x4 acc[NT];                                             // acc[t][r] = O[query c][16t + 4g + r]
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0, 0, 0, 0};
    float sum = 0.0f;
    const int nt = (hd + 15) / 16;
    for (int j0 = 0; j0 < T; j0 += GENHL_KB) {
        scores(j0);
        gen_h8 p[2];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = j0 + 16 * kt + 4 * g + r < T ? exp2f(fmaf(s[kt][r], sc, nms)) : 0.0f;
                sum += v;
                p[kt >> 1][4 * (kt & 1) + r] = (_Float16)v;
            }
#pragma unroll
        for (int vs = 0; vs < (NT + 3) / 4; ++vs) {            // V^T in steps of 64 head dims
            if (64 * vs >= hd) break;
            float v[16];
            const int key = j0 + sr, e0 = 64 * vs + 16 * (tid & 3);
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = ldb(key, 2 * d, e0 + i);
            __syncthreads();                                  // the previous reads of Vt are done
#pragma unroll
            for (int i = 0; i < 16; ++i) Vt[(16 * (tid & 3) + i) * GENHL_LDV + sr] = (_Float16)v[i];
            __syncthreads();
#pragma unroll
            for (int et = 0; et < 4; ++et) {
                const int t = 4 * vs + et;
                if (t >= NT || t >= nt) break;
                const _Float16* vr = Vt + (16 * et + c) * GENHL_LDV + 4 * g;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const gen_h4 lo = *reinterpret_cast<const gen_h4*>(vr + 32 * kb);
                    const gen_h4 hi = *reinterpret_cast<const gen_h4*>(vr + 32 * kb + 16);
                    acc[t] = GEN_MFMA_H((gen_h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}), p[kb], acc[t]);
                }
            }
        }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (!qin) return;                                          // (no barriers below)
    float* orow = base + (long long)q * ld;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (16 * t >= hd) break;
        const bool full = 16 * t + 16 <= hd;                   // (uniform: no per-element test but in the last, partial tile)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = 16 * t + 4 * g + r;
            if (full || e < hd) orow[e] = acc[t][r] / sum;
        }
    }
}
