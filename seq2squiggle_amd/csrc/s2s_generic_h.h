// s2s_generic_h.h -- the decoder FFT blocks of the reduced-precision size-generic instance (S2S_MODE_GENERIC_F16), included by
// s2s_hip.hip after s2s_generic.h.
//
// Everything else of that instance -- embedding, pre-net, the encoder FFT blocks, the heads, dwell, the length regulator and
// out_linear / noise / clamp -- is S2S_MODE_GENERIC's fp32 code (s2s_generic.h), launched the same way.  In the decoder every matrix
// product takes its two operands rounded to f16 once (round to nearest even) and accumulates in fp32 on v_mfma_f32_16x16x32_f16:
//   gen_gemm_h_kernel<EPI>   QKV, fc, w_1, w_2: the epilogues of gen_gemm_kernel<EPI> (bias, ReLU, residual) in fp32
//   gen_attention_h_kernel   Q.K^T and P.V of one (chunk, head) over the 250 decoder keys, fp32 softmax with its exact row maximum
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
//      on the QKV rows [row][3d] = q | k | v as gen_attention_kernel reads them; O overwrites Q in place.
//      16 waves, wave w the queries 16w .. 16w+15 (queries 250..255 are computed on zero rows and never stored); the 250 keys padded to
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
__global__ void __launch_bounds__(1024) gen_attention_h_kernel(float* __restrict__ QKV, int d, int H) {
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * GENH_TP * GENH_LDQ];
    _Float16* Ks = lds;
    _Float16* Qs = lds + GENH_TP * GENH_LDQ;
    _Float16* Vt = lds;
    const int hd = d / H, ld = 3 * d;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    float* base = QKV + (long long)b * GEN_T_DEC * ld + h * hd;
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
            const bool in = sr < GEN_T_DEC && e < hd;
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
            const float v = 16 * jt + 4 * g + r < GEN_T_DEC ? s[jt][r] * sc : -__builtin_inff();
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
            v0[i] = (_Float16)(k0 < GEN_T_DEC && e < hd ? base[(long long)k0 * ld + 2 * d + e] : 0.0f);
            v1[i] = (_Float16)(k1 < GEN_T_DEC && e < hd ? base[(long long)k1 * ld + 2 * d + e] : 0.0f);
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
                if (q < GEN_T_DEC && eo < hd) base[(long long)q * ld + eo] = o[r];
            }
        }
    }
}
