// s2s_generic.h -- device code of the size-generic fp32 instance (S2S_MODE_GENERIC), included by s2s_hip.hip.
//
// The tuned instances (s2s_fused_kernel) keep one chunk's activations in registers and are written for dmodel 64 / dff 256 /
// 8 heads.  This instance runs any size within the limits of include/s2s_hip.h as a layer-wise pipeline over a slice of the
// launch's chunks: every stage is one kernel over all rows of the slice (row = chunk * T + t, activations row-major [row][feature]
// in a workspace the handle grows on demand), so the matrix products see tens of thousands of rows and tile like any GEMM.
//   gen_embed_kernel       k gathered columns of src_emb + bias, ReLU                                 (modules.py:70-73)
//   gen_gemm_kernel<EPI>   Y = X W^T + b [ReLU | + residual] on v_mfma_f32_16x16x4_f32                 (pre-net, QKV, fc, FFN, heads)
//   gen_layernorm_kernel   nn.LayerNorm(dmodel, eps 1e-5) per row, one wave per row                   (layers.py:86, 112)
//   gen_attention_kernel   one workgroup per (chunk, head): exact fp32 softmax with its row maximum    (layers.py:19-41, 64-88)
//   gen_attention_long_kernel  the same for more than 256 keys, on v_mfma_f32_16x16x4_f32: one workgroup per (chunk, head, 64 queries)
//   gen_dwell_kernel       Linear(d,1) + Softplus of the three heads, the dwell source, + position_enc (modules.py:197-225, 275-278, 396-438, 80)
//   gen_lenreg_kernel      length regulator gather + decoder positions                                (modules.py:344-392, 136)
//   gen_emit_kernel        out_linear + ReLU, x scale, noise, clamp                                   (modules.py:140-141, model.py:221-240)
// The random draws use the tuned instances' Philox counters (s2s_device.h), so a default-size checkpoint gets the same dwell
// stream and noise under either instance.  The chunk geometry is a run-time argument of every kernel here: te k-mers in (max_dna_len)
// and ts samples out (max_signal_len) per chunk -- 16 / 250 for S2S_MODE_GENERIC, the checkpoint's own for
// S2S_MODE_GENERIC_GEOMETRY.
#pragma once
#include "s2s_device.h"

#define GEN_T_DEC 250          // the decoder length of S2S_MODE_GENERIC_F16's attention (s2s_generic_h.h)

// fp32 blob offsets of one FFT block (host: pack_generic); wqkv is [3d][d] (w_qs | w_ks | w_vs rows), bqkv [3d]
struct GenLayer { long long wqkv, bqkv, wfc, bfc, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b; };

__device__ __forceinline__ float gen_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float gen_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int gen_base_code(unsigned char ch) {       // utils.py:74 letter_to_int
    return ch == 'A' ? 1 : ch == 'C' ? 2 : ch == 'G' ? 3 : ch == 'T' ? 4 : ch == '_' ? 0 : -1;
}

// ---- src_emb on the one-hot k-mer == bias + sum of k gathered columns of W_emb (added in k order), then ReLU.  One thread per
//      (row, feature); emb_wt is W_emb^T [5k][d].  chunk_start (nullable): packed reads, chunk b at bases + chunk_start[b].
__global__ void __launch_bounds__(256) gen_embed_kernel(const float* __restrict__ emb_wt, const float* __restrict__ emb_b, int k, int d,
                                                        const uint8_t* __restrict__ bases, const long long* __restrict__ chunk_start,
                                                        const uint8_t* __restrict__ n_valid, int S, int te, float* __restrict__ X) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)S * te * d) return;
    const int f = (int)(i % d);
    const long long row = i / d;
    const int b = (int)(row / te), c = (int)(row % te);
    const uint8_t* bp = chunk_start ? bases + chunk_start[b] : bases + (long long)b * (te + k - 1);
    const bool pad = c >= n_valid[b];                                       // pad k-mer = "_" * k (utils.py:342-347)
    float x = emb_b[f];
    for (int j = 0; j < k; ++j) {
        const int code = pad ? 0 : gen_base_code(bp[c + j]);
        if (code >= 0) x += emb_wt[(long long)(5 * j + code) * d + f];        // unknown letter: all-zero one-hot row (utils.py:86)
    }
    X[i] = relu1(x);
}

// ---- C[m][n] = epilogue(sum_k A[m][k] W[n][k] + bias[n]) for M x N x K, W in nn.Linear's native [out][in] layout.
//      EPI 0: + bias; 1: + bias, ReLU; 2: + bias + R[m][n] (the residual; R may alias C: each element is read, then written, by
//      the same lane).  A 64 x 64 output tile per 4-wave workgroup, 32 x 32 per wave (2 x 2 MFMA tiles), K in steps of 16 staged
//      through LDS k-major, so that the 16 lanes of an MFMA operand row read 16 consecutive words.  Requires K % 4 == 0, lda and
//      ldw multiples of 4 and 16-byte aligned bases (float4 loads): every dmodel and dff of the generic limits qualifies.
#define GEN_BM 64
#define GEN_BN 64
#define GEN_BK 16
#define GEN_LDT (GEN_BM + 4)
template <int EPI>
__global__ void __launch_bounds__(256) gen_gemm_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Wt, int ldw,
                                                       const float* __restrict__ bias, float* C, int ldc, const float* R, int ldr,
                                                       int M, int N, int K) {
    __shared__ float As[GEN_BK][GEN_LDT];
    __shared__ float Ws[GEN_BK][GEN_LDT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int m0 = blockIdx.x * GEN_BM, n0 = blockIdx.y * GEN_BN;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int lr = tid >> 2, lq = (tid & 3) * 4;              // staging: row lr of the tile, k-quad lq
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    const long long am = m0 + lr, wn_ = n0 + lr;
    for (int k0 = 0; k0 < K; k0 += GEN_BK) {
        const int kk = k0 + lq;
        const f32x4 av = (am < M && kk < K) ? ldg4(A + am * lda + kk) : f32x4{0, 0, 0, 0};
        const f32x4 wv = (wn_ < N && kk < K) ? ldg4(Wt + wn_ * ldw + kk) : f32x4{0, 0, 0, 0};
        __syncthreads();                                      // the previous step's reads are done
#pragma unroll
        for (int r = 0; r < 4; ++r) { As[lq + r][lr] = av[r]; Ws[lq + r][lr] = wv[r]; }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < GEN_BK / 4; ++ks) {
            const int kr = 4 * ks + g;                        // MFMA k-index g of this 4-step
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[kr][wm + 16 * i + c];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Ws[kr][wn + 16 * j + c];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = MFMA4(a[i], b[j], acc[i][j]);
        }
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

// ---- nn.LayerNorm over the d features of each row, in place: one wave per row, two passes (mean, then the centred squares).
__global__ void __launch_bounds__(256) gen_layernorm_kernel(float* __restrict__ X, const float* __restrict__ gam, const float* __restrict__ bet,
                                                            long long M, int d) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    float* x = X + row * d;
    float v[8];                                               // d <= 512 = 8 x 64
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + 64 * i;
        v[i] = f < d ? x[f] : 0.0f;
        s += v[i];
    }
    const float mean = gen_wave_sum(s) / (float)d;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float e = (lane + 64 * i < d) ? v[i] - mean : 0.0f;
        q += e * e;
    }
    const float rstd = 1.0f / sqrtf(gen_wave_sum(q) / (float)d + 1e-5f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + 64 * i;
        if (f < d) x[f] = (v[i] - mean) * rstd * gam[f] + bet[f];
    }
}

// ---- scaled dot-product attention of one (chunk, head) (layers.py:19-41, 64-88; no mask in predict), on the QKV rows
//      [row][3d] = q | k | v, head h at columns h*hd .. h*hd+hd-1 of each.  The result O overwrites Q in place (row t's Q is read
//      only by the wave that writes row t's O; K and V are untouched), so fc reads it with stride 3d.
//      4 waves, wave w takes the queries t = w, w+4, ...: scores with one lane per key, the row maximum and sum over the wave,
//      p = exp(s - max) / sum (torch.softmax), then P.V with the lanes split into 64/hp groups of keys x hp head dims (hp = hd
//      rounded up to a power of two, at most 64) and a reduction over the groups.  STAGE: K and V are copied into LDS first
//      (the host decides by size, gen_attn_lds_bytes against GEN_ATTN_STAGE_BYTES: always for 16 keys; while hd <= 38 for 250 keys,
//      <= 37 for 256, <= 76 for 128); otherwise they are read from the L2.
#define GEN_ATTN_STAGE_BYTES (80 * 1024)
__host__ __device__ constexpr size_t gen_attn_lds_bytes(int T, int hd, bool stage) {
    return ((stage ? (size_t)T * (2 * hd + 1) : 0) + 4 * (size_t)(hd + T)) * sizeof(float);
}
template <bool STAGE>
__global__ void __launch_bounds__(256) gen_attention_kernel(float* __restrict__ QKV, int d, int H, int T) {
    extern __shared__ float gen_lds[];
    const int hd = d / H, ld = 3 * d;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* base = QKV + (long long)b * T * ld + h * hd;
    // LDS: [K: T][hd + 1] [V: T][hd] (STAGE only) | per wave q [hd], p [T]
    float* kv = gen_lds;
    float* wq = gen_lds + (STAGE ? T * (2 * hd + 1) : 0) + wave * (hd + T);
    float* wp = wq + hd;
    const float* Kp; const float* Vp;
    int ks, vs;
    if (STAGE) {
        for (int i = threadIdx.x; i < T * hd; i += 256) {
            const int j = i / hd, e = i % hd;
            kv[j * (hd + 1) + e] = base[(long long)j * ld + d + e];
            kv[T * (hd + 1) + i] = base[(long long)j * ld + 2 * d + e];
        }
        __syncthreads();
        Kp = kv; ks = hd + 1; Vp = kv + T * (hd + 1); vs = hd;
    } else {
        Kp = base + d; ks = ld; Vp = base + 2 * d; vs = ld;
    }
    const float temp = sqrtf((float)hd);                       // temperature d_k ** 0.5 (layers.py:58)
    int hp = 1;
    while (hp < hd && hp < 64) hp <<= 1;
    const int ng = 64 / hp, dl = lane % hp, jg = lane / hp;
    for (int t = wave; t < T; t += 4) {
        float* qrow = base + (long long)t * ld;
        for (int e = lane; e < hd; e += 64) wq[e] = qrow[e];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float s[4];
        float mx = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            s[i] = -__builtin_inff();
            if (j < T) {
                const float* kr = Kp + (long long)j * ks;
                float a = 0.0f;
                for (int e = 0; e < hd; ++e) a += wq[e] * kr[e];
                s[i] = a / temp;
                mx = fmaxf(mx, s[i]);
            }
        }
        mx = gen_wave_max(mx);
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            s[i] = j < T ? expf(s[i] - mx) : 0.0f;
            sum += s[i];
        }
        sum = gen_wave_sum(sum);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            if (j < T) wp[j] = s[i] / sum;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int e0 = 0; e0 < hd; e0 += hp) {
            const int e = e0 + dl;
            float o = 0.0f;
            if (e < hd)
                for (int j = jg; j < T; j += ng) o += wp[j] * Vp[(long long)j * vs + e];
            for (int off = hp; off < 64; off <<= 1) o += __shfl_xor(o, off, 64);
            if (jg == 0 && e < hd) qrow[e] = o;
        }
        // (the next query's q / p stores follow this query's last reads of them in the wave's program order)
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- scaled dot-product attention of one (chunk, head) over more than 256 keys (the decoder of S2S_MODE_GENERIC_GEOMETRY at
//      max_signal_len > 256; gen_attention_kernel holds one query's scores as one register per key and lane, at most 256 keys),
//      on v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation.  One workgroup per (chunk, head, 64 queries), wave w
//      owning queries 16w .. 16w + 15 of the tile; no LDS -- K and V are read through the L1 / L2, which the four waves share.
//      Keys go 16 at a time, in two passes:
//        1. S^T = K Q^T / temperature (A = 16 keys x 4 head dims, B = 4 head dims x the wave's 16 queries), each query's exact
//           row maximum;
//        2. S^T again, p = exp(s - max), the row sum, and O^T += V^T P^T: lane (g, c) holds the scores of keys 4g + r of query c
//           in accumulator register r, so step r of the product takes register r as its B operand as it stands (its k-index g is
//           key 4g + r) and reads V in that key order as the A operand; then O = O^T^T / sum.
//      A two-pass softmax, as torch.softmax computes it: p is exp(s - max) with the exact row maximum and O is never rescaled;
//      the price is the score product done twice (an online softmax would rescale O once per new maximum, one more rounding
//      each time, against the exact-fp32 parity bound).  NT output tiles of 16 head dims, 16 NT >= hd (NT 1 | 8 | 32 for
//      hd <= 16 | 128 | 512); for NT = 1 the wave's four Q fragments stay in registers.  O overwrites Q in place,
//      as in gen_attention_kernel: query q's row is read only by the wave that owns it, and written after its last read.
template <int NT>
__global__ void __launch_bounds__(256) gen_attention_long_kernel(float* __restrict__ QKV, int d, int H, int T) {
    constexpr int QF = NT == 1 ? 4 : 0;                        // Q fragments held in registers (hd <= 16)
    const int nqt = (T + 63) / 64;
    const int b = blockIdx.x / (H * nqt), h = (blockIdx.x / nqt) % H, qt = blockIdx.x % nqt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int hd = d / H, ld = 3 * d;
    const int q0 = qt * 64 + wave * 16;
    if (q0 >= T) return;                                       // (no barriers below)
    float* base = QKV + (long long)b * T * ld + h * hd;
    const int q = q0 + c;                                      // this lane's query: B-operand and output column c
    const bool qin = q < T;
    const float* qrow = base + (long long)(qin ? q : T - 1) * ld;
    const float temp = sqrtf((float)hd);                       // temperature d_k ** 0.5 (layers.py:58)
    // Loads stay inside the chunk's rows and the head's columns by clamping the index; what a clamped load brings in is multiplied
    // by zero (a Q element past hd) or lands in an output row that is not stored (a V column past hd), and a key past T gets p = 0.
    float qf[QF > 0 ? QF : 1];
#pragma unroll
    for (int i = 0; i < QF; ++i) qf[i] = 4 * i + g < hd ? qrow[min(4 * i + g, hd - 1)] : 0.0f;
    auto scores = [&](int j0) {                                // lane (g, c), register r: key j0 + 4g + r, query c (unscaled)
        const float* krow = base + (long long)min(j0 + c, T - 1) * ld + d;   // A-operand row c: key j0 + c
        f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
        if (QF > 0) {
#pragma unroll
            for (int i = 0; i < QF; ++i)
                if (4 * i < hd) s = MFMA4(krow[min(4 * i + g, hd - 1)], qf[i], s);
        } else {
            for (int e0 = 0; e0 < hd; e0 += 4) {
                const int e = min(e0 + g, hd - 1);
                const float qv = qrow[e];
                s = MFMA4(krow[e], e0 + g < hd ? qv : 0.0f, s);
            }
        }
        return s;
    };
    float mx = -__builtin_inff();
    for (int j0 = 0; j0 < T; j0 += 16) {
        const f32x4 s = scores(j0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (j0 + 4 * g + r < T) mx = fmaxf(mx, s[r] / temp);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));                    // the four lanes of query c: c, c + 16, c + 32, c + 48
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float sum = 0.0f;
    const int nt = (hd + 15) / 16;
    for (int j0 = 0; j0 < T; j0 += 16) {
        const f32x4 s = scores(j0);
        float p[4];
        const float* vrow[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = j0 + 4 * g + r;
            p[r] = key < T ? expf(s[r] / temp - mx) : 0.0f;
            sum += p[r];
            vrow[r] = base + (long long)min(key, T - 1) * ld + 2 * d;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t < nt) {
                const int e = min(16 * t + c, hd - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t] = MFMA4(vrow[r][e], p[r], acc[t]);
            }
        }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (!qin) return;
    float* orow = base + (long long)q * ld;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = 16 * t + 4 * g + r;                  // acc[t][r] of lane (g, c) = O[query c][16t + 4g + r]
            if (e < hd) orow[e] = acc[t][r] / sum;
        }
}

// ---- the three heads' second layer (Linear(d,1) + Softplus, modules.py:182-195, 267-278) on the ReLU'd hidden rows
//      hid [row][3d] (noise | conc | rate), the dwell source (modules.py:396-438) and, on the same rows, + position_enc for the
//      encoder (modules.py:80).  One wave per encoder row (chunk b, position c).
struct GenHeads { long long w3[3], b3[3]; };
__global__ void __launch_bounds__(256) gen_dwell_kernel(const float* __restrict__ W, GenHeads hw, long long pe_enc, int d, int S,
                                                        const float* __restrict__ hid, float* __restrict__ X, float* __restrict__ sigma_out,
                                                        long long first_chunk, ParamsDev P, const float* __restrict__ inj_g,
                                                        const float* __restrict__ inj_zdw, int* __restrict__ out_dur, DebugDev dbg, int te) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)S * te) return;
    const int c = (int)(row % te);
    const unsigned long long chunk = (unsigned long long)(first_chunk + row / te);
    float hv[3] = {0.0f, 1.0f, 1.0f};
    const int nh = P.duration_sampling ? 3 : 1;
    for (int q = 0; q < nh; ++q) {
        float part = 0.0f;
        for (int f = lane; f < d; f += 64) part += hid[row * 3 * d + q * d + f] * W[hw.w3[q] + f];
        hv[q] = softplus_t(gen_wave_sum(part) + W[hw.b3[q]]);
    }
    float* xr = X + row * d;
    const float* pe = W + pe_enc + (long long)c * d;
    for (int f = lane; f < d; f += 64) xr[f] += pe[f];
    if (lane != 0) return;
    const long long drow = row;                               // (the caller's [B][te] arrays come offset to the slice)
    const float sg = hv[0];
    sigma_out[row] = sg;
    if (dbg.sigma) dbg.sigma[drow] = sg;
    float gv;
    if (P.duration_sampling) {
        const float conc = fmaxf(hv[1], 1e-8f), rate = fmaxf(hv[2], 1e-8f);   // modules.py:215-218
        if (dbg.conc) dbg.conc[drow] = conc;
        if (dbg.rate) dbg.rate[drow] = rate;
        if (inj_g) {
            gv = inj_g[drow];
        } else {
            const float s = standard_gamma(conc, (unsigned)chunk, (unsigned)(chunk >> 32), c, P.seed_lo, P.seed_hi);
            gv = fmaxf(s / rate, 1.17549435e-38f);           // Gamma.sample: /rate, clamp_(tiny)
        }
        gv = fmaxf(gv, 1.0f);                                // modules.py:223
        gv = fmaxf(gv, P.min_duration);                      // modules.py:414-416
    } else if (P.dwell_std <= 0.0f) {
        gv = P.dwell_mean;                                   // modules.py:420-423
    } else {
        float z;
        if (inj_zdw) {
            z = inj_zdw[drow];
        } else {
            const u32x4 r = philox4x32_10((unsigned)chunk, (unsigned)(chunk >> 32), c | (S2S_KIND_DWELL << 16), 0, P.seed_lo, P.seed_hi);
            z = box_muller(r.x, r.y);
        }
        gv = fmaxf(mul_then_add(z, P.dwell_std, P.dwell_mean), P.min_duration);   // modules.py:425-432
    }
    const float rd = fminf(fmaxf(rintf(gv), -1.0e9f), 1.0e9f);   // torch.round: half-to-even (modules.py:437)
    out_dur[drow] = (int)rd;
    if (dbg.g) dbg.g[drow] = gv;
}

// ---- length regulator (modules.py:344-392) as a gather: decoder row t copies encoder row i(t) = #{j : cum[j] <= t}, zero past
//      cum[te - 1], + position_enc (modules.py:136); sigma_ext likewise.  dec_in (nullable): the rows come from memory instead (the
//      stand-alone Decoder operator; it adds position_enc itself).  One thread per (row, feature group of 64).
__global__ void __launch_bounds__(256) gen_lenreg_kernel(const float* __restrict__ W, long long pe_dec, int d, int S,
                                                         const float* __restrict__ Xe, const float* __restrict__ sigma,
                                                         const int* __restrict__ dur, float* __restrict__ Xd, float* __restrict__ sig_ext,
                                                         const float* __restrict__ dec_in, int te, int ts) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)S * ts) return;
    const long long b = row / ts;
    const int t = (int)(row % ts);
    float* xo = Xd + row * d;
    if (dec_in) {
        for (int f = lane; f < d; f += 64) xo[f] = dec_in[row * d + f];
        return;
    }
    int idx = 0, run = 0;
    for (int j = 0; j < te; ++j) {                            // a dwell past the crop at ts (modules.py:386) acts like ts + 1
        const int dj = dur[b * te + j];
        run += dj < ts + 1 ? dj : ts + 1;
        idx += run <= t ? 1 : 0;
    }
    const bool live = idx < te;
    const float* er = Xe + (b * te + (live ? idx : 0)) * d;
    const float* pe = W + pe_dec + (long long)t * d;
    for (int f = lane; f < d; f += 64) xo[f] = (live ? er[f] : 0.0f) + pe[f];
    if (lane == 0) sig_ext[row] = live ? sigma[b * te + idx] : 0.0f;
}

// ---- out_linear + ReLU (modules.py:140-141), x scale (model.py:221), noise where != 0 (model.py:224-238), clamp (model.py:240).
//      One wave per decoder row.
__global__ void __launch_bounds__(256) gen_emit_kernel(const float* __restrict__ W, long long out_w, long long out_b, float scale, int d, int S,
                                                       const float* __restrict__ Xd, const float* __restrict__ sig_ext,
                                                       long long first_chunk, ParamsDev P, const float* __restrict__ inj_z01,
                                                       float* __restrict__ out_signal, DebugDev dbg, int ts) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)S * ts) return;
    const int t = (int)(row % ts);
    const unsigned long long chunk = (unsigned long long)(first_chunk + row / ts);
    float part = 0.0f;
    for (int f = lane; f < d; f += 64) part += Xd[row * d + f] * W[out_w + f];
    const float ys = relu1(gen_wave_sum(part) + W[out_b]);
    if (lane != 0) return;
    if (dbg.y_scaled) dbg.y_scaled[row] = ys;
    float y = __fmul_rn(ys, scale);
    if (P.noise_std > 0.0f) {
        float z;
        if (inj_z01) {
            z = inj_z01[row];
        } else {
            const u32x4 r = philox4x32_10((unsigned)chunk, (unsigned)(chunk >> 32), (unsigned)t | (S2S_KIND_NOISE << 16), 0, P.seed_lo, P.seed_hi);
            z = box_muller(r.x, r.y);
        }
        if (dbg.z01) dbg.z01[row] = z;
        const float sd = P.noise_sampling ? __fmul_rn(__fmul_rn(fmaxf(sig_ext[row], P.min_noise), P.noise_std), scale) : P.noise_std;
        if (y != 0.0f) y = mul_then_add(z, sd, y);
    }
    out_signal[row] = fmaxf(y, 0.0f);
}

// ---- s2s_evaluate_chunks (teacher forcing, modules.py:434-435) on this pipeline: three kernels take the place of gen_embed_kernel,
//      gen_dwell_kernel and gen_emit_kernel; gen_lenreg_kernel reads the measured dwell counts as they are.
// src_emb of a preprocess chunk: letter j of k-mer (b, c) at kmers[(b * te + c) * k + j], every position counts.  One thread per
// (row, feature), the k columns added in k order as in gen_embed_kernel.
__global__ void __launch_bounds__(256) gen_embed_kmers_kernel(const float* __restrict__ emb_wt, const float* __restrict__ emb_b, int k, int d,
                                                              const uint8_t* __restrict__ kmers, int S, int te, float* __restrict__ X) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)S * te * d) return;
    const int f = (int)(i % d);
    const long long row = i / d;
    const uint8_t* kp = kmers + row * k;
    float x = emb_b[f];
    for (int j = 0; j < k; ++j) {
        const int code = gen_base_code(kp[j]);
        if (code >= 0) x += emb_wt[(long long)(5 * j + code) * d + f];        // unknown letter: all-zero one-hot row (utils.py:86)
    }
    X[i] = relu1(x);
}

// gen_dwell_kernel's heads and + position_enc without a dwell source: sigma, and conc / rate clamped at 1e-8 (modules.py:215-218),
// whatever a predict call would sample.  One wave per encoder row.
__global__ void __launch_bounds__(256) gen_dwell_teacher_kernel(const float* __restrict__ W, GenHeads hw, long long pe_enc, int d, int S,
                                                                const float* __restrict__ hid, float* __restrict__ X,
                                                                float* __restrict__ sigma_out, float* __restrict__ conc_out,
                                                                float* __restrict__ rate_out, int te) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)S * te) return;
    const int c = (int)(row % te);
    float hv[3];
    for (int q = 0; q < 3; ++q) {
        float part = 0.0f;
        for (int f = lane; f < d; f += 64) part += hid[row * 3 * d + q * d + f] * W[hw.w3[q] + f];
        hv[q] = softplus_t(gen_wave_sum(part) + W[hw.b3[q]]);
    }
    float* xr = X + row * d;
    const float* pe = W + pe_enc + (long long)c * d;
    for (int f = lane; f < d; f += 64) xr[f] += pe[f];
    if (lane != 0) return;
    sigma_out[row] = hv[0];
    conc_out[row] = fmaxf(hv[1], 1e-8f);
    rate_out[row] = fmaxf(hv[2], 1e-8f);
}

// out_linear + ReLU (modules.py:140-141): the decoder output y in scaled units, no scale, noise or clamp.  One wave per decoder row.
__global__ void __launch_bounds__(256) gen_emit_y_kernel(const float* __restrict__ W, long long out_w, long long out_b, int d, int S,
                                                         const float* __restrict__ Xd, float* __restrict__ y, int ts) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)S * ts) return;
    float part = 0.0f;
    for (int f = lane; f < d; f += 64) part += Xd[row * d + f] * W[out_w + f];
    const float ys = relu1(gen_wave_sum(part) + W[out_b]);
    if (lane == 0) y[row] = ys;
}
