// s2s_train.h -- device code of the trainer (s2s_trainer_*, include/s2s_hip.h), included by s2s_hip.hip: the backward pass of the
// size-generic fp32 instance, the global gradient norm and the Adam / AdamW step.  The forward pass is s2s_generic.h's, kernel for
// kernel as s2s_evaluate_chunks runs it, with every layer writing into buffers of its own (the tape, s2s_train_host.h).
//
// Exact fp32, plain FMA (no MFMA yet), no float atomics: every sum over rows is formed as per-tile partials in row order and one
// ordered pass over the tiles, so a call's result depends on its inputs, B and the memory budget only.
//   train_mm_kernel<LT, EPI>     C[i][j] = sum_r L(r, i) R[r][j] on 64 x 64 tiles, 4 x 4 outputs per thread:
//                                LT = false: L[r][i] -- weight gradients dW[n][k] = sum_rows dY[row][n] X[row][k], rows split over
//                                            gridDim.z into TR_GRAD_ROWS-row partials;
//                                LT = true:  L[i][r] -- input gradients dX = dY W on nn.Linear's native [out][in] weight
//                                            (gen_gemm_kernel wants W^T for this product, hence the sibling);
//                                EPI 0: store; 1: x (E > 0), the ReLU mask of the activation E; 2: + E, the residual branch
//   train_colsum_kernel          bias / gamma / beta gradients: column sums of a row tile
//   train_reduce_kernel          grad[i] += sum over the tiles' partials, in tile order
//   train_layernorm_bwd_kernel   one row per wave: mean and rstd recomputed from the pre-LayerNorm sum as the forward pass forms them
//   train_attention_bwd_kernel   one workgroup per (chunk, head); the probabilities are recomputed from Q and K (below)
//   train_lenreg_bwd_kernel      segment sum of the decoder-input gradient over each k-mer's samples, one wave per (chunk, k-mer)
//   train_heads_bwd_kernel       the three heads' Linear(d,1) + Softplus + clamp and the Gamma / noise loss gradients
//   train_emit_bwd_kernel        signal loss gradient through out_linear's ReLU
//   train_sumsq_kernel / train_norm_kernel   global L2 norm: per-block partials (double), then one ordered pass; clip scale
//   train_adam_kernel            Adam (coupled L2) / AdamW (decoupled) with the clip scale read from device memory
//
// digamma (train_digamma): psi(x) = psi(x + 1) - 1/x until x >= 6, then the asymptotic series
// ln x - 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) + 1/(240x^8) - 1/(132x^10), in double (truncation below 3e-12 at x = 6).
//
// Attention backward, per (chunk, head) with T keys and head_dim hd, S = Q K^T / sqrt(hd), P = softmax(S):
//   dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dP o P)), dQ = dS K / sqrt(hd), dK = dS^T Q / sqrt(hd)
// in two phases of one wave per row, 4 waves: phase A takes a query (scores, softmax as gen_attention_kernel forms it, dS, dQ, and
// the row's max / sum / rowsum into LDS), phase B takes a key (the same scores and probabilities again from the stored row
// statistics, then dK and dV).  T <= 1024, hd <= 512.  Static LDS: 3 x 1024 row statistics + per wave 2 x 512 (the row's two vectors)
// + 2 x 1024 (its p and dS) floats = TRAIN_ATTN_LDS_BYTES = 61,440 B.
#pragma once
#include "s2s_generic.h"

#define TR_TILE 64
#define TR_RK 16
#define TR_LDT (TR_TILE + 4)
#define TR_GRAD_ROWS 512        // rows per weight-gradient partial
#define TRAIN_ATTN_MAX_T 1024
#define TRAIN_ATTN_MAX_HD 512
#define TRAIN_ATTN_LDS_BYTES ((3 * TRAIN_ATTN_MAX_T + 4 * (2 * TRAIN_ATTN_MAX_HD + 2 * TRAIN_ATTN_MAX_T)) * 4)

template <bool LT, int EPI>
__global__ void __launch_bounds__(256) train_mm_kernel(const float* __restrict__ L, int ldl, const float* __restrict__ R, int ldr,
                                                       float* C, int ldc, const float* E, int lde, int I, int J, int Rn,
                                                       int rows_per_z) {
    __shared__ float Ls[TR_RK][TR_LDT];
    __shared__ float Rs[TR_RK][TR_LDT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long i0 = (long long)blockIdx.x * TR_TILE;
    const int j0 = blockIdx.y * TR_TILE;
    const int r_lo = blockIdx.z * rows_per_z;
    const int r_hi = min(Rn, r_lo + rows_per_z);
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
    for (int r0 = r_lo; r0 < r_hi; r0 += TR_RK) {
        float lv[4], rv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q;
            {
                const int r = LT ? (idx & 15) : (idx >> 6), i = LT ? (idx >> 4) : (idx & 63);
                const bool in = r0 + r < r_hi && i0 + i < I;
                lv[q] = in ? (LT ? L[(i0 + i) * ldl + r0 + r] : L[(long long)(r0 + r) * ldl + i0 + i]) : 0.0f;
            }
            {
                const int r = idx >> 6, j = idx & 63;
                rv[q] = (r0 + r < r_hi && j0 + j < J) ? R[(long long)(r0 + r) * ldr + j0 + j] : 0.0f;
            }
        }
        __syncthreads();                                      // the previous step's reads are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q;
            if (LT) Ls[idx & 15][idx >> 4] = lv[q]; else Ls[idx >> 6][idx & 63] = lv[q];
            Rs[idx >> 6][idx & 63] = rv[q];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TR_RK; ++r) {
            float a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { a[q] = Ls[r][4 * ty + q]; b[q] = Rs[r][4 * tx + q]; }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] += a[x] * b[y];
        }
    }
    float* Cz = C + (long long)blockIdx.z * I * ldc;          // (partials [z][I][J]; gridDim.z == 1 otherwise)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const long long i = i0 + 4 * ty + x;
        if (i >= I) continue;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int j = j0 + 4 * tx + y;
            if (j >= J) continue;
            float v = acc[x][y];
            if (EPI == 1) v = E[i * lde + j] > 0.0f ? v : 0.0f;
            if (EPI == 2) v += E[i * lde + j];
            Cz[i * ldc + j] = v;
        }
    }
}

// part[z][n] = sum of A[row][n] over the z-th tile of rows_per_z rows: 64 columns x 4 row lanes per workgroup, lane s taking the
// tile's rows s, s + 4, ... in order, the four lanes added in order.
__global__ void __launch_bounds__(256) train_colsum_kernel(const float* __restrict__ A, int lda, int M, int N, int rows_per_z,
                                                           float* __restrict__ part) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int r_lo = blockIdx.y * rows_per_z, r_hi = min(M, r_lo + rows_per_z);
    float acc = 0.0f;
    if (n < N)
        for (int r = r_lo + s; r < r_hi; r += 4) acc += A[(long long)r * lda + n];
    red[s][c] = acc;
    __syncthreads();
    if (s == 0 && n < N) part[(long long)blockIdx.y * N + n] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

__global__ void __launch_bounds__(256) train_reduce_kernel(const float* __restrict__ part, int nz, long long n, float* __restrict__ grad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int z = 0; z < nz; ++z) s += part[z * n + i];
    grad[i] += s;
}

__global__ void __launch_bounds__(256) train_copy_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd,
                                                         long long M, int n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * n) return;
    dst[(i / n) * ldd + i % n] = src[(i / n) * lds + i % n];
}

// dst = act > 0 ? src : 0 (ReLU' at exactly 0 is 0, as in torch); dst may be src
__global__ void __launch_bounds__(256) train_relu_mask_kernel(const float* src, const float* __restrict__ act, float* dst, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = act[i] > 0.0f ? src[i] : 0.0f;
}

// the one-hot k-mer rows [Me][ld] (ld >= 5k, the tail zero) src_emb multiplies: an unknown letter is an all-zero group
__global__ void __launch_bounds__(256) train_onehot_kernel(const uint8_t* __restrict__ kmers, int k, long long Me, int ld,
                                                           float* __restrict__ OH) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Me * ld) return;
    const int col = (int)(i % ld);
    const long long row = i / ld;
    OH[i] = (col < 5 * k && gen_base_code(kmers[row * k + col / 5]) == col % 5) ? 1.0f : 0.0f;
}

// ---- nn.LayerNorm backward on the pre-LayerNorm rows P: dX = rstd (g - mean(g) - xhat mean(g xhat)), g = dY gamma; G = dY xhat
//      (its column sums are dgamma; dbeta is dY's).  One wave per row; dX may be dY (a lane reads its own elements first).
__global__ void __launch_bounds__(256) train_layernorm_bwd_kernel(const float* __restrict__ P, const float* dY, const float* __restrict__ gam,
                                                                  float* dX, float* __restrict__ G, long long M, int d) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* x = P + row * d;
    float v[8], g[8], dy[8];
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
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + 64 * i;
        v[i] = f < d ? (v[i] - mean) * rstd : 0.0f;          // xhat
        dy[i] = f < d ? dY[row * d + f] : 0.0f;
        g[i] = f < d ? dy[i] * gam[f] : 0.0f;
        s1 += g[i];
        s2 += g[i] * v[i];
    }
    s1 = gen_wave_sum(s1) / (float)d;
    s2 = gen_wave_sum(s2) / (float)d;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + 64 * i;
        if (f < d) {
            dX[row * d + f] = rstd * (g[i] - s1 - v[i] * s2);
            G[row * d + f] = dy[i] * v[i];
        }
    }
}

// ---- attention backward of one (chunk, head) (the header comment).  Qc [row][d] is the tape's copy of Q (the forward pass writes
//      O over Q), K and V come from QKV [row][3d], dO [row][d]; dQKV [row][3d] gets dq | dk | dv at the head's columns.
__device__ __forceinline__ void train_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__global__ void __launch_bounds__(256) train_attention_bwd_kernel(const float* __restrict__ Qc, const float* __restrict__ QKV,
                                                                  const float* __restrict__ dO, float* __restrict__ dQKV, int d, int H, int T) {
    __shared__ float stat[3][TRAIN_ATTN_MAX_T];               // row max, row sum, rowsum(dP o P)
    __shared__ float wbuf[4][2 * TRAIN_ATTN_MAX_HD + 2 * TRAIN_ATTN_MAX_T];
    const int hd = d / H, ld = 3 * d;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)b * T;
    const float* Qp = Qc + r0 * d + h * hd;
    const float* dOp = dO + r0 * d + h * hd;
    const float* Kp = QKV + r0 * ld + d + h * hd;
    const float* Vp = Kp + d;
    float* dQp = dQKV + r0 * ld + h * hd;
    float* wa = wbuf[wave];                                   // the row's first vector (q | k)
    float* wb = wa + TRAIN_ATTN_MAX_HD;                       // its second (dO | v)
    float* wp = wb + TRAIN_ATTN_MAX_HD;                       // p over the other side's rows
    float* wd = wp + TRAIN_ATTN_MAX_T;                        // dP, then dS
    const float temp = sqrtf((float)hd);
    int hp = 1;
    while (hp < hd && hp < 64) hp <<= 1;
    const int ng = 64 / hp, dl = lane % hp, jg = lane / hp;
    // phase A: one query per wave
    for (int t = wave; t < T; t += 4) {
        for (int e = lane; e < hd; e += 64) { wa[e] = Qp[(long long)t * d + e]; wb[e] = dOp[(long long)t * d + e]; }
        train_wave_sync();
        float mx = -__builtin_inff();
        for (int j = lane; j < T; j += 64) {
            const float* kr = Kp + (long long)j * ld;
            const float* vr = Vp + (long long)j * ld;
            float a = 0.0f, c = 0.0f;
            for (int e = 0; e < hd; ++e) { a += wa[e] * kr[e]; c += wb[e] * vr[e]; }
            a = a / temp;
            wp[j] = a; wd[j] = c;
            mx = fmaxf(mx, a);
        }
        mx = gen_wave_max(mx);
        float sum = 0.0f;
        for (int j = lane; j < T; j += 64) { const float p = expf(wp[j] - mx); wp[j] = p; sum += p; }
        sum = gen_wave_sum(sum);
        float D = 0.0f;
        for (int j = lane; j < T; j += 64) D += (wp[j] / sum) * wd[j];
        D = gen_wave_sum(D);
        for (int j = lane; j < T; j += 64) wd[j] = (wp[j] / sum) * (wd[j] - D);
        if (lane == 0) { stat[0][t] = mx; stat[1][t] = sum; stat[2][t] = D; }
        train_wave_sync();
        for (int e0 = 0; e0 < hd; e0 += hp) {
            const int e = e0 + dl;
            float o = 0.0f;
            if (e < hd)
                for (int j = jg; j < T; j += ng) o += wd[j] * Kp[(long long)j * ld + e];
            for (int off = hp; off < 64; off <<= 1) o += __shfl_xor(o, off, 64);
            if (jg == 0 && e < hd) dQp[(long long)t * ld + e] = o / temp;
        }
        train_wave_sync();
    }
    __syncthreads();
    // phase B: one key per wave
    for (int j = wave; j < T; j += 4) {
        for (int e = lane; e < hd; e += 64) { wa[e] = Kp[(long long)j * ld + e]; wb[e] = Vp[(long long)j * ld + e]; }
        train_wave_sync();
        for (int t = lane; t < T; t += 64) {
            const float* qr = Qp + (long long)t * d;
            const float* gr = dOp + (long long)t * d;
            float a = 0.0f, c = 0.0f;
            for (int e = 0; e < hd; ++e) { a += qr[e] * wa[e]; c += gr[e] * wb[e]; }
            const float p = expf(a / temp - stat[0][t]) / stat[1][t];
            wp[t] = p;
            wd[t] = p * (c - stat[2][t]);
        }
        train_wave_sync();
        for (int e0 = 0; e0 < hd; e0 += hp) {
            const int e = e0 + dl;
            float ok = 0.0f, ov = 0.0f;
            if (e < hd)
                for (int t = jg; t < T; t += ng) {
                    ok += wd[t] * Qp[(long long)t * d + e];
                    ov += wp[t] * dOp[(long long)t * d + e];
                }
            for (int off = hp; off < 64; off <<= 1) { ok += __shfl_xor(ok, off, 64); ov += __shfl_xor(ov, off, 64); }
            if (jg == 0 && e < hd) {
                dQp[(long long)j * ld + d + e] = ok / temp;
                dQp[(long long)j * ld + 2 * d + e] = ov;
            }
        }
        train_wave_sync();
    }
}

// ---- length regulator backward: k-mer (b, j) owns the samples cum[j-1] <= t < min(cum[j], ts) (gen_lenreg_kernel's cropped running
//      sum); its gradient is their sum in t order, zero for a dwell of 0 or a k-mer past the crop.  One wave per (chunk, k-mer).
__global__ void __launch_bounds__(256) train_lenreg_bwd_kernel(const float* __restrict__ dXd, const int* __restrict__ dur, float* __restrict__ dXe,
                                                               long long Me, int d, int te, int ts) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= Me) return;
    const long long b = row / te;
    const int j = (int)(row % te);
    int lo = 0;
    for (int i = 0; i < j; ++i) { const int di = dur[b * te + i]; lo += di < ts + 1 ? di : ts + 1; }
    const int dj = dur[b * te + j];
    int hi = lo + (dj < ts + 1 ? dj : ts + 1);
    if (hi > ts) hi = ts;
    if (lo < 0) lo = 0;                                       // (dwell >= 0 is the entry's precondition; a negative one reads nothing out of range)
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
    for (int t = lo; t < hi; ++t) {
        const float* g = dXd + (b * ts + t) * d;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int f = lane + 64 * i;
            if (f < d) acc[i] += g[f];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + 64 * i;
        if (f < d) dXe[row * d + f] = acc[i];
    }
}

__device__ __forceinline__ double train_digamma(double x) {
    double r = 0.0;
    while (x < 6.0) { r -= 1.0 / x; x += 1.0; }
    const double i2 = 1.0 / (x * x);
    return r + log(x) - 0.5 / x - i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0)))));
}

// ---- the heads' backward (model.py:458-475, modules.py:182-225, 267-278) on the ReLU'd hidden rows hid [row][3d]: the pre-activation
//      z of each Linear(d,1) again as gen_dwell_teacher_kernel forms it, then
//        dsigma = c_noise (sigma - stdev); dconc = c_dur (digamma(conc) - ln rate - ln x); drate = c_dur (x - conc / rate),
//      x = max(|dwell|, 1), the last two zero where the clamp at 1e-8 is active; dz = . x softplus'(z) (the sigmoid; 1 above the
//      threshold of 20).  c_noise = 2 / (B te), c_dur = 0.0005 / (B te) of the whole batch.  DZ [row][4] gets dz, dHid [row][3d]
//      the gradient at the first layers' pre-activations (ReLU mask applied).  One wave per encoder row.
__global__ void __launch_bounds__(256) train_heads_bwd_kernel(const float* __restrict__ W, GenHeads hw, int d, long long Me,
                                                              const float* __restrict__ hid, const float* __restrict__ stdev,
                                                              const int* __restrict__ dwell, float c_noise, float c_dur,
                                                              float* __restrict__ DZ, float* __restrict__ dHid) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= Me) return;
    float z[3], hv[3];
    for (int q = 0; q < 3; ++q) {
        float part = 0.0f;
        for (int f = lane; f < d; f += 64) part += hid[row * 3 * d + q * d + f] * W[hw.w3[q] + f];
        z[q] = gen_wave_sum(part) + W[hw.b3[q]];
        hv[q] = softplus_t(z[q]);
    }
    const int dv = dwell[row];
    const double x = dv == 0 ? 1.0 : (double)(dv < 0 ? -dv : dv);
    const double conc = fmaxf(hv[1], 1e-8f), rate = fmaxf(hv[2], 1e-8f);
    float dh[3];
    dh[0] = c_noise * (hv[0] - stdev[row]);
    dh[1] = hv[1] >= 1e-8f ? (float)((double)c_dur * (train_digamma(conc) - log(rate) - log(x))) : 0.0f;
    dh[2] = hv[2] >= 1e-8f ? (float)((double)c_dur * (x - conc / rate)) : 0.0f;
    for (int q = 0; q < 3; ++q) {
        const float sg = z[q] > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-z[q]));
        const float dz = dh[q] * sg;
        if (lane == 0) DZ[row * 4 + q] = dz;
        for (int f = lane; f < d; f += 64) {
            const long long i = row * 3 * d + q * d + f;
            dHid[i] = hid[i] > 0.0f ? dz * W[hw.w3[q] + f] : 0.0f;
        }
    }
    if (lane == 0) DZ[row * 4 + 3] = 0.0f;
}

// ---- signal loss through out_linear + ReLU: dy = c_sig (y - target) where y > 0 (c_sig = 2 / (B ts) of the whole batch);
//      DY [row] = dy, dXd [row][f] = dy out_w[f].  One wave per decoder row.
__global__ void __launch_bounds__(256) train_emit_bwd_kernel(const float* __restrict__ W, long long out_w, int d, long long Md,
                                                             const float* __restrict__ y, const float* __restrict__ target, float c_sig,
                                                             float* __restrict__ DY, float* __restrict__ dXd) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= Md) return;
    const float yv = y[row];
    const float dy = yv > 0.0f ? c_sig * (yv - target[row]) : 0.0f;
    if (lane == 0) DY[row] = dy;
    for (int f = lane; f < d; f += 64) dXd[row * d + f] = dy * W[out_w + f];
}

// ---- global L2 norm of the gradient: block b sums the squares of its 2048 elements (a thread its 8 in index order, the threads in
//      a fixed tree), double; train_norm_kernel (one workgroup) adds the blocks' partials the same way and writes
//      stats[4] = the norm, stats[5] = the clip scale: clip / (norm + 1e-6) where clip > 0 and norm > clip, else 1 (clip_grad_norm_).
__device__ __forceinline__ double train_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}
__global__ void __launch_bounds__(256) train_sumsq_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
    __shared__ double red[256];
    double s = 0.0;
    for (int q = 0; q < 8; ++q) {
        const long long i = (long long)blockIdx.x * 2048 + threadIdx.x + 256 * q;
        if (i < n) s += (double)g[i] * (double)g[i];
    }
    s = train_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void __launch_bounds__(256) train_norm_kernel(const double* __restrict__ part, int nb, float clip, float* __restrict__ stats) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
    s = train_block_sum(s, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        stats[4] = norm;
        stats[5] = (clip > 0.0f && norm > clip) ? clip / (norm + 1e-6f) : 1.0f;
    }
}

// the batch's loss means from the per-chunk sums, in chunk order (double): stats[0..3] = signal, duration x 0.0005, noise, total
__global__ void train_loss_stats_kernel(const float* __restrict__ per_chunk, int B, int te, int ts, float* __restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < 3; ++q) s[q] += (double)per_chunk[b * 3 + q];
    const double a = s[0] / ((double)B * ts), c = 0.0005 * s[1] / ((double)B * te), e = s[2] / ((double)B * te);
    stats[0] = (float)a; stats[1] = (float)c; stats[2] = (float)e; stats[3] = (float)(a + c + e);
}

// ---- one optimizer step on w[lo .. hi) (torch.optim.Adam / AdamW, single-tensor form): g = grad x clip scale (stats[5]);
//      coupled: g += wd w; decoupled: w *= 1 - lr wd; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
//      w -= step_size m / (sqrt(v) / sqrt(bias2) + eps), step_size = lr / bias1.  1 - b1 and 1 - b2 (omb1, omb2) are formed in
//      double and rounded once, as torch passes them to lerp_ / addcmul_: 1 - fp32(0.999) is 1.3e-5 away from 0.001.
struct TrainAdam { float lr, b1, b2, omb1, omb2, eps, wd, step_size, bias2_sqrt; int decoupled; };
__global__ void __launch_bounds__(256) train_adam_kernel(float* __restrict__ w, const float* __restrict__ grad, float* __restrict__ m,
                                                         float* __restrict__ v, long long lo, long long hi, TrainAdam A,
                                                         const float* __restrict__ stats) {
    const long long i = lo + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hi) return;
    float g = grad[i] * stats[5];
    float wv = w[i];
    if (A.decoupled) wv *= 1.0f - A.lr * A.wd; else if (A.wd != 0.0f) g += A.wd * wv;
    const float mv = A.b1 * m[i] + A.omb1 * g;
    const float vv = A.b2 * v[i] + A.omb2 * g * g;
    m[i] = mv; v[i] = vv;
    w[i] = wv - A.step_size * (mv / (sqrtf(vv) / A.bias2_sqrt + A.eps));
}

// out[i] = src[map[i]]: the trainer's arena (the generic handle's packing: aligned pieces, src_emb transposed) read in blob order
__global__ void __launch_bounds__(256) train_gather_kernel(const float* __restrict__ src, const int* __restrict__ map, long long n,
                                                           float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = src[map[i]];
}
