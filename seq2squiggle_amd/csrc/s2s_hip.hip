// s2s_hip.hip -- kernels and C ABI (include/s2s_hip.h) of the MI355X-native seq2squiggle
// predict path.  gfx950 only; no fallbacks.
//
// One launch per tile of chunks, s2s_fused_kernel: persistent 8-wave workgroups, each walking its share of the chunks in
// groups of 16:
//   frontend   wave w, two chunks at a time: k-mer embedding gather, pre-net, the noise / duration heads, Philox Gamma or
//              Normal dwell, encoder FFT blocks -> enc_out, sigma, dur in the workgroup's L2-resident hand-off slots
//   decoder    all 8 waves, one chunk after the other: length-regulator gather + positional add, decoder FFT blocks
//              (T = 250 padded to 256; 32 time columns per wave), output projection, x165, Philox noise, clamp -> signal[250]
// plus s2s_export_* for the per-read zero-strip / int16 conversion and s2s_svb_* for the containers' signal codecs.
#include "s2s_device.h"
#include "s2s_device_h.h"
#include "s2s_schedule.h"
#include "s2s_generic.h"
#include "s2s_generic_h.h"
#include "s2s_train.h"
#include "../../include/s2s_hip.h"
#include "s2s_event_fixed.h"
#define S2S_DTW_KERNELS
#include "s2s_dtw.h"
#include "s2s_sdtw.h"
#include "s2s_resquiggle.h"
#include "s2s_prims.h"
#include "s2s_segment.h"
#include "s2s_eventalign.h"
#include "s2s_chunk.h"
#include "s2s_kmer_model_events.h"

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <immintrin.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>

// ================================================================================ frontend
// The frontend of a chunk is run by ONE wave (T = 16: every chunk is a single time tile and a sequence of its own): embedding,
// pre-net, the three heads and the dwell source, encoder blocks.  Two chunks per wave (f16x3) give the in-order wave two
// independent dependency chains to interleave; the eight waves of the workgroup work side by side on different chunks.
template <int NQ>
__device__ __forceinline__ void relu_tiles(f32x4 (&x)[NQ][4]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) x[q][mt][r] = relu1(x[q][mt][r]);
}

__device__ __forceinline__ int base_code(unsigned char ch) {       // utils.py:74 letter_to_int
    return ch == 'A' ? 1 : ch == 'C' ? 2 : ch == 'G' ? 3 : ch == 'T' ? 4 : ch == '_' ? 0 : -1;
}

// One chunk as the frontend sees it.  bp: its 16+k-1 bases; inj_g / inj_zdw: its 16 injected variates (or null); slot: where
// the decoder picks it up -- enc_out [16][64], sigma [16] at +1024, dur [16] (int32) at +1040; out_dur: the caller's [16] row;
// dbg_idx: its row in the debug arrays; live = false: a filler (an odd chunk count), computed and thrown away.
// s2s_eval_kernel (EVAL = true): bp is the chunk's [16][k] k-mer letters and out_dur its [16] measured dwell counts (read, not
// written); nv is unused.
struct FrontChunk {
    const uint8_t* bp;
    int nv;
    unsigned long long chunk;
    const float* inj_g;
    const float* inj_zdw;
    float* slot;
    int* out_dur;
    long long dbg_idx;
    bool live;
};
#define S2S_SLOT_FLOATS S2S_PF_FLOATS

// ---- src_emb on the one-hot k-mer == bias + sum of k gathered columns of W_emb, then ReLU (modules.py:70-73).  EVAL: letter j
//      of k-mer c at bp[c * k + j] (independent k-mers of a preprocess chunk), every position counts
template <int NQ, bool EVAL = false>
__device__ __forceinline__ void front_embed(const ModelDev& M, const float* __restrict__ W, const FrontChunk (&io)[NQ], const int lane,
                                            f32x4 (&X)[NQ][4]) {
    const int g = lane >> 4, c = lane & 15;
    f32x4 eb[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) eb[ft] = ldg4(W + M.emb_b + 16 * ft + 4 * g);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) X[q][ft] = eb[ft];
    for (int j = 0; j < M.k; ++j) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int code = EVAL ? base_code(io[q].bp[c * M.k + j])
                                  : (c < io[q].nv) ? base_code(io[q].bp[c + j]) : 0;   // pad k-mer = "_" * k (utils.py:342-347)
            const float* row = W + M.emb_wt + (5 * j + (code < 0 ? 0 : code)) * 64 + 4 * g;
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                const f32x4 w = ldg4(row + 16 * ft);
                if (code >= 0) X[q][ft] += w;                        // unknown letter: all-zero one-hot row (utils.py:86)
            }
        }
    }
    relu_tiles<NQ>(X);
}

// ---- second layer of a head: Linear(64,1) + Softplus on the ReLU'd hidden tile (modules.py:267-278, 182-195)
template <int NQ>
__device__ __forceinline__ void head_out(const float* __restrict__ W, const MlpOff m, f32x4 (&hid)[NQ][4], const int lane, float (&out)[NQ]) {
    const int g = lane >> 4;
    relu_tiles<NQ>(hid);
    f32x4 w[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) w[mt] = ldg4(W + m.w3 + 16 * mt + 4 * g);
    const float b3 = W[m.b3];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        float part = 0.0f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) part += hid[q][mt][r] * w[mt][r];
        out[q] = softplus_t(sum_g(part) + b3);
    }
}

// ---- the dwell source (modules.py:396-438) and the sigma / dur stores, given the heads' values.  Every lane group holds the
//      heads' values of all tiles (sum_g is an all-reduce), so lane group q finishes chunk q: ONE pass of the sampler per wave.
//      EVAL (teacher forcing, modules.py:434-435): conc / rate clamped and stored, the measured dwell goes to the slot, no sampler.
template <int NQ, bool EVAL = false>
__device__ __forceinline__ void front_dwell(const FrontChunk (&io)[NQ], const ParamsDev& P, const float (&sig)[NQ], const float (&cq)[NQ],
                                            const float (&rq)[NQ], const DebugDev& dbg, const int lane) {
    const int g = lane >> 4, c = lane & 15;
    float sigma = sig[0], conc = cq[0], rate = rq[0];
    FrontChunk me = io[0];
#pragma unroll
    for (int q = 1; q < NQ; ++q)
        if (g == q) { sigma = sig[q]; conc = cq[q]; rate = rq[q]; me = io[q]; }
    const bool mine = g < NQ && me.live;
    if (mine) {
        me.slot[1024 + c] = sigma;
        if (dbg.sigma) dbg.sigma[me.dbg_idx * 16 + c] = sigma;
    }
    if constexpr (EVAL) {
        if (mine) {
            dbg.conc[me.dbg_idx * 16 + c] = fmaxf(conc, 1e-8f);          // modules.py:215-218
            dbg.rate[me.dbg_idx * 16 + c] = fmaxf(rate, 1e-8f);
            reinterpret_cast<int*>(me.slot + 1040)[c] = me.out_dur[c];
        }
        return;
    }
    float gv;
    if (P.duration_sampling) {
        conc = fmaxf(conc, 1e-8f);                                   // modules.py:215-216
        rate = fmaxf(rate, 1e-8f);                                   // modules.py:217-218
        if (mine) {
            if (dbg.conc) dbg.conc[me.dbg_idx * 16 + c] = conc;
            if (dbg.rate) dbg.rate[me.dbg_idx * 16 + c] = rate;
        }
        if (me.inj_g) {
            gv = mine ? me.inj_g[c] : 1.0f;
        } else {
            float sg = 0.0f;
            if (mine) sg = standard_gamma(conc, (unsigned)me.chunk, (unsigned)(me.chunk >> 32), c, P.seed_lo, P.seed_hi);
            gv = fmaxf(sg / rate, 1.17549435e-38f);                 // Gamma.sample: /rate, clamp_(tiny)
        }
        gv = fmaxf(gv, 1.0f);                                       // modules.py:223
        gv = fmaxf(gv, P.min_duration);                             // modules.py:414-416
    } else if (P.dwell_std <= 0.0f) {
        gv = P.dwell_mean;                                          // modules.py:420-423
    } else {
        float z;
        if (me.inj_zdw) {
            z = mine ? me.inj_zdw[c] : 0.0f;
        } else {
            const u32x4 r = philox4x32_10((unsigned)me.chunk, (unsigned)(me.chunk >> 32), c | (S2S_KIND_DWELL << 16), 0,
                                          P.seed_lo, P.seed_hi);
            z = box_muller(r.x, r.y);
        }
        gv = fmaxf(mul_then_add(z, P.dwell_std, P.dwell_mean), P.min_duration);   // modules.py:425-432
    }
    if (mine) {
        const float rd = fminf(fmaxf(rintf(gv), -1.0e9f), 1.0e9f);  // torch.round: half-to-even (modules.py:437)
        reinterpret_cast<int*>(me.slot + 1040)[c] = (int)rd;
        store_stream(me.out_dur + c, (int)rd);
        if (dbg.g) dbg.g[me.dbg_idx * 16 + c] = gv;
    }
}

// stand-alone operators (TEST instance, dbg.emb_in): the pre-net output is replaced by rows the caller supplies
template <int NQ>
__device__ __forceinline__ void front_emb_in(const FrontChunk (&io)[NQ], const DebugDev& dbg, f32x4 (&X)[NQ][4], const int lane) {
    if (!dbg.emb_in) return;
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) X[q][ft] = ldg4(dbg.emb_in + (io[q].dbg_idx * 16 + c) * 64 + 16 * ft + 4 * g);
}

// X -> the chunks' hand-off slots (enc = true: enc_out) and, for the tests, the debug array of that stage (emb_out / enc_out)
template <int NQ>
__device__ __forceinline__ void front_store(const FrontChunk (&io)[NQ], const DebugDev& dbg, const f32x4 (&X)[NQ][4], const int lane,
                                            const bool enc) {
    const int g = lane >> 4, c = lane & 15;
    float* const dbg_dst = enc ? dbg.enc_out : dbg.emb_out;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (!io[q].live) continue;
        if (enc) {
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) *reinterpret_cast<f32x4*>(io[q].slot + c * 64 + 16 * ft + 4 * g) = X[q][ft];
        }
        if (dbg_dst) {
#pragma unroll
            for (int ft = 0; ft < 4; ++ft)
                *reinterpret_cast<f32x4*>(dbg_dst + (io[q].dbg_idx * 16 + c) * 64 + 16 * ft + 4 * g) = X[q][ft];
        }
    }
}

// ---- f32 mode: one chunk per wave, every product on the f32-input MFMA, weights as f32 fragments from L2, encoder K/V in the
//      wave's own slice of LDS (AttnLds<1>)
struct FrontLdsF32 { static constexpr int BYTES = AttnLds<1>::BYTES; };
template <bool EVAL = false>
__device__ __forceinline__ void frontend_f32(const ModelDev& M, const float* __restrict__ W, const FrontChunk (&io)[1],
                                             const ParamsDev& P, char* __restrict__ lds_raw, const DebugDev& dbg, const int lane) {
    const int g = lane >> 4, c = lane & 15;
    f32x4 X[1][4];
    front_embed<1, EVAL>(M, W, io, lane, X);
#pragma unroll 1
    for (int i = 0; i < M.pre_layers; ++i) {                         // modules.py:74-77
        f32x4 Y[1][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) Y[0][mt] = ldg4(W + M.pre_b[i] + 16 * mt + 4 * g);
        gemm_acc<1, 4, 4>(W + M.pre_w[i], lane, Y, X);
        relu_tiles<1>(Y);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) X[0][mt] = Y[0][mt];
    }
    front_emb_in<1>(io, dbg, X, lane);
    front_store<1>(io, dbg, X, lane, false);                // emb_out (debug only)
    float sig[1], cq[1] = {1.0f}, rq[1] = {1.0f};
    auto head = [&](const MlpOff m, float (&out)[1]) {
        f32x4 hid[1][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) hid[0][mt] = ldg4(W + m.b0 + 16 * mt + 4 * g);
        gemm_acc<1, 4, 4>(W + m.w0, lane, hid, X);
        head_out<1>(W, m, hid, lane, out);
    };
    head(M.noise, sig);                                              // modules.py:275-278
    if (P.duration_sampling) { head(M.conc, cq); head(M.rate, rq); }
    front_dwell<1, EVAL>(io, P, sig, cq, rq, dbg, lane);
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) X[0][ft] += ldg4(W + M.pe_enc + c * 64 + 16 * ft + 4 * g);   // modules.py:80
#pragma unroll 1
    for (int l = 0; l < M.enc_layers; ++l) fft_block<1, 1, 16>(W, M.enc[l], X, reinterpret_cast<float*>(lds_raw), 0, lane);
    front_store<1>(io, dbg, X, lane, true);
}

// ---- f16x3: two chunks per wave, every product as three f16 MFMA terms, weights as f16 hi/lo units from L2, encoder attention
//      in registers (s2s_device_h.h: enc_attention_h) -- no LDS at all.  (Measured: the phase is bound by its instruction count,
//      about 6 k per chunk, like the decoder's; where the weights come from -- eight copies through the vector L1, or one copy
//      staged in LDS behind ten barriers per group -- made no difference to its 71 us per 16 chunks.)
template <int NQ, bool EVAL = false>
__device__ __forceinline__ void frontend_h16(const ModelDev& M, const float* __restrict__ W, const FrontChunk (&io)[NQ],
                                             const ParamsDev& P, const DebugDev& dbg, const int lane, const float one) {
    const int g = lane >> 4, c = lane & 15;
    DIAG_DECL;
#define FDIAG(slot) DIAG_STAMP(32 + (slot))
    f32x4 X[NQ][4];
    front_embed<NQ, EVAL>(M, W, io, lane, X);
    FDIAG(0);
#pragma unroll 1
    for (int i = 0; i < M.pre_layers; ++i) {                         // modules.py:74-77
        HL xb[NQ][2];
        f32x4 Y[NQ][4];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { xb[q][0] = split8(X[q][0], X[q][1], one); xb[q][1] = split8(X[q][2], X[q][3], one); }
        linear64_h<NQ>(W + M.pre_wh[i], W + M.pre_b[i], lane, xb, Y);
        relu_tiles<NQ>(Y);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) X[q][mt] = Y[q][mt];
    }
    front_emb_in<NQ>(io, dbg, X, lane);
    front_store<NQ>(io, dbg, X, lane, false);                        // emb_out (debug only)
    FDIAG(1);
    {   // the three heads read emb_out only (modules.py:275-278, 197-225), so they run BEFORE the encoder blocks: emb_out is dead
        // by then instead of being carried (and spilled) through them
        HL Sb[NQ][2];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { Sb[q][0] = split8(X[q][0], X[q][1], one); Sb[q][1] = split8(X[q][2], X[q][3], one); }
        float sig[NQ], cq[NQ], rq[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { cq[q] = 1.0f; rq[q] = 1.0f; }
        auto head = [&](const MlpOff m, float (&out)[NQ]) {
            f32x4 hid[NQ][4];
            linear64_h<NQ>(W + m.w0h, W + m.b0, lane, Sb, hid);
            head_out<NQ>(W, m, hid, lane, out);
        };
        head(M.noise, sig);
        if (P.duration_sampling) { head(M.conc, cq); head(M.rate, rq); }
        FDIAG(4);
        front_dwell<NQ, EVAL>(io, P, sig, cq, rq, dbg, lane);
    }
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) {
        const f32x4 pe = ldg4(W + M.pe_enc + c * 64 + 16 * ft + 4 * g);
#pragma unroll
        for (int q = 0; q < NQ; ++q) X[q][ft] += pe;                 // modules.py:80
    }
    FDIAG(5);
#pragma unroll 1
    for (int l = 0; l < M.enc_layers; ++l) {
        const LayerOff L = M.enc[l];
        const float* const wl = W + L.stream_h;                      // pack_layer: units 0-15 attention, 16-47 FFN
        f32x4 acc[NQ][4];
        HL x1b[NQ][2];
        enc_attention_h<NQ>(W, L, wl, X, acc, lane, one);
        FDIAG(2);
        enc_ffn_begin_h<NQ>(W, L, acc, X, x1b, lane, one);
        enc_ffn_half_h<NQ>(W, L, wl + 16 * 1024, 0, x1b, X, lane, one);
        enc_ffn_half_h<NQ>(W, L, wl + 32 * 1024, 2, x1b, X, lane, one);
        layer_norm64<NQ, true>(X, W + L.ln2g, W + L.ln2b, g);
        FDIAG(3);
    }
    front_store<NQ>(io, dbg, X, lane, true);
}

// ================================================================================ decoder
#define DEC_WAVES 8
#define DEC_NQ 2            // 16-column time tiles per wave: 8 waves x 2 x 16 = 256 >= 250
#define DEC_WPS (DEC_WAVES / 4)   // waves per SIMD
#define DEC_NKT 16
static constexpr int DEC_LDS_F32 = AttnLds<DEC_NKT>::BYTES;
static constexpr int DEC_LDS_H = AttnLdsH<DEC_NQ, DEC_WAVES, DEC_NKT>::BYTES;

// The decoder of ONE chunk, run by the 8 waves of a workgroup, in three pieces so that the fused kernel can request the next
// chunk's rows before it finishes the current one: dec_gather (length regulator), dec_blocks, dec_emit (projection, noise).
// slot: the chunk's frontend outputs -- enc_out [16][64], sigma [16] at +1024, dur [16] (int32) at +1040.

// ---- length regulator (modules.py:344-392) as a gather: row t copies encoder row i(t) = #{j : cum[j] <= t}; rows past
//      cum[15] are zero; crop at 250; then + position_enc (modules.py:136, also on the zero rows).  Two halves: dec_gather_issue
//      requests the rows, dec_gather_finish combines them -- whatever the caller puts in between runs under the loads.
struct GatherRaw {
    f32x4 e[DEC_NQ][4], pe[DEC_NQ][4];
    float sg[DEC_NQ];
    int idx[DEC_NQ];
};
__device__ __forceinline__ void dec_gather_issue(const ModelDev& M, const float* __restrict__ W, const float* __restrict__ slot,
                                                 const int wave, const int lane, GatherRaw& R) {
    const int g = lane >> 4, c = lane & 15;
    const int qt0 = DEC_NQ * wave;
    int cum[16];
    {
        // a lane-indexed (vector) load, then broadcasts: in the fused kernel the dwell counts were stored by another wave of
        // this launch, and a uniform-address load could be served from the scalar cache, which vector stores do not update
        const int dv = reinterpret_cast<const int*>(slot + 1040)[c];
        int run = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {          // a dwell past the crop at 250 (modules.py:386) acts like 251: no int32 overflow
            const int dj = __builtin_amdgcn_readlane(dv, j);
            run += dj < S2S_T_DEC + 1 ? dj : S2S_T_DEC + 1;
            cum[j] = run;
        }
    }
#pragma unroll
    for (int q = 0; q < DEC_NQ; ++q) {
        const int t = 16 * (qt0 + q) + c;
        int idx = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) idx += (cum[j] <= t) ? 1 : 0;
        R.idx[q] = idx;
        const int row = idx < 16 ? idx : 0;
        const float* er = slot + row * 64 + 4 * g;
        const float* pr = W + M.pe_dec + (t < S2S_T_DEC ? t : 0) * 64 + 4 * g;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) { R.e[q][ft] = ldg4(er + 16 * ft); R.pe[q][ft] = ldg4(pr + 16 * ft); }
        R.sg[q] = slot[1024 + row];
    }
}
__device__ __forceinline__ void dec_gather_finish(const GatherRaw& R, const int wave, const int lane, f32x4 (&X)[DEC_NQ][4],
                                                  float (&sig_ext)[DEC_NQ]) {
    const int c = lane & 15;
#pragma unroll
    for (int q = 0; q < DEC_NQ; ++q) {
        const int t = 16 * (DEC_NQ * wave + q) + c;
        const bool live = R.idx[q] < 16, real = t < S2S_T_DEC;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
            X[q][ft] = real ? ((live ? R.e[q][ft] : f32x4{0, 0, 0, 0}) + R.pe[q][ft]) : f32x4{0, 0, 0, 0};
        sig_ext[q] = live ? R.sg[q] : 0.0f;
    }
}

// stand-alone Decoder (TEST instance, dbg.dec_in): the chunk's decoder input comes from memory instead of the gather
__device__ __forceinline__ void dec_override(const float* __restrict__ dec_in, const long long dbg_idx, const int wave, const int lane,
                                             f32x4 (&X)[DEC_NQ][4]) {
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int q = 0; q < DEC_NQ; ++q) {
        const int t = 16 * (DEC_NQ * wave + q) + c;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
            X[q][ft] = t < S2S_T_DEC ? ldg4(dec_in + (dbg_idx * S2S_T_DEC + t) * 64 + 16 * ft + 4 * g) : f32x4{0, 0, 0, 0};
    }
}

// next_slot (MODE 1 only): the NEXT chunk's hand-off slot, copied into the LDS words behind the block's own image by the last
// layer's FFN weight staging step (one more load per lane before its barrier, one more LDS store after it), so that the gather
// that follows this chunk reads LDS instead of paying two dependent L2 round trips.
template <int MODE, bool EXACT = false>   // 0: f32-input MFMA block, 1: split-f16 block (s2s_device_h.h), 3: the same block with single f16 products
__device__ __forceinline__ void dec_blocks(const ModelDev& M, const float* __restrict__ W, f32x4 (&X)[DEC_NQ][4],
                                           char* __restrict__ lds_raw, const int wave, const int lane, const float one,
                                           unsigned long long* diag, const float* __restrict__ next_slot = nullptr) {
    const int qt0 = DEC_NQ * wave;
#pragma unroll 1
    for (int l = 0; l < M.dec_layers; ++l) {
        float* const slot_lds = reinterpret_cast<float*>(lds_raw + DEC_LDS_H), *const sv_lds = slot_lds + S2S_SLOT_FLOATS;
        if (MODE == 1) fft_block_h<DEC_NQ, DEC_WAVES, DEC_NKT, S2S_T_DEC, true, EXACT>(W, M.dec[l], X, lds_raw, qt0, wave, lane, one, diag,
                                                                          l == M.dec_layers - 1 ? next_slot : nullptr, slot_lds, sv_lds);
        else if (MODE == 3) fft_block_h<DEC_NQ, DEC_WAVES, DEC_NKT, S2S_T_DEC, false, EXACT>(W, M.dec[l], X, lds_raw, qt0, wave, lane, one, diag,
                                                                                      nullptr, slot_lds, sv_lds);
        else           fft_block<DEC_NQ, DEC_NKT, S2S_T_DEC>(W, M.dec[l], X, reinterpret_cast<float*>(lds_raw), qt0, lane, diag);
    }
}

// ---- out_linear + ReLU (modules.py:140-141).  Every lane group ends up with the row sums of all tiles (sum_g is an
//      all-reduce), so lane group q keeps tile q: ys = its sample (scaled units), se = its expanded sigma.
__device__ __forceinline__ void dec_project(const ModelDev& M, const float* __restrict__ W, const f32x4 (&X)[DEC_NQ][4],
                                            const float (&sig_ext)[DEC_NQ], const int lane, float& ys, float& se) {
    const int g = lane >> 4;
    f32x4 wo[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) wo[ft] = ldg4(W + M.out_w + 16 * ft + 4 * g);
    const float bo = W[M.out_b];
    ys = 0.0f; se = 0.0f;
#pragma unroll
    for (int q = 0; q < DEC_NQ; ++q) {
        float part = 0.0f;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
#pragma unroll
            for (int r = 0; r < 4; ++r) part += X[q][ft][r] * wo[ft][r];
        const float v = relu1(sum_g(part) + bo);
        if (g == q) { ys = v; se = sig_ext[q]; }
    }
}

// ---- x165 (model.py:221), noise where != 0 (model.py:224-238), clamp (model.py:240): ONE pass of Philox + Box-Muller per
//      wave for its DEC_NQ <= 4 tiles.  inj_z01 / out_signal: the chunk's [250] rows.
__device__ __forceinline__ void dec_emit(const ModelDev& M, const float ys, const float se, const unsigned long long chunk,
                                         const ParamsDev& P, const float* __restrict__ inj_z01, float* __restrict__ out_signal,
                                         const DebugDev& dbg, const long long dbg_idx, const int wave, const int lane) {
    const int g = lane >> 4, c = lane & 15;
    const int t = 16 * (DEC_NQ * wave + g) + c;
    float y = __fmul_rn(ys, M.scale);
    if (g < DEC_NQ && t < S2S_T_DEC) {
        if (dbg.y_scaled) dbg.y_scaled[dbg_idx * S2S_T_DEC + t] = ys;
        if (P.noise_std > 0.0f) {
            float z;
            if (inj_z01) {
                z = inj_z01[t];
            } else {
                const u32x4 r = philox4x32_10((unsigned)chunk, (unsigned)(chunk >> 32),
                                              (unsigned)t | (S2S_KIND_NOISE << 16), 0, P.seed_lo, P.seed_hi);
                z = box_muller(r.x, r.y);
            }
            if (dbg.z01) dbg.z01[dbg_idx * S2S_T_DEC + t] = z;
            const float sd = P.noise_sampling
                                 ? __fmul_rn(__fmul_rn(fmaxf(se, P.min_noise), P.noise_std), M.scale)
                                 : P.noise_std;
            if (y != 0.0f) y = mul_then_add(z, sd, y);
        }
        store_stream(out_signal + t, fmaxf(y, 0.0f));
    }
}

// ONE launch per tile of chunks, nothing but the bases comes in and nothing but dwell counts and
// signal goes out.  A persistent 8-wave workgroup owns a contiguous range of the tile's chunks and walks it in groups of up
// to 8 * FNQ: wave w runs the one-wave frontend of chunks FNQ*w .. FNQ*w+FNQ-1 of the group (their encoder K/V in a slice of
// the decoder's K/V region, dead between chunks), then all 8 waves decode the group's chunks one after the other.  The
// frontend outputs of a group (4.2 KB per chunk) wait in the workgroup's own slots of `handoff` -- rewritten every group by the
// CU that reads them back, so the reads hit that XCD's L2.  The dirty lines do get written back once per group, though: an XCD's
// L2 keeps about 1.5 MB of rewritten data (tools/probes/l2_writeback_probe.hip) and 32 workgroups x 16 slots are 2.2 MB.
template <int MODE> struct Fused {
    static constexpr int FMODE = (MODE == 3) ? 1 : MODE;          // the reduced-precision decoder keeps the f16x3 frontend
    static constexpr int FNQ = (FMODE == 1) ? 2 : 1;              // chunks per frontend wave
    static constexpr int GROUP = DEC_WAVES * FNQ;
    static constexpr bool PF = (MODE == 1);                       // next chunk's slot prefetched into LDS (dec_blocks)
    static constexpr int LDS = (MODE == 0) ? DEC_LDS_F32 : DEC_LDS_H + (S2S_SLOT_FLOATS + S2S_SV_FLOATS + S2S_PROG_INTS + S2S_Z2_FLOATS) * 4;   // + next slot, small vectors, progress counters, 2nd zeros row
    // (the static arrays sit in front, largest alignment first; the dynamic region follows on its own 16-byte alignment.  The
    //  diagnostic build -- 3 KB of per-wave stamps -- fills the CU's 160 KB to the byte.)
    static_assert(LDS + S2S_STATIC_LDS_BYTES + 16 <= 160 * 1024, "LDS per workgroup: dynamic + the static arrays in front of it");
    static_assert(FMODE == 1 || DEC_WAVES * FrontLdsF32::BYTES <= LDS, "the f32 frontend waves' K/V images share the decoder's LDS");
};
#define S2S_MAX_GROUP (2 * DEC_WAVES)
// TEST = false is the production instance: no injected variates and no stage outputs, whose address arithmetic would otherwise
// sit (and spill) in the hot loop; the parity tests that inject or ask for stage outputs run the TEST = true instance of the
// same code.
// EXACT: the decoder attention's exact path (the online softmax, s2s_device_h.h) instead of "fast path, redone on overflow" -- a
// kernel instance of its own, so that neither path's registers and schedule depend on the other (split-f16 modes only).
template <int MODE, bool TEST, bool EXACT = false>
__global__ __launch_bounds__(DEC_WAVES * 64, DEC_WPS) void s2s_fused_kernel(
    const ModelDev M, const float* __restrict__ W, const uint8_t* __restrict__ bases,
    const long long* __restrict__ chunk_start, const uint8_t* __restrict__ n_valid, int n_chunks, long long first_chunk,
    ParamsDev P, const float* __restrict__ inj_g_, const float* __restrict__ inj_zdw_, const float* __restrict__ inj_z01_,
    float* __restrict__ handoff, int* __restrict__ out_dur, float* __restrict__ out_signal, DebugDev dbg_, long long dbg_base,
    unsigned* __restrict__ sched) {
    using F = Fused<MODE>;
    const float* const inj_g = TEST ? inj_g_ : nullptr;
    const float* const inj_zdw = TEST ? inj_zdw_ : nullptr;
    const float* const inj_z01 = TEST ? inj_z01_ : nullptr;
    DebugDev dbg = dbg_;
    if (!TEST) { dbg = DebugDev{}; dbg.diag = dbg_.diag; dbg.stats = dbg_.stats; }
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int nb = S2S_T_ENC + M.k - 1;
    if constexpr (MODE != 0) att32_consts<AttnLdsH<DEC_NQ, DEC_WAVES, DEC_NKT>>(lds_raw, threadIdx.x, DEC_WAVES * 64);   // (visible after the group loop's first barrier)
    if constexpr (MODE != 0) {                                     // the attention loop's progress counters (prio_balance)
        if (threadIdx.x < S2S_PROG_INTS + S2S_Z2_FLOATS)              // (and the second zeros row behind them)
            reinterpret_cast<int*>(lds_raw + DEC_LDS_H + (S2S_SLOT_FLOATS + S2S_SV_FLOATS) * 4)[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) {                // production counters: redo count, entry stamps (kept in LDS, not in SGPRs, across the kernel)
        const unsigned long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
        s2s_stats_lds[0] = 0;
        s2s_stats_lds[4] = (unsigned)c0; s2s_stats_lds[5] = (unsigned)(c0 >> 32);
        s2s_stats_lds[6] = (unsigned)r0; s2s_stats_lds[7] = (unsigned)(r0 >> 32);
    }
#ifdef S2S_TILEHIST
    for (int i = threadIdx.x; i < 2 * 2 * 64; i += DEC_WAVES * 64) s2s_hist_lds[i] = 0;
#endif
#ifdef S2S_DIAG
    for (int i = threadIdx.x; i < 8 * S2S_DIAG_SLOTS; i += DEC_WAVES * 64) s2s_diag_lds[i] = 0;
    const unsigned long long diag_c0 = __builtin_readcyclecounter(), diag_r0 = __builtin_amdgcn_s_memrealtime();
    __syncthreads();
#endif
    float* const slot0 = handoff + (size_t)blockIdx.x * S2S_MAX_GROUP * S2S_SLOT_FLOATS;
    // The workgroup's next group of chunks waits in LDS (S2S_LDS_G0 / _N), put there by thread 0 one group ahead and read by every
    // wave behind the barrier that opens the group loop.  sched == nullptr, the static split: workgroup b walks [b n / G,
    // (b + 1) n / G) in groups.  Else claims (s2s_schedule.h) from the handle's counter sched[0], one returning atomic per group.
    // A workgroup's one empty claim counts it into sched[1], which wraps at G by itself; the last one in puts the counter back
    // to 0 for the handle's next launch (launches of a handle are stream-ordered: include/s2s_hip.h).
    // (what thread 0 needs for that -- the counter's address, the grid, the end of the range -- waits in LDS too, S2S_LDS_SCHED / _GRID / _END: not
    //  one register stays live across the group loop for the schedule)
    auto put_group = [&](const int start, const int count) {
        s2s_stats_lds[S2S_LDS_G0] = (unsigned)start; s2s_stats_lds[S2S_LDS_N] = (unsigned)count;
    };
    auto sched_of = [&]() {
        return reinterpret_cast<unsigned*>(((unsigned long long)s2s_stats_lds[S2S_LDS_SCHED + 1] << 32) | s2s_stats_lds[S2S_LDS_SCHED]);
    };
    auto put_claim = [&](unsigned* const q, const unsigned c) {
        int start, count;
        const unsigned G = s2s_stats_lds[S2S_LDS_GRID];
        s2s_claim_range((int)s2s_stats_lds[S2S_LDS_END], (int)G, F::GROUP, (int)c, &start, &count);
        put_group(start, count);
        if (count == 0) {
            __threadfence();
            if (atomicInc(q + 1, G - 1) == G - 1) atomicExch(q, 0u);
        }
    };
    if (threadIdx.x == 0) {
        s2s_stats_lds[S2S_LDS_SCHED] = (unsigned)(unsigned long long)sched;
        s2s_stats_lds[S2S_LDS_SCHED + 1] = (unsigned)((unsigned long long)sched >> 32);
        s2s_stats_lds[S2S_LDS_GRID] = gridDim.x;
        if (sched) {
            s2s_stats_lds[S2S_LDS_END] = (unsigned)n_chunks;
            put_claim(sched, atomicAdd(sched, 1u));
        } else {
            const int lo = (int)((long long)blockIdx.x * n_chunks / gridDim.x), hi = (int)((long long)(blockIdx.x + 1) * n_chunks / gridDim.x);
            s2s_stats_lds[S2S_LDS_END] = (unsigned)hi;
            put_group(lo, hi - lo < F::GROUP ? hi - lo : F::GROUP);
        }
    }
#pragma unroll 1
    for (;;) {
        float one = 1.0f;                  // opaque to the optimiser: see split2 in s2s_device_h.h
        asm volatile("" : "+s"(one));
        DIAG_DECL;
        __syncthreads();                   // the previous group's last block is done with the K/V region and with the slots
        const int g0 = __builtin_amdgcn_readfirstlane((int)s2s_stats_lds[S2S_LDS_G0]);
        const int n_here = __builtin_amdgcn_readfirstlane((int)s2s_stats_lds[S2S_LDS_N]);
        if (n_here <= 0) break;
        {
            int lnf = lane;                // (opaque per group, like `ln` below: nothing lane-dependent is hoisted out of the loops and spilled)
            asm volatile("" : "+v"(lnf));
            auto chunk_of = [&](const int j, const int j_filler) {
                const bool live = j < n_here;
                const int b = g0 + (live ? j : j_filler);            // a filler repeats the wave's first chunk
                return FrontChunk{chunk_start ? bases + chunk_start[b] : bases + (size_t)b * nb, n_valid[b],
                                  (unsigned long long)(first_chunk + b), inj_g ? inj_g + (size_t)b * 16 : nullptr,
                                  inj_zdw ? inj_zdw + (size_t)b * 16 : nullptr, slot0 + j * S2S_SLOT_FLOATS,
                                  out_dur + (size_t)b * 16, dbg_base + b, live};
            };
            if constexpr (F::FMODE == 1) {
                if (n_here > DEC_WAVES) {                            // two chunks per wave
                    const FrontChunk io[2] = {chunk_of(2 * wave, 2 * wave), chunk_of(2 * wave + 1, 2 * wave)};
                    if (2 * wave < n_here) frontend_h16<2>(M, W, io, P, dbg, lnf, one);
                } else {                                             // a short group (small batches): one chunk per wave, more waves busy
                    const FrontChunk io[1] = {chunk_of(wave, 0)};
                    if (wave < n_here) frontend_h16<1>(M, W, io, P, dbg, lnf, one);
                }
            } else {
                const FrontChunk io[1] = {chunk_of(wave, 0)};
                if (wave < n_here) frontend_f32(M, W, io, P, lds_raw + wave * FrontLdsF32::BYTES, dbg, lnf);
            }
        }
        __syncthreads();                   // the group's slots are written (global stores: workgroup-scope release/acquire)
        DIAG_STAMP(7);                     // frontend phase and its two barriers
        // the next group: every wave has read this one's (g0, n_here) before the barrier above
        if (threadIdx.x == 0) {
            if (unsigned* const q = sched_of()) {
                put_claim(q, atomicAdd(q, 1u));
            } else {
                const int hi = (int)s2s_stats_lds[S2S_LDS_END], nx = g0 + F::GROUP;
                put_group(nx, nx >= hi ? 0 : hi - nx < F::GROUP ? hi - nx : F::GROUP);
            }
        }
        f32x4 X[DEC_NQ][4];
        float sig_ext[DEC_NQ];
        {
            int lg = lane;                 // (opaque, like lnf / ln: the gather's per-lane addresses are not kept across the group loop)
            asm volatile("" : "+v"(lg));
            GatherRaw R;
            dec_gather_issue(M, W, slot0, wave, lg, R);
            dec_gather_finish(R, wave, lg, X, sig_ext);
            if (TEST && dbg.dec_in) dec_override(dbg.dec_in, dbg_base + g0, wave, lg, X);
        }
        DIAG_STAMP(8);
#pragma unroll 1
        for (int j = 0; j < ((S2S_ABL & 65536) ? 0 : n_here); ++j) {      // (65536: timing of the frontend phase alone)
            const int b = g0 + j;
            // (after the group's last chunk everything "next" is that chunk again, computed and thrown away: no branches here,
            // the register allocator spills values that live from one conditional block to another)
            const float* next = slot0 + (j + 1 < n_here ? j + 1 : j) * S2S_SLOT_FLOATS;
            dec_blocks<MODE, EXACT>(M, W, X, lds_raw, wave, lane, one, dbg.diag, F::PF ? next : nullptr);
            DIAG_STAMP(15);   // (time inside the blocks is accounted by their own stamps)
            // (an opaque copy of the lane id: the per-lane addresses below are recomputed per chunk, a handful of VALU
            // instructions, instead of being hoisted out of the loop and spilled across the blocks -- a scratch reload here
            // would also wait for every load issued before it)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            float ys, se;
            dec_project(M, W, X, sig_ext, ln, ys, se);
            // the next chunk's rows are requested before this one's noise is drawn, from the copy of its slot that the last
            // block left in LDS (f16x3), or from the slot itself: two dependent L2 round trips behind Philox + Box-Muller
            GatherRaw R;
            if constexpr (F::PF) dec_gather_issue(M, W, reinterpret_cast<const float*>(lds_raw + DEC_LDS_H), wave, ln, R);
            else                 dec_gather_issue(M, W, next, wave, ln, R);
            dec_emit(M, ys, se, (unsigned long long)(first_chunk + b), P, inj_z01 ? inj_z01 + (size_t)b * S2S_T_DEC : nullptr,
                     out_signal + (size_t)b * S2S_T_DEC, dbg, dbg_base + b, wave, ln);
            dec_gather_finish(R, wave, ln, X, sig_ext);
            if (TEST && dbg.dec_in) dec_override(dbg.dec_in, dbg_base + g0 + (j + 1 < n_here ? j + 1 : j), wave, ln, X);
            DIAG_STAMP(9);
        }
    }
#ifdef S2S_DIAG
    // slots 16 / 17: this wave's whole-kernel time on the shader clock (s_memtime) and on the constant 100 MHz clock (s_memrealtime):
    // their ratio is the clock the SIMDs actually ran at (MI355X_MICROARCH.md, DVFS)
    DIAG_COUNT(16, __builtin_readcyclecounter() - diag_c0);
    DIAG_COUNT(17, __builtin_amdgcn_s_memrealtime() - diag_r0);
    DIAG_COUNT(18, 1ull);
    __syncthreads();
    if (dbg.diag)
        for (int i = threadIdx.x; i < 8 * S2S_DIAG_SLOTS; i += DEC_WAVES * 64)
            if (s2s_diag_lds[i]) atomicAdd(dbg.diag + i, s2s_diag_lds[i]);        // [wave][slot], summed over the workgroups
#endif
    __syncthreads();                       // every wave's redo count is in LDS
#ifdef S2S_TILEHIST
    if (dbg.diag)
        for (int i = threadIdx.x; i < 2 * 2 * 64; i += DEC_WAVES * 64)
            if (s2s_hist_lds[i]) atomicAdd(dbg.diag + i, (unsigned long long)s2s_hist_lds[i]);
#endif
    if (threadIdx.x == 0 && dbg.stats) {
        const unsigned long long c0 = ((unsigned long long)s2s_stats_lds[5] << 32) | s2s_stats_lds[4];
        const unsigned long long r0 = ((unsigned long long)s2s_stats_lds[7] << 32) | s2s_stats_lds[6];
        if (s2s_stats_lds[0]) atomicAdd(dbg.stats + S2S_STAT_REDO, (unsigned long long)s2s_stats_lds[0]);
        atomicAdd(dbg.stats + S2S_STAT_CYCLES, __builtin_readcyclecounter() - c0);
        const unsigned long long span = __builtin_amdgcn_s_memrealtime() - r0;
        atomicAdd(dbg.stats + S2S_STAT_TICKS, span);
        atomicAdd(dbg.stats + S2S_STAT_WGS, 1ull);
        atomicMax(dbg.stats + S2S_STAT_SPAN_MAX, span);
        atomicMax(dbg.stats + S2S_STAT_SPAN_MIN_INV, ~span);          // (the slab is reset to zeros: the minimum rides as its complement)
    }
}

// ================================================================================ evaluate
// s2s_evaluate_chunks on the tuned instances: s2s_fused_kernel's group walk with the teacher-forced frontend (EVAL: k-mer rows,
// measured dwell into the slot, conc / rate always formed) and the decoder output y stored where dec_emit would draw noise.  The
// decoder arithmetic is the predict instance's (the same dec_gather / dec_blocks / dec_project), so y is that mode's; the loss sums
// are s2s_eval_loss_kernel's.  dbg_.sigma / conc / rate are required ([B][16]), its other fields are ignored; y: [B][250].
template <int MODE, bool EXACT>
__global__ __launch_bounds__(DEC_WAVES * 64, DEC_WPS) void s2s_eval_kernel(
    const ModelDev M, const float* __restrict__ W, const uint8_t* __restrict__ kmers, const int* __restrict__ dwell, int n_chunks,
    ParamsDev P, float* __restrict__ handoff, float* __restrict__ y, DebugDev dbg_) {
    using F = Fused<MODE>;
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if constexpr (MODE != 0) att32_consts<AttnLdsH<DEC_NQ, DEC_WAVES, DEC_NKT>>(lds_raw, threadIdx.x, DEC_WAVES * 64);
    if constexpr (MODE != 0) {
        if (threadIdx.x < S2S_PROG_INTS + S2S_Z2_FLOATS)
            reinterpret_cast<int*>(lds_raw + DEC_LDS_H + (S2S_SLOT_FLOATS + S2S_SV_FLOATS) * 4)[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) s2s_stats_lds[0] = 0;
    DebugDev dbg{};                                                // the three head outputs only: no stage images in the hot loop
    dbg.sigma = dbg_.sigma; dbg.conc = dbg_.conc; dbg.rate = dbg_.rate;
    float* const slot0 = handoff + (size_t)blockIdx.x * S2S_MAX_GROUP * S2S_SLOT_FLOATS;
    const int lo = (int)((long long)blockIdx.x * n_chunks / gridDim.x), hi = (int)((long long)(blockIdx.x + 1) * n_chunks / gridDim.x);
    const int kb = S2S_T_ENC * M.k;                                 // k-mer letters per chunk
#pragma unroll 1
    for (int g0 = lo; g0 < hi; g0 += F::GROUP) {
        const int n_here = hi - g0 < F::GROUP ? hi - g0 : F::GROUP;
        float one = 1.0f;
        asm volatile("" : "+s"(one));
        __syncthreads();
        {
            int lnf = lane;
            asm volatile("" : "+v"(lnf));
            auto chunk_of = [&](const int j, const int j_filler) {
                const bool live = j < n_here;
                const int b = g0 + (live ? j : j_filler);
                return FrontChunk{kmers + (size_t)b * kb, S2S_T_ENC, (unsigned long long)b, nullptr, nullptr, slot0 + j * S2S_SLOT_FLOATS,
                                  const_cast<int*>(dwell) + (size_t)b * S2S_T_ENC, (long long)b, live};
            };
            if constexpr (F::FMODE == 1) {
                if (n_here > DEC_WAVES) {
                    const FrontChunk io[2] = {chunk_of(2 * wave, 2 * wave), chunk_of(2 * wave + 1, 2 * wave)};
                    if (2 * wave < n_here) frontend_h16<2, true>(M, W, io, P, dbg, lnf, one);
                } else {
                    const FrontChunk io[1] = {chunk_of(wave, 0)};
                    if (wave < n_here) frontend_h16<1, true>(M, W, io, P, dbg, lnf, one);
                }
            } else {
                const FrontChunk io[1] = {chunk_of(wave, 0)};
                if (wave < n_here) frontend_f32<true>(M, W, io, P, lds_raw + wave * FrontLdsF32::BYTES, dbg, lnf);
            }
        }
        __syncthreads();
        f32x4 X[DEC_NQ][4];
        float sig_ext[DEC_NQ];
        {
            int lg = lane;
            asm volatile("" : "+v"(lg));
            GatherRaw R;
            dec_gather_issue(M, W, slot0, wave, lg, R);
            dec_gather_finish(R, wave, lg, X, sig_ext);
        }
#pragma unroll 1
        for (int j = 0; j < n_here; ++j) {
            const int b = g0 + j;
            const float* next = slot0 + (j + 1 < n_here ? j + 1 : j) * S2S_SLOT_FLOATS;
            dec_blocks<MODE, EXACT>(M, W, X, lds_raw, wave, lane, one, nullptr, F::PF ? next : nullptr);
            int ln = lane;
            asm volatile("" : "+v"(ln));
            float ys, se;
            dec_project(M, W, X, sig_ext, ln, ys, se);
            GatherRaw R;
            if constexpr (F::PF) dec_gather_issue(M, W, reinterpret_cast<const float*>(lds_raw + DEC_LDS_H), wave, ln, R);
            else                 dec_gather_issue(M, W, next, wave, ln, R);
            {
                const int g = ln >> 4, t = 16 * (DEC_NQ * wave + g) + (ln & 15);
                if (g < DEC_NQ && t < S2S_T_DEC) store_stream(y + (size_t)b * S2S_T_DEC + t, ys);
            }
            dec_gather_finish(R, wave, ln, X, sig_ext);
        }
    }
}

// The three per-chunk sums of get_loss (model.py:458-475) from the stage outputs, one wave per chunk, each in a fixed order (lane
// partials in index order, then the butterfly of gen_wave_sum): a chunk's sums depend on its own rows only.
//   [0] sum_t (y - target)^2   [1] sum_c -Gamma(conc, rate).log_prob(|d| + (d == 0))   [2] sum_c (stdev - sigma)^2
// log_prob in torch's form: xlogy(conc, rate) + xlogy(conc - 1, x) - rate * x - lgamma(conc), each k-mer's term formed in double and
// rounded to fp32, the sums in fp32.  te <= 64: one lane per k-mer.
__global__ __launch_bounds__(256) void s2s_eval_loss_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                            const float* __restrict__ sigma, const float* __restrict__ stdev,
                                                            const float* __restrict__ conc, const float* __restrict__ rate,
                                                            const int* __restrict__ dwell, int B, int te, int ts, float* __restrict__ out_loss) {
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    float se = 0.0f;
    for (int t = lane; t < ts; t += 64) {
        const float e = y[b * ts + t] - target[b * ts + t];
        se += e * e;
    }
    float nll = 0.0f, ne = 0.0f;
    if (lane < te) {
        const long long i = b * te + lane;
        const int dv = dwell[i];
        const float x = dv == 0 ? 1.0f : (float)(dv < 0 ? -dv : dv);
        // each k-mer's term in double, rounded once: where the density is near 1 (conc ~ rate ~ 20 at a dwell of 1) the four parts
        // are of the order of 60 and cancel to a term below 1, and a chunk of such k-mers left float32 parts 1e-5 of its sum apart
        const double a = conc[i], r = rate[i];
        const double am1 = a - 1.0;
        const double lp = a * log(r) + (am1 == 0.0 ? 0.0 : am1 * log((double)x)) - r * (double)x - lgamma(a);
        nll = (float)-lp;
        const float e = stdev[i] - sigma[i];
        ne = e * e;
    }
    se = gen_wave_sum(se);
    nll = gen_wave_sum(nll);
    ne = gen_wave_sum(ne);
    if (lane == 0) { out_loss[b * 3 + 0] = se; out_loss[b * 3 + 1] = nll; out_loss[b * 3 + 2] = ne; }
}

// ================================================================================ export
// per-chunk count of non-zero samples (model.py:286 strips by value).  The export kernels take rows of TD samples: the tuned
// instance TD = S2S_T_DEC, and TD = 0 for the row length `ts` of a S2S_MODE_GENERIC_GEOMETRY handle at another max_signal_len.
template <int TD>
__global__ __launch_bounds__(256) void s2s_count_kernel(const float* __restrict__ signal, int B, int* __restrict__ counts, int ts) {
    const int T = TD ? TD : ts;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    int n = 0;
    for (int t = lane; t < T; t += 64) n += signal[(size_t)b * T + t] != 0.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) counts[b] = n;
}

// the exclusive scan of counts[B] -> offs[B+1] (int64) is s2s_scan_kernel<8, S2SScanInts> (s2s_prims.h): 131,072 chunk counts = 16 steps

__global__ __launch_bounds__(256) void s2s_read_offsets_kernel(const long long* __restrict__ offs, const int* __restrict__ read_first,
                                                               int R, long long* __restrict__ out_offsets) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r <= R) out_offsets[r] = offs[read_first[r]];
}

// The int16 a stored sample becomes (s2s_export_reads) -- the ONE place that states it: s2s_compact_kernel stores it,
// s2s_event_stats_kernel sums it.  signal_io.py:135-138: float32 ops, no contraction; round half-to-even; int16 wrap.
__device__ __forceinline__ short s2s_dac_of(float v, float dig, float range, float offset) {
    const float raw = rintf(__fsub_rn(__fdiv_rn(__fmul_rn(v, dig), range), offset));
    return (short)(int)fminf(fmaxf(raw, -2147483648.0f), 2147483520.0f);
}

template <int TD>
__global__ __launch_bounds__(256) void s2s_compact_kernel(const float* __restrict__ signal, int B, const long long* __restrict__ offs,
                                                          const int* __restrict__ read_first, int R, float* __restrict__ out_pa,
                                                          short* __restrict__ out_dac, long long capacity, float dig, float range,
                                                          float offset, int rna, int ts) {
    const int T = TD ? TD : ts;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    long long pos = offs[b];
    long long r_lo = 0, r_hi = 0;
    if (rna && out_dac) {                      // read that owns chunk b: last r with read_first[r] <= b
        int lo = 0, hi = R;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (read_first[mid] <= b) lo = mid; else hi = mid; }
        r_lo = offs[read_first[lo]];
        r_hi = offs[read_first[lo + 1]];
    }
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const float v = (t < T) ? signal[(size_t)b * T + t] : 0.0f;
        const bool keep = v != 0.0f;
        const unsigned long long mask = __ballot(keep);
        const long long dst = pos + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep) {                            // every store tests the index IT uses: pa is never reversed, dac is when rna
            if (out_pa && dst < capacity) out_pa[dst] = v;
            if (out_dac) {
                const long long at = rna ? (r_lo + (r_hi - 1 - dst)) : dst;      // r_lo <= at < r_hi
                if (at < capacity) out_dac[at] = s2s_dac_of(v, dig, range, offset);
            }
        }
        pos += __popcll(mask);
    }
}

// s2s_align_chunks: where every k-mer of a chunk ended up in the stored signal.  One wave per chunk, lane j owns k-mer j (te <= 64).
// c[j] = min(T, sum_{i<=j} max(dur[i], 0)) is the length regulator's cumulative dwell cropped at the window; every dwell is clamped
// to T BEFORE the scan, which gives the same minimum and keeps the sum below 64 * 1024 (no wrap for any int32 input).  The rows
// the export keeps are one ballot mask per 64 samples (wave-uniform), P(x) = kept samples in rows [0, x) a sum of popcounts over
// the masks; k-mer j holds P(c[j]) - P(c[j-1]) of them and the tail P(T) - P(c[te-1]).  Integers only, no LDS, no atomics.
template <int TD>
__global__ __launch_bounds__(256) void s2s_align_kernel(const float* __restrict__ signal, const int* __restrict__ dur, int B,
                                                        unsigned short* __restrict__ out_seg, int te, int ts) {
    const int T = TD ? TD : ts;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    int c = 0;
    if (lane < te) {
        const int d = dur[(size_t)b * te + lane];
        c = d < 0 ? 0 : (d > T ? T : d);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(c, o, 64); if (lane >= o) c += y; }
    c = c > T ? T : c;                          // lanes >= te carry c[te-1]
    int below = 0, total = 0;                   // P(c) of this lane; P(T)
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const float v = (t < T) ? signal[(size_t)b * T + t] : 0.0f;
        const unsigned long long mask = __ballot(v != 0.0f);
        const int k = c - t0;                   // rows of this mask in front of c: all 64, none, or the low k bits
        const unsigned long long low = k >= 64 ? ~0ull : (k <= 0 ? 0ull : ((1ull << k) - 1ull));
        below += __popcll(mask & low);
        total += __popcll(mask);
    }
    const int before = __shfl_up(below, 1, 64);
    const int last = __shfl(below, te - 1, 64);
    unsigned short* row = out_seg + (size_t)b * (te + 1);
    if (lane < te) row[lane] = (unsigned short)(below - (lane ? before : 0));
    if (lane == 0) row[te] = (unsigned short)(total - last);
}

// s2s_event_stats: the level statistics of every k-mer's STORED samples.  Same wave-per-chunk layout and the same c[] and counts as
// s2s_align_kernel; beside the ballot of a 64-sample pass the wave forms inclusive prefix sums of q and q^2 over the pass (q the
// int16 of s2s_dac_of, 0 for a stripped row), and lane j adds the prefix in front of its c[j]: S(x) = sum of q over rows [0, x) is
// additive over passes exactly like the popcount prefix P(x), and slot j holds S(c[j]) - S(c[j-1]), the tail S(T) - S(c[te-1]).
// A k-mer's run is contiguous in t, so differences of prefixes replace any per-slot accumulation: no LDS array, no atomics, and
// every sum is an exact integer (|S| <= 1024 * 2^15 in int32, Q <= 1024 * 2^30 in int64) whatever the order.
// The wave routine (one wave, one chunk b; every lane of the wave calls it): lane j < te returns slot j's n / S / Q, lane 0 also
// the tail's.  s2s_event_stats_kernel stores them, s2s_kmer_table_kernel adds them to the table row of the slot's k-mer.
template <int TD>
__device__ __forceinline__ void s2s_slot_stats_wave(const float* __restrict__ signal, const int* __restrict__ dur, int b, int lane,
                                                    float dig, float range, float offset, int te, int ts, int& n, int& S, long long& Q,
                                                    int& n_tail, int& s_tail, long long& q_tail) {
    const int T = TD ? TD : ts;
    int c = 0;
    if (lane < te) {
        const int d = dur[(size_t)b * te + lane];
        c = d < 0 ? 0 : (d > T ? T : d);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(c, o, 64); if (lane >= o) c += y; }
    c = c > T ? T : c;                          // lanes >= te carry c[te-1]
    int below = 0, total = 0;                   // P(c) of this lane; P(T)
    int s_below = 0, s_total = 0;               // S(c), S(T)
    long long q_below = 0, q_total = 0;         // the same of q^2
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const float v = (t < T) ? signal[(size_t)b * T + t] : 0.0f;
        const bool keep = v != 0.0f;
        const unsigned long long mask = __ballot(keep);
        const int q = keep ? (int)s2s_dac_of(v, dig, range, offset) : 0;
        int s = q;                              // inclusive prefixes over the pass: |s| <= 64 * 2^15, qq <= 64 * 2^30
        long long qq = (long long)(q * q);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int ys = __shfl_up(s, o, 64);
            const long long yq = __shfl_up(qq, o, 64);
            if (lane >= o) { s += ys; qq += yq; }
        }
        const int k = c - t0;                   // rows of this pass in front of c: all 64, none, or the first k
        const int src = k >= 64 ? 63 : (k <= 0 ? 0 : k - 1);
        const int ps = __shfl(s, src, 64);
        const long long pq = __shfl(qq, src, 64);
        const unsigned long long low = k >= 64 ? ~0ull : (k <= 0 ? 0ull : ((1ull << k) - 1ull));
        below += __popcll(mask & low);
        total += __popcll(mask);
        if (k > 0) { s_below += ps; q_below += pq; }
        s_total += __shfl(s, 63, 64);
        q_total += __shfl(qq, 63, 64);
    }
    const int before = __shfl_up(below, 1, 64), last = __shfl(below, te - 1, 64);
    const int s_before = __shfl_up(s_below, 1, 64), s_last = __shfl(s_below, te - 1, 64);
    const long long q_before = __shfl_up(q_below, 1, 64), q_last = __shfl(q_below, te - 1, 64);
    n = below - (lane ? before : 0);
    S = s_below - (lane ? s_before : 0);
    Q = q_below - (lane ? q_before : 0);
    n_tail = total - last;
    s_tail = s_total - s_last;
    q_tail = q_total - q_last;
}

template <int TD>
__global__ __launch_bounds__(256) void s2s_event_stats_kernel(const float* __restrict__ signal, const int* __restrict__ dur, int B,
                                                              float dig, float range, float offset,
                                                              unsigned short* __restrict__ out_seg, int* __restrict__ out_sum,
                                                              long long* __restrict__ out_sumsq, int te, int ts) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    int n, S, n_tail, s_tail;
    long long Q, q_tail;
    s2s_slot_stats_wave<TD>(signal, dur, b, lane, dig, range, offset, te, ts, n, S, Q, n_tail, s_tail, q_tail);
    const size_t row = (size_t)b * (te + 1);
    if (lane < te) {
        out_seg[row + lane] = (unsigned short)n;
        out_sum[row + lane] = S;
        out_sumsq[row + lane] = Q;
    }
    if (lane == 0) {
        out_seg[row + te] = (unsigned short)n_tail;
        out_sum[row + te] = s_tail;
        out_sumsq[row + te] = q_tail;
    }
}

// s2s_kmer_table_accumulate: every real k-mer slot's n / S / Q (the wave routine above) ADDED to the table row of the slot's k-mer.
// One wave per chunk.  Lane j < n_valid[b] forms the base-4 code of its k letters (row 4^k for a k-mer with a byte outside ACGT).
// Then the wave merges the lanes that share a row: per distinct code one ballot; a code held by one lane costs nothing more, a
// code held by several lanes is summed into its first lane by a wave reduction, so that a homopolymer or a tandem repeat issues
// one set of adds per wave and not one per slot.  The first lane of every code then adds its six fields with return-less 64-bit
// integer atomics: integer adds commute, so the table does not depend on the order, the grid or the batching.
//   LDS == false (k >= S2S_KMER_TABLE_LDS_MAX_K + 1): the adds go to the table in global memory, one workgroup per four chunks.
//   LDS == true  (k <= S2S_KMER_TABLE_LDS_MAX_K): the (4^k + 1) * 6 counters fit in 49,200 bytes of LDS; a workgroup walks its share
//       of the chunks adding into its own zeroed copy and adds the copy's non-zero words to the global table once at the end, so
//       that the few rows of a short k do not take every global atomic of the launch.  At most 512 workgroups.
#define S2S_KMER_TABLE_LDS_MAX_K 5
template <int TD, bool LDS>
__global__ __launch_bounds__(256) void s2s_kmer_table_kernel(const float* __restrict__ signal, const int* __restrict__ dur,
                                                             const unsigned char* __restrict__ read_bytes,
                                                             const long long* __restrict__ chunk_start,
                                                             const unsigned char* __restrict__ n_valid, int B, float dig, float range,
                                                             float offset, unsigned long long* __restrict__ table, int te, int ts, int k) {
    extern __shared__ unsigned long long s2s_kmer_lds[];        // LDS only: [4^k + 1][6]
    const int lane = threadIdx.x & 63, rows = (1 << (2 * k)) + 1;
    if (LDS) {
        for (int i = threadIdx.x; i < rows * S2S_KMER_TABLE_FIELDS; i += 256) s2s_kmer_lds[i] = 0ull;
        __syncthreads();
    }
    // (every wave of a workgroup runs the same number of rounds; a wave without a chunk skips the body -- wave-uniformly)
    for (int b0 = blockIdx.x * 4; b0 < B; b0 += gridDim.x * 4) {
        const int b = b0 + (threadIdx.x >> 6);
        if (b >= B) continue;
        int n, S, n_tail, s_tail;
        long long Q, q_tail;
        s2s_slot_stats_wave<TD>(signal, dur, b, lane, dig, range, offset, te, ts, n, S, Q, n_tail, s_tail, q_tail);
        int nv = n_valid[b];
        nv = nv > te ? te : nv;
        const bool real = lane < nv;
        int code = 0;
        if (real) {
            const unsigned char* p = read_bytes + chunk_start[b] + lane;
            bool other = false;
            for (int i = 0; i < k; ++i) {
                const unsigned char ch = p[i];
                const int d = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
                other |= d < 0;
                code = code * 4 + (d & 3);
            }
            if (other) code = rows - 1;
        }
        // the six fields of this lane's slot; a lane that is no real slot holds zeros and takes no part
        int occ = real ? 1 : 0, ev = (real && n > 0) ? 1 : 0;
        if (!ev) { n = 0; S = 0; Q = 0; }
        long long nn = (long long)n * n;
        bool issue = real;
        unsigned long long todo = __ballot(real);
        while (todo) {                                          // wave-uniform: one round per distinct code of the chunk
            const int first = __ffsll((long long)todo) - 1;
            const int lc = __shfl(code, first, 64);
            const bool mine = real && code == lc;
            const unsigned long long same = __ballot(mine);
            todo &= ~same;
            if (__popcll(same) < 2) continue;
            int r_ev = mine ? ev : 0, r_n = mine ? n : 0, r_s = mine ? S : 0;
            long long r_nn = mine ? nn : 0, r_q = mine ? Q : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                r_ev += __shfl_xor(r_ev, o, 64);
                r_n += __shfl_xor(r_n, o, 64);
                r_s += __shfl_xor(r_s, o, 64);
                r_nn += __shfl_xor(r_nn, o, 64);
                r_q += __shfl_xor(r_q, o, 64);
            }
            if (lane == first) { occ = __popcll(same); ev = r_ev; n = r_n; S = r_s; nn = r_nn; Q = r_q; }
            else if (mine) issue = false;
        }
        if (issue) {
            const unsigned long long f[S2S_KMER_TABLE_FIELDS] = {(unsigned long long)occ, (unsigned long long)ev, (unsigned long long)(long long)n,
                                                                 (unsigned long long)nn, (unsigned long long)(long long)S,
                                                                 (unsigned long long)Q};
            const int fields = ev ? S2S_KMER_TABLE_FIELDS : 1;  // a k-mer without samples counts as an occurrence only
            if (LDS) {
                unsigned long long* row = s2s_kmer_lds + code * S2S_KMER_TABLE_FIELDS;
#pragma unroll
                for (int i = 0; i < S2S_KMER_TABLE_FIELDS; ++i)
                    if (i < fields) atomicAdd(row + i, f[i]);
            } else {
                unsigned long long* row = table + (size_t)code * S2S_KMER_TABLE_FIELDS;
#pragma unroll
                for (int i = 0; i < S2S_KMER_TABLE_FIELDS; ++i)
                    if (i < fields) __hip_atomic_fetch_add(row + i, f[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < rows * S2S_KMER_TABLE_FIELDS; i += 256) {
            const unsigned long long v = s2s_kmer_lds[i];
            if (v) __hip_atomic_fetch_add(table + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// s2s_kmer_model_accumulate: every real k-mer slot with samples adds its event to the row of its k-mer -- 1, the fixed-point
// event mean M and deviation D (s2s_event_fixed_point) and their squares.  The slot statistics, the code and the wave merge of
// equal codes are those of s2s_kmer_table_kernel; what differs is where the first lane of every code adds: into a write-combining
// cache in LDS, one per workgroup, so that a homopolymer or a repeat that sends every chunk's adds to one row costs one set of
// global adds per flush and not one per wave.
//   The cache: S2S_KMER_MODEL_SLOTS slots, each a key (the code, or EMPTY) and five counters (field-major: one bank pattern per
//   field).  A code's slot is the code itself up to k = S2S_KMER_MODEL_DIRECT_MAX_K, else a multiplicative hash of it.
//   Insertion: atomicCAS(key, EMPTY, code); EMPTY or `code` back means the slot is this code's (its counters are zero or hold this
//   code's sums) and the five adds are LDS atomics; any other value: the next slot, S2S_KMER_MODEL_PROBES in all; no place found:
//   the adds go to the global table as in the table kernel.  Nothing waits for another wave.
//   Flush: every S2S_KMER_MODEL_FLUSH_ROUNDS rounds and after the walk every occupied slot adds its non-zero counters to the global
//   table and is cleared.  Whether a round flushes depends on the round number, the grid and B alone: uniform over the workgroup,
//   with a barrier before (every insertion of the interval has landed) and after (no insertion meets a half-cleared slot).
// Persistent workgroups: at most S2S_KMER_MODEL_MAX_WORKGROUPS (three per CU by LDS: 3 * 45,100 bytes of 160 KiB).
#define S2S_KMER_MODEL_EMPTY (-1)
__device__ __forceinline__ void s2s_kmer_model_flush(int* keys, unsigned long long (*cnt)[S2S_KMER_MODEL_SLOTS],
                                                     unsigned long long* __restrict__ table) {
    for (int i = threadIdx.x; i < S2S_KMER_MODEL_SLOTS; i += 256) {
        const int key = keys[i];
        if (key == S2S_KMER_MODEL_EMPTY) continue;
        unsigned long long* row = table + (size_t)key * S2S_KMER_MODEL_FIELDS;
#pragma unroll
        for (int f = 0; f < S2S_KMER_MODEL_FIELDS; ++f) {
            const unsigned long long v = cnt[f][i];
            if (v) __hip_atomic_fetch_add(row + f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cnt[f][i] = 0ull;
        }
        keys[i] = S2S_KMER_MODEL_EMPTY;
    }
}

template <int TD>
__global__ __launch_bounds__(256) void s2s_kmer_model_kernel(const float* __restrict__ signal, const int* __restrict__ dur,
                                                             const unsigned char* __restrict__ read_bytes,
                                                             const long long* __restrict__ chunk_start,
                                                             const unsigned char* __restrict__ n_valid, int B, float dig, float range,
                                                             float offset, unsigned long long* __restrict__ table, int te, int ts, int k) {
    __shared__ int keys[S2S_KMER_MODEL_SLOTS];
    __shared__ unsigned long long cnt[S2S_KMER_MODEL_FIELDS][S2S_KMER_MODEL_SLOTS];
    const int lane = threadIdx.x & 63, rows = (1 << (2 * k)) + 1;
    const bool direct = k <= S2S_KMER_MODEL_DIRECT_MAX_K;
    for (int i = threadIdx.x; i < S2S_KMER_MODEL_SLOTS; i += 256) {
        keys[i] = S2S_KMER_MODEL_EMPTY;
#pragma unroll
        for (int f = 0; f < S2S_KMER_MODEL_FIELDS; ++f) cnt[f][i] = 0ull;
    }
    __syncthreads();
    int round = 0;
    // (every wave of a workgroup runs the same rounds; a wave without a chunk skips the body -- wave-uniformly -- not the barriers)
    for (int b0 = blockIdx.x * 4; b0 < B; b0 += gridDim.x * 4) {
        const int b = b0 + (threadIdx.x >> 6);
        if (b < B) {
            int n, S, n_tail, s_tail;
            long long Q, q_tail;
            s2s_slot_stats_wave<TD>(signal, dur, b, lane, dig, range, offset, te, ts, n, S, Q, n_tail, s_tail, q_tail);
            int nv = n_valid[b];
            nv = nv > te ? te : nv;
            const bool real = lane < nv && n > 0;                   // an event: a real slot that owns stored samples
            int code = 0;
            long long ev = 0, m = 0, d = 0;
            if (real) {
                const unsigned char* p = read_bytes + chunk_start[b] + lane;
                bool other = false;
                for (int i = 0; i < k; ++i) {
                    const unsigned char ch = p[i];
                    const int dg = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
                    other |= dg < 0;
                    code = code * 4 + (dg & 3);
                }
                if (other) code = rows - 1;
                int64_t M, D;
                s2s_event_fixed_point(n, S, Q, M, D);
                ev = 1; m = M; d = D;
            }
            long long m2 = m * m, d2 = d * d;
            bool issue = real;
            unsigned long long todo = __ballot(real);
            while (todo) {                                          // wave-uniform: one round per distinct code of the chunk
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
                unsigned slot = direct ? (unsigned)code
                                       : (unsigned)(((unsigned long long)((unsigned)code * S2S_KMER_MODEL_HASH_MUL) * S2S_KMER_MODEL_SLOTS) >> 32);
                bool placed = false;
#pragma unroll
                for (int probe = 0; probe < S2S_KMER_MODEL_PROBES; ++probe) {
                    if (!placed) {
                        const int old = atomicCAS(&keys[slot], S2S_KMER_MODEL_EMPTY, code);
                        if (old == S2S_KMER_MODEL_EMPTY || old == code) placed = true;
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
        }
        ++round;
        if (round % S2S_KMER_MODEL_FLUSH_ROUNDS == 0 && b0 + (int)gridDim.x * 4 < B) {     // (the last round's flush is the one below)
            __syncthreads();
            s2s_kmer_model_flush(keys, cnt, table);
            __syncthreads();
        }
    }
    __syncthreads();
    s2s_kmer_model_flush(keys, cnt, table);
}

// ---- StreamVByte encoders of the output containers (codecs.py states the formats): one 256-thread workgroup per row.
// VARIANT 32 (slow5 svb-zd): [u32 n][(n+3)/4 control bytes, 2 bits per value][data: 1..4 bytes per value] of the zig-zag
// deltas widened to 32 bits; VARIANT 16 (pod5 VBZ before zstd): [(n+7)/8 control bytes, 1 bit per value][1..2 bytes per value]
// of the zig-zag deltas in 16-bit arithmetic.  A thread owns 8 consecutive values = one (svb16) or two (svb32) control bytes;
// their data bytes are placed by a block-wide prefix sum with a running carry.  WRITE = false only sizes the row.
template <int VARIANT, bool WRITE>
__global__ __launch_bounds__(256) void s2s_svb_kernel(const short* __restrict__ samples, const long long* __restrict__ read_offs,
                                                      const int* __restrict__ row_read, const int* __restrict__ row_index,
                                                      long long row_samples, int* __restrict__ row_bytes,
                                                      const long long* __restrict__ out_offs, unsigned char* __restrict__ out,
                                                      long long capacity) {
    __shared__ int wsum[4];
    __shared__ int carry_s;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rd = row_read[row];
    const long long r0 = read_offs[rd], rn = read_offs[rd + 1] - r0;
    const long long lo = (long long)row_index[row] * row_samples;
    long long n = rn - lo;
    if (n > row_samples) n = row_samples;
    if (n <= 0) {                                            // a candidate row the read turned out not to need
        if (!WRITE && tid == 0) row_bytes[row] = 0;
        return;
    }
    const short* x = samples + r0 + lo;
    const long long nkeys = (VARIANT == 32) ? (n + 3) / 4 : (n + 7) / 8;
    const int hdr = (VARIANT == 32) ? 4 : 0;
    unsigned char* o = nullptr;
    if (WRITE) {
        const long long base = out_offs[row];
        if (out_offs[row + 1] > capacity) return;            // does not fit: skipped, and s2s_svb_check_kernel reports it
        o = out + base;
        if (VARIANT == 32 && tid == 0) { const unsigned nn = (unsigned)n; o[0] = nn; o[1] = nn >> 8; o[2] = nn >> 16; o[3] = nn >> 24; }
    }
    if (tid == 0) carry_s = 0;
    __syncthreads();
    // a thread's nine samples of a step (its eight + the one before them) are loaded one step ahead: the steps of a row are a
    // serial chain (the carry), and without the prefetch each one began with a full memory round trip
    short raw[9];
    auto fetch = [&](long long t0) {
        const long long j0 = t0 + 8 * (long long)tid;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const long long j = j0 + i - 1;
            raw[i] = (j >= 0 && j < n) ? x[j] : (short)0;     // (the delta of a row's first value is against 0)
        }
    };
    fetch(0);
    for (long long t0 = 0; t0 < n; t0 += 2048) {
        const long long j0 = t0 + 8 * (long long)tid;
        unsigned v[8];
        int len[8], tot = 0;
        unsigned key = 0;
        int prev = raw[0];
        short now[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) now[i] = raw[i + 1];
        if (t0 + 2048 < n) fetch(t0 + 2048);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            len[i] = 0; v[i] = 0;
            if (j0 + i < n) {
                const int cur = now[i];
                if (VARIANT == 32) {
                    const int d = cur - prev;
                    v[i] = ((unsigned)d << 1) ^ (unsigned)(d >> 31);
                    len[i] = 1 + (v[i] > 0xFFu) + (v[i] > 0xFFFFu) + (v[i] > 0xFFFFFFu);
                    key |= (unsigned)(len[i] - 1) << (2 * i);
                } else {
                    const short d = (short)((unsigned short)cur - (unsigned short)prev);
                    v[i] = (unsigned short)(((int)d + (int)d) ^ ((int)d >> 15));
                    len[i] = 1 + (v[i] > 0xFFu);
                    key |= (unsigned)(len[i] - 1) << i;
                }
                prev = cur;
                tot += len[i];
            }
        }
        int incl = tot;                                       // block-wide exclusive prefix of `tot`
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(incl, off, 64); if (lane >= off) incl += y; }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int pre = carry_s + incl - tot;
        for (int k = 0; k < w; ++k) pre += wsum[k];
        if (WRITE && j0 < n) {
            if (VARIANT == 32) {
                o[hdr + j0 / 4] = (unsigned char)key;
                if (j0 + 4 < n) o[hdr + j0 / 4 + 1] = (unsigned char)(key >> 8);
            } else {
                o[j0 / 8] = (unsigned char)key;
            }
            unsigned char* d = o + hdr + nkeys + pre;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                for (int k = 0; k < len[i]; ++k) *d++ = (unsigned char)(v[i] >> (8 * k));
        }
        __syncthreads();
        if (tid == 255) carry_s = pre + tot;
        __syncthreads();
    }
    if (!WRITE && tid == 0) row_bytes[row] = (int)(hdr + nkeys + carry_s);
}

// s2s_svb_encode's overflow report: rows that do not fit are skipped by the WRITE pass; the total then comes back negative
__global__ void s2s_svb_check_kernel(long long* __restrict__ out_offs, int n, long long capacity) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && out_offs[n] > capacity) out_offs[n] = -out_offs[n];
}

__global__ void s2s_philox_kernel(unsigned seed_lo, unsigned seed_hi, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                  int n, unsigned* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32x4 r = philox4x32_10(c0 + (unsigned)i, c1, c2, c3, seed_lo, seed_hi);
    out[4 * i + 0] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
}

// ================================================================================ host side
namespace {

thread_local std::string g_create_error;

struct EventPair { hipEvent_t a, b; int chunks; };

}  // namespace

struct s2s_handle {
    s2s_config cfg;
    int device = 0;
    ModelDev model;
    char* slab = nullptr;             // ONE device allocation made by s2s_create: weights, hand-off slots, first scratch buffers
    size_t slab_bytes = 0;
    float* d_arena = nullptr;
    size_t arena_floats = 0;
    int tile = 0;                     // chunks per launch pair
    int n_wg = 256;                   // decoder grid: persistent workgroups, one per CU
    float* handoff = nullptr;         // frontend -> decoder slots: [n_wg][S2S_MAX_GROUP][S2S_SLOT_FLOATS] (L2-resident)
    int* ws_counts = nullptr;         // export scratch, grown on demand outside of launches
    long long* ws_offs = nullptr;
    int ws_export_cap = 0;
    int* ws_svb = nullptr;            // s2s_svb_encode scratch: bytes per row
    int ws_svb_cap = 0;
    bool profiling = false;
    unsigned long long* d_diag = nullptr;   // S2S_DIAG builds: [8 waves][48] per-phase wave-cycle sums (S2S_TILEHIST: the tile histogram)
    unsigned long long* d_stats = nullptr;  // S2S_STAT_* counters of the predict kernel (inside the slab; s2s_stats_read)
    long long stat_chunks = 0;              // chunks launched since the last s2s_stats_read
    int attn_exact = 0;                     // decoder attention path of the split-f16 modes (s2s_set_attention_path)
    long long stat_exact_chunks = 0;        // ... chunks launched on the exact path since the last s2s_stats_read
    int schedule = S2S_SCHEDULE_AUTO;       // how a launch is dealt out to the workgroups (s2s_set_schedule)
    long long stat_dynamic_chunks = 0;      // ... chunks launched on the dynamic schedule since the last s2s_stats_read
    double calib_redo_rate = -1.0;          // share of the calibration launch's softmax runs that overflowed the fast path (-1: not calibrated)
    std::vector<EventPair> events;
    std::string err;
    // S2S_MODE_GENERIC / _GENERIC_F16 / _GENERIC_GEOMETRY / _GENERIC_GEOMETRY_F16 (s2s_generic.h, s2s_generic_h.h): blob offsets into d_arena, and the slice workspace (grown on
    // demand, s2s_predict_*)
    struct Generic {
        int d = 0, dff = 0, h_enc = 0, h_dec = 0;
        int te = 16, ts = 250;        // chunk geometry: max_dna_len, max_signal_len (the checkpoint's in the two geometry modes)
        bool f16 = false;             // S2S_MODE_GENERIC_F16 / _GEOMETRY_F16: the decoder FFT blocks on f16 operands (dech)
        long long pe_enc = 0, pe_dec = 0, emb_wt = 0, emb_b = 0, out_w = 0, out_b = 0, w0cat = 0, b0cat = 0;
        long long pre_w[S2S_MAX_LAYERS] = {}, pre_b[S2S_MAX_LAYERS] = {};
        GenLayer enc[S2S_MAX_LAYERS] = {}, dec[S2S_MAX_LAYERS] = {};
        GenLayerH dech[S2S_MAX_LAYERS] = {};
        GenHeads heads = {};
        int ld_d = 0, ld_f = 0;       // row pitch (halves) of the f16 weights with K = dmodel / dff
        int slice_max = 0;            // chunks per slice (S2S_GENERIC_WORKSPACE_BYTES)
        float* ws = nullptr;
        int ws_chunks = 0;            // slice capacity of ws
    } gen;
    float* ev_ws = nullptr;           // s2s_evaluate_chunks: y, sigma, conc, rate of one slice (grown on demand)
    int ev_chunks = 0;
};

namespace {

int fail(s2s_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((h), S2S_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// A kernel launch and the error it left, if any.  A kernel with a comma in its template arguments goes in parentheses.
#define S2S_LAUNCH(h, kernel, grid, block, lds, stream, ...)                    \
    do {                                                                        \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);      \
        HIP_TRY(h, hipGetLastError());                                          \
    } while (0)

// The ABI's int64_t is the kernels' long long.
static_assert(sizeof(int64_t) == sizeof(long long), "int64_t arrays are passed to the kernels as long long");
inline const long long* as_ll(const int64_t* p) { return reinterpret_cast<const long long*>(p); }
inline long long* as_ll(int64_t* p) { return reinterpret_cast<long long*>(p); }

// Scratch that has outgrown its first home inside the handle's slab is an allocation of its own.
void free_scratch(s2s_handle* h, void* p) {
    const char* c = static_cast<const char*>(p);
    if (p && !(h->slab && c >= h->slab && c < h->slab + h->slab_bytes)) (void)hipFree(p);
}

// Makes the handle's device current for the duration of a call and restores the caller's device afterwards.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
        else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// The guard of a handle-free entry, `guard`, for the rest of the function; RETURNS S2S_ERR_HIP where the device cannot be made current.
// Two statements: it stands as a statement of its own at function scope, never under an un-braced `if` or `else`.
#define GUARD_OR_RETURN(h, dev) \
    DeviceGuard guard(dev);     \
    if (!guard.ok) return fail((h), S2S_ERR_HIP, "hipSetDevice failed")

size_t layer_floats() { return 4 * (64 * 64 + 64) + 2 * 64 + (256 * 64 + 256) + (64 * 256 + 64) + 2 * 64; }
size_t mlp_floats() { return 64 * 64 + 64 + 64 + 1; }

bool mode_generic(int m) {
    return m == S2S_MODE_GENERIC || m == S2S_MODE_GENERIC_F16 || m == S2S_MODE_GENERIC_GEOMETRY || m == S2S_MODE_GENERIC_GEOMETRY_F16;
}
bool mode_geometry(int m) { return m == S2S_MODE_GENERIC_GEOMETRY || m == S2S_MODE_GENERIC_GEOMETRY_F16; }

// S2S_MODE_GENERIC_GEOMETRY_F16 has S2S_MODE_GENERIC_GEOMETRY's limits; its refusals name it instead (the other modes' messages
// are unchanged: text + tag)
#define GEN_REFUSE(text, tag) return g7 ? text " (S2S_MODE_GENERIC_GEOMETRY_F16)" : text tag
const char* check_cfg_generic(const s2s_config* c) {
    const bool g7 = c->compute_mode == S2S_MODE_GENERIC_GEOMETRY_F16;
    if (mode_geometry(c->compute_mode)) {
        if (c->max_dna_len < 1 || c->max_dna_len > S2S_GEOMETRY_MAX_DNA_LEN) GEN_REFUSE("max_dna_len must be 1..64", " (S2S_MODE_GENERIC_GEOMETRY)");
        if (c->max_signal_len < 1 || c->max_signal_len > S2S_GEOMETRY_MAX_SIGNAL_LEN)
            GEN_REFUSE("max_signal_len must be 1..1024", " (S2S_MODE_GENERIC_GEOMETRY)");
    } else {
        if (c->max_dna_len != S2S_T_ENC) return "max_dna_len must be 16";
        if (c->max_signal_len != S2S_T_DEC) return "max_signal_len must be 250";
    }
    if (c->dmodel < 16 || c->dmodel > 512 || c->dmodel % 16) GEN_REFUSE("dmodel must be a multiple of 16 in 16..512", " (S2S_MODE_GENERIC)");
    if (c->dff < 8 || c->dff > 2048 || c->dff % 8) GEN_REFUSE("dff must be a multiple of 8 in 8..2048", " (S2S_MODE_GENERIC)");
    if (c->n_heads < 1 || c->n_heads > 16 || c->dmodel % c->n_heads)
        GEN_REFUSE("n_heads (encoder heads) must be 1..16 and divide dmodel", " (S2S_MODE_GENERIC)");
    if (c->decoder_heads < 0 || c->decoder_heads > 16 || (c->decoder_heads && c->dmodel % c->decoder_heads))
        GEN_REFUSE("decoder_heads must be 0 (= n_heads) or 1..16 and divide dmodel", " (S2S_MODE_GENERIC)");
    if (c->encoder_layers < 1 || c->encoder_layers > S2S_MAX_LAYERS) GEN_REFUSE("encoder_layers must be 1..4", "");
    if (c->decoder_layers < 1 || c->decoder_layers > S2S_MAX_LAYERS) GEN_REFUSE("decoder_layers must be 1..4", "");
    if (c->pre_layers < 0 || c->pre_layers > S2S_MAX_LAYERS) GEN_REFUSE("pre_layers must be 0..4", "");
    return nullptr;
}
#undef GEN_REFUSE

const char* check_cfg(const s2s_config* c) {
    if (!c) return "config is NULL";
    if (c->seq_kmer < 1 || c->seq_kmer > 16) return "seq_kmer must be 1..16";
    if (mode_generic(c->compute_mode)) return check_cfg_generic(c);
    if (c->max_dna_len != S2S_T_ENC) return "max_dna_len must be 16";
    if (c->max_signal_len != S2S_T_DEC) return "max_signal_len must be 250";
    if (c->dmodel != S2S_DMODEL) return "dmodel must be 64";
    if (c->dff != S2S_DFF) return "dff must be 256";
    if (c->n_heads != S2S_HEADS) return "n_heads must be 8";
    if (c->encoder_layers < 1 || c->encoder_layers > S2S_MAX_LAYERS) return "encoder_layers must be 1..4";
    if (c->decoder_layers < 1 || c->decoder_layers > S2S_MAX_LAYERS) return "decoder_layers must be 1..4";
    if (c->pre_layers < 0 || c->pre_layers > S2S_MAX_LAYERS) return "pre_layers must be 0..4";
    if (c->compute_mode != S2S_MODE_F32 && c->compute_mode != S2S_MODE_F16X3 && c->compute_mode != S2S_MODE_F16)
        return "compute_mode must be S2S_MODE_F32, S2S_MODE_F16X3 or S2S_MODE_F16";
    if (c->decoder_heads != 0 && c->decoder_heads != c->n_heads) return "decoder_heads must be 0 or equal to n_heads (8)";
    return nullptr;
}

int cfg_dec_heads(const s2s_config* c) { return c->decoder_heads ? c->decoder_heads : c->n_heads; }

size_t generic_layer_floats(size_t d, size_t f) { return 4 * (d * d + d) + 2 * d + (f * d + f) + (d * f + d) + 2 * d; }

// fp32 floats of one chunk in the generic workspace: XE [te][d], SIG [te], XD [ts][d], SE [ts], BIG [max(te, ts)][max(3d, dff)]
// (te / ts = max_dna_len / max_signal_len: 16 / 250 outside S2S_MODE_GENERIC_GEOMETRY and S2S_MODE_GENERIC_GEOMETRY_F16)
size_t generic_chunk_floats(const s2s_config* c) {
    const size_t d = c->dmodel, big = 3 * d > (size_t)c->dff ? 3 * d : (size_t)c->dff;
    const size_t te = c->max_dna_len, ts = c->max_signal_len, tb = te > ts ? te : ts;
    return te * d + te + ts * d + ts + tb * big;
}

// Arena builder: every piece starts on a 16-byte boundary (float4 loads).
struct Arena {
    std::vector<float> v;
    int put(const float* p, size_t n) {
        while (v.size() % 4) v.push_back(0.0f);
        const int off = (int)v.size();
        v.insert(v.end(), p, p + n);
        return off;
    }
    // W [M][K] row-major -> A fragments [M/16][K/16][64 lanes][4]; lane (g, i): W[perm(16mt+i)][16kt+4g+r]
    int put_afrag(const float* W, int M, int K, bool qk_perm) {
        std::vector<float> t((size_t)M * K);
        for (int mt = 0; mt < M / 16; ++mt)
            for (int kt = 0; kt < K / 16; ++kt)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15;
                    const int row = 16 * mt + (qk_perm ? perm16(i) : i);
                    for (int r = 0; r < 4; ++r)
                        t[(((size_t)mt * (K / 16) + kt) * 64 + lane) * 4 + r] = W[(size_t)row * K + 16 * kt + 4 * g + r];
                }
        return put(t.data(), t.size());
    }
    int put_bias_perm(const float* b, int M) {
        std::vector<float> t(M);
        for (int i = 0; i < M; ++i) t[i] = b[16 * (i / 16) + perm16(i % 16)];
        return put(t.data(), t.size());
    }
    // packed row i = 4g'+r' of a q/k tile takes natural row 8*(r'>>1) + 2g' + (r'&1): after the MFMA,
    // accumulator registers {0,1} hold head 0 (d = 2g, 2g+1) and {2,3} head 1 of the pair.
    static int perm16(int i) { return 8 * ((i & 3) >> 1) + 2 * (i >> 2) + (i & 1); }
};

const float* take(const float*& p, size_t n) { const float* q = p; p += n; return q; }

// w = hi + lo with hi = f16(w), lo = f16(w - hi) (round to nearest even), for a whole matrix at once.  The host compiler turns a
// plain _Float16 cast into a library call unless F16C code generation is on, and s2s_create converts half a million weights:
// the F16C instance does eight per instruction and is picked at run time where the CPU has it.
struct SplitF16 {
    std::vector<_Float16> hi, lo;
};
void split_f16_generic(const float* w, size_t n, _Float16* hi, _Float16* lo) {
    for (size_t i = 0; i < n; ++i) {
        hi[i] = (_Float16)w[i];
        lo[i] = (_Float16)(w[i] - (float)hi[i]);
    }
}
__attribute__((target("avx,f16c"))) void split_f16_f16c(const float* w, size_t n, _Float16* hi, _Float16* lo) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const __m256 x = _mm256_loadu_ps(w + i);
        const __m128i h = _mm256_cvtps_ph(x, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC);
        const __m128i l = _mm256_cvtps_ph(_mm256_sub_ps(x, _mm256_cvtph_ps(h)), _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC);
        _mm_storeu_si128(reinterpret_cast<__m128i*>(hi + i), h);
        _mm_storeu_si128(reinterpret_cast<__m128i*>(lo + i), l);
    }
    for (; i < n; ++i) {
        const __m128i h = _mm_cvtps_ph(_mm_set_ss(w[i]), _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC);
        const float back = _mm_cvtss_f32(_mm_cvtph_ps(h));
        const __m128i l = _mm_cvtps_ph(_mm_set_ss(w[i] - back), _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC);
        const unsigned short hb = (unsigned short)_mm_extract_epi16(h, 0), lb = (unsigned short)_mm_extract_epi16(l, 0);
        std::memcpy(hi + i, &hb, 2);
        std::memcpy(lo + i, &lb, 2);
    }
}
SplitF16 split_f16(const float* w, size_t n) {
    SplitF16 s;
    s.hi.resize(n);
    s.lo.resize(n);
    static const bool fast = __builtin_cpu_supports("f16c") && __builtin_cpu_supports("avx");
    (fast ? split_f16_f16c : split_f16_generic)(w, n, s.hi.data(), s.lo.data());
    return s;
}

LayerOff pack_layer(Arena& A, const float*& p) {
    LayerOff L;
    const float* wq = take(p, 4096); const float* bq = take(p, 64);
    const float* wk = take(p, 4096); const float* bk = take(p, 64);
    const float* wv = take(p, 4096); const float* bv = take(p, 64);
    const float* wfc = take(p, 4096); const float* bfc = take(p, 64);
    const float* ln1g = take(p, 64); const float* ln1b = take(p, 64);
    const float* w1 = take(p, 256 * 64); const float* b1 = take(p, 256);
    const float* w2 = take(p, 64 * 256); const float* b2 = take(p, 64);
    const float* ln2g = take(p, 64); const float* ln2b = take(p, 64);
    // weight stream in the order fft_block consumes it (one unit = 4 fragments = 4 KiB):
    //   K/V phase : per head pair p: Wk rows of p (k-tiles 0..3), Wv rows of p
    //   attention : per pair p: Wq rows of p, Wfc columns of p (m-tiles 0..3)
    //   FFN       : per 64-wide hidden slice hc: W1 m-tiles 4hc..4hc+3, then W2 m-tiles 0..3 x k-tiles 4hc..4hc+3
    std::vector<float> st;
    st.reserve(4 * 4096 + 2 * 256 * 64 + 1024);
    auto frag = [&](const float* Wm, int K, int mt, int kt, bool perm) {
        for (int lane = 0; lane < 64; ++lane) {
            const int g = lane >> 4, i = lane & 15;
            const int row = 16 * mt + (perm ? Arena::perm16(i) : i);
            for (int r = 0; r < 4; ++r) st.push_back(Wm[(size_t)row * K + 16 * kt + 4 * g + r]);
        }
    };
    for (int p_ = 0; p_ < 4; ++p_) {
        for (int kt = 0; kt < 4; ++kt) frag(wk, 64, p_, kt, true);
        for (int kt = 0; kt < 4; ++kt) frag(wv, 64, p_, kt, false);
    }
    for (int p_ = 0; p_ < 4; ++p_) {
        for (int kt = 0; kt < 4; ++kt) frag(wq, 64, p_, kt, true);
        for (int mt = 0; mt < 4; ++mt) frag(wfc, 64, mt, p_, false);
    }
    for (int hc = 0; hc < 4; ++hc) {
        for (int mt = 0; mt < 4; ++mt)
            for (int kt = 0; kt < 4; ++kt) frag(w1, 64, 4 * hc + mt, kt, false);
        for (int mt = 0; mt < 4; ++mt)
            for (int kt = 0; kt < 4; ++kt) frag(w2, 256, mt, 4 * hc + kt, false);
    }
    st.resize(st.size() + 1024, 0.0f);       // the block's last prefetch reads one unit past its stream
    L.stream = A.put(st.data(), st.size());
    // the same units for the split-f16 block: per (m-tile, k-block of 32) a hi and a lo fragment of
    // 64 lanes x 8 halves; lane (g, i), element j: W[16mt + i][kbase + 16(j>>2) + 4g + (j&3)].
    // Wq and bq go in pre-multiplied by log2(e)/sqrt(d_k): Q leaves its GEMM in the units the softmax wants (layers.py:32-33).
    const float c1 = 1.4426950408889634f * 0.35355339059327373f;
    std::vector<float> wq_s(wq, wq + 4096), bq_s(bq, bq + 64);
    for (float& v : wq_s) v *= c1;
    for (float& v : bq_s) v *= c1;
    std::vector<_Float16> sh;
    sh.reserve(2 * (4 * 4096 + 2 * 256 * 64) + 4 * 2048);
    const SplitF16 hk = split_f16(wk, 4096), hv = split_f16(wv, 4096), hq = split_f16(wq_s.data(), 4096), hfc = split_f16(wfc, 4096);
    const SplitF16 h1 = split_f16(w1, 256 * 64), h2 = split_f16(w2, 64 * 256);
    auto frag_h = [&](const SplitF16& Wm, int K, int mt, int kbase, bool lo) {
        const _Float16* src = lo ? Wm.lo.data() : Wm.hi.data();
        for (int lane = 0; lane < 64; ++lane) {
            const int g = lane >> 4, i = lane & 15;
            for (int j = 0; j < 8; ++j) sh.push_back(src[(size_t)(16 * mt + i) * K + kbase + 16 * (j >> 2) + 4 * g + (j & 3)]);
        }
    };
    auto unit_h = [&](const SplitF16& Wm, int K, int mt, int kbase) {      // [kb0 hi][kb0 lo][kb1 hi][kb1 lo]
        for (int kb = 0; kb < 2; ++kb) { frag_h(Wm, K, mt, kbase + 32 * kb, false); frag_h(Wm, K, mt, kbase + 32 * kb, true); }
    };
    for (int p_ = 0; p_ < 4; ++p_) { unit_h(hk, 64, p_, 0); unit_h(hv, 64, p_, 0); }
    for (int u = 0; u < 2; ++u) {
        unit_h(hq, 64, 2 * u, 0);
        unit_h(hq, 64, 2 * u + 1, 0);
        for (int mt = 0; mt < 4; ++mt) { frag_h(hfc, 64, mt, 32 * u, false); frag_h(hfc, 64, mt, 32 * u, true); }
    }
    for (int hc = 0; hc < 4; ++hc) {
        for (int mt = 0; mt < 4; ++mt) unit_h(h1, 64, 4 * hc + mt, 0);
        for (int mt = 0; mt < 4; ++mt) unit_h(h2, 256, mt, 64 * hc);
    }
    sh.resize(sh.size() + 4 * 2048, (_Float16)0.0f);   // the FFN ring runs three units past the end of the stream
    {
        std::vector<float> raw(sh.size() / 2);
        std::memcpy(raw.data(), sh.data(), sh.size() * sizeof(_Float16));
        L.stream_h = A.put(raw.data(), raw.size());
        // hi-only stream for the single-product mode: every even 512-half fragment of the stream above
        std::vector<_Float16> sf;
        for (size_t f0 = 0; f0 + 1024 <= sh.size(); f0 += 1024) sf.insert(sf.end(), sh.begin() + f0, sh.begin() + f0 + 512);
        std::vector<float> rawf(sf.size() / 2);
        std::memcpy(rawf.data(), sf.data(), sf.size() * sizeof(_Float16));
        L.stream_f = A.put(rawf.data(), rawf.size());
    }
    L.bq_nat = A.put(bq_s.data(), 64);         // (f16 blocks only; the f32 block reads L.bq)
    L.bk_nat = A.put(bk, 64);
    L.bq = A.put_bias_perm(bq, 64);
    L.bk = A.put_bias_perm(bk, 64);
    L.bv = A.put(bv, 64);
    L.bfc = A.put(bfc, 64);
    L.b1 = A.put(b1, 256);
    L.b2 = A.put(b2, 64);
    L.ln1g = A.put(ln1g, 64); L.ln1b = A.put(ln1b, 64);
    L.ln2g = A.put(ln2g, 64); L.ln2b = A.put(ln2b, 64);
    return L;
}

// a 64x64 Linear as 4 f16 units (one per m-tile): [kb0 hi][kb0 lo][kb1 hi][kb1 lo], same fragment order as pack_layer
int pack_linear64_h(Arena& A, const float* Wm) {
    const SplitF16 hw = split_f16(Wm, 4096);
    std::vector<_Float16> sh;
    sh.reserve(2 * 4096);
    for (int mt = 0; mt < 4; ++mt)
        for (int kb = 0; kb < 2; ++kb)
            for (int lo = 0; lo < 2; ++lo) {
                const _Float16* src = lo ? hw.lo.data() : hw.hi.data();
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15;
                    for (int j = 0; j < 8; ++j) sh.push_back(src[(size_t)(16 * mt + i) * 64 + 32 * kb + 16 * (j >> 2) + 4 * g + (j & 3)]);
                }
            }
    std::vector<float> raw(sh.size() / 2);
    std::memcpy(raw.data(), sh.data(), sh.size() * sizeof(_Float16));
    return A.put(raw.data(), raw.size());
}

MlpOff pack_mlp(Arena& A, const float*& p) {
    MlpOff m;
    const float* w0 = take(p, 4096); const float* b0 = take(p, 64);
    const float* w3 = take(p, 64);   const float* b3 = take(p, 1);
    m.w0 = A.put_afrag(w0, 64, 64, false); m.b0 = A.put(b0, 64);
    m.w0h = pack_linear64_h(A, w0);
    m.w3 = A.put(w3, 64); m.b3 = A.put(b3, 1);
    return m;
}

// S2S_MODE_GENERIC: the blob in its native [out][in] layouts (the GEMM reads nn.Linear weights as they are), except src_emb.weight
// transposed to [5k][d] (a one-hot column is one contiguous row) and the three q/k/v projections and the three heads' first
// layers each concatenated into one [3d][d] matrix with its [3d] bias.
void pack_generic(Arena& A, s2s_handle::Generic& G, const s2s_config* cfg, const float* p) {
    const int d = cfg->dmodel, f = cfg->dff, k = cfg->seq_kmer;
    const size_t dd = (size_t)d * d;
    G.d = d; G.dff = f; G.h_enc = cfg->n_heads; G.h_dec = cfg_dec_heads(cfg);
    G.te = cfg->max_dna_len; G.ts = cfg->max_signal_len;
    G.pe_enc = A.put(take(p, G.te * (size_t)d), G.te * (size_t)d);
    {
        const float* w = take(p, (size_t)d * 5 * k);
        std::vector<float> wt((size_t)5 * k * d);
        for (int o = 0; o < d; ++o)
            for (int i = 0; i < 5 * k; ++i) wt[(size_t)i * d + o] = w[(size_t)o * 5 * k + i];
        G.emb_wt = A.put(wt.data(), wt.size());
        G.emb_b = A.put(take(p, d), d);
    }
    for (int i = 0; i < cfg->pre_layers; ++i) { G.pre_w[i] = A.put(take(p, dd), dd); G.pre_b[i] = A.put(take(p, d), d); }
    auto layer = [&](GenLayer& L) {
        std::vector<float> w(3 * dd), b(3 * (size_t)d);
        for (int j = 0; j < 3; ++j) {                        // w_qs, w_ks, w_vs: weight then bias each
            std::memcpy(w.data() + j * dd, take(p, dd), dd * sizeof(float));
            std::memcpy(b.data() + (size_t)j * d, take(p, d), d * sizeof(float));
        }
        L.wqkv = A.put(w.data(), w.size()); L.bqkv = A.put(b.data(), b.size());
        L.wfc = A.put(take(p, dd), dd); L.bfc = A.put(take(p, d), d);
        L.ln1g = A.put(take(p, d), d); L.ln1b = A.put(take(p, d), d);
        L.w1 = A.put(take(p, (size_t)f * d), (size_t)f * d); L.b1 = A.put(take(p, f), f);
        L.w2 = A.put(take(p, (size_t)d * f), (size_t)d * f); L.b2 = A.put(take(p, d), d);
        L.ln2g = A.put(take(p, d), d); L.ln2b = A.put(take(p, d), d);
    };
    for (int l = 0; l < cfg->encoder_layers; ++l) layer(G.enc[l]);
    {   // noise_sampler.stdv_layer, duration_sampler.conc_layer, .rate_layer: 0.weight [d][d], 0.bias [d], 3.weight [d], 3.bias [1]
        std::vector<float> w(3 * dd), b(3 * (size_t)d);
        std::vector<float> w3[3], b3[3];
        for (int j = 0; j < 3; ++j) {
            std::memcpy(w.data() + j * dd, take(p, dd), dd * sizeof(float));
            std::memcpy(b.data() + (size_t)j * d, take(p, d), d * sizeof(float));
            const float* x = take(p, d); w3[j].assign(x, x + d);
            const float* y = take(p, 1); b3[j].assign(y, y + 1);
        }
        G.w0cat = A.put(w.data(), w.size()); G.b0cat = A.put(b.data(), b.size());
        for (int j = 0; j < 3; ++j) { G.heads.w3[j] = A.put(w3[j].data(), d); G.heads.b3[j] = A.put(b3[j].data(), 1); }
    }
    G.pe_dec = A.put(take(p, G.ts * (size_t)d), G.ts * (size_t)d);
    for (int l = 0; l < cfg->decoder_layers; ++l) layer(G.dec[l]);
    G.f16 = cfg->compute_mode == S2S_MODE_GENERIC_F16 || cfg->compute_mode == S2S_MODE_GENERIC_GEOMETRY_F16;
    if (G.f16) {   // the decoder's four weight matrices once more, rounded to f16, rows zero-padded to K rounded up to 32 (gen_gemm_h_kernel)
        G.ld_d = (d + 31) & ~31;
        G.ld_f = (f + 31) & ~31;
        auto put_h = [&](long long off, int rows, int K, int ldw) {
            const SplitF16 h = split_f16(A.v.data() + off, (size_t)rows * K);
            std::vector<_Float16> t((size_t)rows * ldw, (_Float16)0.0f);
            for (int r = 0; r < rows; ++r) std::memcpy(t.data() + (size_t)r * ldw, h.hi.data() + (size_t)r * K, K * sizeof(_Float16));
            std::vector<float> raw(t.size() / 2);
            std::memcpy(raw.data(), t.data(), t.size() * sizeof(_Float16));
            return (long long)A.put(raw.data(), raw.size());
        };
        for (int l = 0; l < cfg->decoder_layers; ++l) {
            const GenLayer& L = G.dec[l];
            G.dech[l].wqkv = put_h(L.wqkv, 3 * d, d, G.ld_d);
            G.dech[l].wfc = put_h(L.wfc, d, d, G.ld_d);
            G.dech[l].w1 = put_h(L.w1, f, d, G.ld_d);
            G.dech[l].w2 = put_h(L.w2, d, f, G.ld_f);
        }
    }
    G.out_w = A.put(take(p, d), d);
    G.out_b = A.put(take(p, 1), 1);
    size_t slice = S2S_GENERIC_WORKSPACE_BYTES / (4 * generic_chunk_floats(cfg));
    // The attention kernels launch one workgroup per (chunk, head) -- per (chunk, head, 64 queries) beyond 256 keys -- of up to 1024
    // threads, and a launch holds fewer than 2^32 threads in all: at a tiny geometry (1 / 1: 82 floats per chunk) the workspace
    // alone would allow a slice whose attention grid wraps, and the chunks past the wrap would keep Q where O belongs.
    const size_t heads = cfg->n_heads > cfg_dec_heads(cfg) ? cfg->n_heads : cfg_dec_heads(cfg);
    const size_t per_head = cfg->max_signal_len > 256 ? (size_t)((cfg->max_signal_len + 63) / 64) * 256 : 1024;
    const size_t grid_cap = 0xFFFFFFFFull / (heads * per_head);
    if (slice > grid_cap) slice = grid_cap;
    G.slice_max = slice < 1 ? 1 : (int)slice;
}

ParamsDev to_dev(const s2s_params* p) {
    ParamsDev d;
    d.dwell_mean = p->dwell_mean; d.dwell_std = p->dwell_std; d.noise_std = p->noise_std;
    d.min_noise = p->min_noise; d.min_duration = p->min_duration;
    d.noise_sampling = p->noise_sampling; d.duration_sampling = p->duration_sampling;
    d.seed_lo = (unsigned)p->seed; d.seed_hi = (unsigned)(p->seed >> 32);
    return d;
}

}  // namespace

// ---- S2S_MODE_GENERIC and its three siblings: the launch side of the size-generic pipeline
#include "s2s_generic_host.h"

extern "C" {

size_t s2s_blob_floats(const s2s_config* c) {
    if (check_cfg(c)) return 0;
    if (mode_generic(c->compute_mode)) {
        const size_t d = c->dmodel, f = c->dff;
        const size_t te = c->max_dna_len, ts = c->max_signal_len;     // 16 / 250 outside the two geometry modes
        return te * d + d * 5 * c->seq_kmer + d + (size_t)c->pre_layers * (d * d + d) +
               (size_t)(c->encoder_layers + c->decoder_layers) * generic_layer_floats(d, f) + 3 * (d * d + d + d + 1) + ts * d + d + 1;
    }
    return (size_t)16 * 64 + (size_t)64 * 5 * c->seq_kmer + 64 + (size_t)c->pre_layers * (4096 + 64) +
           (size_t)(c->encoder_layers + c->decoder_layers) * layer_floats() + 3 * mlp_floats() + (size_t)250 * 64 + 64 + 1;
}

static int predict_impl(s2s_handle* h, void* stream_, const uint8_t* bases, const int64_t* chunk_start, const uint8_t* n_valid, int64_t first_global_chunk,
                        int32_t B, const s2s_params* params, const float* inject_g, const float* inject_zdw,
                        const float* inject_z01, float* out_signal, int32_t* out_dur, const s2s_debug* dbg);

// Which softmax path the split-f16 decoder tries first is a property of the WEIGHTS: one launch of 512 pseudo-random chunks with the
// default samplers on the fast path counts the heads it had to redo (the production counters); above S2S_ATTENTION_REDO_THRESHOLD the handle starts
// every head on the exact path (s2s_device_h.h: the online softmax as its own kernel instance).  A fixed input, so the same weights always get the same
// answer, on any device.  The export scratch inside the slab holds the launch's buffers.
static int calibrate_attention(s2s_handle* h) {
    if (h->cfg.compute_mode == S2S_MODE_F32 || mode_generic(h->cfg.compute_mode)) return S2S_OK;
    const int B = 512, nb = S2S_T_ENC + h->cfg.seq_kmer - 1;
    std::vector<uint8_t> host((size_t)B * nb + B);
    uint32_t x = 0x9E3779B9u;
    for (size_t i = 0; i < (size_t)B * nb; ++i) { x = x * 1664525u + 1013904223u; host[i] = "ACGT"[x >> 30]; }
    for (int i = 0; i < B; ++i) host[(size_t)B * nb + i] = S2S_T_ENC;
    char* base = reinterpret_cast<char*>(h->ws_offs);               // (5 * 32768 + 1) * 8 bytes
    float* sig = reinterpret_cast<float*>(base);
    int32_t* dur = reinterpret_cast<int32_t*>(base + (size_t)B * S2S_T_DEC * 4);
    uint8_t* d_bases = reinterpret_cast<uint8_t*>(base + (size_t)B * S2S_T_DEC * 4 + (size_t)B * 16 * 4);
    static_assert((size_t)512 * S2S_T_DEC * 4 + 512 * 16 * 4 + 512 * 32 + 512 <= (size_t)(5 * 32768 + 1) * 8, "calibration buffers fit the export scratch");
    HIP_TRY(h, hipMemcpy(d_bases, host.data(), host.size(), hipMemcpyHostToDevice));
    const s2s_params P = {12.5f, 0.0f, 2.0f, 0.0f, 3.0f, 1, 1, 0};
    h->attn_exact = 0;
    // (an empty s2s_debug selects the TEST instance of the kernel -- same arithmetic, same counters: the production instance's
    // first dispatch and its average in a profile stay those of the caller's launches)
    s2s_debug none;
    std::memset(&none, 0, sizeof none);
    const int rc = predict_impl(h, nullptr, d_bases, nullptr, d_bases + (size_t)B * nb, 0, B, &P, nullptr, nullptr, nullptr, sig, dur, &none);
    if (rc != S2S_OK) return rc;
    uint64_t st[10];
    const int rs = s2s_stats_read(h, st);
    if (rs != S2S_OK) return rs;
    h->calib_redo_rate = st[1] ? (double)st[2] / (double)st[1] : 0.0;
    // (measured: a redone head also holds its seven partner waves at the next barrier, so a redo share r costs ~ 235 k x r cycles per
    //  chunk while r is small -- 6.4 %: + 14.7 k -- and 153 k x r once most heads redo; the exact instance costs + 11.4 k whatever the
    //  weights (201.6 k against 190.2 k, profiles/r05/attention_paths.txt): they break even at r = 5 - 5.5 % in cycles; in
    //  chunks per second -- the clock follows the operands -- the two are level at 6.4 %)
    h->attn_exact = h->calib_redo_rate > S2S_ATTENTION_REDO_THRESHOLD ? 1 : 0;
    return S2S_OK;
}

double s2s_attention_redo_threshold(void) { return S2S_ATTENTION_REDO_THRESHOLD; }

int s2s_create(const s2s_config* cfg, const void* blob, size_t blob_bytes, int device, s2s_handle** out) {
    if (!out) return fail(nullptr, S2S_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (const char* m = check_cfg(cfg)) return fail(nullptr, S2S_ERR_ARG, m);
    if (!blob) return fail(nullptr, S2S_ERR_ARG, "weights_blob is NULL");
    if (blob_bytes != s2s_blob_floats(cfg) * sizeof(float)) {
        char buf[160];
        snprintf(buf, sizeof buf, "weight blob is %zu bytes, expected %zu", blob_bytes, s2s_blob_floats(cfg) * sizeof(float));
        return fail(nullptr, S2S_ERR_BLOB, buf);
    }
    int ndev = 0;
    HIP_TRY(nullptr, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(nullptr, S2S_ERR_ARG, "no such HIP device");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(nullptr, S2S_ERR_HIP, "hipSetDevice failed");
    std::string arch;
    int n_cu = 0;
    {   // hipGetDeviceProperties is a millisecond-class call: asked once per device and process
        static std::mutex mu;
        static std::map<int, std::pair<std::string, int>> seen;
        std::lock_guard<std::mutex> lock(mu);
        auto it = seen.find(device);
        if (it == seen.end()) {
            hipDeviceProp_t prop;
            HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device));
            it = seen.emplace(device, std::make_pair(std::string(prop.gcnArchName), prop.multiProcessorCount)).first;
        }
        arch = it->second.first;
        n_cu = it->second.second;
    }
    if (arch.compare(0, 6, "gfx950") != 0)
        return fail(nullptr, S2S_ERR_ARG, "device is " + arch + ", this library is gfx950 only");

    s2s_handle* h = new s2s_handle();
    h->cfg = *cfg;
    h->device = device;
    h->n_wg = n_cu > 0 ? n_cu : 256;
    const int k = cfg->seq_kmer;
    Arena A;
    ModelDev& M = h->model;
    std::memset(&M, 0, sizeof M);
    if (mode_generic(cfg->compute_mode)) {
        pack_generic(A, h->gen, cfg, static_cast<const float*>(blob));
    } else {
    M.k = k; M.enc_layers = cfg->encoder_layers; M.dec_layers = cfg->decoder_layers; M.pre_layers = cfg->pre_layers;
    M.scale = cfg->scaling_max_value;
    const float* p = static_cast<const float*>(blob);
    M.pe_enc = A.put(take(p, 16 * 64), 16 * 64);
    {   // src_emb.weight [64][5k] -> transposed [5k][64] so a one-hot column is one contiguous row
        const float* w = take(p, (size_t)64 * 5 * k);
        std::vector<float> wt((size_t)5 * k * 64);
        for (int f = 0; f < 64; ++f)
            for (int i = 0; i < 5 * k; ++i) wt[(size_t)i * 64 + f] = w[(size_t)f * 5 * k + i];
        M.emb_wt = A.put(wt.data(), wt.size());
        M.emb_b = A.put(take(p, 64), 64);
    }
    for (int i = 0; i < cfg->pre_layers; ++i) {
        const float* w = take(p, 4096);
        M.pre_w[i] = A.put_afrag(w, 64, 64, false);
        M.pre_wh[i] = pack_linear64_h(A, w);
        M.pre_b[i] = A.put(take(p, 64), 64);
    }
    for (int l = 0; l < cfg->encoder_layers; ++l) M.enc[l] = pack_layer(A, p);
    M.noise = pack_mlp(A, p);
    M.conc = pack_mlp(A, p);
    M.rate = pack_mlp(A, p);
    M.pe_dec = A.put(take(p, 250 * 64), 250 * 64);
    for (int l = 0; l < cfg->decoder_layers; ++l) M.dec[l] = pack_layer(A, p);
    M.out_w = A.put(take(p, 64), 64);
    M.out_b = A.put(take(p, 1), 1);
    }
    while (A.v.size() % 4) A.v.push_back(0.0f);
    h->arena_floats = A.v.size();

    auto bail = [&](hipError_t e, const char* what) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(e);
        s2s_destroy(h);
        return S2S_ERR_HIP;
    };
    hipError_t e;
    // chunks per launch: the kernel needs no per-chunk workspace, so a launch is as long as 32-bit chunk indices allow
    // comfortably (every launch ends in a tail of up to one chunk time per workgroup)
    h->tile = 1 << 20;
    {   // one allocation (each hipMalloc is a driver round trip): weights | hand-off slots | export scratch for the streaming
        // path's usual super-batch, so that its first s2s_export_reads does not have to drain the stream in order to grow it |
        // s2s_svb_encode scratch (rows of a super-batch; POD5: ~6 per 10 kb read)
        const int cap = 5 * 32768 + 1, rows = 16384;   // run_streaming's largest super-batches (131,072 chunks + one read) fit without a re-allocation
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t o_hand = up(h->arena_floats * sizeof(float));
        const size_t o_counts = o_hand + up((size_t)h->n_wg * S2S_MAX_GROUP * S2S_SLOT_FLOATS * sizeof(float));
        const size_t o_offs = o_counts + up((size_t)cap * sizeof(int));
        const size_t o_svb = o_offs + up((size_t)cap * sizeof(long long));
        const size_t o_stats = o_svb + up((size_t)rows * sizeof(int));
        h->slab_bytes = o_stats + 256;
        if ((e = hipMalloc(&h->slab, h->slab_bytes)) != hipSuccess) return bail(e, "hipMalloc(handle)");
        h->d_arena = reinterpret_cast<float*>(h->slab);
        h->handoff = reinterpret_cast<float*>(h->slab + o_hand);
        h->ws_counts = reinterpret_cast<int*>(h->slab + o_counts);
        h->ws_offs = reinterpret_cast<long long*>(h->slab + o_offs);
        h->ws_svb = reinterpret_cast<int*>(h->slab + o_svb);
        h->d_stats = reinterpret_cast<unsigned long long*>(h->slab + o_stats);
        h->ws_export_cap = cap;
        h->ws_svb_cap = rows;
    }
    if ((e = hipMemcpy(h->d_arena, A.v.data(), h->arena_floats * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
        return bail(e, "hipMemcpy(arena)");
    if ((e = hipMemset(h->d_stats, 0, 256)) != hipSuccess) return bail(e, "hipMemset(stats)");
    const struct { const void* fn; int bytes; } dyn_lds[] = {
        {reinterpret_cast<const void*>(s2s_fused_kernel<0, false>), Fused<0>::LDS}, {reinterpret_cast<const void*>(s2s_fused_kernel<1, false>), Fused<1>::LDS},
        {reinterpret_cast<const void*>(s2s_fused_kernel<3, false>), Fused<3>::LDS}, {reinterpret_cast<const void*>(s2s_fused_kernel<0, true>), Fused<0>::LDS},
        {reinterpret_cast<const void*>(s2s_fused_kernel<1, true>), Fused<1>::LDS},  {reinterpret_cast<const void*>(s2s_fused_kernel<3, true>), Fused<3>::LDS},
        {reinterpret_cast<const void*>(s2s_fused_kernel<1, false, true>), Fused<1>::LDS}, {reinterpret_cast<const void*>(s2s_fused_kernel<3, false, true>), Fused<3>::LDS},
        {reinterpret_cast<const void*>(s2s_fused_kernel<1, true, true>), Fused<1>::LDS},  {reinterpret_cast<const void*>(s2s_fused_kernel<3, true, true>), Fused<3>::LDS},
        {reinterpret_cast<const void*>(s2s_eval_kernel<0, false>), Fused<0>::LDS}, {reinterpret_cast<const void*>(s2s_eval_kernel<1, false>), Fused<1>::LDS},
        {reinterpret_cast<const void*>(s2s_eval_kernel<3, false>), Fused<3>::LDS}, {reinterpret_cast<const void*>(s2s_eval_kernel<1, true>), Fused<1>::LDS},
        {reinterpret_cast<const void*>(s2s_eval_kernel<3, true>), Fused<3>::LDS}};
    for (const auto& k : dyn_lds)
        if ((e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes)) != hipSuccess)
            return bail(e, "hipFuncSetAttribute(dynamic LDS)");
    if (mode_generic(cfg->compute_mode) &&
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(gen_attention_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 GEN_ATTN_STAGE_BYTES)) != hipSuccess)
        return bail(e, "hipFuncSetAttribute(generic attention LDS)");
#if defined(S2S_DIAG) || defined(S2S_TILEHIST)
    if ((e = hipMalloc(&h->d_diag, 8 * 48 * sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMalloc(diag)");
    if ((e = hipMemset(h->d_diag, 0, 8 * 48 * sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMemset(diag)");
#endif
    {   // S2S_SCHEDULE = auto | static | dynamic (any case; unset or empty: auto); anything else is refused
        std::string sch;
        if (const char* env = getenv("S2S_SCHEDULE"))
            for (const char* c = env; *c; ++c) sch += (char)std::tolower((unsigned char)*c);
        if (sch.empty() || sch == "auto") h->schedule = S2S_SCHEDULE_AUTO;
        else if (sch == "static") h->schedule = S2S_SCHEDULE_STATIC;
        else if (sch == "dynamic") h->schedule = S2S_SCHEDULE_DYNAMIC;
        else {
            g_create_error = "S2S_SCHEDULE must be auto, static or dynamic (got \"" + sch + "\")";
            s2s_destroy(h);
            return S2S_ERR_ARG;
        }
    }
    // S2S_ATTENTION_PATH = fast | exact (any case): that path, no calibration launch; unset, empty or "auto": calibrate;
    // anything else is refused (a typo must not pin the fast path silently)
    std::string want;
    if (const char* env = getenv("S2S_ATTENTION_PATH"))
        for (const char* c = env; *c; ++c) want += (char)std::tolower((unsigned char)*c);
    if (want == "fast" || want == "exact") {
        h->attn_exact = want == "exact" ? 1 : 0;
    } else if (!want.empty() && want != "auto") {
        g_create_error = "S2S_ATTENTION_PATH must be fast, exact or auto (got \"" + want + "\")";
        s2s_destroy(h);
        return S2S_ERR_ARG;
    } else if (calibrate_attention(h) != S2S_OK) {
        g_create_error = "attention-path calibration launch: " + h->err;
        s2s_destroy(h);
        return S2S_ERR_HIP;
    }
    *out = h;
    return S2S_OK;
}

int s2s_set_attention_path(s2s_handle* h, int32_t path) {
    if (!h) return S2S_ERR_ARG;
    if (path != 0 && path != 1) return fail(h, S2S_ERR_ARG, "attention path must be 0 (fast path first) or 1 (exact path)");
    h->attn_exact = path;
    return S2S_OK;
}

int s2s_get_attention_path(const s2s_handle* h, int32_t* path, double* calibration_redo_rate) {
    if (!h) return S2S_ERR_ARG;
    if (path) *path = h->attn_exact;
    if (calibration_redo_rate) *calibration_redo_rate = h->calib_redo_rate;
    return S2S_OK;
}

int s2s_set_schedule(s2s_handle* h, int32_t schedule) {
    if (!h) return S2S_ERR_ARG;
    if (schedule != S2S_SCHEDULE_AUTO && schedule != S2S_SCHEDULE_STATIC && schedule != S2S_SCHEDULE_DYNAMIC)
        return fail(h, S2S_ERR_ARG, "schedule must be 0 (auto), 1 (static) or 2 (dynamic)");
    h->schedule = schedule;
    return S2S_OK;
}

int s2s_get_schedule(const s2s_handle* h, int32_t* schedule) {
    if (!h || !schedule) return S2S_ERR_ARG;
    *schedule = h->schedule;
    return S2S_OK;
}

void s2s_schedule_claim(int64_t n, int32_t n_wg, int32_t group, int64_t c, int64_t* start, int32_t* count) {
    int s = 0, k = 0;               // (a launch is at most 2^20 chunks; out of range: an empty claim)
    if (n >= 0 && n <= (1 << 30) && n_wg > 0 && group > 0 && (int64_t)n_wg * group <= (1 << 30) && c >= 0 && c < (1ll << 31))
        s2s_claim_range((int)n, n_wg, group, (int)c, &s, &k);
    if (start) *start = s;
    if (count) *count = k;
}

int32_t s2s_schedule_is_dynamic(int64_t n, int32_t n_wg, int32_t group) { return s2s_auto_takes_claims(n, n_wg, group) ? 1 : 0; }

void s2s_destroy(s2s_handle* h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    for (auto& ev : h->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    free_scratch(h, h->ws_counts);
    free_scratch(h, h->ws_offs);
    free_scratch(h, h->ws_svb);
    if (h->gen.ws) (void)hipFree(h->gen.ws);
    if (h->ev_ws) (void)hipFree(h->ev_ws);
    if (h->slab) (void)hipFree(h->slab);
    if (h->d_diag) (void)hipFree(h->d_diag);
    delete h;
}

const char* s2s_last_error(const s2s_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static int predict_impl(s2s_handle* h, void* stream_, const uint8_t* bases, const int64_t* chunk_start, const uint8_t* n_valid, int64_t first_global_chunk,
                       int32_t B, const s2s_params* params, const float* inject_g, const float* inject_zdw,
                       const float* inject_z01, float* out_signal, int32_t* out_dur, const s2s_debug* dbg) {
    if (!h) return S2S_ERR_ARG;
    if (B < 0) return fail(h, S2S_ERR_ARG, "B < 0");
    if (B == 0) return S2S_OK;
    if (!bases || !n_valid || !params || !out_signal || !out_dur) return fail(h, S2S_ERR_ARG, "NULL argument");
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    if (!(params->min_duration >= 0.0f)) return fail(h, S2S_ERR_ARG, "min_duration must be >= 0");
    if (!params->duration_sampling && !(params->dwell_std > 0.0f) && !(params->dwell_mean >= 0.0f))
        return fail(h, S2S_ERR_ARG, "dwell_mean must be >= 0");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const ParamsDev P = to_dev(params);
    DebugDev D;
    std::memset(&D, 0, sizeof D);
    if (dbg) {
        D.emb_out = dbg->emb_out; D.enc_out = dbg->enc_out; D.sigma = dbg->sigma; D.conc = dbg->conc;
        D.rate = dbg->rate; D.g = dbg->g; D.y_scaled = dbg->y_scaled; D.z01 = dbg->z01;
        D.emb_in = dbg->emb_in; D.dec_in = dbg->dec_in;
    }
    D.diag = h->d_diag;
    D.stats = h->d_stats;
    h->stat_chunks += B;
    if (mode_generic(h->cfg.compute_mode))
        return predict_generic(h, stream, bases, chunk_start, n_valid, first_global_chunk, B, P, inject_g, inject_zdw, inject_z01,
                               out_signal, out_dur, D);
    const int nb = S2S_T_ENC + h->cfg.seq_kmer - 1;
    for (int64_t s = 0; s < B; s += h->tile) {
        const int n = (int)((B - s < h->tile) ? (B - s) : h->tile);
        const uint8_t* tb = chunk_start ? bases : bases + (size_t)s * nb;
        const long long* tcs = reinterpret_cast<const long long*>(chunk_start ? chunk_start + s : nullptr);
        const float* tg = inject_g ? inject_g + s * 16 : nullptr;
        const float* tzdw = inject_zdw ? inject_zdw + s * 16 : nullptr;
        const float* tz01 = inject_z01 ? inject_z01 + (size_t)s * S2S_T_DEC : nullptr;
        float* tsig = out_signal + (size_t)s * S2S_T_DEC;
        const long long fc = (long long)(first_global_chunk + s);
        const dim3 grid(n < h->n_wg ? n : h->n_wg), block(DEC_WAVES * 64);
        const int mode = h->cfg.compute_mode;
        EventPair ev{};
        if (h->profiling) {
            HIP_TRY(h, hipEventCreate(&ev.a));
            HIP_TRY(h, hipEventCreate(&ev.b));
            HIP_TRY(h, hipEventRecord(ev.a, stream));
        }
        const bool test = dbg || inject_g || inject_zdw || inject_z01;
        const bool exact = h->attn_exact && mode != S2S_MODE_F32;
        auto fused = exact ? (test ? (mode == S2S_MODE_F16 ? s2s_fused_kernel<3, true, true> : s2s_fused_kernel<1, true, true>)
                                   : (mode == S2S_MODE_F16 ? s2s_fused_kernel<3, false, true> : s2s_fused_kernel<1, false, true>))
                   : test  ? (mode == S2S_MODE_F16 ? s2s_fused_kernel<3, true> : mode == S2S_MODE_F16X3 ? s2s_fused_kernel<1, true> : s2s_fused_kernel<0, true>)
                           : (mode == S2S_MODE_F16 ? s2s_fused_kernel<3, false> : mode == S2S_MODE_F16X3 ? s2s_fused_kernel<1, false> : s2s_fused_kernel<0, false>);
        if (exact) h->stat_exact_chunks += n;
        // claims from the handle's counter, or the static split (s2s_schedule.h; `auto` decides per launch, on the full grid)
        const bool dynamic = h->schedule == S2S_SCHEDULE_DYNAMIC ||
                             (h->schedule == S2S_SCHEDULE_AUTO && s2s_auto_takes_claims(n, h->n_wg, mode == S2S_MODE_F32 ? Fused<0>::GROUP : Fused<1>::GROUP));
        if (dynamic) h->stat_dynamic_chunks += n;
        unsigned* const sched = dynamic ? reinterpret_cast<unsigned*>(h->d_stats + S2S_STAT_SCHED) : nullptr;
        hipLaunchKernelGGL(fused, grid, block, mode == S2S_MODE_F16 ? Fused<3>::LDS : mode == S2S_MODE_F16X3 ? Fused<1>::LDS : Fused<0>::LDS, stream, h->model, h->d_arena, tb, tcs,
                           n_valid + s, n, fc, P, tg, tzdw, tz01, h->handoff, out_dur + s * 16, tsig, D, (long long)s, sched);
        if (h->profiling) {
            HIP_TRY(h, hipEventRecord(ev.b, stream));
            ev.chunks = n;
            h->events.push_back(ev);
        }
    }
    HIP_TRY(h, hipGetLastError());
    return S2S_OK;
}

#define S2S_EVAL_SLICE 32768                  // chunks per slice of s2s_evaluate_chunks (its y / sigma / conc / rate scratch)

int s2s_evaluate_chunks(s2s_handle* h, void* stream_, const uint8_t* kmers, const int32_t* dwell, const float* target, const float* stdev,
                        int32_t B, float* out_loss, float* out_y, const s2s_debug* dbg) {
    if (!h) return S2S_ERR_ARG;
    if (B < 0) return fail(h, S2S_ERR_ARG, "B < 0");
    if (B == 0) return S2S_OK;
    if (!kmers || !dwell || !target || !stdev || !out_loss) return fail(h, S2S_ERR_ARG, "NULL argument");
    if (dbg && (dbg->emb_in || dbg->dec_in || dbg->emb_out || dbg->enc_out || dbg->g || dbg->y_scaled || dbg->z01))
        return fail(h, S2S_ERR_ARG, "s2s_evaluate_chunks writes only dbg->sigma / conc / rate (and y through out_y)");
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const int mode = h->cfg.compute_mode, k = h->cfg.seq_kmer;
    const bool gen = mode_generic(mode);
    const int te = gen ? h->gen.te : S2S_T_ENC, ts = gen ? h->gen.ts : S2S_T_DEC;
    const int want = B < S2S_EVAL_SLICE ? B : S2S_EVAL_SLICE;
    const size_t per = (size_t)ts + 3 * (size_t)te;
    HIP_TRY(h, grow_device(h->ev_ws, h->ev_chunks, want, (size_t)want * per * sizeof(float), st));
    const size_t S = h->ev_chunks;
    ParamsDev P;
    std::memset(&P, 0, sizeof P);
    P.duration_sampling = 1;                  // the heads run; the sampler does not (teacher forcing)
    EventPair ev{};
    if (h->profiling) {
        HIP_TRY(h, hipEventCreate(&ev.a));
        HIP_TRY(h, hipEventCreate(&ev.b));
        HIP_TRY(h, hipEventRecord(ev.a, st));
    }
    for (int64_t s = 0; s < B; s += S) {
        const int n = (int)((B - s < (int64_t)S) ? (B - s) : (int64_t)S);
        auto pick = [&](float* user, size_t row, float* scratch) { return user ? user + (size_t)s * row : scratch; };
        float* y = pick(out_y, ts, h->ev_ws);
        float* sg = pick(dbg ? dbg->sigma : nullptr, te, h->ev_ws + S * ts);
        float* cq = pick(dbg ? dbg->conc : nullptr, te, h->ev_ws + S * ts + S * te);
        float* rq = pick(dbg ? dbg->rate : nullptr, te, h->ev_ws + S * ts + 2 * S * te);
        const uint8_t* km = kmers + (size_t)s * te * k;
        const int32_t* dw = dwell + (size_t)s * te;
        if (gen) {
            const int rc = evaluate_generic(h, st, km, dw, n, y, sg, cq, rq);
            if (rc != S2S_OK) return rc;
        } else {
            DebugDev D;
            std::memset(&D, 0, sizeof D);
            D.sigma = sg; D.conc = cq; D.rate = rq;
            const dim3 grid(n < h->n_wg ? n : h->n_wg), block(DEC_WAVES * 64);
            const bool exact = h->attn_exact && mode != S2S_MODE_F32;
            auto kern = mode == S2S_MODE_F32 ? s2s_eval_kernel<0, false>
                        : mode == S2S_MODE_F16 ? (exact ? s2s_eval_kernel<3, true> : s2s_eval_kernel<3, false>)
                                               : (exact ? s2s_eval_kernel<1, true> : s2s_eval_kernel<1, false>);
            hipLaunchKernelGGL(kern, grid, block, mode == S2S_MODE_F16 ? Fused<3>::LDS : mode == S2S_MODE_F16X3 ? Fused<1>::LDS : Fused<0>::LDS,
                               st, h->model, h->d_arena, km, dw, n, P, h->handoff, y, D);
        }
        hipLaunchKernelGGL(s2s_eval_loss_kernel, dim3((n + 3) / 4), dim3(256), 0, st, y, target + (size_t)s * ts, sg, stdev + (size_t)s * te,
                           cq, rq, dw, n, te, ts, out_loss + (size_t)s * 3);
    }
    if (h->profiling) {
        HIP_TRY(h, hipEventRecord(ev.b, st));
        ev.chunks = B;
        h->events.push_back(ev);
    }
    HIP_TRY(h, hipGetLastError());
    return S2S_OK;
}

int s2s_predict_chunks(s2s_handle* h, void* stream, const uint8_t* bases, const uint8_t* n_valid, int64_t first_global_chunk,
                       int32_t B, const s2s_params* params, const float* inject_g, const float* inject_zdw,
                       const float* inject_z01, float* out_signal, int32_t* out_dur, const s2s_debug* dbg) {
    return predict_impl(h, stream, bases, nullptr, n_valid, first_global_chunk, B, params, inject_g, inject_zdw, inject_z01,
                        out_signal, out_dur, dbg);
}

int s2s_predict_packed(s2s_handle* h, void* stream, const uint8_t* read_bytes, const int64_t* chunk_start,
                       const uint8_t* n_valid, int64_t first_global_chunk, int32_t B, const s2s_params* params,
                       float* out_signal, int32_t* out_dur) {
    if (h && !chunk_start) return fail(h, S2S_ERR_ARG, "chunk_start is NULL");
    return predict_impl(h, stream, read_bytes, chunk_start, n_valid, first_global_chunk, B, params, nullptr, nullptr, nullptr,
                        out_signal, out_dur, nullptr);
}

int s2s_export_reads(s2s_handle* h, void* stream_, const float* signal, int32_t B, const int32_t* read_first, int32_t R,
                     int64_t* out_offsets, float* out_pa, int16_t* out_dac, int64_t capacity, float digitisation,
                     float range, float offset_mean, int32_t rna) {
    if (!h) return S2S_ERR_ARG;
    if (B < 0 || R < 0) return fail(h, S2S_ERR_ARG, "negative size");
    if (!signal || !read_first || !out_offsets) return fail(h, S2S_ERR_ARG, "NULL argument");
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (B + 1 > h->ws_export_cap) {          // grows outside of the steady state only
        HIP_TRY(h, hipStreamSynchronize(stream));
        free_scratch(h, h->ws_counts);
        free_scratch(h, h->ws_offs);
        h->ws_counts = nullptr; h->ws_offs = nullptr; h->ws_export_cap = 0;
        const int cap = B + 1 + B / 4;
        HIP_TRY(h, hipMalloc(&h->ws_counts, (size_t)cap * sizeof(int)));
        HIP_TRY(h, hipMalloc(&h->ws_offs, (size_t)cap * sizeof(long long)));
        h->ws_export_cap = cap;
    }
    const int ts = h->cfg.max_signal_len;    // S2S_T_DEC except for a S2S_MODE_GENERIC_GEOMETRY(_F16) handle
    const bool tuned_rows = ts == S2S_T_DEC;
    if (B > 0)
        hipLaunchKernelGGL(tuned_rows ? s2s_count_kernel<S2S_T_DEC> : s2s_count_kernel<0>, dim3((B + 3) / 4), dim3(256), 0, stream, signal, B,
                           h->ws_counts, ts);
    hipLaunchKernelGGL((s2s_scan_kernel<8, S2SScanInts>), dim3(1), dim3(1024), 0, stream, S2SScanInts{h->ws_counts}, (long long)B,
                       h->ws_offs);
    hipLaunchKernelGGL(s2s_read_offsets_kernel, dim3((R + 256) / 256), dim3(256), 0, stream, h->ws_offs, read_first, R,
                       reinterpret_cast<long long*>(out_offsets));
    if (B > 0 && (out_pa || out_dac))
        hipLaunchKernelGGL(tuned_rows ? s2s_compact_kernel<S2S_T_DEC> : s2s_compact_kernel<0>, dim3((B + 3) / 4), dim3(256), 0, stream,
                           signal, B, h->ws_offs, read_first, R, out_pa, reinterpret_cast<short*>(out_dac), (long long)capacity,
                           digitisation, range, offset_mean, rna, ts);
    HIP_TRY(h, hipGetLastError());
    return S2S_OK;
}

int s2s_align_chunks(s2s_handle* h, void* stream_, const float* signal, const int32_t* dur, int32_t B, uint16_t* out_seg) {
    if (!h) return S2S_ERR_ARG;
    if (B < 0) return fail(h, S2S_ERR_ARG, "negative size");
    if (!signal || !dur || !out_seg) return fail(h, S2S_ERR_ARG, "NULL argument");
    if (B == 0) return S2S_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    const int te = h->cfg.max_dna_len, ts = h->cfg.max_signal_len;    // S2S_T_ENC / S2S_T_DEC except for a geometry-mode handle
    S2S_LAUNCH(h, ts == S2S_T_DEC ? s2s_align_kernel<S2S_T_DEC> : s2s_align_kernel<0>, dim3((B + 3) / 4), dim3(256), 0,
               static_cast<hipStream_t>(stream_), signal, dur, B, reinterpret_cast<unsigned short*>(out_seg), te, ts);
    return S2S_OK;
}

int s2s_event_stats(s2s_handle* h, void* stream_, const float* signal, const int32_t* dur, int32_t B, float digitisation, float range,
                    float offset, uint16_t* out_seg, int32_t* out_sum, int64_t* out_sumsq) {
    if (!h) return S2S_ERR_ARG;
    if (B < 0) return fail(h, S2S_ERR_ARG, "negative size");
    if (!signal || !dur || !out_seg || !out_sum || !out_sumsq) return fail(h, S2S_ERR_ARG, "NULL argument");
    if (range == 0.0f || digitisation == 0.0f) return fail(h, S2S_ERR_ARG, "range and digitisation must not be 0");
    if (B == 0) return S2S_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    const int te = h->cfg.max_dna_len, ts = h->cfg.max_signal_len;    // S2S_T_ENC / S2S_T_DEC except for a geometry-mode handle
    S2S_LAUNCH(h, ts == S2S_T_DEC ? s2s_event_stats_kernel<S2S_T_DEC> : s2s_event_stats_kernel<0>, dim3((B + 3) / 4), dim3(256), 0,
               static_cast<hipStream_t>(stream_), signal, dur, B, digitisation, range, offset, reinterpret_cast<unsigned short*>(out_seg),
               out_sum, reinterpret_cast<long long*>(out_sumsq), te, ts);
    return S2S_OK;
}

int64_t s2s_kmer_table_rows(int32_t k) {
    return (k < 1 || k > S2S_KMER_TABLE_MAX_K) ? -1 : ((int64_t)1 << (2 * k)) + 1;
}

int s2s_kmer_table_accumulate(s2s_handle* h, void* stream_, const float* signal, const int32_t* dur, const uint8_t* read_bytes,
                              const int64_t* chunk_start, const uint8_t* n_valid, int32_t B, float digitisation, float range,
                              float offset, int64_t* table) {
    if (!h) return S2S_ERR_ARG;
    const int k = h->cfg.seq_kmer;
    if (k > S2S_KMER_TABLE_MAX_K)
        return fail(h, S2S_ERR_ARG, "the k-mer table takes seq_kmer 1.." + std::to_string(S2S_KMER_TABLE_MAX_K) + " (4^k + 1 rows), this model has " +
                                        std::to_string(k));
    if (B < 0) return fail(h, S2S_ERR_ARG, "negative size");
    if (!signal || !dur || !read_bytes || !chunk_start || !n_valid || !table) return fail(h, S2S_ERR_ARG, "NULL argument");
    if (range == 0.0f || digitisation == 0.0f) return fail(h, S2S_ERR_ARG, "range and digitisation must not be 0");
    if (B == 0) return S2S_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    const int te = h->cfg.max_dna_len, ts = h->cfg.max_signal_len;    // S2S_T_ENC / S2S_T_DEC except for a geometry-mode handle
    const bool lds = k <= S2S_KMER_TABLE_LDS_MAX_K, tuned_rows = ts == S2S_T_DEC;
    const int groups = (B + 3) / 4;
    const size_t lds_bytes = lds ? (size_t)s2s_kmer_table_rows(k) * S2S_KMER_TABLE_FIELDS * sizeof(unsigned long long) : 0;
    auto kernel = lds ? (tuned_rows ? s2s_kmer_table_kernel<S2S_T_DEC, true> : s2s_kmer_table_kernel<0, true>)
                      : (tuned_rows ? s2s_kmer_table_kernel<S2S_T_DEC, false> : s2s_kmer_table_kernel<0, false>);
    S2S_LAUNCH(h, kernel, dim3(lds && groups > 512 ? 512 : groups), dim3(256), lds_bytes, static_cast<hipStream_t>(stream_), signal, dur,
               read_bytes, reinterpret_cast<const long long*>(chunk_start), n_valid, B, digitisation, range, offset,
               reinterpret_cast<unsigned long long*>(table), te, ts, k);
    return S2S_OK;
}

int s2s_kmer_model_accumulate(s2s_handle* h, void* stream_, const float* signal, const int32_t* dur, const uint8_t* read_bytes,
                              const int64_t* chunk_start, const uint8_t* n_valid, int32_t B, float digitisation, float range,
                              float offset, int64_t* table) {
    if (!h) return S2S_ERR_ARG;
    const int k = h->cfg.seq_kmer;
    if (k > S2S_KMER_TABLE_MAX_K)
        return fail(h, S2S_ERR_ARG, "the k-mer model takes seq_kmer 1.." + std::to_string(S2S_KMER_TABLE_MAX_K) + " (4^k + 1 rows), this model has " +
                                        std::to_string(k));
    if (B < 0) return fail(h, S2S_ERR_ARG, "negative size");
    if (!signal || !dur || !read_bytes || !chunk_start || !n_valid || !table) return fail(h, S2S_ERR_ARG, "NULL argument");
    if (range == 0.0f || digitisation == 0.0f) return fail(h, S2S_ERR_ARG, "range and digitisation must not be 0");
    if (B == 0) return S2S_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    const int te = h->cfg.max_dna_len, ts = h->cfg.max_signal_len;    // S2S_T_ENC / S2S_T_DEC except for a geometry-mode handle
    const int groups = (B + 3) / 4;
    auto kernel = ts == S2S_T_DEC ? s2s_kmer_model_kernel<S2S_T_DEC> : s2s_kmer_model_kernel<0>;
    S2S_LAUNCH(h, kernel, dim3(groups > S2S_KMER_MODEL_MAX_WORKGROUPS ? S2S_KMER_MODEL_MAX_WORKGROUPS : groups), dim3(256), 0,
               static_cast<hipStream_t>(stream_), signal, dur, read_bytes, reinterpret_cast<const long long*>(chunk_start), n_valid, B,
               digitisation, range, offset, reinterpret_cast<unsigned long long*>(table), te, ts, k);
    return S2S_OK;
}

int s2s_svb_encode(s2s_handle* h, void* stream_, const int16_t* samples, const int64_t* read_offsets, const int32_t* row_read,
                   const int32_t* row_index, int32_t N, int64_t row_samples, int32_t variant, uint8_t* out, int64_t capacity,
                   int64_t* out_offsets) {
    if (!h) return S2S_ERR_ARG;
    if (N < 0 || row_samples <= 0 || (variant != 16 && variant != 32)) return fail(h, S2S_ERR_ARG, "bad argument");
    if (!out_offsets || (N > 0 && (!samples || !read_offsets || !row_read || !row_index || !out)))
        return fail(h, S2S_ERR_ARG, "NULL argument");
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (N + 1 > h->ws_svb_cap) {             // grows outside of the steady state only
        HIP_TRY(h, hipStreamSynchronize(stream));
        free_scratch(h, h->ws_svb);
        h->ws_svb = nullptr; h->ws_svb_cap = 0;
        const int cap = N + 1 + N / 4;
        HIP_TRY(h, hipMalloc(&h->ws_svb, (size_t)cap * sizeof(int)));
        h->ws_svb_cap = cap;
    }
    const short* sp = reinterpret_cast<const short*>(samples);
    const long long* ro = reinterpret_cast<const long long*>(read_offsets);
    long long* oo = reinterpret_cast<long long*>(out_offsets);
    if (N > 0) {
        if (variant == 32)
            hipLaunchKernelGGL((s2s_svb_kernel<32, false>), dim3(N), dim3(256), 0, stream, sp, ro, row_read, row_index,
                               (long long)row_samples, h->ws_svb, nullptr, nullptr, 0LL);
        else
            hipLaunchKernelGGL((s2s_svb_kernel<16, false>), dim3(N), dim3(256), 0, stream, sp, ro, row_read, row_index,
                               (long long)row_samples, h->ws_svb, nullptr, nullptr, 0LL);
    }
    hipLaunchKernelGGL((s2s_scan_kernel<8, S2SScanInts>), dim3(1), dim3(1024), 0, stream, S2SScanInts{h->ws_svb}, (long long)N, oo);
    if (N > 0) {
        if (variant == 32)
            hipLaunchKernelGGL((s2s_svb_kernel<32, true>), dim3(N), dim3(256), 0, stream, sp, ro, row_read, row_index,
                               (long long)row_samples, nullptr, oo, out, (long long)capacity);
        else
            hipLaunchKernelGGL((s2s_svb_kernel<16, true>), dim3(N), dim3(256), 0, stream, sp, ro, row_read, row_index,
                               (long long)row_samples, nullptr, oo, out, (long long)capacity);
    }
    S2S_LAUNCH(h, s2s_svb_check_kernel, dim3(1), dim3(64), 0, stream, oo, N, (long long)capacity);
    return S2S_OK;
}

int s2s_philox_u32(s2s_handle* h, void* stream_, uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                   int32_t n, uint32_t* out) {
    if (!h) return S2S_ERR_ARG;
    if (n < 0 || !out) return fail(h, S2S_ERR_ARG, "bad argument");
    if (n == 0) return S2S_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    S2S_LAUNCH(h, s2s_philox_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream_), (unsigned)seed,
               (unsigned)(seed >> 32), c0, c1, c2, c3, n, out);
    return S2S_OK;
}

int s2s_set_profiling(s2s_handle* h, int32_t enabled) {
    if (!h) return S2S_ERR_ARG;
    h->profiling = enabled != 0;
    return S2S_OK;
}

int s2s_get_kernel_ms(s2s_handle* h, double* ms_total, int64_t* launches, int64_t* chunks) {
    if (!h) return S2S_ERR_ARG;
    double tot = 0.0;
    int64_t nl = 0, nc = 0;
    for (auto& ev : h->events) {
        HIP_TRY(h, hipEventSynchronize(ev.b));
        float ms = 0.0f;
        HIP_TRY(h, hipEventElapsedTime(&ms, ev.a, ev.b));
        tot += ms; nl += 1; nc += ev.chunks;
        (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b);
    }
    h->events.clear();
    if (ms_total) *ms_total = tot;
    if (launches) *launches = nl;
    if (chunks) *chunks = nc;
    return S2S_OK;
}

int s2s_stats_read(s2s_handle* h, uint64_t* out10) {
    if (!h || !out10) return S2S_ERR_ARG;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(h, S2S_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(h, hipDeviceSynchronize());
    unsigned long long raw[8];
    HIP_TRY(h, hipMemcpy(raw, h->d_stats, sizeof raw, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemset(h->d_stats, 0, sizeof raw));
    out10[0] = (uint64_t)h->stat_chunks;
    out10[1] = mode_generic(h->cfg.compute_mode)
                   ? (uint64_t)h->stat_chunks * (uint64_t)cfg_dec_heads(&h->cfg) * (uint64_t)h->cfg.decoder_layers
                   : (uint64_t)h->stat_chunks * DEC_WAVES * S2S_HEADS * (uint64_t)h->cfg.decoder_layers;
    out10[2] = raw[S2S_STAT_REDO];
    out10[3] = raw[S2S_STAT_CYCLES]; out10[4] = raw[S2S_STAT_TICKS]; out10[5] = raw[S2S_STAT_WGS];
    out10[6] = (uint64_t)h->stat_exact_chunks;
    out10[7] = raw[S2S_STAT_SPAN_MAX];
    out10[8] = raw[S2S_STAT_SPAN_MIN_INV] ? ~raw[S2S_STAT_SPAN_MIN_INV] : 0;
    out10[9] = (uint64_t)h->stat_dynamic_chunks;
    h->stat_chunks = 0; h->stat_exact_chunks = 0; h->stat_dynamic_chunks = 0;
    return S2S_OK;
}

int s2s_diag_read(s2s_handle* h, uint64_t* out48) {
    if (!h || !out48) return S2S_ERR_ARG;
    if (!h->d_diag) return fail(h, S2S_ERR_ARG, "not a diagnostic (-DS2S_DIAG) build");
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(out48, h->d_diag, 8 * 48 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemset(h->d_diag, 0, 8 * 48 * sizeof(uint64_t)));
    return S2S_OK;
}

// ---- compare (s2s_dtw.h): handle-free, stream-ordered
int32_t s2s_dtw_max_band(void) { return S2S_DTW_MAX_BAND; }

int s2s_signal_median_mad(int device, void* stream_, const int16_t* samples, const int64_t* offs, int32_t R, int32_t* med, int32_t* mad) {
    if (R < 0 || !offs || (R > 0 && (!samples || !med || !mad))) return fail(nullptr, S2S_ERR_ARG, "s2s_signal_median_mad: bad argument");
    if (R == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    S2S_LAUNCH(nullptr, s2s_median_mad_kernel, dim3(R), dim3(S2S_DTW_SELECT_THREADS), 0, static_cast<hipStream_t>(stream_), samples,
               as_ll(offs), med, mad);
    return S2S_OK;
}

int s2s_signal_normalise(int device, void* stream_, const int16_t* samples, const int64_t* offs, int32_t R, const int32_t* med,
                         const int32_t* mad, int32_t scale, int16_t* out) {
    if (R < 0 || !offs || scale < 1 || scale > S2S_DTW_MAX_SCALE || (R > 0 && (!samples || !med || !mad || !out)))
        return fail(nullptr, S2S_ERR_ARG, "s2s_signal_normalise: bad argument (scale must be 1..8192)");
    if (R == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    S2S_LAUNCH(nullptr, s2s_normalise_kernel, dim3(R, S2S_DTW_NORM_SLICES), dim3(256), 0, static_cast<hipStream_t>(stream_), samples,
               as_ll(offs), med, mad, scale, out);
    return S2S_OK;
}

int s2s_dtw_banded(int device, void* stream_, const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs,
                   int32_t P, int32_t band, int64_t* cost) {
    if (P < 0 || band < 1 || band > S2S_DTW_MAX_BAND || !a_offs || !b_offs || (P > 0 && (!a || !b || !cost)))
        return fail(nullptr, S2S_ERR_ARG, "s2s_dtw_banded: bad argument (band must be 1..S2S_DTW_MAX_BAND)");
    if (P == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    // a diagonal holds at most 2 band + 1 cells: one wave while two strides cover it, else four
    const int threads = 2 * band + 1 <= 128 ? 64 : 256;
    const size_t lds = S2S_DTW_LDS_BYTES(band);      // 58,416 B at S2S_DTW_MAX_BAND
    S2S_LAUNCH(nullptr, s2s_dtw_kernel<false>, dim3(P), dim3(threads), lds, static_cast<hipStream_t>(stream_), a, as_ll(a_offs), b, as_ll(b_offs),
               band, as_ll(cost), static_cast<unsigned char*>(nullptr), static_cast<const long long*>(nullptr));
    return S2S_OK;
}

int64_t s2s_dtw_path_scratch_bytes(int64_t n, int64_t m, int32_t band) {
    if (band < 1 || band > S2S_DTW_MAX_BAND) return S2S_ERR_ARG;
    return s2s_dtw_path_bytes(n, m, band);
}

int s2s_dtw_path(int device, void* stream_, const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs, int32_t P,
                 int32_t band, int64_t* cost, uint8_t* scratch, const int64_t* scratch_offs, uint8_t* ops, const int64_t* path_offs,
                 int64_t* steps) {
    if (P < 0 || band < 1 || band > S2S_DTW_MAX_BAND || !a_offs || !b_offs || !scratch_offs || !path_offs ||
        (P > 0 && (!a || !b || !cost || !scratch || !ops || !steps)) || (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(nullptr, S2S_ERR_ARG, "s2s_dtw_path: bad argument (band must be 1..S2S_DTW_MAX_BAND, scratch 16-byte aligned)");
    if (P == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    const int threads = 2 * band + 1 <= 128 ? 64 : 256;          // as s2s_dtw_banded
    const size_t lds = S2S_DTW_LDS_BYTES(band);
    S2S_LAUNCH(nullptr, s2s_dtw_kernel<true>, dim3(P), dim3(threads), lds, static_cast<hipStream_t>(stream_), a, as_ll(a_offs), b, as_ll(b_offs),
               band, as_ll(cost), scratch, as_ll(scratch_offs));
    S2S_LAUNCH(nullptr, s2s_dtw_trace_kernel, dim3(P), dim3(64), 0, static_cast<hipStream_t>(stream_), as_ll(a_offs), as_ll(b_offs), band,
               as_ll(cost), scratch, as_ll(scratch_offs), ops, as_ll(path_offs), as_ll(steps));
    return S2S_OK;
}

// ---- compare --open-ends (s2s_sdtw.h)
int32_t s2s_sdtw_max_query(void) { return S2S_SDTW_MAX_QUERY; }

int s2s_sdtw(int device, void* stream_, const int16_t* q, const int64_t* q_begin, const int64_t* q_len, const int16_t* t,
             const int64_t* t_begin, const int64_t* t_len, const uint8_t* reverse, int32_t P, int64_t* cost, int64_t* start,
             int64_t* end) {
    if (P < 0 || (P > 0 && (!q || !q_begin || !q_len || !t || !t_begin || !t_len || !reverse || !cost || !start || !end)))
        return fail(nullptr, S2S_ERR_ARG, "s2s_sdtw: bad argument");
    if (P == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    static_assert(S2S_SDTW_LDS_BYTES == 57904, "include/s2s_hip.h states the LDS bytes of s2s_sdtw");
    S2S_LAUNCH(nullptr, s2s_sdtw_kernel, dim3(P), dim3(S2S_SDTW_THREADS), 0, static_cast<hipStream_t>(stream_), q, as_ll(q_begin), as_ll(q_len),
               t, as_ll(t_begin), as_ll(t_len), reverse, as_ll(cost), as_ll(start), as_ll(end));
    return S2S_OK;
}

// ---- resquiggle (s2s_resquiggle.h)
int64_t s2s_resquiggle_scratch_bytes(int64_t n, int64_t K, int32_t band) {
    if (band < 1 || band > S2S_DTW_MAX_BAND) return S2S_ERR_ARG;
    return s2s_rsq_bytes(n, K, band);
}

int s2s_resquiggle(int device, void* stream_, const int16_t* q, const int64_t* q_offs, const int16_t* l, const int64_t* l_offs, int32_t P,
                   int32_t band, int32_t skip_penalty, int32_t unknown_cost, int64_t* cost, uint8_t* scratch, const int64_t* scratch_offs,
                   int32_t* ev_start, int32_t* ev_len) {
    if (P < 0 || band < 1 || band > S2S_DTW_MAX_BAND || skip_penalty < 0 || skip_penalty > S2S_RSQ_MAX_SKIP_PENALTY || unknown_cost < 0 ||
        unknown_cost > S2S_RSQ_MAX_UNKNOWN_COST || !q_offs || !l_offs || !scratch_offs ||
        (P > 0 && (!q || !l || !cost || !scratch || !ev_start || !ev_len)) || (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(nullptr, S2S_ERR_ARG, "s2s_resquiggle: bad argument (band must be 1..S2S_DTW_MAX_BAND, skip_penalty 0..2^20, "
                                          "unknown_cost 0..65535, scratch 16-byte aligned)");
    if (P == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    static_assert(S2S_RSQ_LDS_BYTES(S2S_DTW_MAX_BAND) == 38272 && S2S_RSQ_LDS_BYTES(512) == 19840,
                  "include/s2s_hip.h states the LDS bytes of s2s_resquiggle");
    S2S_LAUNCH(nullptr, s2s_resquiggle_kernel, dim3(P), dim3(64 * s2s_rsq_waves(band)), S2S_RSQ_LDS_BYTES(band),
               static_cast<hipStream_t>(stream_), q, as_ll(q_offs), l, as_ll(l_offs), band, skip_penalty, unknown_cost, as_ll(cost), scratch,
               as_ll(scratch_offs));
    S2S_LAUNCH(nullptr, s2s_resquiggle_trace_kernel, dim3(P), dim3(64), 0, static_cast<hipStream_t>(stream_), as_ll(q_offs), as_ll(l_offs), band,
               as_ll(cost), scratch, as_ll(scratch_offs), ev_start, ev_len);
    return S2S_OK;
}

int s2s_event_sums(int device, void* stream_, const int16_t* samples, const int64_t* s_offs, const int32_t* ev_start, const int32_t* ev_len,
                   const int64_t* l_offs, int32_t P, int64_t* S, int64_t* Q) {
    if (P < 0 || !s_offs || !l_offs || (P > 0 && (!samples || !ev_start || !ev_len || !S || !Q)))
        return fail(nullptr, S2S_ERR_ARG, "s2s_event_sums: bad argument");
    if (P == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    S2S_LAUNCH(nullptr, s2s_event_sums_kernel, dim3(P, S2S_RSQ_SUM_SLICES), dim3(256), 0, static_cast<hipStream_t>(stream_), samples,
               as_ll(s_offs), ev_start, ev_len, as_ll(l_offs), as_ll(S), as_ll(Q));
    return S2S_OK;
}

// ---- the pore model from alignments (s2s_kmer_model_events.h); the host twin is in s2s_host.cpp
int s2s_kmer_model_events(int device, void* stream_, const int32_t* codes, const int32_t* ev_len, const int64_t* S, const int64_t* Q,
                          const int64_t* l_offs, int32_t P, const int64_t* gain, const int64_t* shift, int32_t k, int32_t workgroups,
                          int64_t* table, int64_t* dropped) {
    if (k < 1 || k > S2S_KMER_TABLE_MAX_K || P < 0 || workgroups < 0 || workgroups > S2S_KMER_MODEL_MAX_WORKGROUPS ||
        (P > 0 && (!codes || !ev_len || !S || !Q || !l_offs || !gain || !shift || !table || !dropped)))
        return fail(nullptr, S2S_ERR_ARG, "s2s_kmer_model_events: bad argument (k 1..10, P >= 0, workgroups 0..S2S_KMER_MODEL_MAX_WORKGROUPS)");
    if (P == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    S2SKmeIn in;
    in.codes = codes; in.ev_len = ev_len;
    in.S = as_ll(S); in.Q = as_ll(Q); in.l_offs = as_ll(l_offs);
    in.gain = as_ll(gain); in.shift = as_ll(shift);
    in.P = P; in.k = k;
    // (the slot count l_offs[P] is on the device: the kernel reads it, and a workgroup without a round leaves at once)
    S2S_LAUNCH(nullptr, s2s_kmer_model_events_kernel, dim3(workgroups ? workgroups : S2S_KMER_MODEL_MAX_WORKGROUPS), dim3(256), 0,
               static_cast<hipStream_t>(stream_), in, reinterpret_cast<unsigned long long*>(table), reinterpret_cast<unsigned long long*>(dropped));
    return S2S_OK;
}

// ---- segment (s2s_segment.h)
int64_t s2s_segment_scratch_bytes(int64_t total, int32_t R) {
    if (total < 0 || total > S2S_SEG_MAX_TOTAL || R < 0) return S2S_ERR_ARG;
    return s2s_seg_scratch(total);
}

int s2s_segment(int device, void* stream_, const int16_t* samples, const int64_t* offs, int32_t R, int64_t total, int32_t w_short,
                int32_t w_long, int64_t thr_short, int64_t thr_long, uint8_t* scratch, const int64_t* ev_offs, int32_t* ev_start,
                int32_t* ev_len, int32_t* n_events) {
    if (R < 0 || total < 0 || total > S2S_SEG_MAX_TOTAL || !s2s_seg_params_ok(w_short, w_long, thr_short, thr_long) || !offs || !ev_offs ||
        (R > 0 && total > 0 && (!samples || !scratch || !ev_start || !ev_len || !n_events)) || (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(nullptr, S2S_ERR_ARG, "s2s_segment: bad argument (windows 1 <= short <= long <= 32, thresholds 1..2^40, total 0..2^40, "
                                          "scratch 16-byte aligned)");
    if (R == 0 || total == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    const int64_t tiles = s2s_seg_tiles(total);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(scratch);
    int* wrank = reinterpret_cast<int*>(scratch + tiles * S2S_SEG_WORDS * 8);
    long long* trank = reinterpret_cast<long long*>(scratch + tiles * S2S_SEG_WORDS * 12);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    S2S_LAUNCH(nullptr, s2s_segment_flags_kernel, dim3((unsigned)tiles), dim3(S2S_SEG_THREADS), 0, stream, samples, as_ll(offs), R,
               (long long)total, w_short, w_long, (long long)thr_short, (long long)thr_long, words, wrank, trank);
    S2S_LAUNCH(nullptr, (s2s_scan_kernel<1, S2SScanNext>), dim3(1), dim3(1024), 0, stream, S2SScanNext{trank}, (long long)tiles, trank);
    S2S_LAUNCH(nullptr, s2s_segment_compact_kernel, dim3((unsigned)tiles), dim3(S2S_SEG_THREADS), 0, stream, as_ll(offs), R, (long long)total,
               (long long)tiles, words, wrank, trank, as_ll(ev_offs), ev_start, ev_len, n_events);
    return S2S_OK;
}

// ---- eventalign (s2s_eventalign.h); s2s_eventalign_scratch_bytes is in s2s_host.cpp
int s2s_event_means(int device, void* stream_, const int64_t* S, const int32_t* ev_len, const int64_t* ev_offs, const int32_t* n_events,
                    int32_t R, int64_t capacity, int64_t* m_offs, int16_t* means) {
    if (R < 0 || capacity < 0 || !ev_offs || !m_offs || (R > 0 && (!n_events || (capacity > 0 && (!S || !ev_len || !means)))))
        return fail(nullptr, S2S_ERR_ARG, "s2s_event_means: bad argument");
    GUARD_OR_RETURN(nullptr, device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    S2S_LAUNCH(nullptr, (s2s_scan_kernel<1, S2SEvaCounts>), dim3(1), dim3(1024), 0, stream, S2SEvaCounts{n_events, as_ll(ev_offs)},
               (long long)R, as_ll(m_offs));
    if (R == 0 || capacity == 0) return S2S_OK;
    S2S_LAUNCH(nullptr, s2s_event_means_fill_kernel, dim3(R, S2S_EVA_MEAN_SLICES), dim3(256), 0, stream, as_ll(S), ev_len, as_ll(ev_offs),
               n_events, (long long)capacity, as_ll(m_offs), means);
    return S2S_OK;
}

int s2s_eventalign(int device, void* stream_, const int16_t* m, const int64_t* m_offs, const int16_t* l, const int64_t* l_offs,
                   const int32_t* ev_start, const int32_t* ev_len, const int64_t* ev_offs, int32_t P, int32_t width, int32_t skip_penalty,
                   int32_t trim_penalty, int32_t unknown_cost, int64_t* cost, uint8_t* scratch, const int64_t* scratch_offs,
                   int32_t* first_event, int32_t* end_event, int32_t* ev_kmer, int32_t* k_start, int32_t* k_len, int32_t* k_events) {
    if (P < 0 || !s2s_eva_params_ok(width, skip_penalty, trim_penalty, unknown_cost) || !m_offs || !l_offs || !ev_offs || !scratch_offs ||
        (P > 0 && (!m || !l || !ev_start || !ev_len || !cost || !scratch || !first_event || !end_event || !ev_kmer || !k_start || !k_len ||
                   !k_events)) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(nullptr, S2S_ERR_ARG, "s2s_eventalign: bad argument (width a multiple of 64 in 64..S2S_EVA_MAX_WIDTH, skip_penalty and "
                                          "trim_penalty 0..2^20, unknown_cost 0..65535, scratch 16-byte aligned)");
    if (P == 0) return S2S_OK;
    GUARD_OR_RETURN(nullptr, device);
    static_assert(S2S_EVA_LDS_BYTES(S2S_EVA_MAX_WIDTH) == 29744 && S2S_EVA_LDS_BYTES(128) == 4656,
                  "include/s2s_hip.h states the LDS bytes of s2s_eventalign");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    S2S_LAUNCH(nullptr, s2s_eventalign_kernel, dim3(P), dim3(width), S2S_EVA_LDS_BYTES(width), stream, m, as_ll(m_offs), l, as_ll(l_offs), width,
               skip_penalty, trim_penalty, unknown_cost, as_ll(cost), scratch, as_ll(scratch_offs), end_event);
    S2S_LAUNCH(nullptr, s2s_eventalign_trace_kernel, dim3(P), dim3(64), 0, stream, as_ll(m_offs), as_ll(l_offs), ev_start, ev_len, as_ll(ev_offs),
               width, as_ll(cost), scratch, as_ll(scratch_offs), first_event, end_event, ev_kmer, k_start, k_len, k_events);
    return S2S_OK;
}

// ---- preprocess (s2s_chunk.h); s2s_chunk_scratch_bytes is in s2s_host.cpp
int s2s_chunk_pack(int device, void* stream_, const void* pool, const int64_t* s_offs, int64_t total, int32_t source, const int64_t* l_offs,
                   int64_t slots, const int32_t* ev_start, const int32_t* ev_len, const int64_t* S, const int64_t* Q, const double* cal,
                   const float* stdv, const uint8_t* kmers, int32_t P, int32_t k, int32_t te, int32_t ts, int32_t reverse,
                   int32_t backwards, int64_t chunk_capacity, uint8_t* scratch, uint16_t* chunks, int64_t* chunks_lengths, float* targets,
                   int64_t* targets_lengths, float* stdevs, int32_t* n_rows, int64_t* counters) {
    const bool work = P > 0 && slots > 0;
    if (!s2s_chk_params_ok(source, k, te, ts) || !s2s_chk_counts_ok(P, total, slots, chunk_capacity) || chunk_capacity < P || !s_offs ||
        !l_offs || !counters || (P > 0 && !n_rows) ||
        (work && (!ev_start || !ev_len || !kmers || !scratch || !chunks || !chunks_lengths || !targets || !targets_lengths || !stdevs ||
                  (total > 0 && !pool) || (source == S2S_CHUNK_RAW ? (!S || !Q || !cal) : !stdv))) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(nullptr, S2S_ERR_ARG, "s2s_chunk_pack: bad argument (source 0 / 1, k 1..10, te 1..64, ts 1..1024, P <= 2^22, P <= "
                                          "chunk_capacity < 2^31, slots < 2^31, total <= 2^40, scratch 16-byte aligned)");
    GUARD_OR_RETURN(nullptr, device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(nullptr, hipMemsetAsync(counters, 0, 3 * sizeof(int64_t), stream));
    if (P > 0) HIP_TRY(nullptr, hipMemsetAsync(n_rows, 0, (size_t)P * sizeof(int32_t), stream));
    if (!work) return S2S_OK;
    static_assert(S2S_CHK_LDS_BYTES == 272, "include/s2s_hip.h states the LDS bytes of s2s_chunk_pack");
    const S2SChkScratch at = s2s_chk_layout(slots, P, chunk_capacity);
    const int64_t tiles = s2s_chk_tiles(slots);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(scratch + at.words);
    long long* trank = reinterpret_cast<long long*>(scratch + at.trank);
    long long* nrank = reinterpret_cast<long long*>(scratch + at.nrank);
    long long* r_offs = reinterpret_cast<long long*>(scratch + at.r_offs);
    long long* c_offs = reinterpret_cast<long long*>(scratch + at.c_offs);
    long long* krank = reinterpret_cast<long long*>(scratch + at.krank);
    int* wrank = reinterpret_cast<int*>(scratch + at.wrank);
    int* rows = reinterpret_cast<int*>(scratch + at.rows);
    S2SChkIn in;
    in.pool = pool;
    in.s_offs = as_ll(s_offs); in.l_offs = as_ll(l_offs);
    in.ev_start = ev_start; in.ev_len = ev_len;
    in.S = as_ll(S); in.Q = as_ll(Q);
    in.cal = source == S2S_CHUNK_RAW ? cal : nullptr;
    in.stdv = stdv; in.kmers = kmers;
    in.total = total; in.slots = slots; in.capacity = chunk_capacity;
    in.P = P; in.source = source; in.k = k; in.te = te; in.ts = ts; in.reverse = reverse ? 1 : 0; in.backwards = backwards ? 1 : 0;
    const unsigned waves = (unsigned)((chunk_capacity + S2S_CHK_WAVES - 1) / S2S_CHK_WAVES);
    S2S_LAUNCH(nullptr, s2s_chunk_flags_kernel, dim3((unsigned)tiles), dim3(S2S_CHK_THREADS), 0, stream, in, words, wrank, trank, nrank);
    S2S_LAUNCH(nullptr, (s2s_scan_kernel<1, S2SScanNext>), dim3(1), dim3(1024), 0, stream, S2SScanNext{trank}, (long long)tiles, trank);
    S2S_LAUNCH(nullptr, (s2s_scan_kernel<1, S2SScanNext>), dim3(1), dim3(1024), 0, stream, S2SScanNext{nrank}, (long long)tiles, nrank);
    S2S_LAUNCH(nullptr, s2s_chunk_compact_kernel, dim3((unsigned)tiles), dim3(S2S_CHK_THREADS), 0, stream, in, words, wrank, trank, rows,
               r_offs, c_offs, n_rows);
    S2S_LAUNCH(nullptr, (s2s_scan_kernel<1, S2SScanNext>), dim3(1), dim3(1024), 0, stream, S2SScanNext{c_offs}, (long long)P, c_offs);
    S2S_LAUNCH(nullptr, s2s_chunk_lengths_kernel, dim3(waves), dim3(S2S_CHK_THREADS), 0, stream, in, rows, r_offs, c_offs, n_rows, krank);
    S2S_LAUNCH(nullptr, (s2s_scan_kernel<1, S2SScanNext>), dim3(1), dim3(1024), 0, stream, S2SScanNext{krank}, (long long)chunk_capacity,
               krank);
    S2S_LAUNCH(nullptr, s2s_chunk_write_kernel, dim3(waves), dim3(S2S_CHK_THREADS), 0, stream, in, rows, r_offs, c_offs, n_rows, krank,
               nrank, (long long)tiles, chunks, as_ll(chunks_lengths), targets, as_ll(targets_lengths), stdevs, as_ll(counters));
    return S2S_OK;
}

}  // extern "C"

#include "s2s_train_host.h"
