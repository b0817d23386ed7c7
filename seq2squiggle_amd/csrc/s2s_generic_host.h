// s2s_generic_host.h -- host launch side of the size-generic pipeline (S2S_MODE_GENERIC / _GENERIC_F16 / _GENERIC_GEOMETRY /
// _GENERIC_GEOMETRY_F16), included by s2s_hip.hip after s2s_handle and pack_generic: the GEMM, attention and FFT-block launchers, the
// pre-net, the slice workspace, predict_generic and evaluate_generic.  The trainer (s2s_train_host.h) runs its forward pass through
// the same launchers with the buffers of its tape, which is what keeps its loss sums s2s_evaluate_chunks' bit for bit.
#pragma once

namespace {

size_t up64(size_t n) { return (n + 63) & ~(size_t)63; }

// A device buffer grown on demand (outside of the steady state only): `capacity` counts what the caller counts, `bytes` is the
// allocation that holds `want` of it.  The stream drains before the old buffer goes; a failed call leaves ptr null and capacity 0.
template <class T>
hipError_t grow_device(T*& ptr, int& capacity, int want, size_t bytes, hipStream_t st) {
    if (want <= capacity) return hipSuccess;
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr; capacity = 0;
    if ((e = hipMalloc(&ptr, bytes)) != hipSuccess) return e;
    capacity = want;
    return hipSuccess;
}

// C [M][N] = epilogue(A W^T + bias) (s2s_generic.h; the residual R of EPI 2 has C's pitch and may be C).  W is fp32 [N][K], or, where
// Wh is given, its f16 copy at a row pitch of ldw halves (s2s_generic_h.h).
template <int EPI>
void gen_gemm(hipStream_t st, const float* A, int lda, const float* W, const float* bias, float* C, int ldc, const float* R, int M, int N, int K,
              const float* Wh = nullptr, int ldw = 0) {
    const dim3 grid((M + GEN_BM - 1) / GEN_BM, (N + GEN_BN - 1) / GEN_BN);
    if (Wh)
        hipLaunchKernelGGL(gen_gemm_h_kernel<EPI>, grid, dim3(256), 0, st, A, lda, reinterpret_cast<const _Float16*>(Wh), ldw, bias, C, ldc, R,
                           ldc, M, N, K);
    else
        hipLaunchKernelGGL(gen_gemm_kernel<EPI>, grid, dim3(256), 0, st, A, lda, W, K, bias, C, ldc, R, ldc, M, N, K);
}

void gen_layernorm(hipStream_t st, float* X, const float* gam, const float* bet, int M, int d) {
    hipLaunchKernelGGL(gen_layernorm_kernel, dim3((M + 3) / 4), dim3(256), 0, st, X, gam, bet, (long long)M, d);
}

// dst [M][n] at pitch ldd = src [M][n] at pitch lds
void gen_copy(hipStream_t st, const float* src, int lds, float* dst, int ldd, long long M, int n) {
    hipLaunchKernelGGL(train_copy_kernel, dim3((unsigned)((M * n + 255) / 256)), dim3(256), 0, st, src, lds, dst, ldd, M, n);
}

// Self-attention of n chunks of T rows in qkv [n*T][3d] (O replaces Q): THE choice of the kernel, for every caller.
//   fp32: beyond 256 keys the long kernel by head_dim class; else K and V staged in LDS while they fit GEN_ATTN_STAGE_BYTES.
//   f16:  beyond GENH_TP keys the long kernel by head_dim class; the 250-key instance (S2S_MODE_GENERIC_F16: mode 7 at 250 samples
//         computes mode 5's numbers); else the instance with T at run time.
void gen_attention_fwd(hipStream_t st, float* qkv, int n, int T, int d, int H, bool f16) {
    const int hd = d / H;
    if (T > (f16 ? GENH_TP : 256)) {
        const dim3 grid((unsigned)n * H * ((T + 63) / 64));
        auto k = f16 ? (hd <= 16 ? gen_attention_long_h_kernel<1> : hd <= 128 ? gen_attention_long_h_kernel<8> : gen_attention_long_h_kernel<32>)
                     : (hd <= 16 ? gen_attention_long_kernel<1> : hd <= 128 ? gen_attention_long_kernel<8> : gen_attention_long_kernel<32>);
        hipLaunchKernelGGL(k, grid, dim3(256), 0, st, qkv, d, H, T);
    } else if (f16) {
        if (T == GEN_T_DEC)
            hipLaunchKernelGGL(gen_attention_h_kernel, dim3(n * H), dim3(1024), 0, st, qkv, d, H);
        else
            hipLaunchKernelGGL(gen_attention_h_any_kernel, dim3(n * H), dim3(1024), 0, st, qkv, d, H, T);
    } else {
        const bool stage = gen_attn_lds_bytes(T, hd, true) <= GEN_ATTN_STAGE_BYTES;
        hipLaunchKernelGGL(stage ? gen_attention_kernel<true> : gen_attention_kernel<false>, dim3(n * H), dim3(256),
                           gen_attn_lds_bytes(T, hd, stage), st, qkv, d, H, T);
    }
}

// Where one FFT block over M rows leaves its stages: QKV [M][3d] (O replaces Q), a copy of Q from before that (or nullptr), the
// two pre-LayerNorm sums and their LayerNorms [M][d], the FFN hidden [M][dff].  The trainer's tape gives each a buffer of its own.
struct GenBlock { float *qkv, *qc, *p1, *y1, *hf, *p2, *y2; };

// predict's and evaluate's assignment: the block in place on X, with BIG [M][max(3d, dff)] for QKV and then the FFN hidden
GenBlock gen_in_place(float* X, float* BIG) { return GenBlock{BIG, nullptr, X, X, BIG, X, X}; }

// One FFTBlock (layers.py:116-142) on the rows X [n*T][d] -> B.y2.  LH: the block's f16 weights for the matrix products on f16
// operands (the LayerNorms, the biases, ReLU and the residuals stay fp32), nullptr for fp32.  A stage is copied only into a
// buffer of its own.
void gen_block_fwd(hipStream_t st, const float* W, const s2s_handle::Generic& G, const GenLayer& L, const GenLayerH* LH, const float* X,
                   const GenBlock& B, int n, int T, int H) {
    const int d = G.d, dff = G.dff, M = n * T;
    auto wh = [&](long long GenLayerH::*w) { return LH ? W + LH->*w : nullptr; };
    gen_gemm<0>(st, X, d, W + L.wqkv, W + L.bqkv, B.qkv, 3 * d, nullptr, M, 3 * d, d, wh(&GenLayerH::wqkv), G.ld_d);
    if (B.qc) gen_copy(st, B.qkv, 3 * d, B.qc, d, M, d);
    gen_attention_fwd(st, B.qkv, n, T, d, H, LH != nullptr);
    gen_gemm<2>(st, B.qkv, 3 * d, W + L.wfc, W + L.bfc, B.p1, d, X, M, d, d, wh(&GenLayerH::wfc), G.ld_d);
    if (B.y1 != B.p1) gen_copy(st, B.p1, d, B.y1, d, M, d);
    gen_layernorm(st, B.y1, W + L.ln1g, W + L.ln1b, M, d);
    gen_gemm<1>(st, B.y1, d, W + L.w1, W + L.b1, B.hf, dff, nullptr, M, dff, d, wh(&GenLayerH::w1), G.ld_d);
    gen_gemm<2>(st, B.hf, dff, W + L.w2, W + L.b2, B.p2, d, B.y1, M, d, dff, wh(&GenLayerH::w2), G.ld_f);
    if (B.y2 != B.p2) gen_copy(st, B.p2, d, B.y2, d, M, d);
    gen_layernorm(st, B.y2, W + L.ln2g, W + L.ln2b, M, d);
}

// The pre-net (modules.py:70-77) on the embedded rows x [Me][d]: layer i writes out[i]; -> the last layer's output (x without layers)
const float* gen_prenet(hipStream_t st, const float* W, const s2s_handle::Generic& G, int layers, const float* x, float* const* out, int Me) {
    for (int i = 0; i < layers; ++i) {
        gen_gemm<1>(st, x, G.d, W + G.pre_w[i], W + G.pre_b[i], out[i], G.d, nullptr, Me, G.d, G.d);
        x = out[i];
    }
    return x;
}

// The slice workspace of predict and evaluate for n chunks, carved from one allocation (base == nullptr: the size only): encoder
// rows, sigma, decoder rows, sigma per sample, and BIG: [n * max(te, ts)][max(3d, dff)].
struct GenWorkspace { float *XE, *SIG, *XD, *SE, *BIG; size_t floats; };

GenWorkspace gen_workspace(const s2s_handle::Generic& G, float* base, size_t n) {
    size_t at = 0;
    auto take = [&](size_t k) { float* p = base ? base + at : nullptr; at += up64(k); return p; };
    const size_t d = G.d, te = G.te, ts = G.ts, big_w = 3 * G.d > G.dff ? 3 * G.d : G.dff, tb = te > ts ? te : ts;
    GenWorkspace ws{};
    ws.XE = take(n * te * d); ws.SIG = take(n * te); ws.XD = take(n * ts * d); ws.SE = take(n * ts); ws.BIG = take(n * tb * big_w);
    ws.floats = at;
    return ws;
}

// the handle's workspace, grown to a slice of min(B, slice_max) chunks; its capacity in chunks is h->gen.ws_chunks
int gen_workspace_for(s2s_handle* h, hipStream_t st, int32_t B, GenWorkspace& ws) {
    s2s_handle::Generic& G = h->gen;
    const int want = B < G.slice_max ? B : G.slice_max;
    HIP_TRY(h, grow_device(G.ws, G.ws_chunks, want, gen_workspace(G, nullptr, want).floats * sizeof(float), st));
    ws = gen_workspace(G, G.ws, G.ws_chunks);
    return S2S_OK;
}

// predict's and evaluate's pre-net on the rows in ws.XE: XE and BIG in turn, the result back in XE
int gen_prenet_in_place(s2s_handle* h, hipStream_t st, const GenWorkspace& ws, int Me) {
    float* out[S2S_MAX_LAYERS];
    for (int i = 0; i < h->cfg.pre_layers; ++i) out[i] = i % 2 ? ws.XE : ws.BIG;
    const float* last = gen_prenet(st, h->d_arena, h->gen, h->cfg.pre_layers, ws.XE, out, Me);
    if (last != ws.XE) HIP_TRY(h, hipMemcpyAsync(ws.XE, last, (size_t)Me * h->gen.d * sizeof(float), hipMemcpyDeviceToDevice, st));
    return S2S_OK;
}

// ---- s2s_predict_*: the launch in slices of at most gen.slice_max chunks, each slice stage by stage.
int predict_generic(s2s_handle* h, hipStream_t st, const uint8_t* bases, const int64_t* chunk_start, const uint8_t* n_valid,
                    int64_t first_global_chunk, int32_t B, const ParamsDev& P, const float* inject_g, const float* inject_zdw,
                    const float* inject_z01, float* out_signal, int32_t* out_dur, const DebugDev& D) {
    const s2s_handle::Generic& G = h->gen;
    const int d = G.d, k = h->cfg.seq_kmer, te = G.te, ts = G.ts, nb = te + k - 1;
    GenWorkspace ws;
    if (const int rc = gen_workspace_for(h, st, B, ws)) return rc;
    const size_t S = G.ws_chunks;
    const float* W = h->d_arena;
    EventPair ev{};
    if (h->profiling) {
        HIP_TRY(h, hipEventCreate(&ev.a));
        HIP_TRY(h, hipEventCreate(&ev.b));
        HIP_TRY(h, hipEventRecord(ev.a, st));
    }
    for (int64_t s = 0; s < B; s += S) {
        const int n = (int)((B - s < (int64_t)S) ? (B - s) : (int64_t)S);
        const int Me = n * te, Md = n * ts;
        const long long fc = (long long)(first_global_chunk + s);
        DebugDev Ds = D;                      // the caller's arrays, offset to the slice
        auto off = [&](float* p, size_t per) { return p ? p + (size_t)s * per : nullptr; };
        Ds.sigma = off(D.sigma, te); Ds.conc = off(D.conc, te); Ds.rate = off(D.rate, te); Ds.g = off(D.g, te);
        Ds.y_scaled = off(D.y_scaled, ts); Ds.z01 = off(D.z01, ts);
        // encoder input: src_emb + pre-net (modules.py:70-77), or the caller's rows (s2s_debug.emb_in)
        if (D.emb_in) {
            HIP_TRY(h, hipMemcpyAsync(ws.XE, D.emb_in + (size_t)s * te * d, (size_t)Me * d * sizeof(float), hipMemcpyDeviceToDevice, st));
        } else {
            const uint8_t* tb = chunk_start ? bases : bases + (size_t)s * nb;
            const long long* tcs = reinterpret_cast<const long long*>(chunk_start ? chunk_start + s : nullptr);
            const long long tot = (long long)Me * d;
            hipLaunchKernelGGL(gen_embed_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, W + G.emb_wt, W + G.emb_b, k, d, tb, tcs,
                               n_valid + s, n, te, ws.XE);
            if (const int rc = gen_prenet_in_place(h, st, ws, Me)) return rc;
        }
        if (D.emb_out)
            HIP_TRY(h, hipMemcpyAsync(D.emb_out + (size_t)s * te * d, ws.XE, (size_t)Me * d * sizeof(float), hipMemcpyDeviceToDevice, st));
        // heads (modules.py:182-195, 267-278): the three first layers as one GEMM, then the dwell source; + position_enc
        gen_gemm<1>(st, ws.XE, d, W + G.w0cat, W + G.b0cat, ws.BIG, 3 * d, nullptr, Me, P.duration_sampling ? 3 * d : d, d);
        hipLaunchKernelGGL(gen_dwell_kernel, dim3((Me + 3) / 4), dim3(256), 0, st, W, G.heads, G.pe_enc, d, n, ws.BIG, ws.XE, ws.SIG, fc, P,
                           inject_g ? inject_g + s * te : nullptr, inject_zdw ? inject_zdw + s * te : nullptr, out_dur + s * te, Ds, te);
        for (int l = 0; l < h->cfg.encoder_layers; ++l)
            gen_block_fwd(st, W, G, G.enc[l], nullptr, ws.XE, gen_in_place(ws.XE, ws.BIG), n, te, G.h_enc);
        if (D.enc_out)
            HIP_TRY(h, hipMemcpyAsync(D.enc_out + (size_t)s * te * d, ws.XE, (size_t)Me * d * sizeof(float), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(gen_lenreg_kernel, dim3((Md + 3) / 4), dim3(256), 0, st, W, G.pe_dec, d, n, ws.XE, ws.SIG, out_dur + s * te, ws.XD,
                           ws.SE, D.dec_in ? D.dec_in + (size_t)s * ts * d : nullptr, te, ts);
        for (int l = 0; l < h->cfg.decoder_layers; ++l)
            gen_block_fwd(st, W, G, G.dec[l], G.f16 ? &G.dech[l] : nullptr, ws.XD, gen_in_place(ws.XD, ws.BIG), n, ts, G.h_dec);
        hipLaunchKernelGGL(gen_emit_kernel, dim3((Md + 3) / 4), dim3(256), 0, st, W, G.out_w, G.out_b, h->cfg.scaling_max_value, d, n, ws.XD,
                           ws.SE, fc, P, inject_z01 ? inject_z01 + (size_t)s * ts : nullptr, out_signal + (size_t)s * ts, Ds, ts);
    }
    if (h->profiling) {
        HIP_TRY(h, hipEventRecord(ev.b, st));
        ev.chunks = B;
        h->events.push_back(ev);
    }
    HIP_TRY(h, hipGetLastError());
    return S2S_OK;
}

// ---- s2s_evaluate_chunks on the generic pipeline: predict_generic's stages with the teacher-forced embed / heads / emit kernels
// (s2s_generic.h); gen_lenreg_kernel reads the measured dwell.  y [B][ts], sigma / conc / rate [B][te] (the caller's slice).
int evaluate_generic(s2s_handle* h, hipStream_t st, const uint8_t* kmers, const int32_t* dwell, int32_t B, float* y, float* sigma, float* conc,
                     float* rate) {
    const s2s_handle::Generic& G = h->gen;
    const int d = G.d, k = h->cfg.seq_kmer, te = G.te, ts = G.ts;
    GenWorkspace ws;
    if (const int rc = gen_workspace_for(h, st, B, ws)) return rc;
    const size_t S = G.ws_chunks;
    const float* W = h->d_arena;
    for (int64_t s = 0; s < B; s += S) {
        const int n = (int)((B - s < (int64_t)S) ? (B - s) : (int64_t)S);
        const int Me = n * te, Md = n * ts;
        const long long tot = (long long)Me * d;
        hipLaunchKernelGGL(gen_embed_kmers_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, W + G.emb_wt, W + G.emb_b, k, d,
                           kmers + (size_t)s * te * k, n, te, ws.XE);
        if (const int rc = gen_prenet_in_place(h, st, ws, Me)) return rc;
        gen_gemm<1>(st, ws.XE, d, W + G.w0cat, W + G.b0cat, ws.BIG, 3 * d, nullptr, Me, 3 * d, d);
        float* sg = sigma + (size_t)s * te;
        hipLaunchKernelGGL(gen_dwell_teacher_kernel, dim3((Me + 3) / 4), dim3(256), 0, st, W, G.heads, G.pe_enc, d, n, ws.BIG, ws.XE, sg,
                           conc + (size_t)s * te, rate + (size_t)s * te, te);
        for (int l = 0; l < h->cfg.encoder_layers; ++l)
            gen_block_fwd(st, W, G, G.enc[l], nullptr, ws.XE, gen_in_place(ws.XE, ws.BIG), n, te, G.h_enc);
        hipLaunchKernelGGL(gen_lenreg_kernel, dim3((Md + 3) / 4), dim3(256), 0, st, W, G.pe_dec, d, n, ws.XE, sg, dwell + (size_t)s * te, ws.XD,
                           ws.SE, nullptr, te, ts);
        for (int l = 0; l < h->cfg.decoder_layers; ++l)
            gen_block_fwd(st, W, G, G.dec[l], G.f16 ? &G.dech[l] : nullptr, ws.XD, gen_in_place(ws.XD, ws.BIG), n, ts, G.h_dec);
        hipLaunchKernelGGL(gen_emit_y_kernel, dim3((Md + 3) / 4), dim3(256), 0, st, W, G.out_w, G.out_b, d, n, ws.XD, y + (size_t)s * ts, ts);
    }
    return S2S_OK;
}

}  // namespace
