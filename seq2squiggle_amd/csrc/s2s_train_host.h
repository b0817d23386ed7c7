// s2s_train_host.h -- host side of the trainer (s2s_trainer_*, include/s2s_hip.h), included at the end of s2s_hip.hip: the tape,
// the launch order of the forward (evaluate_generic's stages through the launchers it uses, s2s_generic_host.h) and backward
// (s2s_train.h) passes, micro-batching and the optimizer step.
//
// Weights, gradient, m and v live in the generic handle's arena layout (pack_generic: every piece 16-byte aligned for the GEMM's
// float4 loads, src_emb.weight transposed, q/k/v and the heads' first layers concatenated), not in the blob's: the blob's own
// offsets are odd after the first Linear(d,1) bias.  Every entry that hands values out (s2s_trainer_weights, out_grad) gathers
// them into blob order through `map`; the padding between pieces has weight 0 and gradient 0 and stays 0 under every step.
#pragma once

struct s2s_trainer {
    s2s_config cfg;
    int device = 0;
    std::string err;
    s2s_handle::Generic G;
    size_t arena_floats = 0, blob_floats = 0;
    float *w = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;
    int* map = nullptr;               // blob index -> arena index
    float* blob_tmp = nullptr;        // [blob_floats]: a gather's destination when the caller's buffer is on the host
    size_t budget = S2S_TRAINER_DEFAULT_MEMORY;  // bytes of tape + backward scratch per micro-batch (s2s_trainer_set_memory)
    float* ws = nullptr;              // the tape and the backward scratch of one micro-batch
    int ws_chunks = 0;
    float* losses = nullptr;          // [B][3] per-chunk sums of the last call
    int losses_cap = 0;
    float* stats = nullptr;           // [8]: 0-3 loss means, 4 gradient norm, 5 clip scale
    double* nrm_part = nullptr;
    int nrm_blocks = 0;
};

namespace {

thread_local std::string g_trainer_error;

int tfail(s2s_trainer* t, int code, const std::string& msg) {
    if (t) t->err = msg; else g_trainer_error = msg;
    return code;
}
#define TR_TRY(t, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return tfail((t), S2S_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

// the tape of one FFT block over M rows: every stage of gen_block_fwd in a buffer of its own
using TrainBlock = GenBlock;

// Every buffer of a micro-batch of n chunks, carved from one allocation (base == nullptr: sizes only).
struct TrainTape {
    float *e0, *pre[S2S_MAX_LAYERS], *hid, *xe0, *sig, *conc, *rate, *dz, *dhid, *oh;
    TrainBlock enc[S2S_MAX_LAYERS], dec[S2S_MAX_LAYERS];
    float *xd0, *se, *y, *dy;
    float *da, *db, *gg, *dbig, *part;
    int oh_ld = 0, nz_max = 0;
    size_t floats = 0;
};

TrainTape train_tape(const s2s_config& c, float* base, size_t n) {
    TrainTape T{};
    size_t at = 0;
    auto take_ = [&](size_t k) { float* p = base ? base + at : nullptr; at += up64(k); return p; };
    const size_t d = c.dmodel, f = c.dff, te = c.max_dna_len, ts = c.max_signal_len, tb = te > ts ? te : ts;
    const size_t Me = n * te, Md = n * ts, Mb = n * tb, big = 3 * d > f ? 3 * d : f;
    T.oh_ld = (5 * c.seq_kmer + 3) & ~3;
    T.e0 = take_(Me * d);
    for (int i = 0; i < c.pre_layers; ++i) T.pre[i] = take_(Me * d);
    T.hid = take_(Me * 3 * d); T.xe0 = take_(Me * d);
    T.sig = take_(Me); T.conc = take_(Me); T.rate = take_(Me);
    T.dz = take_(Me * 4); T.dhid = take_(Me * 3 * d); T.oh = take_(Me * T.oh_ld);
    auto block = [&](TrainBlock& b, size_t M) {
        b.qkv = take_(M * 3 * d); b.qc = take_(M * d); b.p1 = take_(M * d); b.y1 = take_(M * d);
        b.hf = take_(M * f); b.p2 = take_(M * d); b.y2 = take_(M * d);
    };
    for (int l = 0; l < c.encoder_layers; ++l) block(T.enc[l], Me);
    T.xd0 = take_(Md * d); T.se = take_(Md); T.y = take_(Md); T.dy = take_(Md);
    for (int l = 0; l < c.decoder_layers; ++l) block(T.dec[l], Md);
    T.da = take_(Mb * d); T.db = take_(Mb * d); T.gg = take_(Mb * d); T.dbig = take_(Mb * big);
    T.nz_max = (int)((Mb + TR_GRAD_ROWS - 1) / TR_GRAD_ROWS);
    size_t nk = 3 * d * d > f * d ? 3 * d * d : f * d;
    if ((size_t)T.oh_ld * d > nk) nk = (size_t)T.oh_ld * d;
    T.part = take_((size_t)T.nz_max * nk);
    T.floats = at;
    return T;
}

struct TrainRun {
    s2s_trainer* t;
    hipStream_t st;
    const float* W;
    TrainTape T;

    // grad[off .. off + I J) += sum_rows L[row][i] R[row][j]
    void wgrad(const float* L, int ldl, const float* R, int ldr, int I, int J, int M, long long off) {
        const int nz = (M + TR_GRAD_ROWS - 1) / TR_GRAD_ROWS;
        const dim3 grid((I + TR_TILE - 1) / TR_TILE, (J + TR_TILE - 1) / TR_TILE, nz);
        hipLaunchKernelGGL((train_mm_kernel<false, 0>), grid, dim3(256), 0, st, L, ldl, R, ldr, T.part, J, (const float*)nullptr, 0, I, J, M,
                           TR_GRAD_ROWS);
        const long long n = (long long)I * J;
        hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, T.part, nz, n, t->g + off);
    }
    // grad[off .. off + N) += column sums of A [M][N]
    void colsum(const float* A, int lda, int M, int N, long long off) {
        const int nz = (M + TR_GRAD_ROWS - 1) / TR_GRAD_ROWS;
        hipLaunchKernelGGL(train_colsum_kernel, dim3((N + 63) / 64, nz), dim3(256), 0, st, A, lda, M, N, TR_GRAD_ROWS, T.part);
        hipLaunchKernelGGL(train_reduce_kernel, dim3((N + 255) / 256), dim3(256), 0, st, T.part, nz, (long long)N, t->g + off);
    }
    // C [M][K] = epilogue(dY [M][N] W [N][K])
    template <int EPI>
    void dgrad(const float* dY, int N, long long w, float* C, const float* E, int M, int K) {
        const dim3 grid((M + TR_TILE - 1) / TR_TILE, (K + TR_TILE - 1) / TR_TILE, 1);
        hipLaunchKernelGGL((train_mm_kernel<true, EPI>), grid, dim3(256), 0, st, dY, N, W + w, K, C, K, E, K, M, K, N, N);
    }
    // dio: in the gradient at the block's output, out the gradient at its input X
    void block_bwd(const GenLayer& L, const float* X, const TrainBlock& B, float* dio, int n, int Tn, int H) {
        const int d = t->G.d, dff = t->G.dff, M = n * Tn;
        const dim3 rows((M + 3) / 4);
        hipLaunchKernelGGL(train_layernorm_bwd_kernel, rows, dim3(256), 0, st, B.p2, dio, W + L.ln2g, T.db, T.gg, (long long)M, d);
        colsum(T.gg, d, M, d, L.ln2g);
        colsum(dio, d, M, d, L.ln2b);
        wgrad(T.db, d, B.hf, dff, d, dff, M, L.w2);
        colsum(T.db, d, M, d, L.b2);
        dgrad<1>(T.db, d, L.w2, T.dbig, B.hf, M, dff);
        wgrad(T.dbig, dff, B.y1, d, dff, d, M, L.w1);
        colsum(T.dbig, dff, M, dff, L.b1);
        dgrad<2>(T.dbig, dff, L.w1, dio, T.db, M, d);
        hipLaunchKernelGGL(train_layernorm_bwd_kernel, rows, dim3(256), 0, st, B.p1, dio, W + L.ln1g, T.db, T.gg, (long long)M, d);
        colsum(T.gg, d, M, d, L.ln1g);
        colsum(dio, d, M, d, L.ln1b);
        wgrad(T.db, d, B.qkv, 3 * d, d, d, M, L.wfc);
        colsum(T.db, d, M, d, L.bfc);
        dgrad<0>(T.db, d, L.wfc, T.gg, nullptr, M, d);
        hipLaunchKernelGGL(train_attention_bwd_kernel, dim3(n * H), dim3(256), 0, st, B.qc, B.qkv, T.gg, T.dbig, d, H, Tn);
        wgrad(T.dbig, 3 * d, X, d, 3 * d, d, M, L.wqkv);
        colsum(T.dbig, 3 * d, M, 3 * d, L.bqkv);
        dgrad<2>(T.dbig, 3 * d, L.wqkv, dio, T.db, M, d);
    }

    // one micro-batch of n chunks out of a batch of B: forward with the tape, the per-chunk loss sums, backward into t->g
    void micro(const uint8_t* kmers, const int32_t* dwell, const float* target, const float* stdev, int n, int B, float* loss) {
        const s2s_handle::Generic& G = t->G;
        const s2s_config& c = t->cfg;
        const int d = G.d, k = c.seq_kmer, te = G.te, ts = G.ts;
        const int Me = n * te, Md = n * ts;
        const long long tot = (long long)Me * d;
        hipLaunchKernelGGL(gen_embed_kmers_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, W + G.emb_wt, W + G.emb_b, k, d, kmers,
                           n, te, T.e0);
        const float* emb = gen_prenet(st, W, G, c.pre_layers, T.e0, T.pre, Me);
        gen_gemm<1>(st, emb, d, W + G.w0cat, W + G.b0cat, T.hid, 3 * d, nullptr, Me, 3 * d, d);
        gen_copy(st, emb, d, T.xe0, d, Me, d);
        hipLaunchKernelGGL(gen_dwell_teacher_kernel, dim3((Me + 3) / 4), dim3(256), 0, st, W, G.heads, G.pe_enc, d, n, T.hid, T.xe0, T.sig, T.conc,
                           T.rate, te);
        const float* x = T.xe0;
        for (int l = 0; l < c.encoder_layers; ++l) { gen_block_fwd(st, W, G, G.enc[l], nullptr, x, T.enc[l], n, te, G.h_enc); x = T.enc[l].y2; }
        hipLaunchKernelGGL(gen_lenreg_kernel, dim3((Md + 3) / 4), dim3(256), 0, st, W, G.pe_dec, d, n, x, T.sig, dwell, T.xd0, T.se,
                           (const float*)nullptr, te, ts);
        x = T.xd0;
        for (int l = 0; l < c.decoder_layers; ++l) { gen_block_fwd(st, W, G, G.dec[l], nullptr, x, T.dec[l], n, ts, G.h_dec); x = T.dec[l].y2; }
        hipLaunchKernelGGL(gen_emit_y_kernel, dim3((Md + 3) / 4), dim3(256), 0, st, W, G.out_w, G.out_b, d, n, x, T.y, ts);
        hipLaunchKernelGGL(s2s_eval_loss_kernel, dim3((n + 3) / 4), dim3(256), 0, st, T.y, target, T.sig, stdev, T.conc, T.rate, dwell, n, te, ts,
                           loss);
        // ---- backward: the signal loss down to src_emb
        const float c_sig = (float)(2.0 / ((double)B * ts)), c_noise = (float)(2.0 / ((double)B * te));
        const float c_dur = (float)(0.0005 / ((double)B * te));
        hipLaunchKernelGGL(train_emit_bwd_kernel, dim3((Md + 3) / 4), dim3(256), 0, st, W, G.out_w, d, (long long)Md, T.y, target, c_sig, T.dy,
                           T.da);
        wgrad(T.dy, 1, x, d, 1, d, Md, G.out_w);
        colsum(T.dy, 1, Md, 1, G.out_b);
        for (int l = c.decoder_layers - 1; l >= 0; --l) block_bwd(G.dec[l], l ? T.dec[l - 1].y2 : T.xd0, T.dec[l], T.da, n, ts, G.h_dec);
        // (T.db is free between blocks: the regulator's sum lands there, then moves to T.da, the blocks' in / out buffer)
        hipLaunchKernelGGL(train_lenreg_bwd_kernel, dim3((Me + 3) / 4), dim3(256), 0, st, T.da, dwell, T.db, (long long)Me, d, te, ts);
        gen_copy(st, T.db, d, T.da, d, Me, d);
        for (int l = c.encoder_layers - 1; l >= 0; --l) block_bwd(G.enc[l], l ? T.enc[l - 1].y2 : T.xe0, T.enc[l], T.da, n, te, G.h_enc);
        float* de = T.da;
        float* other = T.db;
        hipLaunchKernelGGL(train_relu_mask_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, de, emb, de, tot);
        for (int i = c.pre_layers - 1; i >= 0; --i) {
            const float* in = i ? T.pre[i - 1] : T.e0;
            wgrad(de, d, in, d, d, d, Me, G.pre_w[i]);
            colsum(de, d, Me, d, G.pre_b[i]);
            dgrad<1>(de, d, G.pre_w[i], other, in, Me, d);
            float* s = de; de = other; other = s;
        }
        const long long ohn = (long long)Me * T.oh_ld;
        hipLaunchKernelGGL(train_onehot_kernel, dim3((unsigned)((ohn + 255) / 256)), dim3(256), 0, st, kmers, k, (long long)Me, T.oh_ld, T.oh);
        wgrad(T.oh, T.oh_ld, de, d, 5 * k, d, Me, G.emb_wt);
        colsum(de, d, Me, d, G.emb_b);
        // ---- the three heads on emb_out.detach(): nothing flows into the pre-net
        hipLaunchKernelGGL(train_heads_bwd_kernel, dim3((Me + 3) / 4), dim3(256), 0, st, W, G.heads, d, (long long)Me, T.hid, stdev, dwell, c_noise,
                           c_dur, T.dz, T.dhid);
        wgrad(T.dhid, 3 * d, emb, d, 3 * d, d, Me, G.w0cat);
        colsum(T.dhid, 3 * d, Me, 3 * d, G.b0cat);
        for (int q = 0; q < 3; ++q) {
            wgrad(T.dz + q, 4, T.hid + (size_t)q * d, 3 * d, 1, d, Me, G.heads.w3[q]);
            colsum(T.dz + q, 4, Me, 1, G.heads.b3[q]);
        }
    }
};

// chunks per micro-batch of a batch of B: what the budget holds (one chunk always runs), at most the generic handle's slice (an
// attention launch holds fewer than 2^32 threads, pack_generic) and at most 65,535 weight-gradient row tiles (they ride in gridDim.z)
size_t train_micro_batch(const s2s_trainer* t, int32_t B) {
    const s2s_config& c = t->cfg;
    size_t cap = t->budget / (train_tape(c, nullptr, 1).floats * sizeof(float));
    if (cap < 1) cap = 1;
    if (cap > (size_t)B) cap = B;
    if (cap > (size_t)t->G.slice_max) cap = t->G.slice_max;
    const size_t tb = c.max_dna_len > c.max_signal_len ? c.max_dna_len : c.max_signal_len;
    const size_t rows_cap = (size_t)65535 * TR_GRAD_ROWS / tb;
    if (cap > rows_cap) cap = rows_cap;
    while (cap > 1 && train_tape(c, nullptr, cap).floats * sizeof(float) > t->budget) --cap;
    return cap;
}

// forward + backward of the whole batch in micro-batches: t->g = the gradient, t->losses = the per-chunk sums
int train_gradients(s2s_trainer* t, hipStream_t st, const uint8_t* kmers, const int32_t* dwell, const float* target, const float* stdev,
                    int32_t B) {
    const s2s_config& c = t->cfg;
    const size_t cap = train_micro_batch(t, B);
    TR_TRY(t, grow_device(t->ws, t->ws_chunks, (int)cap, train_tape(c, nullptr, cap).floats * sizeof(float), st));
    TR_TRY(t, grow_device(t->losses, t->losses_cap, B, (size_t)B * 3 * sizeof(float), st));
    TrainRun R{t, st, t->w, train_tape(c, t->ws, cap)};
    TR_TRY(t, hipMemsetAsync(t->g, 0, t->arena_floats * sizeof(float), st));
    const int te = c.max_dna_len, ts = c.max_signal_len, k = c.seq_kmer;
    for (int64_t s = 0; s < B; s += (int64_t)cap) {
        const int n = (int)((B - s < (int64_t)cap) ? (B - s) : (int64_t)cap);
        R.micro(kmers + (size_t)s * te * k, dwell + (size_t)s * te, target + (size_t)s * ts, stdev + (size_t)s * te, n, B, t->losses + s * 3);
    }
    TR_TRY(t, hipGetLastError());
    return S2S_OK;
}

// src (arena) -> dst in blob order; dst may be a host pointer
int train_gather_out(s2s_trainer* t, hipStream_t st, const float* src, float* dst) {
    hipPointerAttribute_t at;
    const bool on_device = hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    const long long n = (long long)t->blob_floats;
    float* out = on_device ? dst : t->blob_tmp;
    hipLaunchKernelGGL(train_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, t->map, n, out);
    TR_TRY(t, hipGetLastError());
    if (!on_device) {
        TR_TRY(t, hipMemcpyAsync(dst, out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
        TR_TRY(t, hipStreamSynchronize(st));
    }
    return S2S_OK;
}

const char* train_check_args(const s2s_trainer* t, const void* kmers, const void* dwell, const void* target, const void* stdev, int32_t B) {
    if (B < 1) return "B < 1";
    if (!kmers || !dwell || !target || !stdev) return "NULL argument";
    hipPointerAttribute_t at;
    const bool known = hipPointerGetAttributes(&at, kmers) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    if (known && at.device != t->device) return "the inputs lie on another device than the trainer";
    return nullptr;
}

}  // namespace

extern "C" {

const char* s2s_trainer_last_error(const s2s_trainer* t) { return t ? t->err.c_str() : g_trainer_error.c_str(); }

void s2s_trainer_destroy(s2s_trainer* t) {
    if (!t) return;
    DeviceGuard guard(t->device);
    for (void* p : {(void*)t->w, (void*)t->g, (void*)t->m, (void*)t->v, (void*)t->map, (void*)t->blob_tmp, (void*)t->ws, (void*)t->losses,
                    (void*)t->stats, (void*)t->nrm_part})
        if (p) (void)hipFree(p);
    delete t;
}

int s2s_trainer_create(const s2s_config* cfg, const void* blob, size_t blob_bytes, int device, s2s_trainer** out) {
    if (!out) return tfail(nullptr, S2S_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!cfg || !blob) return tfail(nullptr, S2S_ERR_ARG, "NULL argument");
    if (cfg->compute_mode != S2S_MODE_GENERIC_GEOMETRY)
        return tfail(nullptr, S2S_ERR_ARG, "the trainer runs S2S_MODE_GENERIC_GEOMETRY only (exact fp32)");
    if (const char* why = check_cfg(cfg)) return tfail(nullptr, S2S_ERR_ARG, why);
    if (blob_bytes != s2s_blob_floats(cfg) * sizeof(float)) {
        char buf[160];
        snprintf(buf, sizeof buf, "weight blob is %zu bytes, expected %zu", blob_bytes, s2s_blob_floats(cfg) * sizeof(float));
        return tfail(nullptr, S2S_ERR_BLOB, buf);
    }
    int ndev = 0;
    TR_TRY(nullptr, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return tfail(nullptr, S2S_ERR_ARG, "no such HIP device");
    DeviceGuard guard(device);
    if (!guard.ok) return tfail(nullptr, S2S_ERR_HIP, "hipSetDevice failed");
    s2s_trainer* t = new s2s_trainer;
    t->cfg = *cfg; t->device = device;
    t->blob_floats = blob_bytes / sizeof(float);
    Arena A;
    pack_generic(A, t->G, cfg, static_cast<const float*>(blob));
    while (A.v.size() % 64) A.v.push_back(0.0f);
    t->arena_floats = A.v.size();
    // blob index -> arena index: the same packing run on a blob that holds its own indices + 1 as bit patterns (it only moves
    // values), read back from the arena; the padding is 0
    std::vector<int> map(t->blob_floats, -1);
    {
        std::vector<float> idx(t->blob_floats);
        for (size_t i = 0; i < idx.size(); ++i) { const uint32_t u = (uint32_t)i + 1; std::memcpy(&idx[i], &u, 4); }
        Arena I;
        s2s_handle::Generic tmp;
        pack_generic(I, tmp, cfg, idx.data());
        for (size_t a = 0; a < I.v.size(); ++a) {
            uint32_t u;
            std::memcpy(&u, &I.v[a], 4);
            if (u) map[u - 1] = (int)a;
        }
        for (int v : map)
            if (v < 0) { delete t; return tfail(nullptr, S2S_ERR_ARG, "internal: blob element without an arena slot"); }
    }
    const size_t ab = t->arena_floats * sizeof(float);
    t->nrm_blocks = (int)((t->arena_floats + 2047) / 2048);
    auto bail = [&](const char* what, hipError_t e) {
        const std::string msg = std::string(what) + ": " + hipGetErrorString(e);
        s2s_trainer_destroy(t);
        return tfail(nullptr, S2S_ERR_HIP, msg);
    };
    hipError_t e;
    // (the staged forward attention takes up to GEN_ATTN_STAGE_BYTES of dynamic LDS: as s2s_create, for a process without a generic handle)
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(gen_attention_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 GEN_ATTN_STAGE_BYTES)) != hipSuccess)
        return bail("hipFuncSetAttribute(generic attention LDS)", e);
    if ((e = hipMalloc(&t->w, ab)) != hipSuccess) return bail("hipMalloc(weights)", e);
    if ((e = hipMalloc(&t->g, ab)) != hipSuccess) return bail("hipMalloc(gradient)", e);
    if ((e = hipMalloc(&t->m, ab)) != hipSuccess) return bail("hipMalloc(m)", e);
    if ((e = hipMalloc(&t->v, ab)) != hipSuccess) return bail("hipMalloc(v)", e);
    if ((e = hipMalloc(&t->map, t->blob_floats * sizeof(int))) != hipSuccess) return bail("hipMalloc(map)", e);
    if ((e = hipMalloc(&t->blob_tmp, t->blob_floats * sizeof(float))) != hipSuccess) return bail("hipMalloc(blob)", e);
    if ((e = hipMalloc(&t->stats, 8 * sizeof(float))) != hipSuccess) return bail("hipMalloc(stats)", e);
    if ((e = hipMalloc(&t->nrm_part, (size_t)t->nrm_blocks * sizeof(double))) != hipSuccess) return bail("hipMalloc(norm)", e);
    if ((e = hipMemcpy(t->w, A.v.data(), ab, hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy(weights)", e);
    if ((e = hipMemcpy(t->map, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy(map)", e);
    if ((e = hipMemset(t->g, 0, ab)) != hipSuccess) return bail("hipMemset", e);
    if ((e = hipMemset(t->m, 0, ab)) != hipSuccess) return bail("hipMemset", e);
    if ((e = hipMemset(t->v, 0, ab)) != hipSuccess) return bail("hipMemset", e);
    if ((e = hipMemset(t->stats, 0, 8 * sizeof(float))) != hipSuccess) return bail("hipMemset", e);
    *out = t;
    return S2S_OK;
}

int s2s_trainer_set_memory(s2s_trainer* t, size_t bytes) {
    if (!t) return S2S_ERR_ARG;
    if (bytes < 1) return tfail(t, S2S_ERR_ARG, "the memory budget must be at least 1 byte (one chunk always runs)");
    t->budget = bytes;
    return S2S_OK;
}

int64_t s2s_trainer_micro_batch(const s2s_trainer* t, int32_t B) {
    if (!t || B < 1) return S2S_ERR_ARG;
    return (int64_t)train_micro_batch(t, B);
}

int s2s_trainer_weights(s2s_trainer* t, void* stream, float* out_blob) {
    if (!t) return S2S_ERR_ARG;
    if (!out_blob) return tfail(t, S2S_ERR_ARG, "NULL argument");
    DeviceGuard guard(t->device);
    if (!guard.ok) return tfail(t, S2S_ERR_HIP, "hipSetDevice failed");
    return train_gather_out(t, static_cast<hipStream_t>(stream), t->w, out_blob);
}

int s2s_trainer_gradients(s2s_trainer* t, void* stream, const uint8_t* kmers, const int32_t* dwell, const float* target, const float* stdev,
                          int32_t B, float* out_loss, float* out_grad) {
    if (!t) return S2S_ERR_ARG;
    if (const char* why = train_check_args(t, kmers, dwell, target, stdev, B)) return tfail(t, S2S_ERR_ARG, why);
    if (!out_loss || !out_grad) return tfail(t, S2S_ERR_ARG, "NULL argument");
    DeviceGuard guard(t->device);
    if (!guard.ok) return tfail(t, S2S_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = train_gradients(t, st, kmers, dwell, target, stdev, B);
    if (rc != S2S_OK) return rc;
    TR_TRY(t, hipMemcpyAsync(out_loss, t->losses, (size_t)B * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return train_gather_out(t, st, t->g, out_grad);
}

int s2s_trainer_step(s2s_trainer* t, void* stream, const uint8_t* kmers, const int32_t* dwell, const float* target, const float* stdev,
                     int32_t B, const s2s_adam* hyper, float* out_stats) {
    if (!t) return S2S_ERR_ARG;
    if (const char* why = train_check_args(t, kmers, dwell, target, stdev, B)) return tfail(t, S2S_ERR_ARG, why);
    if (!hyper || !out_stats) return tfail(t, S2S_ERR_ARG, "NULL argument");
    if (hyper->step < 1) return tfail(t, S2S_ERR_ARG, "step counts from 1");
    if (!(hyper->beta1 >= 0.0 && hyper->beta1 < 1.0) || !(hyper->beta2 >= 0.0 && hyper->beta2 < 1.0) || !(hyper->eps > 0.0))
        return tfail(t, S2S_ERR_ARG, "betas must lie in [0, 1) and eps must be positive");
    DeviceGuard guard(t->device);
    if (!guard.ok) return tfail(t, S2S_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = train_gradients(t, st, kmers, dwell, target, stdev, B);
    if (rc != S2S_OK) return rc;
    hipLaunchKernelGGL(train_loss_stats_kernel, dim3(1), dim3(64), 0, st, t->losses, B, t->cfg.max_dna_len, t->cfg.max_signal_len, t->stats);
    hipLaunchKernelGGL(train_sumsq_kernel, dim3(t->nrm_blocks), dim3(256), 0, st, t->g, (long long)t->arena_floats, t->nrm_part);
    hipLaunchKernelGGL(train_norm_kernel, dim3(1), dim3(256), 0, st, t->nrm_part, t->nrm_blocks, (float)hyper->clip, t->stats);
    TrainAdam A;
    A.lr = (float)hyper->lr; A.b1 = (float)hyper->beta1; A.b2 = (float)hyper->beta2; A.eps = (float)hyper->eps;
    A.omb1 = (float)(1.0 - hyper->beta1); A.omb2 = (float)(1.0 - hyper->beta2);
    A.wd = (float)hyper->weight_decay; A.decoupled = hyper->decoupled ? 1 : 0;
    A.step_size = (float)(hyper->lr / (1.0 - std::pow(hyper->beta1, (double)hyper->step)));
    A.bias2_sqrt = (float)std::sqrt(1.0 - std::pow(hyper->beta2, (double)hyper->step));
    // everything but the two position tables, which have no gradient and never change
    const s2s_handle::Generic& G = t->G;
    const long long d = G.d;
    const long long cut[4] = {G.pe_enc, G.pe_enc + G.te * d, G.pe_dec, G.pe_dec + G.ts * d};
    const long long range[3][2] = {{0, cut[0]}, {cut[1], cut[2]}, {cut[3], (long long)t->arena_floats}};
    for (const auto& r : range) {
        if (r[1] <= r[0]) continue;
        hipLaunchKernelGGL(train_adam_kernel, dim3((unsigned)((r[1] - r[0] + 255) / 256)), dim3(256), 0, st, t->w, t->g, t->m, t->v, r[0], r[1], A,
                           t->stats);
    }
    TR_TRY(t, hipGetLastError());
    TR_TRY(t, hipMemcpyAsync(out_stats, t->stats, 5 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return S2S_OK;
}

}  // extern "C"
