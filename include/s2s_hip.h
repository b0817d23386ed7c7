/* s2s_hip.h -- C ABI of the MI355X-native seq2squiggle predict path.
 *
 * The reference (ZKI-PH-ImageAnalysis/seq2squiggle v0.3.4) is pure Python and has no FFI of
 * its own; this header is the boundary a maintainer binds with ctypes (INTEGRATION.md shows
 * the stub).  Each entry point names the reference code it replaces (paths relative to the
 * reference's src/seq2squiggle/).
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is owned by the caller;
 *   - pointers marked "device" are HIP device pointers on the handle's device;
 *   - all launches are stream-ordered on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) and asynchronous w.r.t. the host;
 *   - return value 0 = success, negative = error; s2s_last_error() gives the message;
 *   - a handle may be used from one host thread and on one stream at a time (it owns the per-workgroup hand-off slots that
 *     consecutive launches reuse in stream order); every call makes the handle's device current for its duration
 *     and restores the caller's; there is no global state.
 */
#ifndef S2S_HIP_H
#define S2S_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2S_OK 0
#define S2S_ERR_ARG (-1)     /* bad argument / unsupported configuration */
#define S2S_ERR_HIP (-2)     /* a HIP runtime call failed                 */
#define S2S_ERR_BLOB (-3)    /* weight blob has the wrong size            */
#define S2S_ERR_CODEC (-4)   /* a host compression codec is unavailable (libzstd.so.1 not loadable) or failed */

/* Decoder arithmetic.  F32 stays inside the 1e-4 pA MAE parity bound whatever the magnitudes of the weights (it is bit-invariant
 * under the power-of-two rescalings below); F16X3 stays inside it over the measured range stated with the mode.
 *   S2S_MODE_F32    every product on the f32-input MFMA (v_mfma_f32_16x16x4_f32), exact fp32;
 *   S2S_MODE_F16X3  operands split into two f16 halves, three f16 MFMA products with fp32 accumulation per original product
 *                   (v_mfma_f32_16x16x32_f16).  The pair carries 22 significant bits only while |x| >= 2^-3 (the lo half a normal
 *                   f16); below, the lo half is a subnormal and the pair has an absolute error near 2^-25 whatever the size of
 *                   x.  Nothing rescales before the split, so the bound depends on where a checkpoint puts its magnitudes.
 *                   Measured range (one MI355X, the synthetic k = 9 checkpoint, tests/test_gpu_magnitudes.py, LABNOTES.md round
 *                   16): with a function-preserving rewrite by s = 2^e in every FFT block of the decoder and the encoder, the
 *                   parity bounds (MAE < 1e-4 pA, max < 2e-3 pA, within 5 x the fp32 oracle's distance to fp64, dwell indices
 *                   exact) hold for
 *                     pos_ffn.w_1 x s, w_2 / s      e = -3 ... +2   (decoder alone -4 ... +3, encoder alone -4 ... +2)
 *                     slf_attn.w_vs x s, fc / s     e = -3 ... +2   (decoder alone -4 ... +2, encoder alone -3 ... +4)
 *                     slf_attn.w_qs x s, w_ks / s   e = -4 ... +6   (decoder alone -4 ... +4, encoder alone -6 ... +4)
 *                   Outside, the error grows by about 2 x per binade (MAE 4e-4 ... 1e-3 pA at e = +-6, 3e-3 ... 8e-3 pA at
 *                   e = +-10) while the signal stays finite and the dwell indices exact.  Range: a value of magnitude >= 65,504
 *                   in the FFN hidden activation, V, the attention output, Q or K (or in a weight) becomes inf in its hi half and
 *                   NaN in the product; the ReLU turns that into 0 and the zero-strip removes the sample, so the read gets
 *                   shorter without an error -- such a checkpoint is outside the mode's range; use S2S_MODE_F32. */
#define S2S_MODE_F32 0
#define S2S_MODE_F16X3 1
/* (value 2 is retired: a 32x32x16-tiled variant of F16X3 that never beat it) */
#define S2S_MODE_F16 3      /* REDUCED PRECISION, outside the 1e-4 pA bound: decoder operands rounded to f16 once (the
                             * precision class of the reference's own fp16-autocast GPU path, inference.py:404), one MFMA
                             * product per product; the frontend stays F16X3, so dwell indices remain bit-exact */
/*   S2S_MODE_GENERIC  any model size within the limits below, exact fp32 (the parity contract of S2S_MODE_F32): a layer-wise
 *                   pipeline of its own kernels (csrc/s2s_generic.h) over slices of the launch's chunks, the f32-input MFMA for every
 *                   matrix product, an exact softmax with its own row maximum.  Same Philox counters as the tuned instances. */
#define S2S_MODE_GENERIC 4
/*   S2S_MODE_GENERIC_F16  REDUCED PRECISION, outside the 1e-4 pA bound, opt-in (never chosen by default): every size
 *                   S2S_MODE_GENERIC accepts, at the precision class of the reference's 16-mixed GPU path (inference.py:403-404).
 *                   Embedding, pre-net, encoder FFT blocks, the noise and duration heads, dwell and the length regulator are
 *                   S2S_MODE_GENERIC's exact fp32 code (emb_out, enc_out, sigma, conc, rate, g and the dwell indices are bit-equal to
 *                   it); in the decoder FFT blocks every matrix product (QKV, fc, w_1, w_2, Q.K^T, P.V) takes its operands rounded to
 *                   f16 once and accumulates in fp32 (v_mfma_f32_16x16x32_f16, csrc/s2s_generic_h.h), with fp32 bias, ReLU, residual
 *                   and LayerNorm, an fp32 softmax with its exact row maximum, P rounded to f16 after the normalisation;
 *                   out_linear, scale, noise and clamp stay fp32.  Range: a decoder activation or weight of magnitude >= 65,504
 *                   becomes inf in f16 -- the limit of the reference's own 16-mixed run. */
#define S2S_MODE_GENERIC_F16 5
/*   S2S_MODE_GENERIC_GEOMETRY  S2S_MODE_GENERIC (every size it accepts, exact fp32, the same parity bound) with the chunk geometry
 *                   a property of the handle: max_dna_len 1..S2S_GEOMETRY_MAX_DNA_LEN k-mers in and max_signal_len
 *                   1..S2S_GEOMETRY_MAX_SIGNAL_LEN samples out per chunk, the checkpoint's own.  At 16 / 250 it runs
 *                   S2S_MODE_GENERIC's kernels on S2S_MODE_GENERIC's numbers; beyond 256 samples the decoder attention is an
 *                   MFMA kernel of its own (csrc/s2s_generic.h, gen_attention_long_kernel).  Every [16] and [250] of this header
 *                   reads as [max_dna_len] and [max_signal_len] for such a handle.  Its reduced-precision counterpart is
 *                   S2S_MODE_GENERIC_GEOMETRY_F16. */
#define S2S_MODE_GENERIC_GEOMETRY 6
/*   S2S_MODE_GENERIC_GEOMETRY_F16  REDUCED PRECISION, outside the 1e-4 pA bound, opt-in (never chosen by default):
 *                   S2S_MODE_GENERIC_GEOMETRY's sizes and chunk geometries (max_dna_len 1..S2S_GEOMETRY_MAX_DNA_LEN,
 *                   max_signal_len 1..S2S_GEOMETRY_MAX_SIGNAL_LEN, the checkpoint's own) at S2S_MODE_GENERIC_F16's precision class,
 *                   the reference's 16-mixed GPU path (inference.py:403-404).  The encoder side is S2S_MODE_GENERIC_GEOMETRY's exact
 *                   fp32 code (emb_out, enc_out, sigma, conc, rate, g and the dwell indices are bit-equal to it); in the decoder
 *                   FFT blocks every matrix product takes its operands rounded to f16 once and accumulates in fp32
 *                   (v_mfma_f32_16x16x32_f16), with fp32 bias, ReLU, residual, LayerNorm and softmax (exact row maximum).  Up to
 *                   256 samples the decoder attention is S2S_MODE_GENERIC_F16's kernel; beyond, gen_attention_long_h_kernel
 *                   (csrc/s2s_generic_h.h) rounds the unnormalised P = exp(s - max) to f16 and divides O by the fp32 row sum.
 *                   At 16 / 250 it computes S2S_MODE_GENERIC_F16's numbers bit for bit.  Range: a decoder activation or weight
 *                   of magnitude >= 65,504 becomes inf in f16 -- the limit of the reference's own 16-mixed run. */
#define S2S_MODE_GENERIC_GEOMETRY_F16 7
#define S2S_GEOMETRY_MAX_DNA_LEN 64
#define S2S_GEOMETRY_MAX_SIGNAL_LEN 1024

#define S2S_T_ENC 16         /* config.yaml:18 max_dna_len    */
#define S2S_T_DEC 250        /* config.yaml:19 max_signal_len */
#define S2S_DMODEL 64        /* config.yaml:25 dmodel         */
#define S2S_DFF 256          /* config.yaml:26 dff            */
#define S2S_HEADS 8          /* config.yaml:28,30             */

/* Model hyper-parameters that change the predict arithmetic (config.yaml:17-31; the keys
 * Encoder/Decoder.__init__ read, modules.py:22-63, 97-131).  Every mode but S2S_MODE_GENERIC_GEOMETRY and
 * S2S_MODE_GENERIC_GEOMETRY_F16: 16 k-mers in, 250 samples out (the chunk geometry of the export kernels and the host framing);
 * those two: max_dna_len 1..64, max_signal_len 1..1024.  Every mode: seq_kmer 1..16, encoder and decoder layers 1..4,
 * pre_layers 0..4.  Sizes:
 *   tuned modes (F32, F16X3, F16): the shipped architecture family only -- dmodel 64, dff 256,
 *                   8 heads in encoder and decoder;
 *   S2S_MODE_GENERIC, S2S_MODE_GENERIC_F16, S2S_MODE_GENERIC_GEOMETRY and S2S_MODE_GENERIC_GEOMETRY_F16: dmodel a multiple of 16
 *                   in 16..512, dff a multiple of 8 in 8..2048, encoder and decoder heads each 1..16 and a divisor of dmodel
 *                   (head_dim = dmodel / heads).
 * A refused configuration is S2S_ERR_ARG from s2s_create (the message names the key) and
 * s2s_blob_floats returns 0 for it. */
typedef struct s2s_config {
    int32_t seq_kmer;          /* 9 (dna-r10*, rna-004*) or 6 (dna-r9*), utils.py:257-260 */
    int32_t max_dna_len;       /* must be 16;  S2S_MODE_GENERIC_GEOMETRY(_F16): 1..64   */
    int32_t max_signal_len;    /* must be 250; S2S_MODE_GENERIC_GEOMETRY(_F16): 1..1024 */
    int32_t dmodel;            /* tuned: 64;  generic: 16..512, a multiple of 16 */
    int32_t dff;               /* tuned: 256; generic: 8..2048, a multiple of 8 */
    int32_t n_heads;           /* encoder heads; tuned: 8; generic: 1..16, divides dmodel */
    int32_t encoder_layers;    /* 1..4 */
    int32_t decoder_layers;    /* 1..4 */
    int32_t pre_layers;        /* 0..4 */
    float scaling_max_value;   /* 165.0, model.py:221 */
    int32_t compute_mode;      /* arithmetic of the decoder FFT blocks: one of the S2S_MODE_* values */
    int32_t decoder_heads;     /* 0 = n_heads; tuned: 0 or n_heads; generic: 1..16, divides dmodel */
} s2s_config;

/* Per-call scalars: the attributes predict_step reads from the LightningModule
 * (model.py:55-63, 207-240). */
typedef struct s2s_params {
    float dwell_mean;          /* used when duration_sampling == 0 (modules.py:420-432) */
    float dwell_std;           /* > 0: dwell ~ N(dwell_mean, dwell_std), clamp(min_duration) */
    float noise_std;           /* <= 0: no noise (model.py:224) */
    float min_noise;           /* clamp of the predicted sigma (model.py:228) */
    float min_duration;        /* clamp of the dwell (modules.py:414-416, 430-432) */
    int32_t noise_sampling;    /* 1: per-sample sigma from the NoiseSampler (model.py:227-234) */
    int32_t duration_sampling; /* 1: Gamma(conc, rate) dwell from the DurationSampler (modules.py:410-416) */
    uint64_t seed;             /* key of the counter-based Philox4x32-10 generator */
} s2s_params;

/* Optional stage outputs for parity tests (all nullable, device).  [64] below is [dmodel] for a generic handle; [16] and [250]
 * are [max_dna_len] and [max_signal_len] for a S2S_MODE_GENERIC_GEOMETRY or S2S_MODE_GENERIC_GEOMETRY_F16 handle. */
typedef struct s2s_debug {
    float* emb_out;            /* [B][16][64]  Encoder.forward 2nd result (modules.py:72-77) */
    float* enc_out;            /* [B][16][64]  Encoder.forward 1st result (modules.py:80-89) */
    float* sigma;              /* [B][16]      NoiseSampler.forward (modules.py:275-278) */
    float* conc;               /* [B][16]      DurationSampler conc, clamped (modules.py:215-216) */
    float* rate;               /* [B][16]      DurationSampler rate, clamped (modules.py:217-218) */
    float* g;                  /* [B][16]      the dwell value before round() (modules.py:414-416/420-432) */
    float* y_scaled;           /* [B][250]     Decoder.forward output (modules.py:140-141) */
    float* z01;                /* [B][250]     the standard normals used for the noise term */
    /* stage INPUTS (nullable): with these the launch serves as a stand-alone sub-module operator, the reference's
     * NoiseSampler(x) / DurationSampler(x) on any emb_out and Decoder(x) on any [B,250,64] tensor (modules.py:275-278, 197-225, 133-142) */
    const float* emb_in;       /* [B][16][64]  replaces the pre-net output: heads, dwell and encoder blocks run on it */
    const float* dec_in;       /* [B][250][64] replaces the length-regulated + position-encoded decoder input */
} s2s_debug;

typedef struct s2s_handle s2s_handle;

/* Number of fp32 values the weight blob must hold for `cfg` (0 for a refused configuration), and the order, written for the
 * tuned sizes -- for S2S_MODE_GENERIC, S2S_MODE_GENERIC_F16, S2S_MODE_GENERIC_GEOMETRY and S2S_MODE_GENERIC_GEOMETRY_F16 (the
 * same blob) read every 64 as dmodel and every 256 as dff, and for the two geometry modes 16 as max_dna_len and 250 as
 * max_signal_len in the position tables:
 *   encoders.position_enc[16*64]; src_emb.weight[64][5k], .bias[64];
 *   pre_net_stack.i.weight[64][64], .bias[64]                               (i < pre_layers)
 *   per encoder layer: LAYER (below)
 *   noise_sampler.stdv_layer: 0.weight[64][64], 0.bias[64], 3.weight[64], 3.bias[1]
 *   duration_sampler.conc_layer: same four; duration_sampler.rate_layer: same four
 *   decoders.position_enc[250*64]; per decoder layer: LAYER;
 *   decoders.out_linear.weight[64], .bias[1]
 * LAYER = slf_attn.{w_qs,w_ks,w_vs}.{weight[64][64],bias[64]}, slf_attn.fc.{weight,bias},
 *         slf_attn.layer_norm.{weight,bias}[64], pos_ffn.w_1.{weight[256][64],bias[256]},
 *         pos_ffn.w_2.{weight[64][256],bias[64]}, pos_ffn.layer_norm.{weight,bias}[64]
 * i.e. the reference state_dict (SURVEY.md section 8 a-W) in its native [out][in] layouts.
 *
 * A generic handle runs a launch in slices of at most S2S_GENERIC_WORKSPACE_BYTES / (4 * per-chunk floats) chunks, per-chunk
 * floats = te dmodel + ts dmodel + max(te, ts) max(3 dmodel, dff) + te + ts, te / ts = max_dna_len / max_signal_len (16 / 250
 * outside the two geometry modes; each buffer is then rounded up to a multiple of
 * 64 floats), and of at most (2^32 - 1) / (max(n_heads, decoder_heads) * threads per (chunk, head)) chunks, threads = 1024
 * up to 256 samples and 256 * ceil(max_signal_len / 64) beyond: an attention launch holds fewer than 2^32 threads (this binds at
 * tiny geometries only); the workspace grows on demand (the first launch of a larger batch synchronises the stream) and is reused. */
#define S2S_GENERIC_WORKSPACE_BYTES (512u << 20)
size_t s2s_blob_floats(const s2s_config* cfg);

/* Replaces seq2squiggle.load_from_checkpoint + .to(device) (inference.py:386-399): takes the
 * host fp32 blob, re-packs it into MFMA fragment order and uploads it to `device`. */
int s2s_create(const s2s_config* cfg, const void* weights_blob, size_t blob_bytes, int device,
               s2s_handle** out);
void s2s_destroy(s2s_handle* h);

/* Last error of this handle (or of the last failed s2s_create when h == NULL, thread-local). */
const char* s2s_last_error(const s2s_handle* h);

/* Replaces seq2squiggle.predict_step up to the clamp (model.py:195-240) for B chunks.
 *
 *  bases    device [B][16+k-1] ASCII: chunk c of a read is read[16c : 16c+15+k]
 *           (split_sequence, utils.py:350-356); bytes past the read's end are ignored;
 *  n_valid  device [B], 1..16: k-mers j >= n_valid are the all-"_" pad k-mer
 *           (add_remainder, utils.py:342-347), not a shifted window;
 *  first_global_chunk  index of chunk 0 in the whole job: the RNG counter is
 *           (first_global_chunk + b, position, draw kind), so results do not depend on batch
 *           size or on how chunks are sharded over GPUs.  Word for word, in every compute mode and chunk geometry: the
 *           Philox4x32-10 counter is {chunk low word, chunk high word, position | kind << 16, draw index} with chunk =
 *           first_global_chunk + b as an unsigned 64-bit number, the key {seed low word, seed high word}.  position is the
 *           k-mer c (kinds 1 and 2) or the sample t (kind 3) inside the chunk; kind is 1 for the Gamma dwell, 2 for the dwell
 *           normal, 3 for the noise normal; the draw index is 0 except in the Gamma sampler, which counts its draws from 0
 *           (the alpha < 1 boost first, then one per trip of the rejection loop).  A normal of output words {x, y, ..} is
 *           sqrt(-2 ln u1) * cos(2 pi u2), u1 = ((x >> 8) + 1) * 2^-24, u2 = (y >> 8) * 2^-24;
 *  inject_g   nullable device [B][16]: value of Gamma.sample() (modules.py:221-222) to use
 *             instead of the built-in sampler (duration_sampling only);
 *  inject_zdw nullable device [B][16]: standard normals for the dwell_std > 0 mode;
 *  inject_z01 nullable device [B][250]: standard normals for the noise term;
 *  out_signal device [B][250] fp32 pA (rows of `prediction`, model.py:240);
 *  out_dur    device [B][16] int32 rounded dwell (modules.py:437-438);
 *  dbg        nullable.
 */
int s2s_predict_chunks(s2s_handle* h, void* stream, const uint8_t* bases, const uint8_t* n_valid,
                       int64_t first_global_chunk, int32_t B, const s2s_params* params,
                       const float* inject_g, const float* inject_zdw, const float* inject_z01,
                       float* out_signal, int32_t* out_dur, const s2s_debug* dbg);

/* Same as s2s_predict_chunks without materialising the chunk windows: `read_bytes` (device) holds whole reads back
 * to back, each padded with '_' to 16*C + k - 1 bytes (C = its chunk count); chunk b is the 16+k-1 bytes at
 * read_bytes + chunk_start[b] (device int64 [B]).  This is what process_read/split_sequence (dataloader.py:358-398,
 * utils.py:350-356) produce, minus the one-hot: adjacent chunks of a read overlap by k-1 bytes in place. */
int s2s_predict_packed(s2s_handle* h, void* stream, const uint8_t* read_bytes, const int64_t* chunk_start,
                       const uint8_t* n_valid, int64_t first_global_chunk, int32_t B, const s2s_params* params,
                       float* out_signal, int32_t* out_dur);

/* Replaces the first (teacher-forced) pass of seq2squiggle.validation_step + get_loss (model.py:107-143, 419-480) for B
 * chunks: encoder, noise and duration heads, the length regulator on the MEASURED dwell of every k-mer (LR(x, ..., target),
 * modules.py:434-435), decoder, and the three per-chunk loss sums.  Every compute mode, at the handle's te / ts (16 / 250, the
 * checkpoint's max_dna_len / max_signal_len in the two geometry modes); the same model arithmetic as s2s_predict_chunks in that mode.
 *  kmers    device [B][te][k]: the letters of each k-mer ('_','A','C','G','T'; any other byte = an all-zero one-hot row,
 *           utils.py:86); k-mers are independent (no window overlap assumed) and every position counts (pads are explicit
 *           "_"*k k-mers);
 *  dwell    device [B][te] int32 >= 0: the measured samples per k-mer (chunks_lengths), used as they are (0 = k-mer skipped,
 *           the cumulative sum cropped at ts);
 *  target   device [B][ts] fp32, already divided by scaling_max_value; stdev device [B][te] fp32, likewise;
 *  out_loss device [B][3] fp32 per chunk: sum over ts of (y - target)^2; sum over te of -Gamma(conc, rate).log_prob(max(dwell, 1))
 *           (unscaled: get_loss's 0.0005 is the caller's); sum over te of (stdev - sigma)^2.  conc and rate are clamped at 1e-8
 *           (modules.py:215-218), sigma enters unclamped (min_noise plays no part);
 *  out_y    nullable device [B][ts]: the decoder output y (scaled units, modules.py:140-141: no scale, noise or clamp);
 *  dbg      nullable: sigma, conc, rate ([B][te]) as for s2s_predict_chunks; a call that sets any other field is refused.
 * Deterministic: a chunk's sums are formed in a fixed order from its own rows only, so they do not depend on B, on how the
 * chunks are sliced or on their neighbours (no float atomics). */
int s2s_evaluate_chunks(s2s_handle* h, void* stream, const uint8_t* kmers, const int32_t* dwell, const float* target,
                        const float* stdev, int32_t B, float* out_loss, float* out_y, const s2s_debug* dbg);

/* Replaces the per-read cat + zero-strip of export_and_clear_results (model.py:284-286) and the
 * pA -> int16 conversion of BLOW5Writer/POD5Writer.save (signal_io.py:134-141, 246-253).
 *
 *  signal       device [B][250] (output of s2s_predict_chunks), chunks of a read contiguous;
 *  read_first   device [R+1]: read r owns chunks read_first[r] .. read_first[r+1]-1;
 *  out_offsets  device [R+1] int64: on return out_offsets[r] is the start of read r in the
 *               packed output, out_offsets[R] the total sample count;
 *  out_pa       nullable device fp32 [capacity]: packed non-zero samples (the tensors handed to
 *               writer.signals, model.py:290);
 *  out_dac      nullable device int16 [capacity]: round_half_even(pa*digitisation/range - offset)
 *               wrapped to int16; reversed per read when rna != 0 (signal_io.py:140-141);
 *  capacity     size of out_pa/out_dac in samples (B*250 always suffices).  A capacity below the sample count truncates and
 *               never writes out of bounds: out_offsets is complete whatever the capacity (out_offsets[R] > capacity tells the
 *               caller), and in each of out_pa / out_dac exactly the elements whose own index is below capacity are written,
 *               with the value a call with enough capacity puts there -- for rna != 0 too, where the element at an index is
 *               not the sample that was found at it.  Nothing else is touched.
 * Only out_dac is reversed when rna != 0; out_pa keeps the order of the signal.  Reads may be empty (read_first[r] ==
 * read_first[r+1]); read_first[0] == 0, read_first[R] == B, non-decreasing.  B == 0 writes R+1 zero offsets.
 * Rows are 250 samples, max_signal_len for a S2S_MODE_GENERIC_GEOMETRY(_F16) handle.
 */
int s2s_export_reads(s2s_handle* h, void* stream, const float* signal, int32_t B,
                     const int32_t* read_first, int32_t R, int64_t* out_offsets, float* out_pa,
                     int16_t* out_dac, int64_t capacity, float digitisation, float range,
                     float offset_mean, int32_t rna);

/* The ground-truth base-to-signal map of a batch: how many STORED samples (the ones s2s_export_reads keeps) every k-mer of every
 * chunk owns.  The reference has no counterpart (it writes the signal only); the definitions are the length regulator's
 * (DESIGN.md section 4).  With te / ts = max_dna_len / max_signal_len of the handle (16 / 250 outside the two geometry modes):
 *
 *  signal   device [B][ts], dur device [B][te]: out_signal / out_dur of s2s_predict_chunks / s2s_predict_packed;
 *  c[j]     = min(ts, sum_{i<=j} max(dur[b][i], 0)), c[-1] = 0 -- saturating: no int32 dwell, however large, wraps the sum;
 *  out_seg  device uint16 [B][te+1]: out_seg[b][j] = #{t in [c[j-1], c[j]) : signal[b][t] != 0.0f} for j < te (the rows the
 *           regulator gathers from k-mer j), out_seg[b][te] the same count over the tail [c[te-1], ts) (rows past the last dwell:
 *           the decoder runs unmasked, so they can be non-zero and survive the strip).
 * A row sums to the chunk's count of stored samples; counts are exact integers that depend on the chunk's own rows only (not on
 * B or its neighbours).  B == 0 is a successful no-op; a NULL pointer or B < 0 is S2S_ERR_ARG. */
int s2s_align_chunks(s2s_handle* h, void* stream, const float* signal /* device [B][ts] */, const int32_t* dur /* device [B][te] */,
                     int32_t B, uint16_t* out_seg /* device [B][te+1] */);

/* The level statistics of every k-mer's STORED samples: what s2s_align_chunks counts, summed.  No counterpart in the reference.
 *
 *  signal, dur, B, te / ts   as for s2s_align_chunks;
 *  digitisation, range, offset   the calibration s2s_export_reads is given (offset_mean there);
 *  q(t)       for a stored sample t (signal[b][t] != 0.0f) the int16 s2s_export_reads stores for it: the same float32 expression,
 *             round-half-even and int16 wrap (one device function serves both kernels);
 *  out_seg    device uint16 [B][te+1]: by definition what s2s_align_chunks writes (same c[j], saturation and tail slot te);
 *  out_sum    device int32 [B][te+1]: the sum of q(t) over the stored samples of slot j;
 *  out_sumsq  device int64 [B][te+1]: the sum of q(t)^2 over the same samples.
 * Integers only: |sum| <= 1024 * 32768 = 2^25 and sumsq <= 2^40, so both are exact for every input and depend neither on the
 * order of summation nor on B or a chunk's neighbours.  B == 0 is a successful no-op; a NULL pointer, B < 0, range == 0 or
 * digitisation == 0 is S2S_ERR_ARG. */
int s2s_event_stats(s2s_handle* h, void* stream, const float* signal /* device [B][ts] */, const int32_t* dur /* device [B][te] */,
                    int32_t B, float digitisation, float range, float offset, uint16_t* out_seg /* device [B][te+1] */,
                    int32_t* out_sum /* device [B][te+1] */, int64_t* out_sumsq /* device [B][te+1] */);

/* The k-mer table of a run (`predict --kmer-table`): the slot statistics of s2s_event_stats, summed per k-mer over every chunk
 * handed to it.  No counterpart in the reference.
 *
 *  k          the handle's seq_kmer, 1..S2S_KMER_TABLE_MAX_K (above: S2S_ERR_ARG, s2s_last_error names the limit); te / ts the
 *             handle's geometry, as for s2s_event_stats;
 *  signal, dur, digitisation, range, offset   as for s2s_event_stats;
 *  read_bytes, chunk_start, n_valid   those of s2s_predict_packed: chunk b's k-mer j is the k bytes at
 *             read_bytes[chunk_start[b] + j ..], real for j < n_valid[b];
 *  n, S, Q    slot j's count, sum and sum of squares of the stored int16 samples: by definition what s2s_event_stats writes to
 *             out_seg / out_sum / out_sumsq for the same inputs (same c[j], saturation and s2s_dac_of; one wave routine serves both);
 *  code       the base-4 number of the k letters, A, C, G, T = 0..3, the FIRST letter most significant -- the row order of a
 *             published k-mer model; a k-mer with any other byte (genome mode maps non-ACGT to N) has code 4^k, the extra row;
 *  table      device int64 [4^k + 1][S2S_KMER_TABLE_FIELDS], zeroed by the caller once, ADDED to by every call.  Every real slot
 *             (j < n_valid[b]) adds to row `code`:
 *                 [0] occ += 1
 *             and, if n >= 1,
 *                 [1] events += 1   [2] samples += n   [3] samples_sq += n*n   [4] sum += S   [5] sumsq += Q
 *             The tail slot te and pad k-mers (j >= n_valid[b]) add nothing.
 * All fields are 64-bit integers added with integer atomics (never float atomics): the table depends only on the SET of chunks, not
 * on B, slicing, call order, neighbours or the number of GPUs whose tables are summed.  Ranges: per slot n <= 1024, |S| <= 2^25,
 * Q <= 2^40; occ, events, samples and samples_sq are far from 2^63 for any run; |sum| <= 2^15 * samples; sumsq <= 2^30 * samples
 * stays exact up to 2^33 full-scale samples per k-mer.  Beyond that the fields wrap; there is no check.
 * Two paths, chosen by k alone: k <= 5 -- the table (at most 1,025 rows, 49,200 bytes) is kept per workgroup in LDS, at most 512
 * workgroups walk the chunks and each adds its non-zero words to `table` once at the end; k >= 6 -- one workgroup per four chunks
 * adds straight to `table`.  On both a wave first merges the slots of its chunk that share a row.
 * B == 0 is a successful no-op; a NULL pointer, B < 0, range == 0 or digitisation == 0 is S2S_ERR_ARG. */
#define S2S_KMER_TABLE_MAX_K   10
#define S2S_KMER_TABLE_FIELDS  6
int64_t s2s_kmer_table_rows(int32_t k);          /* 4^k + 1 for 1 <= k <= S2S_KMER_TABLE_MAX_K, else -1 */
int s2s_kmer_table_accumulate(s2s_handle* h, void* stream, const float* signal /* device [B][ts] */,
                              const int32_t* dur /* device [B][te] */, const uint8_t* read_bytes, const int64_t* chunk_start /* device [B] */,
                              const uint8_t* n_valid /* device [B] */, int32_t B, float digitisation, float range, float offset,
                              int64_t* table /* device [4^k + 1][6] */);

/* The k-mer model of a run (`predict --kmer-model`): the statistics of event MEANS per k-mer -- what the `level_mean level_stdv
 * sd_mean sd_stdv` columns of a nanopolish-style model file hold -- summed over every chunk handed to it.  No counterpart in the
 * reference.  The k-mer table above pools SAMPLES; here every EVENT counts once.
 *
 * The fixed-point statistics of one event (s2s_event_fixed: no handle, no GPU; the kernel calls the same inline function).  For a
 * slot with 1 <= n <= 1024 stored samples, S and Q the n / S / Q of s2s_event_stats, in 64-bit integers only:
 *   M   the event mean in units of 2^-8 ADC counts: round-half-even of 256*S / n.  num = 256*S; q = floor_div(num, n);
 *       r = num - q*n (0 <= r < n); q += 1 if 2r > n, or if 2r == n and q is odd.  |M| <= 2^23.
 *   D   the event's population deviation in the same units: floor(sqrt(x)), x = floor(V * 2^16 / n^2), V = n*Q - S*S (>= 0,
 *       <= 2^50; a negative V, which no samples give, counts as 0), x formed as (a << 16) + ((b << 16) / n^2) with a = V / n^2,
 *       b = V % n^2 (b << 16 < 2^36, x <= 2^46); D from a double sqrt, corrected by integer comparison until
 *       D*D <= x < (D+1)*(D+1).  D <= 2^23.
 * s2s_event_fixed returns S2S_ERR_ARG for n < 1, n > 1024 or a NULL pointer.
 *
 * s2s_kmer_model_accumulate takes the arguments of s2s_kmer_table_accumulate (same k, code, extra row 4^k, slot statistics and
 * errors), except
 *  table      device int64 [4^k + 1][S2S_KMER_MODEL_FIELDS], zeroed by the caller once, ADDED to by every call.  Every real slot
 *             (j < n_valid[b]) with n >= 1 adds to row `code`:
 *                 [0] events += 1   [1] sum_m += M   [2] sum_m2 += M*M   [3] sum_d += D   [4] sum_d2 += D*D
 *             Slots without samples, pad slots and the tail add nothing.
 * All adds are 64-bit integer adds: the table depends only on the SET of chunks.  Ranges: M*M, D*D <= 2^46, exact up to 2^17
 * full-scale events per k-mer; beyond that the fields wrap; there is no check.
 * One path for every k.  At most S2S_KMER_MODEL_MAX_WORKGROUPS persistent workgroups of four waves walk the chunks, four per
 * round.  A wave merges the slots of its chunk that share a row; the first lane of every code then adds its five fields into the
 * workgroup's write-combining cache in LDS: S2S_KMER_MODEL_SLOTS slots of a key and five counters.  Slot of a code: the code
 * itself for k <= S2S_KMER_MODEL_DIRECT_MAX_K (4^k + 1 <= the slot count), otherwise
 *                 (uint64)(uint32)(code * S2S_KMER_MODEL_HASH_MUL) * S2S_KMER_MODEL_SLOTS >> 32
 * and on a slot held by another code the next one (cyclically), S2S_KMER_MODEL_PROBES slots in all; a code that finds no place
 * adds straight to `table`.  The cache is added to `table` and cleared every S2S_KMER_MODEL_FLUSH_ROUNDS rounds and at the end
 * of the walk: at the model's 16 k-mers per chunk that is at most 512 insertions into 1,025 slots between two flushes. */
#define S2S_KMER_MODEL_FIELDS          5
#define S2S_KMER_MODEL_SLOTS           1025
#define S2S_KMER_MODEL_DIRECT_MAX_K    5
#define S2S_KMER_MODEL_PROBES          4
#define S2S_KMER_MODEL_HASH_MUL        2654435761u
#define S2S_KMER_MODEL_FLUSH_ROUNDS    8
#define S2S_KMER_MODEL_MAX_WORKGROUPS  768
int s2s_event_fixed(int32_t n, int32_t S, int64_t Q, int64_t* M, int64_t* D);
int s2s_kmer_model_accumulate(s2s_handle* h, void* stream, const float* signal /* device [B][ts] */,
                              const int32_t* dur /* device [B][te] */, const uint8_t* read_bytes, const int64_t* chunk_start /* device [B] */,
                              const uint8_t* n_valid /* device [B] */, int32_t B, float digitisation, float range, float offset,
                              int64_t* table /* device [4^k + 1][5] */);

/* The pore model from ALIGNMENTS (`resquiggle --kmer-model-out`, `eventalign --kmer-model-out`): the same table, summed over the
 * k-mer slots of stored records that an alignment cut, each record with its own calibration.  No handle; the conventions of the
 * other handle-free entries (device and stream first, stream-ordered, device pointers; the host twin is the definition the kernel
 * equals bit for bit).  No counterpart in the reference; unvalidated against nanopolish / f5c / uncalled4.
 *
 *  l_offs     [P + 1]: record p owns the pooled slots l_offs[p] .. l_offs[p + 1] - 1 -- the layout s2s_event_sums writes;
 *  codes, ev_len, S, Q   per pooled slot: the row of the slot's k-mer (the `code` above; 4^k is the pooled row of k-mers with a
 *             letter outside ACGT, which s2s_kmer_model_format never prints), the samples of its event and their sum and sum of
 *             squares (s2s_event_sums);
 *  gain, shift   [P], formed by the caller in double from the record's (digitisation, offset, range):
 *                 gain = rint(range / digitisation * 2^24), 1 .. 2^30       shift = rint(offset * 256), |shift| <= 2^30
 *             gain == 0: the record contributes nothing, neither to the table nor to `dropped` (what the caller passes for a
 *             record whose calibration is outside these ranges).
 * A slot (n = ev_len, S, Q, c = code) of a record with gain != 0, in integers only:
 *   1. n < 1: no event; nothing is added.
 *   2. n > 1024: a stalled k-mer, for which s2s_event_fixed is not defined and which a model does not want: OVERLONG, nothing added.
 *   3. c < 0 or c > 4^k: BAD_CODE, nothing added (no write ever lands outside the table).
 *   4. (M, D) = s2s_event_fixed(n, (int32)S, Q), in 2^-8 ADC counts, become 2^-8 pA:
 *        Mp = round-half-even((M + shift) * gain / 2^24): num = (M + shift) * gain; q = floor_div(num, 2^24); r = num - q * 2^24;
 *             q += 1 if 2r > 2^24, or if 2r == 2^24 and q is odd;
 *        Dp = floor(D * gain / 2^24).
 *      |Mp| > 2^23 or Dp > 2^23: OUT_OF_RANGE, nothing added -- the squares stay <= 2^46, the exactness statement above.
 *   5. Otherwise row c gets  [0] events += 1  [1] sum_m += Mp  [2] sum_m2 += Mp*Mp  [3] sum_d += Dp  [4] sum_d2 += Dp*Dp: COUNTED.
 *  table      int64 [4^k + 1][S2S_KMER_MODEL_FIELDS], ADDED to: s2s_kmer_model_format(table, k, 1.0f, 1.0f, 0.0f, ...) prints pA.
 *             With gain = 2^24 and shift = 0, Mp = M and Dp = D: on the same events the table of s2s_kmer_model_accumulate.
 *  dropped    int64 [4], ADDED to: {overlong, out_of_range, bad_code, counted}.
 *  workgroups 0: the library's choice; 1 .. S2S_KMER_MODEL_MAX_WORKGROUPS: exactly that many persistent workgroups (a test crosses
 *             the flush interval and the probe overflow with a few thousand slots this way).  The table does not depend on it.
 * All adds are 64-bit integer adds: table and dropped depend only on the SET of slots, not on batching, the grid, or which of the
 * GPU and the host ran.
 * Persistent workgroups of 256 threads walk the POOLED slots, 64 consecutive ones per wave and round, whatever the reads' lengths; a
 * lane finds its record by a search in l_offs (a slot that no record holds adds nothing), lanes of a wave with equal codes are
 * merged, and the first lane of a code adds into the workgroup's write-combining cache -- the cache, constants and rules of
 * s2s_kmer_model_accumulate, flushed every S2S_KMER_MODEL_FLUSH_ROUNDS rounds and at the end.  The four counts are summed per wave:
 * one atomic per wave and non-zero count.  Static LDS: the cache's 45,100 B, nothing else.  The slot count l_offs[P] is on the
 * device: with workgroups == 0 the entry launches S2S_KMER_MODEL_MAX_WORKGROUPS and those without a round leave at once.
 * S2S_ERR_ARG: k outside 1..10, P < 0, a NULL pointer with P > 0, workgroups outside 0..S2S_KMER_MODEL_MAX_WORKGROUPS; on the host
 * twin offsets that decrease or begin below 0, or threads < 1.  P == 0 is a successful no-op that launches nothing; so is, on the
 * host, a call without slots.  The host twin runs on one thread whatever `threads` says. */
int s2s_kmer_model_events(int device, void* stream, const int32_t* codes, const int32_t* ev_len, const int64_t* S, const int64_t* Q,
                          const int64_t* l_offs /* [P + 1] */, int32_t P, const int64_t* gain, const int64_t* shift /* [P] */,
                          int32_t k, int32_t workgroups, int64_t* table /* [4^k + 1][5], ADDED to */, int64_t* dropped /* [4], ADDED to */);
int s2s_kmer_model_events_host(const int32_t* codes, const int32_t* ev_len, const int64_t* S, const int64_t* Q, const int64_t* l_offs,
                               int32_t P, const int64_t* gain, const int64_t* shift, int32_t k, int64_t* table, int64_t* dropped,
                               int32_t threads);

/* Replaces the signal compression that pyslow5.write_record_batch (svb-zd) and pod5.Writer.add_reads (the svb16 stage of
 * VBZ) run on the host (reference signal_io.py:167-171, 268-282): StreamVByte encoding of the zig-zag deltas of the packed
 * int16 samples, one output blob per row, so that only ~1.1 bytes per sample cross PCIe.
 *
 *  samples       device int16: out_dac of s2s_export_reads;
 *  read_offsets  device [R+1]: out_offsets of s2s_export_reads;
 *  row_read, row_index  device [N]: row i covers samples [row_index[i]*row_samples, (row_index[i]+1)*row_samples) of read
 *               row_read[i], clipped to the read; a row that starts past the end of its read yields an empty blob (the
 *               caller enumerates candidate rows from the chunk counts without knowing the stripped lengths);
 *  row_samples   samples per row: 102400 for POD5 signal-table rows, any value >= the longest read for whole reads (SLOW5);
 *  variant       32: slow5 svb-zd blob = u32 n, (n+3)/4 control bytes (2 bits per value), data (zig-zag of 32-bit deltas);
 *               16: pod5 svb16 stream = (n+7)/8 control bytes (1 bit per value), data (zig-zag of 16-bit deltas): the
 *               input of the row's zstd frame;
 *  out           device bytes [capacity]; a row of n samples takes at most 4 + ceil(n/4) + 3n bytes (variant 32: a zig-zag
 *               delta of two int16 samples can need 3 bytes) or ceil(n/8) + 2n (variant 16), so capacity >=
 *               4N + 3 total + (total + 3N)/4 (variant 32) or 2 total + total/8 + N (variant 16) always suffices;
 *  out_offsets   device [N+1] int64: blob i = out[out_offsets[i] : out_offsets[i+1]].  If the rows need more than
 *               `capacity` bytes, the rows that do not fit are NOT written and out_offsets[N] comes back NEGATIVE
 *               (minus the bytes needed): the caller must check it before framing the blobs.
 */
int s2s_svb_encode(s2s_handle* h, void* stream, const int16_t* samples, const int64_t* read_offsets,
                   const int32_t* row_read, const int32_t* row_index, int32_t N, int64_t row_samples, int32_t variant,
                   uint8_t* out, int64_t capacity, int64_t* out_offsets);

/* Test hook: raw Philox4x32-10 words, out[i*4..i*4+3] = philox(counter = {c0+i, c1, c2, c3}, key = seed). */
int s2s_philox_u32(s2s_handle* h, void* stream, uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2,
                   uint32_t c3, int32_t n, uint32_t* out /* device [n][4] */);

/* Device time (ms) of the predict kernel (s2s_fused_kernel: frontend + decoder in one launch) over the launches since the last
 * call, measured with HIP events on the launch stream when profiling is enabled. */
int s2s_set_profiling(s2s_handle* h, int32_t enabled);
int s2s_get_kernel_ms(s2s_handle* h, double* kernel_ms_total, int64_t* launches, int64_t* chunks);

/* ---- host-side helper (no GPU work, no handle): frames and compresses one batch of BLOW5 records on `threads` worker
 * threads -- what pyslow5's write_record_batch(threads = cpu_count) does for the reference (signal_io.py:167-171).
 * Record i's body is prefix[prefix_offs[i] : prefix_offs[i+1]] + signal[signal_offs[i] : signal_offs[i+1]] +
 * suffix[suffix_offs[i] : suffix_offs[i+1]] (the fields before and after raw_signal, built by the caller; the signal bytes
 * are little-endian int16 samples or an svb-zd blob); `out` receives, in record order, [u64 compressed size][body compressed
 * with `method`: 0 none, 1 zlib container (RFC 1950; written by libdeflate when that library loads, else zlib), 2 zstd, 3 zlib
 * container written by the library's own Huffman-only deflate encoder (dynamic blocks of literals, no match search; a record is
 * coded in independent pieces of <= 128 KiB on several threads and is still ONE ordinary zlib stream; `level` is ignored)] at
 * `level`.  `capacity` must be at least s2s_blow5_pack_bound(total body bytes, n).  Returns the bytes written, or < 0. */
int64_t s2s_blow5_pack_bound(int64_t body_bytes_total, int32_t n_records);
int64_t s2s_blow5_pack(const uint8_t* prefix, const int64_t* prefix_offs, const uint8_t* suffix, const int64_t* suffix_offs,
                       const uint8_t* signal, const int64_t* signal_offs, int32_t n_records, int32_t method, int32_t level,
                       int32_t threads, uint8_t* out, int64_t capacity);

/* The same worker threads on plain byte rows: row i = in[in_offs[i] : in_offs[i+1]] is compressed on its own (method 1: zlib
 * container, 2: one zstd frame -- the second stage of POD5's VBZ after s2s_svb_encode's svb16 stream, what pod5.Writer.add_reads
 * runs per signal row, reference signal_io.py:268-282) and the results are laid back to back in `out` with their bounds in
 * out_offs [n+1].  capacity >= s2s_blow5_pack_bound(total bytes, n) always suffices.  Returns the bytes written, or < 0. */
int64_t s2s_compress_rows(const uint8_t* in, const int64_t* in_offs, int32_t n_rows, int32_t method, int32_t level,
                          int32_t threads, uint8_t* out, int64_t capacity, int64_t* out_offs);

/* ---- host-side helper (no GPU work, no handle): the base-to-signal alignment of one batch of reads as PAF text, one line per
 * record of the signal file, formatted on `threads` threads of the same worker pool (an interpreter loop cannot keep up with the
 * 46 M k-mers/s of a run).
 *
 *  seg         [B][te+1]: out_seg of s2s_align_chunks, copied to the host;
 *  read_first  [R+1]: read r owns chunks read_first[r] .. read_first[r+1]-1;
 *  read_kmers  [R]: the read's real k-mers K = te * (chunks - 1) + n_valid of its last chunk (the later k-mers of that chunk
 *              are padding: their samples belong to no base);
 *  read_offs   [R+1]: out_offsets of s2s_export_reads -- a read without samples has no record and gets no line;
 *  ids, id_offs [n_ids+1]: the read_id of every record, in record order (n_ids = reads with samples), as one byte blob;
 *  rna         != 0: the stored signal is reversed per read (s2s_export_reads), so the line walks the k-mers from last to first.
 * A line, tab separated: read_id, len_raw_signal, sig_start, sig_end, "+", read_id, K, kmer_start, kmer_end (0, K; K, 0 for
 * RNA), k-mers with samples, K, 255, "ss:Z:" + tokens in stored-signal order from sig_start to sig_end: "N," the next k-mer with
 * its N >= 1 samples, "ND" the next N k-mers without a sample (zero dwell, cropped away, or stripped), "NI" N samples that belong
 * to no k-mer (chunk tails, pad k-mers); adjacent D / I runs are merged; insertions in front of the first and behind the last
 * k-mer are left out of [sig_start, sig_end), k-mers never.
 * Returns the bytes written (lines in read order), or S2S_ERR_ARG -- also when a read's seg rows do not sum to its samples or
 * n_ids is not the number of reads with samples.  capacity >= the bound function's value always suffices. */
int64_t s2s_paf_format_bound(int64_t n_chunks, int32_t te, int32_t n_reads, int64_t id_bytes_total);
int64_t s2s_paf_format(const uint16_t* seg, int32_t te, const int32_t* read_first, const int64_t* read_kmers,
                       const int64_t* read_offs, int32_t R, const uint8_t* ids, const int64_t* id_offs, int32_t n_ids,
                       int32_t rna, int32_t threads, uint8_t* out, int64_t capacity);

/* ---- host-side helper (no GPU work, no handle): the per-k-mer event table of one batch of reads (`predict --events`) as text, on
 * `threads` threads of the same worker pool.  seg, te, read_first, read_kmers, read_offs, R, ids, id_offs, n_ids, rna, threads, out
 * and capacity are those of s2s_paf_format; further:
 *
 *  sum, sumsq   [B][te+1]: out_sum / out_sumsq of s2s_event_stats, copied to the host;
 *  letters, letter_offs [R+1]: the cleaned letters of every read as one byte blob (the bytes s2s_predict_packed reads); read r owns
 *               letters[letter_offs[r] .. letter_offs[r+1]), at least K + k - 1 of them;   k: the k-mer length;
 *  digitisation, range, offset   the record calibration (floats, widened to double);
 *  dac          NULL, or the packed int16 samples of the batch (out_dac of s2s_export_reads: read r at read_offs[r]);
 *  with_header  != 0: the text starts with the header line.
 * Tab separated, "\n" ended; the header is
 *      read_name  position  model_kmer  start_idx  end_idx  event_level_mean  event_stdv  [samples]
 * and there is one row per REAL k-mer (position < K) that owns >= 1 stored sample, reads in order, k-mers in order; a k-mer
 * without samples, pad k-mers and chunk tails get no row.  read_name: the record's id; position: 0-based k-mer index in the read;
 * model_kmer: the k letters at [position, position + k); [start_idx, end_idx): the k-mer's samples in the record's stored signal,
 * by the walk of s2s_paf_format (insertions advance the cursor and get no row; an RNA signal is stored reversed, so k-mer j with
 * forward range [s, e) gets [L - e, L - s) and start_idx falls as position rises).  With n, S, Q the slot's count, sum and sum of
 * squares, in double and in exactly this order:
 *      event_level_mean = ((double)S / n + offset) * range / digitisation
 *      event_stdv       = sqrt((double)max(n*Q - S*S, 0)) / n * range / digitisation      (n*Q - S*S in int64: at most 2^50)
 * both printed "%.4f".  The deviation is the POPULATION deviation (ddof 0), so it is defined -- 0.0000 -- for a one-sample event.
 * The expressions are taken as written: a negative range prints a negative event_stdv.  These are the levels a reader computes from
 * the stored integers with the `digitisation`, `range` and `offset` GIVEN HERE -- the numbers the conversion to int16 ran with.
 * The signal writers store a per-record draw around that offset as the record's own: a reader that uses the record's offset sees
 * every mean of the record shifted by (offset_record - offset) * range / digitisation, and the deviations unchanged.  samples: only
 * with dac (column and header field are absent without it): the event's samples in stored order, each
 * ((double)q + offset) * range / digitisation printed "%.3f", comma separated.
 * Returns the bytes written, or S2S_ERR_ARG -- also when a read's seg rows do not sum to its samples, its letters are too few, or
 * capacity is below what the rows may take (nothing is written then).  capacity >= the bound function's value always suffices:
 * id_len_max the longest record id, n_samples the stored samples of the batch if dac is given, else 0. */
int64_t s2s_events_format_bound(int64_t n_chunks, int32_t te, int64_t id_len_max, int32_t k, float digitisation, float range,
                                float offset, int64_t n_samples, int32_t with_header);
int64_t s2s_events_format(const uint16_t* seg, const int32_t* sum, const int64_t* sumsq, int32_t te, const int32_t* read_first,
                          const int64_t* read_kmers, const int64_t* read_offs, int32_t R, const uint8_t* ids, const int64_t* id_offs,
                          int32_t n_ids, const uint8_t* letters, const int64_t* letter_offs, int32_t k, float digitisation,
                          float range, float offset, const int16_t* dac, int32_t rna, int32_t with_header, int32_t threads,
                          uint8_t* out, int64_t capacity);

/* ---- host-side helper (no GPU work, no handle): the k-mer table of a run (`predict --kmer-table`) as text.
 *
 *  table      int64 [4^k + 1][S2S_KMER_TABLE_FIELDS]: what s2s_kmer_table_accumulate built, copied to the host (or the sum of
 *             several such tables);   k: 1..S2S_KMER_TABLE_MAX_K;
 *  digitisation, range, offset   the calibration the table was accumulated with (floats, widened to double);
 *  with_header  != 0: the text starts with the header line.
 * Tab separated, "\n" ended; the header is
 *      kmer  n_occ  n_events  n_samples  level_mean  level_stdv  dwell_mean  dwell_stdv
 * and there is one row per k-mer with n_occ >= 1, in code order (AA..A first, the first letter most significant); the extra row
 * prints as k times `N`, last.  n_occ: how often the k-mer occurred as a real k-mer of a chunk; n_events: how often it got at
 * least one stored sample; n_samples: the stored samples it got.  With e, n, nn, S, Q the row's events, samples, samples_sq, sum
 * and sumsq, the products formed in 128-bit integers, then converted to double, exactly as written:
 *      level_mean = ((double)S / (double)n + offset) * range / digitisation
 *      level_stdv = sqrt((double)max(n*Q - S*S, 0)) / (double)n * range / digitisation
 *      dwell_mean = (double)n / (double)e
 *      dwell_stdv = sqrt((double)max(e*nn - n*n, 0)) / (double)e
 * each printed "%.4f"; the four print `nan` when n_events == 0.  Definitions: level_mean / level_stdv are POOLED SAMPLE statistics
 * of the stored int16 levels -- every stored sample of the k-mer counts once, whichever event it belongs to -- with the
 * population deviation (ddof 0); they are not statistics of event means.  "Dwell" is an event's STORED sample count after crop and
 * strip, i.e. end_idx - start_idx of the event table (s2s_events_format), not the drawn duration; its deviation is over the
 * events (ddof 0), so events without samples do not enter.  The levels are those a reader computes from the stored integers with
 * the calibration GIVEN HERE; the remark of s2s_events_format on the per-record offset draw applies unchanged.
 * Returns the bytes written, or S2S_ERR_ARG -- a NULL pointer, k outside 1..10, a calibration that is NaN or has range or
 * digitisation 0, a negative counter other than sum, or capacity below s2s_kmer_table_format_bound's value for the same arguments
 * (nothing is written then); the bound counts the rows with n_occ >= 1 and holds for any counters. */
int64_t s2s_kmer_table_format_bound(const int64_t* table, int32_t k, float digitisation, float range, float offset, int32_t with_header);
int64_t s2s_kmer_table_format(const int64_t* table, int32_t k, float digitisation, float range, float offset, int32_t with_header,
                              uint8_t* out, int64_t capacity);

/* ---- host-side helper (no GPU work, no handle): the k-mer model of a run (`predict --kmer-model`) as text.
 *
 *  table      int64 [4^k + 1][S2S_KMER_MODEL_FIELDS]: what s2s_kmer_model_accumulate built, copied to the host (or the sum of
 *             several such tables);   k: 1..S2S_KMER_TABLE_MAX_K;
 *  digitisation, range, offset   the calibration the table was accumulated with (floats, widened to double);
 *  with_header  != 0: the text starts with the comment lines "#k\t<k>" and "#alphabet\tnucleotide" and the column line
 *      kmer  level_mean  level_stdv  sd_mean  sd_stdv  n_events
 * Tab separated, "\n" ended; one row per ACGT k-mer with events >= 1, in code order.  The extra row 4^k is never printed: a model
 * has no such k-mer.  With e, A, A2, Bs, B2 the row's events, sum_m, sum_m2, sum_d and sum_d2, the products formed in 128-bit
 * integers, then converted to double, exactly as written:
 *      level_mean = ((double)A / (256.0 * e) + offset) * range / digitisation
 *      level_stdv = sqrt((double)max(e*A2 - A*A, 0)) / (256.0 * e) * range / digitisation
 *      sd_mean    = (double)Bs / (256.0 * e) * range / digitisation
 *      sd_stdv    = sqrt((double)max(e*B2 - Bs*Bs, 0)) / (256.0 * e) * range / digitisation
 * each printed "%.4f".  level_mean / level_stdv are the mean and the population deviation (ddof 0) of the k-mer's EVENT MEANS,
 * sd_mean / sd_stdv those of its events' own sample deviations (s2s_events_format's event_stdv, in fixed point): every event
 * counts once, however many samples it has.  The levels are those of the calibration GIVEN HERE; the remark of s2s_events_format
 * on the per-record offset draw applies unchanged.
 * Returns the bytes written, or S2S_ERR_ARG -- a NULL pointer, k outside 1..10, a calibration that is NaN or has range or
 * digitisation 0, a negative counter other than sum_m, or capacity below s2s_kmer_model_format_bound's value for the same
 * arguments (nothing is written then); the bound counts the rows with events >= 1 and holds for any counters. */
int64_t s2s_kmer_model_format_bound(const int64_t* table, int32_t k, float digitisation, float range, float offset, int32_t with_header);
int64_t s2s_kmer_model_format(const int64_t* table, int32_t k, float digitisation, float range, float offset, int32_t with_header,
                              uint8_t* out, int64_t capacity);

/* ---- `compare`: how far two stored signals are apart -- median / MAD normalisation and the banded dynamic-time-warping (DTW)
 * distance, all in integers, so that the same bytes come out for any batching and any workgroup shape and on the host.  The
 * reference has no such command.  No checkpoint is involved: the entries take no handle but `device` and `stream` (a hipStream_t
 * as void*, NULL = default stream), make the device current for their duration, are stream-ordered and asynchronous to the host,
 * and return S2S_OK / S2S_ERR_ARG / S2S_ERR_HIP (message: s2s_last_error(NULL)).  All pointers are device pointers; offs are int64.
 *
 * Median and MAD of a record of n >= 1 stored int16 samples:
 *   med = the lower median: the element of rank (n - 1) / 2 (integer division) of the sorted samples;
 *   mad = the element of the same rank of the sorted |x - med| (0 .. 65,535: it does not fit int16);
 *   both int32; a record with n = 0 (or with n > S2S_DTW_MAX_SAMPLES) gives med = mad = 0.
 * Normalised sample:
 *   q = clamp(floor((2 (x - med) S + d) / (2 d)), -32767, 32767) as int16, d = max(mad, 1), S = `scale` (S2S_DTW_SCALE = 64: one
 *   MAD is 64 units); round-half-up on a true floor division.  1 <= scale <= 8192 (the numerator stays below 2^31); med and mad
 *   outside what int16 samples can give are clamped to -32768 .. 32767 and 1 .. 65,535.
 * Banded DTW of a (n samples) against b (m samples), band R >= 1:
 *   cell (i, j) is inside the band iff |i m - j n| <= R max(n, m) (in int64): symmetric under swapping a and b, +-R samples on
 *   the shorter signal's axis; for R >= 1 it always holds a monotone path from (0, 0) to (n - 1, m - 1) (step i while
 *   i m - j n <= 0, else j);
 *   cost(i, j) = |a[i] - b[j]|;  D(i, j) = cost(i, j) + min(D(i - 1, j), D(i, j - 1), D(i - 1, j - 1)) over the predecessors inside
 *   the band and the matrix, D(0, 0) = cost(0, 0);
 *   the result is D(n - 1, m - 1), an int64 (70,000 samples of opposite extremes pass 2^32).  The per-sample figure of `compare`
 *   is D / (n + m) / S, formed on the host in double.
 *   n = 0 or m = 0: S2S_DTW_COST_EMPTY (-1).
 * Warping path of a pair (s2s_dtw_path; D, the band and the cell cost as above): the walk back from (n - 1, m - 1) to (0, 0) that
 *   steps from (i, j) to the predecessor with the smallest D among (i - 1, j - 1), (i - 1, j), (i, j - 1); a predecessor outside the
 *   matrix, outside the band or unreached does not count; on equal D the preference is (i - 1, j - 1), then (i - 1, j), then
 *   (i, j - 1).  D is unique, so the path is.  The tie rule governs the path only (the cost's `min` does not care).  Written
 *   forward from (0, 0) the path is a string of ops, one byte each:
 *     S2S_DTW_OP_M 0  to (i + 1, j + 1);   S2S_DTW_OP_A 1  to (i + 1, j): one more sample of a on the same sample of b;
 *     S2S_DTW_OP_B 2  to (i, j + 1)        (S2S_DTW_OP_NONE 3 is the code of (0, 0) and of unreached cells in the scratch only).
 *   steps = the number of ops: max(n, m) - 1 <= steps <= n + m - 2, #M + #A = n - 1, #M + #B = m - 1; every visited cell is in the
 *   band and the costs of the visited cells, (0, 0) included, sum to D(n - 1, m - 1).  A pair with an empty or too long member or
 *   an unreached corner has steps = 0; its cost is what s2s_dtw_banded gives.
 *   Boundary map g of a path (formed on the host: compare.boundary_map): g(0) = 0, g(n) = m, for 0 < i < n g(i) = the smallest j
 *   with (i, j) on the path; g never decreases, and the samples [s, e) of a map to [g(s), g(e)) of b: abutting intervals stay
 *   abutting, a sample of b shared by several of a belongs to the last of them, an interval may come out empty.
 * Limits: 1 <= band <= S2S_DTW_MAX_BAND (s2s_dtw_max_band() returns it); n, m <= S2S_DTW_MAX_SAMPLES = 2^22; 0 <= R, P.  A band or
 * a count outside them is S2S_ERR_ARG and nothing is launched.  The lengths of the device entries lie in device memory, which a
 * stream-ordered call cannot read: a pair with a member longer than the limit costs no work and gets S2S_DTW_COST_TOO_LONG (-2);
 * the host twins, which see the lengths, return S2S_ERR_ARG for it before they compute anything.
 *
 *  s2s_signal_median_mad   samples: the records back to back, record r = samples[offs[r] .. offs[r+1]); med, mad [R] out.  One
 *                 workgroup per record, exact rank selection by two 256-bin histogram passes in LDS over x + 32768 (the high byte,
 *                 then the low byte inside the selected bin) and the same two passes over |x - med|.
 *  s2s_signal_normalise    out [offs[R]] int16 (may not alias samples).
 *  s2s_dtw_banded          pair p = a[a_offs[p] .. a_offs[p+1]) against b[b_offs[p] .. b_offs[p+1]); cost [P] out.  One workgroup
 *                 per pair sweeps the anti-diagonals with three rolling diagonals of int64 in LDS (3 (2 band + 2) 8 bytes) and two
 *                 windows of the samples of the next 256 diagonals (2 (2 band + 256) 2 bytes): 58,416 B at S2S_DTW_MAX_BAND; no
 *                 atomics, no traffic between workgroups.
 *  s2s_dtw_path   the same pairs; cost [P] out, identical to s2s_dtw_banded's.  ops: one byte per op; pair p owns
 *                 ops[path_offs[p] .. path_offs[p+1]) (int64 [P + 1], at least n + m - 2 bytes for a pair with two non-empty members)
 *                 and its path comes out RIGHT-ALIGNED there, in forward order: ops[path_offs[p+1] - steps[p] .. path_offs[p+1]);
 *                 steps int64 [P] out.  scratch: device memory for the decisions, 16-byte aligned; pair p owns the bytes
 *                 scratch[scratch_offs[p] .. scratch_offs[p+1]) (int64 [P + 1], every offset a multiple of 16), at least
 *                 s2s_dtw_path_scratch_bytes(n, m, band) = (n + m - 1) * ceil((floor(2 band max(n, m) / (n + m)) + 1) / 64) * 16 of
 *                 them (0 for a pair without path; a host function, S2S_ERR_ARG for a band outside the limits): per diagonal i + j
 *                 a fixed number of 16-byte word pairs, 2 bits per in-band cell.  Two kernels: the sweep of s2s_dtw_banded in an
 *                 instance that also stores the decisions (two wave ballots and one 16-byte store per 64 cells), then one wave per
 *                 pair that walks back.  A pair whose slots are too small or misaligned gets its cost and steps = 0, and nothing
 *                 is written outside a slot; the walk is bounded by n + m - 2 steps whatever the scratch holds. */
#define S2S_DTW_SCALE 64
#define S2S_DTW_OP_M 0
#define S2S_DTW_OP_A 1
#define S2S_DTW_OP_B 2
#define S2S_DTW_OP_NONE 3
#define S2S_DTW_MAX_BAND 1024
#define S2S_DTW_MAX_SAMPLES (1 << 22)
#define S2S_DTW_COST_EMPTY (-1)
#define S2S_DTW_COST_TOO_LONG (-2)
int32_t s2s_dtw_max_band(void);
int s2s_signal_median_mad(int device, void* stream, const int16_t* samples, const int64_t* offs, int32_t R, int32_t* med, int32_t* mad);
int s2s_signal_normalise(int device, void* stream, const int16_t* samples, const int64_t* offs, int32_t R, const int32_t* med,
                         const int32_t* mad, int32_t scale, int16_t* out);
int s2s_dtw_banded(int device, void* stream, const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs,
                   int32_t P, int32_t band, int64_t* cost);
int64_t s2s_dtw_path_scratch_bytes(int64_t n, int64_t m, int32_t band);
int s2s_dtw_path(int device, void* stream, const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs, int32_t P,
                 int32_t band, int64_t* cost, uint8_t* scratch, const int64_t* scratch_offs, uint8_t* ops, const int64_t* path_offs,
                 int64_t* steps);
/* The same three on host pointers, in plain C++ (`compare --cpu`; also the definition the GPU must equal bit for bit): records /
 * pairs are dealt out over `threads` >= 1 host threads; the DTW sweeps rows with two rolling rows.  S2S_ERR_ARG as above, and for a
 * record or a pair member longer than S2S_DTW_MAX_SAMPLES or offsets that decrease. */
int s2s_signal_median_mad_host(const int16_t* samples, const int64_t* offs, int32_t R, int32_t* med, int32_t* mad, int32_t threads);
int s2s_signal_normalise_host(const int16_t* samples, const int64_t* offs, int32_t R, const int32_t* med, const int32_t* mad,
                              int32_t scale, int16_t* out, int32_t threads);
int s2s_dtw_banded_host(const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs, int32_t P, int32_t band,
                        int64_t* cost, int32_t threads);
/* s2s_dtw_path on host pointers (`compare --cpu --path`): a row sweep that keeps 2 bits per in-band cell (n rows of
 * ceil(min(m, 2 floor(band max(n, m) / n) + 3) / 32) 64-bit words per pair in flight), then the walk back; the same cost, ops and
 * steps bit for bit.  No scratch argument.  S2S_ERR_ARG also for a slot of ops shorter than n + m - 2. */
int s2s_dtw_path_host(const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs, int32_t P, int32_t band,
                      int64_t* cost, uint8_t* ops, const int64_t* path_offs, int64_t* steps, int32_t threads);

/* ---- `compare --open-ends`: where a short query sits inside a target -- subsequence DTW (free start, free end), in integers like
 * the entries above and with their conventions (no handle, stream-ordered, S2S_OK / S2S_ERR_ARG / S2S_ERR_HIP).  `compare` runs it
 * on the first and on the last samples of record A against the head and the tail of record B and then hands the interval of B
 * between the two anchors to s2s_dtw_banded / s2s_dtw_path.
 *
 * Subsequence DTW of a query q (L samples) inside a target t (H samples), both int16:
 *   cost(i, j) = |q[i] - t[j]|;
 *   row 0 starts anywhere and has NO horizontal predecessor: E(0, j) = cost(0, j), S(0, j) = j;
 *   for i > 0: E(i, j) = cost(i, j) + min over the predecessors (i - 1, j - 1), (i - 1, j), (i, j - 1) that lie inside the matrix
 *   (column 0 has (i - 1, 0) only), and S(i, j) = S of the predecessor with the smallest E; on equal E the preference is
 *   (i - 1, j - 1), then (i - 1, j), then (i, j - 1) -- the order of s2s_dtw_path.  Ties follow the predecessor order, never the
 *   smaller S;
 *   the result: j* = the SMALLEST j that minimises E(L - 1, j); cost = E(L - 1, j*), start = S(L - 1, j*), end = j* + 1: the query
 *   matched t[start .. end).
 *   reverse != 0 solves the same problem on q and t read back to front (q'[i] = q[L - 1 - i], t'[j] = t[H - 1 - j]; no reversed
 *   copy is made) and reports the interval in forward coordinates of t: start = H - end', end = H - start'.
 *   E fits int32: the vertical path in column j is always available, so E(i, j) <= (i + 1) 65,535 < 2^28 for L <= 2048.  cost leaves
 *   as int64 like the other entries.
 *   L = 0 or H = 0: cost = S2S_DTW_COST_EMPTY, start = end = 0.
 * Limits: L <= S2S_SDTW_MAX_QUERY = 2048 (s2s_sdtw_max_query() returns it), H <= S2S_DTW_MAX_SAMPLES, 0 <= P.  The device entry
 * cannot see the lengths: a problem with L or H beyond the limit, or with a negative begin or len, costs no work and gets
 * cost = S2S_DTW_COST_TOO_LONG, start = end = 0; the host twin returns S2S_ERR_ARG for it before it computes anything.
 *
 *  s2s_sdtw       problem p = q[q_begin[p] .. q_begin[p] + q_len[p]) inside t[t_begin[p] .. t_begin[p] + t_len[p]); q and t may be
 *                 the same pool and the ranges of different problems may overlap (the head and the tail anchor of one pair read
 *                 the same two records); reverse uint8 [P]; cost, start, end int64 [P] out.  P = 0 launches nothing.  One
 *                 workgroup of 1024 threads per problem sweeps the anti-diagonals i + j, one barrier each, with three rolling
 *                 diagonals of (int32 E, int32 S) in LDS (3 (2048 + 2) 8 bytes), the query whole (2048 2 bytes) and a window of
 *                 the target samples of the next 256 diagonals ((2048 + 256) 2 bytes): 57,904 B of static LDS whatever L is;
 *                 a thread keeps the rows i = its index mod 1024, so the running (min E, smallest j, S) of row L - 1 lives in the
 *                 registers of one thread; no atomics, no traffic between workgroups; L + H - 1 diagonals whatever memory holds.
 *  s2s_sdtw_host  the same on host pointers, in plain C++ (`compare --open-ends --cpu`; the definition the kernel must equal bit
 *                 for bit): a row sweep with two rolling rows of (E, S), problems dealt out over `threads` >= 1 host threads. */
#define S2S_SDTW_MAX_QUERY 2048
int32_t s2s_sdtw_max_query(void);
int s2s_sdtw(int device, void* stream, const int16_t* q, const int64_t* q_begin, const int64_t* q_len, const int16_t* t,
             const int64_t* t_begin, const int64_t* t_len, const uint8_t* reverse, int32_t P, int64_t* cost, int64_t* start,
             int64_t* end);
int s2s_sdtw_host(const int16_t* q, const int64_t* q_begin, const int64_t* q_len, const int16_t* t, const int64_t* t_begin,
                  const int64_t* t_len, const uint8_t* reverse, int32_t P, int64_t* cost, int64_t* start, int64_t* end, int32_t threads);

/* ---- `resquiggle`: which samples of a stored signal belong to which k-mer of its sequence, given the level a pore model expects
 * for every k-mer -- a dynamic programme over (sample, k-mer) in integers, with the conventions of the `compare` entries above (no
 * handle, `device` and `stream`, stream-ordered, device pointers, int64 offs, S2S_OK / S2S_ERR_ARG / S2S_ERR_HIP).  The reference
 * has no such command (its event tables come from uncalled4).  Unvalidated against f5c / uncalled4.
 *
 * Per read: q[0 .. n) the normalised int16 samples, l[0 .. K) the normalised int16 levels of its k-mers (s2s_signal_normalise clamps
 * to +-32767, so S2S_RSQ_UNKNOWN = -32768 is free: it marks a k-mer without a level).  Parameters: band R, 1 .. S2S_DTW_MAX_BAND;
 * skip_penalty, 0 .. S2S_RSQ_MAX_SKIP_PENALTY = 2^20; unknown_cost, 0 .. S2S_RSQ_MAX_UNKNOWN_COST = 65,535.
 *   cost(i, j) = |q[i] - l[j]|, or unknown_cost when l[j] == S2S_RSQ_UNKNOWN;
 *   cell (i, j) is inside the band iff |i K - j n| <= R n (in int64): +-R k-mers around the diagonal, at most 2 R + 1 cells per row;
 *   D(0, 0) = cost(0, 0); no other cell of row 0 is reached (both ends are pinned: sample 0 belongs to k-mer 0, sample n - 1 to
 *   k-mer K - 1);
 *   for i > 0: D(i, j) = cost(i, j) + min(D(i - 1, j - 1), D(i - 1, j), D(i - 1, j - 2) + skip_penalty) over the predecessors that lie
 *   inside the matrix and the band and are themselves reached; a cell without such a predecessor is unreached.  Every sample belongs
 *   to exactly one k-mer and the k-mer index never falls; a cell depends on the previous row only;
 *   the result is D(n - 1, K - 1), an int64 (70,000 samples at the opposite extreme of their levels pass 2^32).
 * Path: the walk back from (n - 1, K - 1) that steps to the predecessor with the smallest term of the minimum; on equal terms the
 *   preference is advance (i - 1, j - 1), then stay (i - 1, j), then skip (i - 1, j - 2).  K-mer j owns the samples
 *   [ev_start[j], ev_start[j] + ev_len[j]) of the rows the path spends in column j; a skipped k-mer gets ev_start = -1, ev_len = 0.
 * Result codes (in cost):
 *   n = 0 or K = 0: S2S_DTW_COST_EMPTY;
 *   n or K above S2S_DTW_MAX_SAMPLES: S2S_DTW_COST_TOO_LONG -- the device does no work for it and leaves its ev_start / ev_len
 *   untouched; the host twin, which sees the lengths, returns S2S_ERR_ARG before it computes anything;
 *   K > 2 n (no work: so a row's window moves by at most two columns per row), or the corner unreached (it is never outside the band
 *   for K <= 2 n): S2S_RSQ_UNREACHED (-3).
 *   A read without a solution that is not too long gets ev_start = -1, ev_len = 0 for every k-mer.
 * A solved read: the ev_len sum to n; ev_start[0] = 0; the starts of the unskipped k-mers ascend and abut; k-mers 0 and K - 1 are never
 *   skipped, nor two neighbours; the costs of the visited cells plus skip_penalty x (number of skipped k-mers) equal the result.
 *
 *  s2s_resquiggle  read p = q[q_offs[p] .. q_offs[p+1]) against l[l_offs[p] .. l_offs[p+1]); cost int64 [P] out; ev_start, ev_len
 *                 int32 out, k-mer j of read p at l_offs[p] + j.  scratch: device memory for the decisions, 16-byte aligned; read p
 *                 owns scratch[scratch_offs[p] .. scratch_offs[p+1]) (int64 [P + 1], every offset a multiple of 16), at least
 *                 s2s_resquiggle_scratch_bytes(n, K, band) = n * ceil((2 band + 1) / 64) * 16 of them (0 for a read without a
 *                 solution by its lengths; a host function, S2S_ERR_ARG for a band outside the limits): per row ceil((2 band + 1) /
 *                 64) 16-byte word pairs, 2 bits per slot, cell (i, j) in slot j mod (64 ceil((2 band + 1) / 64)).  A read whose slot
 *                 is too small or misaligned gets its cost and no events (-1 / 0), and nothing is written outside a slot.  Two
 *                 kernels (csrc/s2s_resquiggle.h): one workgroup per read sweeps the sample rows, one barrier each, D of the last
 *                 two rows in LDS rings addressed by j mod ring (nothing is shifted when the window slides), the own column's D in
 *                 a register, two wave ballots and one 16-byte store per 64 cells; then one wave per read walks back, at most n
 *                 steps whatever the scratch holds.  Dynamic LDS: 1024 c + 2 (64 c + 128) bytes, c = ceil((2 band + 1) / 64):
 *                 38,272 B at S2S_DTW_MAX_BAND, 19,840 B at band 512.
 *  s2s_event_sums per k-mer S = sum x and Q = sum x^2 (int64) over the samples [ev_start, ev_start + ev_len) of the read's record in
 *                 `samples` (the RAW stored int16, record p = samples[s_offs[p] .. s_offs[p+1])); S, Q int64 out at l_offs[p] + j.
 *                 A skipped k-mer, and an interval that does not lie inside the record, give 0, 0.  No atomics: 16 lanes share a
 *                 k-mer whatever its length (a stalled k-mer of 30,000 samples is 1,875 strides of its 16 lanes) and add up by
 *                 shuffles.
 *  s2s_resquiggle_host, s2s_event_sums_host   the same on host pointers, in plain C++ (`resquiggle --cpu`; the definition the
 *                 kernels must equal bit for bit): a row sweep with two rolling rows that keeps 2 bits per in-band cell, then the
 *                 walk back; reads dealt out over `threads` >= 1 host threads; no scratch argument.  S2S_ERR_ARG as above, and for a
 *                 read longer than the limits or offsets that decrease. */
#define S2S_RSQ_UNKNOWN (-32768)
#define S2S_RSQ_UNREACHED (-3)
#define S2S_RSQ_MAX_SKIP_PENALTY (1 << 20)
#define S2S_RSQ_MAX_UNKNOWN_COST 65535
int64_t s2s_resquiggle_scratch_bytes(int64_t n, int64_t K, int32_t band);
int s2s_resquiggle(int device, void* stream, const int16_t* q, const int64_t* q_offs, const int16_t* l, const int64_t* l_offs, int32_t P,
                   int32_t band, int32_t skip_penalty, int32_t unknown_cost, int64_t* cost, uint8_t* scratch, const int64_t* scratch_offs,
                   int32_t* ev_start, int32_t* ev_len);
int s2s_event_sums(int device, void* stream, const int16_t* samples, const int64_t* s_offs, const int32_t* ev_start, const int32_t* ev_len,
                   const int64_t* l_offs, int32_t P, int64_t* S, int64_t* Q);
int s2s_resquiggle_host(const int16_t* q, const int64_t* q_offs, const int16_t* l, const int64_t* l_offs, int32_t P, int32_t band,
                        int32_t skip_penalty, int32_t unknown_cost, int64_t* cost, int32_t* ev_start, int32_t* ev_len, int32_t threads);
int s2s_event_sums_host(const int16_t* samples, const int64_t* s_offs, const int32_t* ev_start, const int32_t* ev_len,
                        const int64_t* l_offs, int32_t P, int64_t* S, int64_t* Q, int32_t threads);

/* ---- `segment`: event detection -- a stored record cut into runs of constant level without its sequence, by two windowed
 * t-statistics in integers, with the conventions of the entries above (no handle, `device` and `stream`, stream-ordered, device
 * pointers, int64 offs, S2S_OK / S2S_ERR_ARG / S2S_ERR_HIP).  The reference has no such command.  This is NOT scrappie's detector
 * (there is no peak-height state machine), and it is unvalidated against scrappie / f5c / uncalled4.
 *
 * Per record x[0 .. n) (the raw stored int16).  A detector is a window w and an integer threshold T.
 * Score: for w <= i <= n - w let L = [i - w, i), R = [i, i + w), S and Q the sum and the sum of squares of a window,
 *     d = S_R - S_L,   V = w (Q_L + Q_R) - S_L^2 - S_R^2   (w^2 times the sum of the two population variances: never negative),
 *     score_w(i) = floor(256 w d^2 / max(V, 1))   as int64: 256 times Welch's t^2 between the windows (t^2 = d^2 w / V);
 *   every other i has score 0 -- all i of a record with n < 2 w among them.  With w <= S2S_SEG_MAX_WINDOW = 32: |d| <= 32 * 65,535 <
 *   2^21, so the numerator 256 w d^2 stays below 2^8 2^5 2^42 = 2^55 < 2^56, and V <= w (Q_L + Q_R) <= 32 * 64 * 2^30 = 2^41 < 2^42.
 * Peak: i is a peak of the detector iff score(i) >= T, score(i) > score(i') for every i - w <= i' < i, and score(i) >= score(i')
 *   for every i < i' <= i + w; neighbours outside [0, n] do not count.  On equal scores the leftmost wins, and two peaks of one
 *   detector are more than w apart.  (T >= 1 puts a peak at w <= i <= n - w: all its neighbours lie in [0, n].)
 * Two detectors run together: short (w_s, T_s) and long (w_l, T_l), 1 <= w_s <= w_l <= S2S_SEG_MAX_WINDOW, 1 <= T <=
 *   S2S_SEG_MAX_THRESHOLD = 2^40.
 * Boundaries: every short peak, and every long peak without a short peak at distance <= w_s.  The rule is local: nothing is
 *   greedy, nothing is ordered left to right.
 * Events: with the boundaries b_1 < ... < b_m the events are [0, b_1), [b_1, b_2), ..., [b_m, n); a record with n >= 1 and no
 *   boundary is one event, a record with n = 0 has none.  The events abut and sum to n; the first and the last hold at least w_s
 *   samples and every other at least w_s + 1; so a record has at most s2s_segment_capacity(n, w_s) = max(1, floor(n / w_s)) events
 *   (0 for n = 0).
 * `segment` takes t on its command line: T = floor(256.0 * t * t) in double (segment.threshold_int, the one place).
 *
 *  s2s_segment_capacity       host function: the bound above; S2S_ERR_ARG for n < 0 or w_short outside 1 .. S2S_SEG_MAX_WINDOW.
 *  s2s_segment_scratch_bytes  host function: the bytes of `scratch` s2s_segment needs for `total` pooled samples: per tile of
 *                 S2S_SEG_TILE = 2048 positions 32 flag words of 64 bits and 32 int32 ranks of the words inside the tile, and
 *                 tiles + 1 int64 ranks of the tiles (R does not enter today); S2S_ERR_ARG for total < 0 or R < 0.
 *  s2s_segment    samples: the records back to back, record r = samples[offs[r] .. offs[r+1]); `total` is the caller's offs[R], by
 *                 value: the entry cannot read device memory before the launch and the grid depends on it.  No pooled position
 *                 >= total is ever read, whatever offs holds.  Record r owns the slots [ev_offs[r], ev_offs[r+1]) of ev_start /
 *                 ev_len (int32; event k of the record at ev_offs[r] + k: start in the record, samples) -- the layout
 *                 s2s_event_sums reads through its l_offs, so the two chain on the device without a copy.  n_events int32 [R]: the
 *                 record's events; -(events) for a record whose slot is smaller than that (nothing is written to its slot then);
 *                 S2S_DTW_COST_TOO_LONG for a record of more than S2S_DTW_MAX_SAMPLES samples (no work is done for it and its
 *                 samples are not read).  A record with offs[r] < 0, offs[r+1] < offs[r] or offs[r+1] > total counts as empty: 0
 *                 events.  Nothing is ever written outside a slot.  scratch: 16-byte aligned; it needs no initialisation and may be
 *                 reused by the next call on the stream.  R = 0 or total = 0 launches nothing (and writes nothing: with total = 0
 *                 every record is empty, which the caller knows).  -(events) and S2S_DTW_COST_TOO_LONG can coincide at -2; the
 *                 caller, who knows the lengths, tells them apart.  Windows or thresholds outside the limits: S2S_ERR_ARG, nothing is launched.
 *                 Three launches (csrc/s2s_segment.h), nothing spins or waits between workgroups, no atomics: the work is split over
 *                 the POOLED positions, not over records -- workgroup t owns the positions [2048 t, 2048 (t + 1)) and reads a halo
 *                 of max(2 w_l, 3 w_s) <= 96 on each side; a thread finds its record by a search in offs; a record's edges zero
 *                 the scores, so nothing crosses from one record into the next.  (1) flags: the samples and, per position, its
 *                 distance to its record's two ends (clamped bytes) go to LDS, both detectors' scores come from direct window
 *                 sums (the two 64-bit divisions per position are skipped where d = 0), then the peak and the merge rule; one bit
 *                 per position by wave ballots -- the first sample of every record that is neither empty nor too long is flagged
 *                 too, so the events are exactly the flagged positions -- and one count per tile.  Static LDS: S2S_SEG_LDS_BYTES
 *                 = 47,296 B.  (2) one workgroup scans the tile counts.  (3) compact: a flagged position with global rank g in
 *                 record r writes slot ev_offs[r] + (g - rank(offs[r])); its length runs to the next flagged position, found by
 *                 rank (a search in the tile ranks, never a walk over samples), or to the record's end; n_events from the ranks at
 *                 the record's two ends.  1,000 records of 50,000 samples and one record of 2^22 load the device alike.
 *  s2s_segment_host   the same on host pointers, in plain C++ (`segment --cpu`; the definition the kernels must equal bit for
 *                 bit): records dealt out over `threads` >= 1 host threads, window sums from prefix sums; no scratch argument.
 *                 S2S_ERR_ARG for what the device can only mark: a record longer than S2S_DTW_MAX_SAMPLES or offsets that decrease
 *                 or are negative (before anything is computed), and a slot smaller than its record's events (that record gets
 *                 n_events = -(events) and an untouched slot, the others are complete).
 *  s2s_segment_format_bound, s2s_segment_format   host helpers: the event table of `segment` as text, rows formatted on `threads`
 *                 host threads.  Tab separated, "\n" ended; the header is
 *                      read_name  event_index  start_idx  end_idx  event_level_mean  event_stdv
 *                 and record r gives one row per event k < n_events[r] (a record with n_events <= 0 gives none), records in order:
 *                 its id (ids[id_offs[r] .. id_offs[r+1])), k, ev_start, ev_start + ev_len, and with n = ev_len, S, Q the sums of
 *                 s2s_event_sums in the slot and (digitisation, offset, range) = cal[3 r .. 3 r + 3) the RECORD's own calibration
 *                 (double), the two expressions of s2s_events_format, in double and exactly as written there:
 *                      event_level_mean = ((double)S / n + offset) * range / digitisation
 *                      event_stdv       = sqrt((double)max(n*Q - S*S, 0)) / n * range / digitisation
 *                 both "%.4f" (the population deviation); n*Q - S*S is formed exactly (an event may hold 2^22 samples, so in 128
 *                 bits) and rounded to double once.  Returns the bytes written, or S2S_ERR_ARG: a NULL pointer, a record with
 *                 rows whose calibration is not finite or has digitisation or range 0, an event with ev_len < 1, a slot smaller
 *                 than n_events, or capacity below the bound function's value for the same arguments (nothing is written then). */
#define S2S_SEG_MAX_WINDOW 32
#define S2S_SEG_MAX_THRESHOLD ((int64_t)1 << 40)
#define S2S_SEG_TILE 2048
int64_t s2s_segment_capacity(int64_t n, int32_t w_short);
int64_t s2s_segment_scratch_bytes(int64_t total, int32_t R);
int s2s_segment(int device, void* stream, const int16_t* samples, const int64_t* offs, int32_t R, int64_t total, int32_t w_short,
                int32_t w_long, int64_t thr_short, int64_t thr_long, uint8_t* scratch, const int64_t* ev_offs, int32_t* ev_start,
                int32_t* ev_len, int32_t* n_events);
int s2s_segment_host(const int16_t* samples, const int64_t* offs, int32_t R, int64_t total, int32_t w_short, int32_t w_long,
                     int64_t thr_short, int64_t thr_long, const int64_t* ev_offs, int32_t* ev_start, int32_t* ev_len, int32_t* n_events,
                     int32_t threads);
int64_t s2s_segment_format_bound(const int32_t* n_events, int32_t R, const int64_t* id_offs, const double* cal, int32_t with_header);
int64_t s2s_segment_format(const int32_t* ev_start, const int32_t* ev_len, const int64_t* S, const int64_t* Q, const int64_t* ev_offs,
                           const int32_t* n_events, int32_t R, const uint8_t* ids, const int64_t* id_offs, const double* cal,
                           int32_t with_header, int32_t threads, uint8_t* out, int64_t capacity);

/* ---- `eventalign`: which detected events of an UNTRIMMED stored signal belong to which k-mer of its sequence -- the events of
 * s2s_segment, their means normalised by the entries of `compare`, aligned to the normalised levels inside a narrow band that follows
 * the path (the adaptive band of Suzuki and Kasahara, as nanopolish and f5c use it), with free ends that cost a trim penalty per
 * event.  In integers, with the conventions of the entries above (no handle, `device` and `stream`, stream-ordered, device pointers,
 * int64 offs, S2S_OK / S2S_ERR_ARG / S2S_ERR_HIP).  The reference has no such command.  Unvalidated against f5c / nanopolish /
 * uncalled4.
 *
 * Event means: event e of record r, with S_e the sum of s2s_event_sums and n_e = ev_len, has the mean
 *   x_e = round-half-even(S_e / n_e) as int16 (a sum of n int16 values divided by n fits; any other S is clamped to int16, and an
 *   event with n_e < 1 has mean 0).  Record r contributes c_r = n_events[r] means when 0 < n_events[r] <= ev_offs[r+1] - ev_offs[r]
 *   and ev_offs[r] >= 0, else none (n_events 0, -k and S2S_DTW_COST_TOO_LONG give none).  The means lie back to back, events in
 *   order: m_offs[0] = 0, m_offs[r+1] = m_offs[r] + c_r, mean e of record r at m_offs[r] + e -- the layout s2s_signal_median_mad
 *   and s2s_signal_normalise take.
 *
 * Alignment, per read: m[0 .. E) the normalised int16 event means, l[0 .. K) the normalised int16 levels (S2S_RSQ_UNKNOWN marks a
 * k-mer without a level, as for s2s_resquiggle), the events' (ev_start, ev_len) in the slot layout of s2s_segment.  Parameters: band
 * width W, a multiple of 64 in 64 .. S2S_EVA_MAX_WIDTH = 1024; skip_penalty 0 .. S2S_RSQ_MAX_SKIP_PENALTY and trim_penalty 0 ..
 * S2S_EVA_MAX_TRIM_PENALTY, both 2^20; unknown_cost 0 .. S2S_RSQ_MAX_UNKNOWN_COST; E, K <= S2S_DTW_MAX_SAMPLES.
 *   cost(e, j) = |m[e] - l[j]|, or unknown_cost when l[j] == S2S_RSQ_UNKNOWN.
 *   D(e, j): the best cost of a path that has consumed the events up to e and the k-mers up to j.  Event e belongs to k-mer j iff
 *   the path enters (e, j) by diag, stay or start.  The candidates, tried in this order, strict '<' keeps the earlier one:
 *     diag   D(e - 1, j - 1) + cost(e, j)      j >= 1
 *     stay   D(e - 1, j) + cost(e, j)
 *     skip   D(e, j - 1) + skip_penalty        j >= 1; no cell cost: k-mer j gets no event from this move
 *     start  e trim_penalty + cost(e, j)       j = 0 only: the events 0 .. e - 1 are trimmed
 *   Only predecessors that were inside their own band and are reached count; a cell without a candidate is unreached.
 *   The band: band b, b = 0 .. E + K - 2, holds the W cells o = 0 .. W - 1 with k-mer j = lk(b) + o and event e = b - j; cells
 *   outside the matrix are unreached.  lk(0) = -W / 2, so (0, 0) is cell W / 2 of band 0.  For b >= 1 let ll = D of cell 0 and ur = D
 *   of cell W - 1 of band b - 1, unreached counting as +infinity: if both are unreached the band moves right iff b is odd, else it
 *   moves right iff ll > ur (a tie between reached cells moves down).  Right: lk(b) = lk(b - 1) + 1, r_b = 1; down: lk(b) = lk(b - 1),
 *   r_b = 0.  Seen from cell o of band b, stay is cell o + r_b and skip cell o + r_b - 1 of band b - 1, diag cell o + r_b + r_(b-1) - 1
 *   of band b - 2: three rolling bands suffice and every shift is the same for the whole band.
 *   Result: over all reached cells (e, K - 1) that lie in their band, the smallest D(e, K - 1) + (E - 1 - e) trim_penalty, on a tie
 *   the smallest e; cost is int64.  E = 0 or K = 0: S2S_DTW_COST_EMPTY.  E or K above S2S_DTW_MAX_SAMPLES: S2S_DTW_COST_TOO_LONG --
 *   the device does no work for it and leaves its outputs but cost untouched; the host twin returns S2S_ERR_ARG before it computes
 *   anything.  No such reached cell: S2S_RSQ_UNREACHED.
 *   Walk back: from that cell along the stored 2-bit decisions until a start; at most E + K steps whatever the scratch holds.
 *   Outputs: first_event and end_event per read (0, 0 without a path); per event, at m_offs[p] + e, its k-mer, or -1 when trimmed;
 *   per k-mer, at l_offs[p] + j: k_start = ev_start of its first event, k_len = ev_start + ev_len of its last event - k_start (the
 *   samples of its events: the events of s2s_segment are consecutive and abut), k_events = how many events it got.  A skipped k-mer
 *   gets -1 / 0 / 0, and so does every k-mer of an unsolved read, whose events all get -1.
 * A solved read: the events first_event .. end_event - 1 are all assigned and no other is; the assigned k-mer indices never fall;
 *   the first assigned event is on k-mer 0; the unskipped k-mers' intervals abut; cost = the sum of cost(e, kmer(e)) +
 *   skip_penalty (K - distinct assigned k-mers) + trim_penalty (first_event + E - end_event).  (A k-mer entered by skip never gets
 *   an event: stay out of such a cell would have to beat diag out of the same predecessor, which is tried first and costs no more.)
 *
 *  s2s_event_means  S, ev_len, ev_offs, n_events as s2s_segment and s2s_event_sums leave them; m_offs int64 [R + 1] and means int16
 *                 out.  capacity: the int16 values `means` holds, by value; the sum of the slots, ev_offs[R] - ev_offs[0], always
 *                 suffices; a record whose means would end beyond it writes none (the host twin: S2S_ERR_ARG).  Two launches
 *                 (csrc/s2s_eventalign.h): one workgroup scans the counts, in strides of 1,024 with a carry when R exceeds the
 *                 workgroup; then a fill, record r to the workgroups (r, 0 .. 7).  No atomics, nothing waits between workgroups.
 *                 R = 0 writes m_offs[0] = 0.
 *  s2s_eventalign_scratch_bytes  host function: (E + K - 1) (16 W / 64 + 4) rounded up to 16 -- per band W / 64 16-byte word pairs
 *                 (2 bits per cell: bit 0 of 64 codes, then bit 1) and, behind all of them, one int32 lk; 0 for a read without a
 *                 solution by its lengths; S2S_ERR_ARG for a width outside the limits.  It grows with E, so a slot sized by
 *                 s2s_segment_capacity holds whatever s2s_segment finds.
 *  s2s_eventalign read p = m[m_offs[p] .. m_offs[p+1]) against l[l_offs[p] .. l_offs[p+1]), its events in the slots from ev_offs[p]
 *                 on; cost int64 [P], first_event, end_event int32 [P], ev_kmer int32 at m_offs[p] + e, k_start, k_len, k_events
 *                 int32 at l_offs[p] + j out.  scratch: 16-byte aligned; read p owns scratch[scratch_offs[p] .. scratch_offs[p+1])
 *                 (int64 [P + 1], every offset a multiple of 16).  A read whose slot is too small or misaligned, or whose slot of
 *                 events is smaller than E, gets its cost and no path, and nothing is ever written outside a slot.  Two kernels:
 *                 one workgroup of W threads per read sweeps the bands, one barrier each, with three rolling bands of int64 in LDS;
 *                 a thread keeps its own m[e] and l[j] and reads only the one that changed, from windows staged every 256 bands;
 *                 per 64 cells two wave ballots and one 16-byte store, per band one int32 lk; every thread keeps its best final
 *                 candidate and one reduction picks the result.  Then one wave per read walks back.  Every loop bound is a function
 *                 of E, K and W; no atomics, nothing spins or waits between workgroups.  Width or penalties outside the limits:
 *                 S2S_ERR_ARG, nothing is launched.  Dynamic LDS: 3 (W + 2) 8 + 2 (W + 256) 2 bytes: 29,744 B at W = 1024, 4,656 B
 *                 at W = 128.
 *  s2s_event_means_host, s2s_eventalign_host   the same on host pointers, in plain C++ (`eventalign --cpu`; the definition the
 *                 kernels must equal bit for bit): records / reads dealt out over `threads` >= 1 host threads; no scratch
 *                 argument.  S2S_ERR_ARG as above, and for a read longer than the limits, offsets that decrease or are negative,
 *                 and a slot of events smaller than E. */
#define S2S_EVA_MAX_WIDTH 1024
#define S2S_EVA_MAX_TRIM_PENALTY (1 << 20)
int64_t s2s_eventalign_scratch_bytes(int64_t E, int64_t K, int32_t width);
int s2s_event_means(int device, void* stream, const int64_t* S, const int32_t* ev_len, const int64_t* ev_offs, const int32_t* n_events,
                    int32_t R, int64_t capacity, int64_t* m_offs, int16_t* means);
int s2s_eventalign(int device, void* stream, const int16_t* m, const int64_t* m_offs, const int16_t* l, const int64_t* l_offs,
                   const int32_t* ev_start, const int32_t* ev_len, const int64_t* ev_offs, int32_t P, int32_t width, int32_t skip_penalty,
                   int32_t trim_penalty, int32_t unknown_cost, int64_t* cost, uint8_t* scratch, const int64_t* scratch_offs,
                   int32_t* first_event, int32_t* end_event, int32_t* ev_kmer, int32_t* k_start, int32_t* k_len, int32_t* k_events);
int s2s_event_means_host(const int64_t* S, const int32_t* ev_len, const int64_t* ev_offs, const int32_t* n_events, int32_t R,
                         int64_t capacity, int64_t* m_offs, int16_t* means, int32_t threads);
int s2s_eventalign_host(const int16_t* m, const int64_t* m_offs, const int16_t* l, const int64_t* l_offs, const int32_t* ev_start,
                        const int32_t* ev_len, const int64_t* ev_offs, int32_t P, int32_t width, int32_t skip_penalty,
                        int32_t trim_penalty, int32_t unknown_cost, int64_t* cost, int32_t* first_event, int32_t* end_event,
                        int32_t* ev_kmer, int32_t* k_start, int32_t* k_len, int32_t* k_events, int32_t threads);

/* ---- `preprocess`: the training chunks of the reference's `preprocess` (preprocess.py: process_df -> get_chunks -> pad_lengths ->
 * typical_indices, per read: its partition_by route) cut from alignments that lie in memory as the entries above leave them, with
 * their conventions (no handle, `device` and `stream`, stream-ordered, device pointers, int64 offs, S2S_OK / S2S_ERR_ARG /
 * S2S_ERR_HIP).  Geometry: k = seq_kmer, te = max_dna_len, ts = max_signal_len.
 *
 * Read p owns the slots [l_offs[p], l_offs[p+1]) of ev_start / ev_len / S / Q / stdv (the layout of s2s_resquiggle and
 * s2s_event_sums) and of kmers (uint8 [slots][k]: the k letters of every slot), and the record [s_offs[p], s_offs[p+1]) of the pool.
 * A ROW is a slot with ev_len >= 1 whose interval [ev_start, ev_start + ev_len) lies inside the record (ev_start >= 0, and 0 <=
 * s_offs[p] <= s_offs[p+1] <= total) and whose k letters are not all 'N'; a k-mer with some N is still a row.  Rows are taken in
 * position order: slot order, or slot order reversed with `backwards` (how `resquiggle --rna` lays its slots).  n = the read's rows.
 *   n = 0: the read gives nothing.  Otherwise te - (n mod te) PAD rows follow (1 .. te of them; n a multiple of te gives a whole
 *   chunk of pads, as in the reference): k letters '_', length 1, one sample 0.0, deviation 0.  The read gives floor(n / te) + 1
 *   chunks of te consecutive rows.
 * Per chunk:
 *   chunks          fp16 [te][k][5], one-hot over _ACGT ('_' is column 0); any other letter, N included, is an all-zero row;
 *   chunks_lengths  int64 [te], the rows' lengths;
 *   targets_length  int64, their sum (the true sum: the reference's int16 wraps);
 *   targets         fp32 [ts], the rows' samples back to back in pA, zero behind;
 *   stdevs          fp32 [te].
 * A chunk is KEPT iff targets_length <= ts (it is always >= te > 0).  Kept chunks come out dense, in read order, then chunk order.
 * With `reverse` (RNA) each row's samples are read back to front; the rows stay in position order.
 * Two sample sources:
 *   S2S_CHUNK_RAW  pool = the stored int16 x, cal[3 p .. 3 p + 3) = the record's (digitisation, offset, range) as doubles:
 *                    pA = (float)(((double)x + offset) * range / digitisation)
 *                  and with n the row's length and S, Q the sums s2s_event_sums left in the slot, for n <= 1,024 (n Q < 2^51 fits int64)
 *                    deviation = (float)(sqrt((double)max(n Q - S^2, 0)) / n * range / digitisation)
 *                  (a longer row drops its chunk anyway: its value is 0).  No expression has the shape a b + c: device code is
 *                  built with contraction on, and both sides must round alike.
 *   S2S_CHUNK_PA   pool = fp32 samples in pA, stdv = an fp32 deviation per slot, as an event table gave them; S, Q, cal unused.
 *
 *  s2s_chunk_scratch_bytes  host function: the bytes of `scratch` for `slots` pooled slots, P reads and chunk_capacity chunks (per
 *                 tile of S2S_SEG_TILE slots 32 flag words and 32 int32 ranks, two int64 ranks per tile, per read a rank and a chunk
 *                 offset, per chunk of the capacity a rank, per slot an int32); S2S_ERR_ARG outside the limits.
 *  s2s_chunk_pack `total` = the pool's samples and `slots` = the caller's l_offs[P], by value: the grids depend on them, and no
 *                 sample >= total and no slot >= slots is ever read, whatever the offsets hold.  chunk_capacity, by value: the rows
 *                 (chunks) the five outputs hold; the sum over the reads of floor(slots_p / te) + 1, which the host knows, always
 *                 suffices.  Outputs, dense over the kept chunks: chunks uint16 (fp16 bits) [kept][te][k][5], chunks_lengths int64
 *                 [kept][te], targets fp32 [kept][ts], targets_lengths int64 [kept], stdevs fp32 [kept][te]; nothing behind the kept
 *                 prefix is written.  n_rows int32 [P]; counters int64 [3]: chunks formed, chunks kept, all-N slots that were rows
 *                 otherwise.  Chunks beyond chunk_capacity are not formed (counters[0] still counts them; the host twin:
 *                 S2S_ERR_ARG).  scratch: 16-byte aligned, needs no initialisation.  Eight launches (csrc/s2s_chunk.h), by ranks only:
 *                 no atomics, nothing spins or waits between workgroups.  (1) one flag per slot that is a row, by wave ballots over
 *                 the POOLED slots (a thread finds its read by a search in l_offs), and per tile its rows and all-N rows; (2) one
 *                 workgroup scans the tiles' two counts (the scan of s2s_segment, twice); (3) every row writes its slot at its rank, and every read
 *                 its row count and chunk count; (4) the scan of the chunk counts; (5) per POOLED chunk, a wave: it finds its read
 *                 by a search in the chunk offsets, lane j loads row j, the sum of the lengths decides the keep flag; (6) the scan
 *                 of the flags; (7) per kept chunk, a wave: the lengths' prefix over the lanes by shuffles, every output sample finds
 *                 its row by a search in that prefix, the target row is written coalesced.  One read of 2^22 slots loads the
 *                 device like thousands of short ones.  Static LDS: 272 B in (1), 128 B in the scans, none elsewhere.
 *                 Limits: k 1 .. 10, te 1 .. 64, ts 1 .. 1,024, P <= 2^22, P <= chunk_capacity < 2^31, slots < 2^31, total <= 2^40;
 *                 anything outside is S2S_ERR_ARG and nothing is launched.  P = 0 writes the counters (0) and nothing else.
 *  s2s_chunk_pack_host   the same on host pointers, in plain C++ (`preprocess --cpu`; the definition the kernels must equal bit
 *                 for bit, floats included): reads, then chunks dealt out over `threads` >= 1 host threads; no scratch argument.
 *                 S2S_ERR_ARG as above, and for what the device can only skip: offsets that decrease or are negative, l_offs[P] !=
 *                 slots, s_offs[P] > total, a read of more than 2^22 slots, a calibration that is not finite or has digitisation 0,
 *                 more chunks than chunk_capacity. */
#define S2S_CHUNK_RAW 0
#define S2S_CHUNK_PA 1
#define S2S_CHUNK_MAX_K 10
#define S2S_CHUNK_MAX_TE 64
#define S2S_CHUNK_MAX_TS 1024
#define S2S_CHUNK_MAX_SLOTS (((int64_t)1 << 31) - 1)
int64_t s2s_chunk_scratch_bytes(int64_t slots, int32_t P, int64_t chunk_capacity);
int s2s_chunk_pack(int device, void* stream, const void* pool, const int64_t* s_offs, int64_t total, int32_t source, const int64_t* l_offs,
                   int64_t slots, const int32_t* ev_start, const int32_t* ev_len, const int64_t* S, const int64_t* Q, const double* cal,
                   const float* stdv, const uint8_t* kmers, int32_t P, int32_t k, int32_t te, int32_t ts, int32_t reverse,
                   int32_t backwards, int64_t chunk_capacity, uint8_t* scratch, uint16_t* chunks, int64_t* chunks_lengths, float* targets,
                   int64_t* targets_lengths, float* stdevs, int32_t* n_rows, int64_t* counters);
int s2s_chunk_pack_host(const void* pool, const int64_t* s_offs, int64_t total, int32_t source, const int64_t* l_offs, int64_t slots,
                        const int32_t* ev_start, const int32_t* ev_len, const int64_t* S, const int64_t* Q, const double* cal,
                        const float* stdv, const uint8_t* kmers, int32_t P, int32_t k, int32_t te, int32_t ts, int32_t reverse,
                        int32_t backwards, int64_t chunk_capacity, uint16_t* chunks, int64_t* chunks_lengths, float* targets,
                        int64_t* targets_lengths, float* stdevs, int32_t* n_rows, int64_t* counters, int32_t threads);

/* ---- host-side helper (no GPU work, no handle): replays the DRAWS of the reference's read sampler (utils.py:415-479
 * `sampling`, with the read-length law of utils.py:325-331 `draw_expon_dis`) without building a read, so that a rank of a sharded
 * run finds the generator state of its first read in microseconds per thousand reads instead of replaying them in the
 * interpreter.  Per attempt the reference draws a start position (random.randint on the genome-wide coordinate), a strand
 * (random.choice("+-"), DNA profiles only) and, for an accepted read, one random.choice("ACGT") per N in it; the length of
 * attempt (read_i, retry) is scipy's expon law seeded with seed + read_i * (max_retries + 1) + retry, truncated and clipped to
 * [1, total_len]; an attempt is rejected when a DNA read is cut short by its contig's end, is shorter than min_read_len or
 * holds more than 10 % N (utils.py:381-400).
 *
 *  mt_state       in/out [625]: Python's random.getstate()[1] (624 Mersenne-Twister words + the index); on return the state
 *                 in front of the first draw of read *out_next_read_i;
 *  contig_ends    [n_contigs] running sum of the contig lengths (genome < 2^31 bases);
 *  n_pos, n_pos_count   nullable [n_contigs]: per contig the sorted offsets of its N bases (NULL / 0 for a contig without N);
 *  num_seqs, first_read_i   reads first_read_i .. num_seqs-1 are attempted in order;
 *  stop_after     stop once this many reads have been accepted (< 0: never);
 *  out_lengths    nullable [>= number of accepted reads]: their lengths.
 * Returns the number of accepted reads, or < 0 (S2S_ERR_ARG: also when seed + num_seqs * (max_retries + 1) >= 2^32, where
 * the reference's scipy seed would leave the range this fast path mirrors -- the caller then replays in Python). */
int64_t s2s_sampler_replay(uint32_t* mt_state, const int64_t* contig_ends, int32_t n_contigs,
                           const int64_t* const* n_pos, const int64_t* n_pos_count, int64_t num_seqs, int64_t first_read_i, int64_t r,
                           uint64_t seed, int64_t total_len, int32_t is_dna, int32_t min_read_len, int32_t max_retries,
                           int64_t stop_after, int32_t* out_lengths, int64_t* out_next_read_i);

/* The same replay for any of the reference's three read-length laws (utils.py:311-331; --distr): law 0 = expon (as above), 1 = gamma
 * (scipy gamma.rvs(6.3693711, loc = 0.53834893) * r / 4.39), 2 = beta (beta.rvs(1.778, 7.892, loc = 316.758, scale = 34191.257) * r /
 * 6615): numpy's legacy samplers -- Marsaglia-Tsang on the polar-method normal, whose cached second variate carries over between
 * the two gammas of a beta -- mirrored draw for draw on a generator seeded per (read, retry).  s2s_length_law: one such length
 * (test hook). */
int64_t s2s_sampler_replay_law(uint32_t* mt_state, const int64_t* contig_ends, int32_t n_contigs,
                               const int64_t* const* n_pos, const int64_t* n_pos_count, int64_t num_seqs, int64_t first_read_i, int64_t r,
                               uint64_t seed, int64_t total_len, int32_t is_dna, int32_t min_read_len, int32_t max_retries,
                               int64_t stop_after, int32_t law, int32_t* out_lengths, int64_t* out_next_read_i);
int64_t s2s_length_law(int32_t law, uint32_t seed, double r, int64_t total_len);

/* Plain FASTA text -> cleaned sequences on the host (no GPU): what utils.read_fasta (pysam.FastxFile, utils.py:290-308) and
 * process_genome (upper-case, non-ACGT -> N: utils.py:594-597) do line by line in the interpreter; every rank of a sharded
 * run parses the whole reference before its first kernel.  s2s_fasta_count: number of records ('>' first on a line), -2 when
 * the first non-blank line starts with '@' (FASTQ: s2s_fastq_clean), -3 when a line holds a lone carriage return (a line break
 * of its own for the reference's reader: the caller's line loop decides).  s2s_fasta_clean: out (>= n bytes) receives the sequences back to
 * back, line ends removed and lines stripped of blanks; map_acgtn = 1 applies process_genome's mapping; seq_offs [records+1]
 * delimits them; name_span [2*records]: begin / end of each record's name (first token of its header) inside data.
 * Returns the number of records, -1 when there are more than max_records. */
int64_t s2s_fasta_count(const uint8_t* data, int64_t n);
/* Four-line FASTQ records the same way (--read-input files; pysam.FastxFile reads either format): `out` receives the sequence
 * lines as they stand minus their line ends (map_acgtn as above); -2 for anything the caller's line loop must judge itself (no '@'
 * where a header should be, a missing '+' line, a truncated record, a lone carriage return inside a line); out == NULL with
 * max_records == 0 only counts the records. */
int64_t s2s_fastq_clean(const uint8_t* data, int64_t n, int32_t map_acgtn, uint8_t* out, int64_t* seq_offs,
                        int64_t* name_span, int64_t max_records);
int64_t s2s_fasta_clean(const uint8_t* data, int64_t n, int32_t map_acgtn, uint8_t* out, int64_t* seq_offs,
                        int64_t* name_span, int64_t max_records);

/* ---- host-side helpers of the rank-shard merge (no GPU work, no handle; `predict --gpus N` / `merge-shards`): the reference
 * leaves ONE output file (inference.py:65-79, signal_io.py:167-171, 268-282), a sharded run one per rank.
 * s2s_copy_ranges copies n byte ranges (src_fd[i], src_off[i], len[i]) -> (dst_fd[i], dst_off[i]); ranges must not overlap inside
 * one file.  engine 0: copy_file_range on the descriptors (in the kernel, no user-space buffer; pread / pwrite through a bounce
 * buffer where the file system refuses it), ONE writer whatever `threads` says -- buffered writes of one file take its inode lock and
 * more writers are slower (profiles/r05/fs_write_probe_shm.txt: 6.5 GB/s with one, 3.2-4.1 GB/s with 2-8).  engine 1: where the
 * destination is on tmpfs, its ranges are allocated first (posix_fallocate: 18.6 GB/s on that box) and then filled on `threads`
 * threads, each pread()ing the source into a populated shared mapping of the destination (pages that exist: no lock, no
 * allocation; 8.0 against 5.7 GB/s for engine 0); any other file system, a refused allocation or mapping: engine 0.  engine 2: the
 * same on any file system (A/B: it loses on a disk's page cache).  Returns the bytes copied, or < 0 (S2S_ERR_ARG, or -errno of the
 * failing call; -EIO when a source is shorter than its range).
 * s2s_blow5_scan walks the [u64 size][body] records of a BLOW5 file between byte offsets begin and end (the end of the
 * header and the start of the end-of-file marker) reading the size prefixes only: the record count, or -2 when the chain of
 * sizes does not end exactly at `end` (a truncated shard). */
int64_t s2s_copy_ranges(int32_t n, const int32_t* src_fd, const int64_t* src_off, const int32_t* dst_fd, const int64_t* dst_off,
                        const int64_t* len, int32_t threads, int32_t engine);
int64_t s2s_blow5_scan(int32_t fd, int64_t begin, int64_t end);
/* ... and over a file that is still growing (the live join, seq2squiggle_amd/merge.py: LiveJoin): the complete records from `begin`
 * that end at or before `limit` (the file's size now), at most max_records; *out_end = the offset behind the last of them.  An
 * incomplete record (or the 5-byte end marker) ends the walk without an error.  Returns the number of records, or S2S_ERR_ARG. */
int64_t s2s_blow5_scan_upto(int32_t fd, int64_t begin, int64_t limit, int64_t max_records, int64_t* out_end);

/* Which softmax path the split-f16 decoder attention (S2S_MODE_F16X3 / S2S_MODE_F16) runs (layers.py:20-40 is one unmasked
 * softmax over 250 keys; both paths compute it within the parity bound, with the same error against an fp64 evaluation):
 *   0  the FAST path: shift = the row's maximum over the keys of PASS 0 + 2 log2 units, no maximum in later passes, straight-line
 *      code.  Pass 0 is a SAMPLE of the whole row -- the fast instance stores the K / V^T images with the blocks of four consecutive
 *      keys dealt out over the four 64-key passes, so pass 0 holds the key blocks b = 0 (mod 4).  A head whose later keys beat that
 *      shift by more than the f16 range shows in its row sum and is redone by an out-of-line online softmax.  Best for diffuse
 *      attention (the committed synthetic checkpoints redo nothing; their decoder w_qs / w_ks x 2: 6.4 % of the heads);
 *   1  the EXACT path at once: the online softmax (running row maximum raised and sums rescaled in every 64-key pass, no branch;
 *      the shift rides in the score MFMA's k-slots, a pass's row maxima come from its first score MFMA alone, natural key
 *      order) as the only path of its own kernel instance: 201.6 k shader cycles per chunk and CU against the fast path's 190.2 k
 *      on diffuse attention (6.0 % more), the same for ANY weights -- "fast, then redo" costs 310-328 k once most heads overflow
 *      (sharply peaked attention).
 * s2s_create chooses by a calibration launch on a fixed pseudo-random batch: exact when more than S2S_ATTENTION_REDO_THRESHOLD of
 * its heads had to be redone (where the two cost the same).  The environment variable S2S_ATTENTION_PATH = fast | exact (any
 * case) skips the launch, auto or empty means calibrate, anything else makes s2s_create fail.  `calibration_redo_rate` returns
 * the launch's share (-1 when no calibration ran).  Results are deterministic per chunk for a given path. */
#define S2S_ATTENTION_REDO_THRESHOLD 0.055
double s2s_attention_redo_threshold(void);
int s2s_set_attention_path(s2s_handle* h, int32_t path);
int s2s_get_attention_path(const s2s_handle* h, int32_t* path, double* calibration_redo_rate);

/* How a launch of the predict kernel (S2S_MODE_F32 / _F16X3 / _F16) is dealt out to its persistent workgroups, one per compute
 * unit:
 *   S2S_SCHEDULE_STATIC   workgroup b of G walks the chunks [b n / G, (b + 1) n / G) in groups (16 chunks in the split-f16 modes, 8
 *                         in f32): the launch lasts as long as its slowest workgroup;
 *   S2S_SCHEDULE_DYNAMIC  the workgroups take CLAIMS from one counter of the handle, one atomic per group, a group ahead of their
 *                         need: whole groups first, then the last G x group chunks in shrinking claims (G of group / 2, ... G of
 *                         2, then singles), so that the last thing any workgroup starts is one chunk.  s2s_schedule_claim is that
 *                         list: claim c of a launch of n chunks -> [*start, *start + *count), count 0 past the end;
 *   S2S_SCHEDULE_AUTO     (default) dynamic for a launch of at least S2S_SCHEDULE_AUTO_GROUPS groups per workgroup
 *                         (s2s_schedule_is_dynamic(n, n_wg, group) != 0), static below, where the taper's extra frontend phases
 *                         cost more than the tail they remove.
 * A chunk's output depends on its global index and the seed alone: the schedules give the same bytes.  The environment variable
 * S2S_SCHEDULE = auto | static | dynamic (any case) sets the handle's schedule at s2s_create; anything else makes s2s_create fail.
 * RULE: the launches of ONE handle must be stream-ordered -- issued on one stream, or on streams ordered by events.  The
 * hand-off slots of the workgroups always relied on that; the claim counter does too (a launch leaves it at zero for the next:
 * its last workgroup to run dry resets it, no host operation per launch).  Two handles share nothing. */
#define S2S_SCHEDULE_AUTO 0
#define S2S_SCHEDULE_STATIC 1
#define S2S_SCHEDULE_DYNAMIC 2
int s2s_set_schedule(s2s_handle* h, int32_t schedule);
int s2s_get_schedule(const s2s_handle* h, int32_t* schedule);
void s2s_schedule_claim(int64_t n, int32_t n_wg, int32_t group, int64_t c, int64_t* start, int32_t* count);
int32_t s2s_schedule_is_dynamic(int64_t n, int32_t n_wg, int32_t group);

/* Counters of the predict kernel since the last call (every build; synchronises the device, then resets them).  The fast
 * softmax of the split-f16 decoder is data dependent -- a head whose later keys beat the maximum over its pass-0 key sample (the
 * key blocks b = 0 mod 4, see s2s_set_attention_path) by more than the f16 range is redone on a safe path -- and the chip's clock
 * under this kernel depends on the operands, so a throughput
 * figure is a statement about one set of weights: these counters say how a run behaved.  out10 =
 *   [0] chunks launched, [1] (wave, head, layer) softmax runs (chunks x 8 waves x 8 heads x decoder layers),
 *   [2] ... of them redone on the safe path (0 in S2S_MODE_F32, which has no fast path),
 *   [3] shader-clock cycles (s_memtime) and [4] 100 MHz ticks (s_memrealtime) of one thread per workgroup over the whole
 *       kernel, summed over [5] workgroups: [3] / [4] / 10 is the clock in GHz the SIMDs really ran at,
 *   [6] chunks launched on the exact attention path (s2s_set_attention_path),
 *   [7] the longest and [8] the shortest of those workgroup spans in 100 MHz ticks ([4] / [5] is their mean; a launch lasts as
 *       long as the longest; 0 when nothing ran), [9] chunks launched on the dynamic schedule (s2s_set_schedule).
 * A generic handle counts [0] and [1] (with its decoder head count), and has no redo, clock, span, exact-path or schedule counts
 * ([2..9] 0). */
int s2s_stats_read(s2s_handle* h, uint64_t* out10);

/* Diagnostic builds (-DS2S_DIAG, never the shipped library): per wave of a workgroup (8 rows) 48 per-phase shader-cycle sums
 * since the last call, summed over the workgroups (slots 0-15 decoder phases, 16-18 whole-kernel s_memtime / s_memrealtime /
 * wave count, 32-47 the frontend's own phases; tools/diag_phases.py names them); out384 = [8][48].  S2S_ERR_ARG in a normal build. */
int s2s_diag_read(s2s_handle* h, uint64_t* out384);

/* ---------------------------------------------------------------------------------------------------------------- train
 * Replaces seq2squiggle.training_step + get_loss + configure_optimizers (model.py:65-105, 419-480) for the Adam / AdamW case, in
 * exact fp32 on one device: forward (the kernels of s2s_evaluate_chunks on a S2S_MODE_GENERIC_GEOMETRY handle, each layer writing
 * into buffers of its own -- the tape), backward (csrc/s2s_train.h), global gradient norm, clipping and the optimizer step.
 * The function:
 *   total = mean_{B ts} (y - target)^2 + 0.0005 mean_{B te} -Gamma(conc, rate).log_prob(max(|dwell|, 1)) + mean_{B te} (stdev - sigma)^2
 * with the means over the batch given (a short last batch divides by its own size).  The three heads read emb_out.detach(): their
 * losses reach only the heads' own weights; the signal loss flows through the decoder, the length regulator (a sum over each
 * k-mer's samples; cropped samples and rows behind the last dwell give nothing, a k-mer of dwell 0 gets zero), the encoder, the
 * pre-net and src_emb.  The two position tables have no gradient and never change.  Dropout is NOT applied and there is no
 * reduced-precision mode (the reference trains in 16-mixed with dropout).
 *
 * cfg->compute_mode must be S2S_MODE_GENERIC_GEOMETRY; every size and geometry that mode accepts runs.  A trainer holds fp32
 * weights, a gradient, Adam's m and v (each the size of the weights, m = v = 0 at create) and the tape.  Inside it uses the
 * generic handle's aligned packing; every blob it takes or hands out is in the order of s2s_blob_floats.
 *
 *  s2s_trainer_set_memory   bytes of tape + backward scratch a micro-batch may use (default S2S_TRAINER_DEFAULT_MEMORY, 2 GiB -- a choice: it keeps a default
 *                 batch of 512 chunks of the shipped size in one micro-batch and leaves most of the card free).  A batch whose
 *                 tape exceeds it runs as micro-batches of s2s_trainer_micro_batch(t, B) chunks, the last one shorter; their
 *                 gradients add in micro-batch order.  One chunk always runs.
 *  s2s_trainer_weights      copies the weights out in blob order (out_blob: host or device, [s2s_blob_floats]; a host copy
 *                 synchronises the stream).
 *  s2s_trainer_gradients    forward and backward only; changes no weight.  kmers / dwell / target / stdev as for
 *                 s2s_evaluate_chunks (device; dwell >= 0 is a precondition: a negative dwell reads nothing out of range, but its
 *                 gradient is not defined); out_loss device [B][3]: the per-chunk loss sums, bit-equal to s2s_evaluate_chunks'
 *                 on a S2S_MODE_GENERIC_GEOMETRY handle with the same weights; out_grad host or device [s2s_blob_floats]: the
 *                 gradient of `total` in blob order (the position tables' slots 0).
 *  s2s_trainer_step         the same, then one optimizer step: clip by global L2 norm as clip_grad_norm_ does (scale by
 *                 clip / (norm + 1e-6) when norm > clip; clip <= 0: none), then torch.optim.Adam (decoupled == 0: g += wd w) or
 *                 AdamW (decoupled != 0: w *= 1 - lr wd), bias correction by `step` (counts from 1).  The clip scale stays in
 *                 device memory: nothing returns to the host inside a step.  out_stats device [5] fp32: the three loss means of
 *                 this forward (signal, duration x 0.0005, noise), their total, and the gradient norm before clipping.
 * Deterministic: every sum over rows is per-tile partials in row order and one ordered pass, no float atomics; two calls with
 * the same inputs, B and memory budget give the same bits.  Stream-ordered; scratch grows on demand (the first call of a larger
 * batch synchronises the stream).  S2S_ERR_ARG: B < 1, a NULL pointer, inputs on another device than the trainer's, step < 1,
 * betas outside [0, 1), eps <= 0; message: s2s_trainer_last_error(t) (t == NULL: of the last failed create, thread-local). */
#define S2S_TRAINER_DEFAULT_MEMORY ((size_t)2 << 30)
typedef struct s2s_trainer s2s_trainer;
typedef struct s2s_adam {
    double lr, beta1, beta2, eps, weight_decay;
    double clip;               /* gradient_clip_val; <= 0: no clipping */
    int32_t decoupled;         /* 0: Adam (coupled L2), 1: AdamW */
    int32_t step;              /* 1, 2, ...: the bias-correction exponent */
} s2s_adam;
int s2s_trainer_create(const s2s_config* cfg, const void* weights_blob, size_t blob_bytes, int device, s2s_trainer** out);
void s2s_trainer_destroy(s2s_trainer* t);
const char* s2s_trainer_last_error(const s2s_trainer* t);
int s2s_trainer_set_memory(s2s_trainer* t, size_t bytes);
int64_t s2s_trainer_micro_batch(const s2s_trainer* t, int32_t B);
int s2s_trainer_weights(s2s_trainer* t, void* stream, float* out_blob);
int s2s_trainer_gradients(s2s_trainer* t, void* stream, const uint8_t* kmers, const int32_t* dwell, const float* target,
                          const float* stdev, int32_t B, float* out_loss, float* out_grad);
int s2s_trainer_step(s2s_trainer* t, void* stream, const uint8_t* kmers, const int32_t* dwell, const float* target,
                     const float* stdev, int32_t B, const s2s_adam* hyper, float* out_stats);

#ifdef __cplusplus
}
#endif
#endif /* S2S_HIP_H */
