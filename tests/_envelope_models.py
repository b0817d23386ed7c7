"""Synthetic checkpoints across the size and geometry envelope of the four generic compute modes, and the kernel code each reaches.

The cases use the seeded recipe of tests/_geometry_models.py (its functions take this module's CASES).  classes_of(cfg) restates, in
plain Python, which kernel instance and which remainder class of seq2squiggle_amd/csrc/s2s_generic.h, s2s_generic_h.h and
gen_block_fwd / gen_attention_fwd (s2s_generic_host.h) a configuration runs: the encoder's attention at T = max_dna_len with the
encoder's head_dim, the decoder's at T = max_signal_len with its own; the f16 kernels on the decoder only (the f16 modes keep the encoder
side in fp32).  tests/test_envelope_cpu.py asserts that the union over CASES is LABELS, so a class the kernels distinguish cannot
lose its case unnoticed.  tools/make_envelope_goldens.py records tests/golden/envelope_<tag>.npz from the imported reference."""
import _geometry_models as GM
from _geometry_models import weights_sha256  # noqa: F401  (re-exported for the tests)

# tag: seed, seq_kmer, max_dna_len, max_signal_len, dmodel, dff, encoder_heads, decoder_heads, pre / encoder / decoder layers
def _c(seed, k, te, ts, d, f, he, hd, pre, enc, dec):
    return dict(seed=seed, seq_kmer=k, max_dna_len=te, max_signal_len=ts, dmodel=d, dff=f, encoder_heads=he, decoder_heads=hd,
                pre_layers=pre, encoder_layers=enc, decoder_layers=dec)


CASES = {
    # head_dim 1, one key, one row per chunk (M = 1 at B = 1); dff 24 = one full fp32 K step plus a half step
    "hd1": _c(41, 6, 1, 1, 16, 24, 16, 16, 0, 1, 1),
    # head_dim 3 at the last length before the long kernel
    "hd3": _c(42, 9, 7, 256, 48, 40, 16, 16, 1, 1, 1),
    # long <8> with a partly filled output tile, the first length of the long kernel, dff at its upper edge
    "hd40": _c(43, 6, 33, 257, 80, 2048, 5, 2, 0, 1, 2),
    # long <8>, head_dim 112, T % 64 = 1
    "hd112": _c(44, 9, 16, 321, 224, 72, 7, 2, 0, 1, 1),
    # long <32> with full tiles at the last length but one; 13 encoder heads
    "hd208": _c(52, 9, 17, 1023, 208, 8, 13, 1, 0, 1, 1),
    # head_dim 96 on the short kernel (the e0 loop's partial last pass), 64 staged keys and 251 unstaged; 4 / 4 / 4 layers
    "hd96s": _c(46, 6, 64, 251, 96, 104, 1, 1, 4, 4, 4),
    # the default geometry (also run on "generic" / "generic-f16"): head_dim 64 on both sides, seq_kmer 1
    "hd64": _c(47, 1, 16, 250, 64, 136, 1, 1, 1, 2, 2),
    # head_dim 24 on the decoder, 12 on the encoder, 23 encoder keys, seq_kmer 16
    "hd24": _c(48, 16, 23, 255, 48, 88, 4, 2, 2, 1, 1),
    # the two pairs on either side of the K / V staging switch (gen_attn_lds_bytes against 80 KiB)
    "st36": _c(49, 7, 3, 256, 144, 48, 16, 4, 0, 1, 1),
    "un40": _c(50, 6, 4, 256, 80, 16, 16, 2, 0, 1, 1),
    "st72": _c(51, 9, 5, 128, 144, 56, 3, 2, 1, 1, 1),
    "un80": _c(45, 6, 2, 128, 80, 32, 1, 1, 0, 1, 1),
    # long <32> with a partly filled last tile (head_dim 136), encoder head_dim 17
    "hd136": _c(53, 9, 6, 330, 272, 200, 16, 2, 0, 1, 1),
    # long <1> at head_dim 6: the clamped k-step
    "hd6": _c(54, 5, 4, 704, 96, 40, 2, 16, 0, 1, 1),
    # dmodel 512 on the row kernels; decoder head_dim 128 on 64 staged keys
    "d512": _c(55, 9, 2, 64, 512, 8, 16, 4, 1, 1, 1),
}
TAGS = list(CASES)

GEN_ATTN_STAGE_BYTES = 80 * 1024     # s2s_generic.h


def gen_attn_lds_bytes(T: int, hd: int, stage: bool) -> int:
    """s2s_generic.h's gen_attn_lds_bytes: K [T][hd + 1] and V [T][hd] when staged, and per wave q [hd] and p [T], fp32."""
    return ((T * (2 * hd + 1) if stage else 0) + 4 * (hd + T)) * 4


def envelope_config(tag, base=None):
    return GM.geometry_config(tag, base, CASES)


def envelope_state_dict(tag):
    return GM.geometry_state_dict(tag, CASES)


def checkpoint_path(tag):
    return GM.checkpoint_path(tag, CASES)


def _attention_fp32(T, hd):
    """gen_attention_fwd's fp32 launch at T keys and head_dim hd."""
    out = set()
    if T > 256:
        nt = 1 if hd <= 16 else 8 if hd <= 128 else 32
        out.add(f"attn:long<{nt}>")
        if nt == 1:
            if hd % 4:
                out.add("attn_long<1>:hd%4!=0")                 # the clamped k-step
        else:
            out.add(f"attn_long<{nt}>:hd%16!=0" if hd % 16 else f"attn_long<{nt}>:hd%16==0")
        out.add("attn_long:T%16!=0" if T % 16 else "attn_long:T%16==0")
        if 1 <= T % 64 <= 15:
            out.add("attn_long:T%64 in 1..15")                  # the last query tile's waves 1-3 return at q0 >= T
        return out
    staged = gen_attn_lds_bytes(T, hd, True) <= GEN_ATTN_STAGE_BYTES
    out.add("attn:short_staged" if staged else "attn:short_unstaged")
    if hd < 64:
        out.add("attn_short:hd_pow2<64" if hd & (hd - 1) == 0 else "attn_short:hd_not_pow2<64")
    elif hd == 64:
        out.add("attn_short:hd==64")
    else:
        out.add("attn_short:hd_mult64>64" if hd % 64 == 0 else "attn_short:hd>64_tail")
    if T == 1:
        out.add("attn_short:T==1")
    if T < 64:
        out.add("attn_short:T<64")
        if 17 <= T <= 63 and T % 4:
            out.add("attn_short:T_17..63_%4!=0")
    if T % 64 == 0:
        out.add("attn_short:T%64==0")
    if 251 <= T <= 256:
        out.add("attn_short:T_251..256")
    return out


def _attention_f16(T, hd):
    """gen_attention_fwd's f16 launch (the decoder of the f16 modes)."""
    out = set()
    if T > 256:
        nt = 1 if hd <= 16 else 8 if hd <= 128 else 32
        out.add(f"attn_h:long_h<{nt}>")
        if hd % 16:
            out.add(f"attn_long_h<{nt}>:hd%16!=0")              # a partly filled output tile
        elif nt > 1:                                            # (<1> at head_dim 16 is one full tile: no class of its own)
            out.add(f"attn_long_h<{nt}>:hd%16==0")
    else:
        out.add("attn_h:h" if T == 250 else "attn_h:h_any")
        if T == 1:
            out.add("attn_h:T==1")
    out.add("attn_h:hd%32!=0" if hd % 32 else "attn_h:hd%32==0")
    if hd > 64 and hd % 64:
        out.add("attn_h:hd>64_%64!=0")                          # a second, partly filled V^T step
    out.add("attn_h:T%64!=0" if T % 64 else "attn_h:T%64==0")
    return out


def classes_of(cfg: dict) -> set:
    """The labels (a subset of LABELS) of the kernel code a checkpoint of config `cfg` runs in the generic modes."""
    te, ts, d, f, k = (cfg[n] for n in ("max_dna_len", "max_signal_len", "dmodel", "dff", "seq_kmer"))
    hde, hdd = d // cfg["encoder_heads"], d // cfg["decoder_heads"]
    out = _attention_fp32(te, hde) | _attention_fp32(ts, hdd) | _attention_f16(ts, hdd)
    # the staging switch itself: a (T, hd) within 4 head dims of the last staged one, on either side
    for T, hd in ((te, hde), (ts, hdd)):
        if T <= 256:
            last = max(h for h in range(0, 1024) if gen_attn_lds_bytes(T, h, True) <= GEN_ATTN_STAGE_BYTES)
            if last - 4 <= hd <= last:
                out.add("attn_short:last_staged_hd-4..0")
            if last < hd <= last + 4:
                out.add("attn_short:last_staged_hd+1..4")
    # gen_gemm_kernel: K in steps of 16 (K = dmodel is always whole steps; K = dff at w_2)
    if f % 16 == 8:
        out.add("gemm:K==8" if f == 8 else "gemm:K%16==8_after_full_steps")
    else:
        out.add("gemm:K%16==0")
    if f == 2048:
        out.add("gemm:dff==2048")
    if any(n % 64 for n in (d, 3 * d, f)):
        out.add("gemm:N%64!=0")
    if te == 1 and ts == 1:
        out.add("gemm:M==1_at_one_chunk")
    # gen_gemm_h_kernel: K in steps of 32, rows padded to ld_d / ld_f
    out.add(f"gemm_h:dmodel%32=={d % 32}")
    out.add(f"gemm_h:dff%32=={f % 32}")
    # gen_layernorm_kernel, gen_dwell_kernel, gen_emit_kernel: one wave per row over d features
    out.add("rows:d<64" if d < 64 else "rows:d==512" if d == 512 else "rows:d%64!=0" if d % 64 else "rows:d%64==0")
    # gen_embed_kernel
    out.add("embed:k==1" if k == 1 else "embed:k==16" if k == 16 else "embed:k_odd" if k % 2 else "embed:k_even")
    if (cfg["pre_layers"], cfg["encoder_layers"], cfg["decoder_layers"]) == (4, 4, 4):
        out.add("layers:4/4/4")
    if cfg["pre_layers"] == 0:
        out.add("layers:pre==0")
    return out


LABELS = {
    "attn:short_staged", "attn:short_unstaged", "attn:long<1>", "attn:long<8>", "attn:long<32>",
    "attn_short:hd_pow2<64", "attn_short:hd_not_pow2<64", "attn_short:hd==64", "attn_short:hd>64_tail", "attn_short:hd_mult64>64",
    "attn_short:T==1", "attn_short:T<64", "attn_short:T_17..63_%4!=0", "attn_short:T%64==0", "attn_short:T_251..256",
    "attn_short:last_staged_hd-4..0", "attn_short:last_staged_hd+1..4",
    "attn_long<1>:hd%4!=0", "attn_long<8>:hd%16!=0", "attn_long<8>:hd%16==0", "attn_long<32>:hd%16!=0",
    "attn_long<32>:hd%16==0", "attn_long:T%16!=0", "attn_long:T%16==0", "attn_long:T%64 in 1..15",
    "attn_h:h", "attn_h:h_any", "attn_h:long_h<1>", "attn_h:long_h<8>", "attn_h:long_h<32>", "attn_h:T==1",
    "attn_long_h<1>:hd%16!=0", "attn_long_h<8>:hd%16!=0", "attn_long_h<8>:hd%16==0", "attn_long_h<32>:hd%16!=0",
    "attn_long_h<32>:hd%16==0", "attn_h:hd%32!=0", "attn_h:hd%32==0", "attn_h:hd>64_%64!=0", "attn_h:T%64!=0", "attn_h:T%64==0",
    "gemm:K==8", "gemm:K%16==8_after_full_steps", "gemm:K%16==0", "gemm:dff==2048", "gemm:N%64!=0", "gemm:M==1_at_one_chunk",
    "gemm_h:dmodel%32==0", "gemm_h:dmodel%32==16", "gemm_h:dff%32==0", "gemm_h:dff%32==8", "gemm_h:dff%32==16", "gemm_h:dff%32==24",
    "rows:d<64", "rows:d%64!=0", "rows:d%64==0", "rows:d==512",
    "embed:k==1", "embed:k==16", "embed:k_odd", "embed:k_even",
    "layers:4/4/4", "layers:pre==0",
}
