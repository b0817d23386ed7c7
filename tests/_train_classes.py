"""Which remainder classes of the backward pass and the optimizer step a trainer call reaches, and the calls the GPU tests make.

train_classes_of(cfg, micro_batches) restates, in plain Python, the case distinctions of seq2squiggle_amd/csrc/s2s_train.h and
s2s_train_host.h (the forward launches: s2s_generic_host.h) for a call on a checkpoint of config `cfg` whose batch runs as
micro-batches of the given sizes, as
tests/_envelope_models.py's classes_of does for the forward kernels:
  train_attention_bwd_kernel, per side (the encoder at T = max_dna_len with its head_dim, the decoder at max_signal_len with its
    own): hp = the power of two >= min(head_dim, 64) that deals lanes to feature slots, ng = 64 / hp row groups per wave; a
    head_dim below hp leaves lanes idle inside every group; above 64 the e0 loop makes several passes, the last one partial when
    head_dim % 64 != 0; 512 fills wa / wb.  T against the 4 waves (rows t = wave, wave + 4, ...) and against the 64 lanes (the
    j / t loops of a row), 1024 filling stat / wp / wd; 1 < T < ng leaves row groups without a row.
  train_mm_kernel: 64 x 64 output tiles over (dmodel, dff, 3 dmodel, 5 seq_kmer), the LT = true k-loop over dff in steps of 16, the
    one-hot rows padded to a multiple of 4 (oh_ld).
  rows M = n max_dna_len and n max_signal_len of every micro-batch: 4 rows per workgroup of the row kernels, 16 per k-step and 64
    per tile of the products, TR_GRAD_ROWS = 512 per weight-gradient partial.
  the row kernels (layer norm, length regulator, heads, emit): one wave over dmodel features in passes of 64.
  the split into micro-batches, and (steps=True: the call is s2s_trainer_step) train_norm_kernel's one or several trips over the
    partials of train_sumsq_kernel, one per 2,048 floats of the arena.
tape_floats / micro_batch restate train_tape / train_micro_batch, so that the split a test asks for by a budget is the split this
table says it runs.  RUNS lists every call shape the GPU tests make; tests/test_train_classes_cpu.py holds it to the tests' own
case lists and asserts that its union is LABELS."""
TR_GRAD_ROWS = 512
WORKSPACE_BYTES = 512 << 20          # S2S_GENERIC_WORKSPACE_BYTES (include/s2s_hip.h)
DEFAULT_MEMORY = 2 << 30             # S2S_TRAINER_DEFAULT_MEMORY


def up64(n):
    return (n + 63) & ~63


def tape_floats(cfg, n):
    """train_tape(cfg, nullptr, n).floats."""
    d, f, k, te, ts = (int(cfg[x]) for x in ("dmodel", "dff", "seq_kmer", "max_dna_len", "max_signal_len"))
    Me, Md, Mb, big = n * te, n * ts, n * max(te, ts), max(3 * d, f)
    oh_ld = (5 * k + 3) & ~3
    block = lambda M: up64(M * 3 * d) + 5 * up64(M * d) + up64(M * f)
    at = up64(Me * d) * (2 + int(cfg["pre_layers"])) + 2 * up64(Me * 3 * d) + 3 * up64(Me) + up64(Me * 4) + up64(Me * oh_ld)
    at += int(cfg["encoder_layers"]) * block(Me) + up64(Md * d) + 3 * up64(Md) + int(cfg["decoder_layers"]) * block(Md)
    at += 3 * up64(Mb * d) + up64(Mb * big)
    nz_max = (Mb + TR_GRAD_ROWS - 1) // TR_GRAD_ROWS
    return at + up64(nz_max * max(3 * d * d, f * d, oh_ld * d))


def slice_max(cfg):
    """pack_generic's G.slice_max."""
    d, f, te, ts = (int(cfg[x]) for x in ("dmodel", "dff", "max_dna_len", "max_signal_len"))
    chunk = te * d + te + ts * d + ts + max(te, ts) * max(3 * d, f)
    heads = max(int(cfg["encoder_heads"]), int(cfg["decoder_heads"]))
    per_head = ((ts + 63) // 64) * 256 if ts > 256 else 1024
    return max(1, min(WORKSPACE_BYTES // (4 * chunk), 0xFFFFFFFF // (heads * per_head)))


def micro_batch(cfg, budget, B):
    """train_micro_batch: chunks per micro-batch of a batch of B under a budget of `budget` bytes."""
    cap = max(1, budget // (tape_floats(cfg, 1) * 4))
    cap = min(cap, B, slice_max(cfg), 65535 * TR_GRAD_ROWS // max(int(cfg["max_dna_len"]), int(cfg["max_signal_len"])))
    while cap > 1 and tape_floats(cfg, cap) * 4 > budget:
        cap -= 1
    return cap


def budget_for(cfg, B, n):
    """A budget under which a batch of B runs n chunks per micro-batch: the bisection of test_gpu_train_gradients.budget_for on
    micro_batch above, step for step, so that it returns the very number of bytes the GPU test sets."""
    lo, hi = 1, 1 << 40
    budget = hi
    while micro_batch(cfg, budget, B) != n:
        assert hi - lo > 1, f"no budget gives {n} chunks per micro-batch"
        budget = (lo + hi) // 2
        if micro_batch(cfg, budget, B) < n:
            lo = budget
        else:
            hi = budget
    return budget


def split(B, n):
    """The micro-batch sizes of a batch of B at n chunks per micro-batch."""
    return [min(n, B - s) for s in range(0, B, n)]


def arena_blocks(cfg):
    """-> (lowest, highest) possible ceil(arena floats / 2048): the arena holds the blob's floats, every piece (at most one per
    tensor, the f16 modes' none here) padded to a multiple of 4 floats and the whole to a multiple of 64."""
    import numpy as np
    from seq2squiggle_amd.train import state_shapes
    shapes = state_shapes(cfg)
    floats = sum(int(np.prod(s)) for s in shapes.values())
    return (floats + 2047) // 2048, (floats + 3 * len(shapes) + 63 + 2047) // 2048


def _attention_bwd(T, hd):
    out = set()
    hp = 1
    while hp < hd and hp < 64:
        hp <<= 1
    out.add(f"attn_bwd:hp=={hp}")
    if hd < hp:
        out.add("attn_bwd:hd<hp<=8" if hp <= 8 else "attn_bwd:hd<hp>=16")
    if hd > 64:
        out.add("attn_bwd:hd>64_mult64" if hd % 64 == 0 else "attn_bwd:hd>64_tail")
    if hd == 512:
        out.add("attn_bwd:hd==512")
    if T == 1:
        out.add("attn_bwd:T==1")
    elif T <= 3:
        out.add("attn_bwd:T_2..3")
    elif T % 4:
        out.add("attn_bwd:T>=4_%4!=0")
    if T < 64:
        out.add("attn_bwd:T<64")
    elif T % 64:
        out.add("attn_bwd:T>64_%64!=0")
    else:
        out.add("attn_bwd:T%64==0")
    if T == 1024:
        out.add("attn_bwd:T==1024")
    if 1 < T < 64 // hp:
        out.add("attn_bwd:1<T<ng")
    return out


def train_classes_of(cfg, micro_batches, steps=False):
    """The labels (a subset of LABELS) a trainer call on config `cfg` reaches when its batch runs as micro-batches of the sizes
    `micro_batches`; steps: the call is step(), not gradients()."""
    te, ts, d, f, k = (int(cfg[n]) for n in ("max_dna_len", "max_signal_len", "dmodel", "dff", "seq_kmer"))
    out = _attention_bwd(te, d // int(cfg["encoder_heads"])) | _attention_bwd(ts, d // int(cfg["decoder_heads"]))
    out.add("mm:d%64!=0" if d % 64 else "mm:d%64==0")
    out.add("mm:dff<64" if f < 64 else "mm:dff>64_%64!=0" if f % 64 else "mm:dff%64==0")
    if f % 16:
        out.add("mm:dff%16!=0")
    if f < 16:
        out.add("mm:dff<16")
    if 5 * k > 64:
        out.add("mm:5k>64")
    out.add("mm:5k%4!=0" if (5 * k) % 4 else "mm:5k%4==0")
    for n in micro_batches:
        for M in (n * te, n * ts):
            if M < 4:
                out.add("rows:M<4")
            if M < 16:
                out.add("rows:M<16")
            for q in (4, 16, 64):
                if M % q:
                    out.add(f"rows:M%{q}!=0")
            if M % 64 == 0:
                out.add("rows:M%64==0")
            out.add("wgrad:one_tile" if M <= TR_GRAD_ROWS else "wgrad:ragged_last" if M % TR_GRAD_ROWS else "wgrad:whole_tiles")
    out.add("rowk:d<64" if d < 64 else "rowk:d==512" if d == 512 else "rowk:d%64!=0" if d % 64 else "rowk:d%64==0")
    mb = list(micro_batches)
    if len(mb) == 1:
        out.add("micro:one")
    else:
        out.add("micro:equal" if mb[-1] == mb[0] else "micro:ragged_last")
        if mb[0] == 1:
            out.add("micro:one_chunk_each")
    if steps:
        lo, hi = arena_blocks(cfg)
        assert (lo <= 256) == (hi <= 256), "the arena's padding decides the class"
        out.add("step:norm_blocks<=256" if lo <= 256 else "step:norm_blocks>256")
    return out


LABELS = {
    "attn_bwd:hp==1", "attn_bwd:hp==2", "attn_bwd:hp==4", "attn_bwd:hp==8", "attn_bwd:hp==16", "attn_bwd:hp==32", "attn_bwd:hp==64",
    "attn_bwd:hd<hp<=8", "attn_bwd:hd<hp>=16", "attn_bwd:hd>64_mult64", "attn_bwd:hd>64_tail", "attn_bwd:hd==512",
    "attn_bwd:T==1", "attn_bwd:T_2..3", "attn_bwd:T>=4_%4!=0", "attn_bwd:T<64", "attn_bwd:T>64_%64!=0", "attn_bwd:T%64==0",
    "attn_bwd:T==1024", "attn_bwd:1<T<ng",
    "mm:d%64!=0", "mm:d%64==0", "mm:dff<64", "mm:dff>64_%64!=0", "mm:dff%64==0", "mm:dff%16!=0", "mm:dff<16",
    "mm:5k>64", "mm:5k%4!=0", "mm:5k%4==0",
    "rows:M<4", "rows:M<16", "rows:M%4!=0", "rows:M%16!=0", "rows:M%64!=0", "rows:M%64==0",
    "wgrad:one_tile", "wgrad:whole_tiles", "wgrad:ragged_last",
    "rowk:d<64", "rowk:d%64!=0", "rowk:d%64==0", "rowk:d==512",
    "micro:one", "micro:equal", "micro:ragged_last", "micro:one_chunk_each",
    "step:norm_blocks<=256", "step:norm_blocks>256",
}

def config_of(tag):
    """The config of a tag of RUNS.  d32, d128 and d512 are tests/_sized_models.py's (the trainer's tests never load the envelope
    case of the name d512); k9 and k6 the committed checkpoints'."""
    import _envelope_models as EM
    import _geometry_models as GM
    import _sized_models as SM
    from test_gpu_train_envelope import OWN_CASES                  # hd2: the one case no other table holds
    if tag in OWN_CASES:
        return GM.geometry_config(tag, None, OWN_CASES)
    if tag in SM.CASES:
        c = SM.sized_config(tag)
        c.setdefault("max_dna_len", 16)
        c.setdefault("max_signal_len", 250)
        return c
    if tag in ("k9", "k6"):
        import _eval_data as ED
        from seq2squiggle_amd.checkpoint import load_checkpoint
        return load_checkpoint(ED.checkpoint(tag))[1]
    return EM.envelope_config(tag) if tag in EM.CASES else GM.geometry_config(tag)


def default_batch(cfg):
    """The new tests' batch: 3 chunks where max_signal_len > 256 or dmodel >= 128, else 7."""
    return 3 if int(cfg["max_signal_len"]) > 256 or int(cfg["dmodel"]) >= 128 else 7


# Every call shape the GPU tests make: (test, tag, B, chunks per micro-batch -- B itself: the default budget holds the batch --,
# the micro-batch sizes this gives, whether the call is step()).  A per-micro-batch count below B is what the test bisects the
# budget to (budget_for), 1 with a batch above 1 what set_memory(1) gives.
def _r(test, tag, B, n=None, steps=False):
    n = B if n is None else n
    return (test, tag, B, n, tuple(split(B, n)), steps)


RUNS = (
    [_r("gradients.test_gradients", t, 7) for t in ("k9", "k6", "d32", "hd1", "g5x37", "hd24", "hd64", "hd96s")]
    + [_r("gradients.test_gradients", t, 3) for t in ("r16x500", "g64x1024", "hd208")]
    + [_r("gradients.test_gradients", "k9", 37, 13)]
    + [_r("gradients.test_gradients_at_the_large_sizes", t, 3) for t in ("d128", "d512")]
    + [_r("envelope.test_gradients", t, 7) for t in ("hd3", "un40", "un80", "hd2")]
    + [_r("envelope.test_gradients", t, 3) for t in ("hd6", "hd40", "hd112", "hd136", "st36", "st72")]
    + [_r("envelope.test_gradients", "d512x288", 2)]
    + [_r("envelope.test_sharp_attention", t, 7) for t in ("g5x37", "k6")]
    + [_r("splits.test_splits", "k6", 7, n) for n in (7, 3, 2, 1)]
    + [_r("splits.test_splits", "hd1", 7, n) for n in (7, 1)]
    + [_r("splits.test_splits", "g64x1024", 3, n) for n in (3, 2, 1)]
    + [_r("splits.test_splits", "hd96s", 5, n) for n in (5, 2)]
    + [_r("calls.test_call_sequence", t, B, n) for t in ("g5x37", "hd24") for B, n in ((7, 7), (2, 2), (7, 3), (9, 9), (1, 1))]
    + [_r("calls.test_stream", t, 7, steps=s) for t in ("g5x37", "hd24") for s in (False, True)]
    + [_r("calls.test_interleaved_gradients", t, B, steps=s) for t in ("g5x37", "hd24") for B, s in ((8, True), (3, False))]
    + [_r("calls.test_two_trainers", t, 8, steps=True) for t in ("g5x37", "hd24")]
    + [_r("calls.test_forward_consistency", t, 8, steps=s) for t in ("g5x37", "hd24") for s in (True, False)]
    + [_r("steps.test_one_step_is_adam", "k9", 8, steps=True)]
    + [_r("steps.test_one_step_is_adam", t, 2, steps=True) for t in ("d128", "hd40", "d512")]
    + [_r("steps.test_trajectory", "k9", 8, steps=True), _r("steps.test_trajectory", "g5x37", 16, steps=True)]
    + [_r("steps.test_scheduled_trajectory", "g5x37", B, steps=True) for B in (20, 8)]
)
