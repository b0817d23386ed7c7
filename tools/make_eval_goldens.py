#!/usr/bin/env python
"""Teacher-forced validation goldens, by IMPORTING the reference (build container only).

For the committed synthetic k9 / k6 checkpoints, d32 (tests/_sized_models.py), r16x500, g5x37 and g64x1024 (tests/_geometry_models.py)
and hd1, hd24, hd64, hd96s and hd208 (tests/_envelope_models.py: te 1 / 23 / 16 / 64 / 17, ts 1 / 255 / 250 / 251 / 1023, seq_kmer 6 / 16 /
1 / 6 / 9, hd96s with 4 / 4 / 4 layers -- every row shape of the teacher-forced generic kernels and of the loss kernel) a seeded
dataset in the reference's preprocess layout is run through the reference's own seq2squiggle.validation_step (model.py:107-193,
get_loss :419-480) with self.log captured.  -> tests/golden/eval_<tag>.npz, stored compactly (the tests rebuild the .npy files):

  codes uint8 [N,te,k]    letter codes 0-4 ("_ACGT"), 5 = an all-zero one-hot row
  lengths int16 [N,te]    chunks_lengths: measured samples per k-mer
  targets fp16 [N,ts]     pA (fp16-representable values; the .npy the tests write holds them as float32)
  stdevs fp32 [N,te]      pA
  kind uint8 [N]          0 fit, 1 random target, 2 edge case
  prediction_ref [N,ts], sigma / conc / rate [N,te]   the reference's first-pass tensors (scaled units)
  y16_mae_pa, y16_max_pa  the distance of the same pass under 16-mixed precision to prediction_ref, in pA
  per_chunk16 fp64 [N,3]  per_chunk from the 16-mixed run's first-pass tensors
  per_chunk fp64 [N,3]    sum (y - t)^2, sum -log_prob(|d| + (d == 0)), sum (stdev - sigma)^2 from those tensors
  logged_bs<B> fp64 [4]   the epoch value of valid_signal / duration / noise / total_loss at batch size B: the batch-size weighted
                          mean of the per-batch logged values (Lightning's on-epoch reduction)
  logged16_bs<B> fp64 [4] the same under torch.autocast("cpu", dtype=torch.float16) (the reference's 16-mixed precision class)

Chunk kinds: "fit" chunks, whose targets are the reference's own teacher-forced prediction x scaling + N(0, 2 pA); random targets;
edge cases: dwell sums below, at and above ts (the crop), a zero-length k-mer, trailing "_"*k pad k-mers with length 1 and stdev 0
(as process_df writes them), an unknown-letter row, an all-pad chunk.  Where te < 4 the k-mer positions of these recipes are clipped
into the chunk (fewer zero-length and pad k-mers; none at te 1).  The cases added after the first four also hold a stalled k-mer: one
dwell of 32767, the top of the preprocess files' int16 range, in the middle of the last random-target chunk (marked kind 2).

    python tools/make_eval_goldens.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_goldens as MG      # noqa: E402  (stubs the reference's third-party imports, imports the reference)
import _sized_models as SM     # noqa: E402
import _geometry_models as GM  # noqa: E402
import _envelope_models as EM  # noqa: E402

LOSSES = ("valid_signal_loss", "valid_duration_loss", "valid_noise_loss", "valid_total_loss")
N_CHUNKS = {"k9": 96, "k6": 96, "d32": 96, "r16x500": 64, "hd1": 48, "g5x37": 48, "hd24": 36, "hd64": 48, "hd96s": 36, "g64x1024": 30,
            "hd208": 30}
SEEDS = {"k9": 901, "k6": 902, "d32": 903, "r16x500": 904, "hd1": 905, "g5x37": 906, "hd24": 907, "hd64": 908, "hd96s": 909,
         "g64x1024": 910, "hd208": 911}
STALLED = ("hd1", "g5x37", "hd24", "hd64", "hd96s", "g64x1024", "hd208")       # cases with a dwell-32767 chunk
BATCHES = (32, 96)


def case(tag):
    """-> (config, state_dict) of case `tag`."""
    from seq2squiggle_amd.checkpoint import load_checkpoint
    if tag in ("k9", "k6"):
        sd, cfg = load_checkpoint(os.path.join(MG.OUT, f"synthetic_{tag}.ckpt"))
        return cfg, sd
    if tag == "d32":
        return SM.sized_config(tag, MG.base_config(SM.CASES[tag]["seq_kmer"])), SM.sized_state_dict(tag)
    if tag in EM.CASES:
        return EM.envelope_config(tag, MG.base_config(EM.CASES[tag]["seq_kmer"])), EM.envelope_state_dict(tag)
    return GM.geometry_config(tag, MG.base_config(GM.CASES[tag]["seq_kmer"])), GM.geometry_state_dict(tag)


def onehot(codes):
    x = np.zeros(codes.shape + (5,), np.float16)
    known = codes < 5
    x[known] = np.eye(5, dtype=np.float16)[codes[known]]
    return x


def run_reference(m, codes, lengths, targets, stdevs, scale, bs, fp16=False):
    """validation_step over the dataset in batches of bs -> the epoch losses [4]."""
    sums, N = np.zeros(4), codes.shape[0]
    grab = {}
    m.log = lambda name, value, **kw: grab.__setitem__(name, float(value))
    for i in range(0, N, bs):
        j = min(N, i + bs)
        # ChunkDataSetMemmap.__getitem__: float16 one-hot, targets[:, None] / scaling, stdevs / scaling, int16 lengths
        batch = (torch.from_numpy(onehot(codes[i:j])), torch.from_numpy((targets[i:j, :, None].astype(np.float32) / scale).astype(np.float32)),
                 torch.from_numpy(lengths[i:j].astype(np.int16)), torch.from_numpy(np.full(j - i, targets.shape[1], np.int16)),
                 torch.from_numpy((stdevs[i:j] / scale).astype(np.float32)))
        grab.clear()
        # (the second pass's Gamma draw feeds only the plots; torch has no fp16 CPU sampler: a fixed variate stands in)
        with torch.no_grad(), MG.Inject(sg=torch.full((j - i, codes.shape[1], 1), 5.0)):
            if fp16:
                with torch.autocast("cpu", dtype=torch.float16):
                    m.validation_step(batch, 1)
            else:
                m.validation_step(batch, 1)
        sums += (j - i) * np.array([grab[n] for n in LOSSES])
    return sums / N


def first_pass(m, codes, lengths, te, ts, fp16=False):
    """The first pass of validation_step (model.py:108-140): prediction_ref [N,ts], sigma / conc / rate [N,te] (fp16: under
    torch.autocast("cpu", dtype=torch.float16))."""
    import contextlib
    x = torch.from_numpy(onehot(codes))
    B = x.shape[0]
    with torch.no_grad(), MG.Inject(sg=torch.full((B, te, 1), 5.0)), \
            (torch.autocast("cpu", dtype=torch.float16) if fp16 else contextlib.nullcontext()):
        enc_out, emb_out = m.encoders(x.reshape(B, te, -1))
        sigma = m.noise_sampler(emb_out)[:, :, None]
        out, _, dist, _, _ = m.length_regulator(emb_out=emb_out, x=enc_out, target=torch.from_numpy(lengths.astype(np.int16)),
                                                noise_std_prediction=sigma, max_length=ts, min_length=1)
        y = m.decoders(out)[:, :, 0]
    return tuple(t.float().numpy() for t in (y, sigma[:, :, 0], dist.concentration[:, :, 0], dist.rate[:, :, 0]))


def build(tag):
    cfg, sd = case(tag)
    k, te, ts, scale = int(cfg["seq_kmer"]), int(cfg["max_dna_len"]), int(cfg["max_signal_len"]), float(cfg["scaling_max_value"])
    m = MG.RM.seq2squiggle(config=cfg)
    m.load_state_dict(sd, strict=True)
    m.eval()
    rng = np.random.default_rng(SEEDS[tag])
    N = N_CHUNKS[tag]
    codes = rng.integers(1, 5, (N, te, k)).astype(np.uint8)
    mean = ts / te
    lengths = np.clip(rng.poisson(mean, (N, te)), 0, None).astype(np.int16)
    kind = np.zeros(N, np.uint8)
    kind[N // 3:2 * N // 3] = 1
    kind[2 * N // 3:] = 2
    e = list(range(2 * N // 3, N))
    # edge cases
    lengths[e[0]] = np.full(te, max(1, ts // (2 * te)))                              # sum well below ts
    lengths[e[1]] = np.full(te, ts // te); lengths[e[1], -1] += ts - lengths[e[1]].sum()   # sum exactly ts
    lengths[e[2]] = np.full(te, 3 * ts // te)                                          # sum far above ts: cropped
    lengths[e[3], te // 2] = 0                                                          # a zero-length k-mer
    lengths[e[4], :3] = 0
    pad0 = te - min(4, te - 1)                                                          # (te < 4: fewer pad k-mers, none at te 1)
    for r in (e[5], e[6]):                                                              # trailing pad k-mers, length 1
        codes[r, pad0:] = 0
        lengths[r, pad0:] = 1
    codes[e[7], min(3, te - 1), k // 2] = 5                                                        # an unknown letter (all-zero row)
    codes[e[8], 0, 0] = 5
    codes[e[9]] = 0                                                                     # an all-pad chunk
    lengths[e[9]] = 1
    if tag in STALLED:                                                                  # a stalled k-mer: the top of the int16 range
        lengths[e[0] - 1, te // 2] = 32767
        kind[e[0] - 1] = 2
    y, sigma, conc, rate = first_pass(m, codes, lengths, te, ts)
    targets = np.empty((N, ts), np.float32)
    fit = kind == 0
    targets[fit] = y[fit] * scale + rng.normal(0.0, 2.0, (int(fit.sum()), ts))
    targets[~fit] = rng.uniform(60.0, 130.0, (int((~fit).sum()), ts))
    targets = np.clip(targets, 0.0, None).astype(np.float16)
    stdevs = (rng.uniform(0.5, 3.0, (N, te))).astype(np.float32)
    pads = codes.max(-1) == 0                                                           # pad k-mers: stdev 0 (process_df)
    stdevs[pads] = 0.0
    stdevs[e[9]] = 0.0
    t32 = targets.astype(np.float32) / scale
    s32 = stdevs / scale
    x = lengths.astype(np.float64)
    x = np.where(x == 0, 1.0, np.abs(x))

    def sums(y, sigma, conc, rate):
        from math import lgamma
        c64, r64 = conc.astype(np.float64), rate.astype(np.float64)
        nll = -(c64 * np.log(r64) + (c64 - 1) * np.log(x) - r64 * x - np.vectorize(lgamma)(c64))
        return np.stack([((y.astype(np.float64) - t32) ** 2).sum(1), nll.sum(1), ((s32.astype(np.float64) - sigma) ** 2).sum(1)], 1)
    per_chunk = sums(y, sigma, conc, rate)
    out = dict(codes=codes, lengths=lengths, targets=targets, stdevs=stdevs, kind=kind, prediction_ref=y.astype(np.float32),
               sigma=sigma.astype(np.float32), conc=conc.astype(np.float32), rate=rate.astype(np.float32), per_chunk=per_chunk)
    y16, sigma16, conc16, rate16 = first_pass(m, codes, lengths, te, ts, fp16=True)
    out["per_chunk16"] = sums(y16, sigma16, conc16, rate16)
    out["y16_mae_pa"] = np.float64(np.abs(y16.astype(np.float64) - y).mean() * scale)   # the 16-mixed run's distance to fp32, pA
    out["y16_max_pa"] = np.float64(np.abs(y16.astype(np.float64) - y).max() * scale)
    for bs in BATCHES:
        out[f"logged_bs{bs}"] = run_reference(m, codes, lengths, targets, stdevs, scale, bs)
        out[f"logged16_bs{bs}"] = run_reference(m, codes, lengths, targets, stdevs, scale, bs, fp16=True)
    fin = per_chunk.sum(0) / np.array([N * ts, N * te / 0.0005, N * te])
    print(tag, "logged", out["logged_bs32"], "16-mixed", out["logged16_bs32"], "from per-chunk", fin, fin.sum())
    return out


def main():
    for tag in (sys.argv[1:] or N_CHUNKS):
        out = build(tag)
        path = os.path.join(MG.OUT, f"eval_{tag}.npz")
        np.savez_compressed(path, **out)
        print(tag, "npz bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
