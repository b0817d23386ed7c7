#!/usr/bin/env python
"""Golden vectors across the generic modes' size and geometry envelope, by IMPORTING the reference (build container only).

For the cases of tests/_envelope_models.py: the case's weights (the seeded recipe of tests/_geometry_models.py) are loaded into the
reference's own seq2squiggle(config=...) and recorded as tests/golden/envelope_<tag>.npz:
  codes, n_valid, names        the reference's split_sequence at the case's max_dna_len, per chunk: a read of k bases (n_valid 1), one
                               of k + max_dna_len - 1 (one full chunk), one of k + max_dna_len, an N-bearing read, example/test.fasta
                               material; at most MAX_CHUNKS[tag] <= 24 chunks
  emb_out .. rate, sg, g       stage outputs with injected standard-gamma draws, scaled per chunk so that sum(dwell) lands on both
                               sides of max_signal_len (row 1 far beyond it: the crop; row 2 on the min_duration floor)
  dur_gamma, y_scaled_gamma    the length regulator at max_length = max_signal_len and the Decoder on its output
  y_gamma_nsamp, y_gamma_nconst, y_ideal, y_normal_nsamp, dur_normal     predict_step with injected gamma / normal / z01 draws
  weights_sha256               of the weight blob the vectors were made with
and tests/golden/envelope_mixed16.npz, the keys of geometry_mixed16.npz: predict_step under torch.autocast("cpu", dtype=float16)
on the same chunks and variates (the reference's GPU arithmetic class), the bar of the f16 modes.  The archives are written with a
fixed member date, so a second run gives the same bytes.

    python tools/make_envelope_goldens.py [tag ...]      (with tags: those cases only, envelope_mixed16.npz is not rewritten)
"""
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_goldens as MG        # noqa: E402  (stubs the reference's third-party imports, imports the reference)
import _envelope_models as EM    # noqa: E402

# chunks per case: the stage tensors are [B][max_dna_len][dmodel] fp32, the signals [B][max_signal_len]
MAX_CHUNKS = {"hd1": 24, "hd3": 12, "hd40": 7, "hd112": 7, "hd208": 6, "hd96s": 6, "hd64": 8, "hd24": 8, "st36": 8, "un40": 8,
              "st72": 8, "un80": 8, "hd136": 7, "hd6": 7, "d512": 8}
KW = dict(noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, dwell_mean=12.5, dwell_std=0.0, min_duration=3)


def save_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def case_reads(tag, cfg, fasta):
    """The reads of case `tag` (tests/test_envelope_cpu.py restates this against tests/golden/example_test.fasta)."""
    k, te = cfg["seq_kmer"], cfg["max_dna_len"]
    rng = np.random.default_rng(5)
    rand = list(rng.choice(list("ACGT"), k + te + te // 2))
    rand[len(rand) // 2] = "N"
    reads = [(fasta[0][0][:k], "len_k"), (fasta[1][0][:k + te - 1], "one_full_chunk"), (fasta[2][0][:k + te], "one_chunk_and_one"),
             ("".join(rand), "rand_with_N")]
    left = MAX_CHUNKS[tag] - sum(-(-(len(s) - k + 1) // te) for s, _ in reads)
    for seq, name in fasta[3:]:
        if left <= 0:
            break
        n = min(left, -(-(len(seq) - k + 1) // te))
        # n chunks, the last one short of full where max_dna_len allows it
        reads.append((seq[:min(len(seq), k - 1 + n * te - te // 3)], name))
        left -= n
    return reads


def record(tag, m, cfg, reads, seed):
    te, ts = cfg["max_dna_len"], cfg["max_signal_len"]
    names, chunks = [], []
    for seq, name in reads:
        for c in MG.RU.split_sequence(seq, cfg):
            names.append(name)
            chunks.append(c)
    x = np.stack(chunks)                                  # [B,te,k,5] fp16
    B = x.shape[0]
    assert B <= MAX_CHUNKS[tag] <= 24, (tag, B)
    codes = MG.codes_from_onehot(x)
    x16 = torch.from_numpy(x)
    nvalid = (~(codes == 0).all(-1)).sum(-1).astype(np.uint8)     # the pad k-mers ("_" * k, add_remainder) trail the chunk
    g = {"codes": codes, "n_valid": nvalid, "names": np.array(names)}

    enc_out, emb_out = m.encoders(x16.reshape(B, te, -1))
    sigma = m.noise_sampler(emb_out)
    ds = m.length_regulator.duration_sampler
    conc = torch.clamp(ds.conc_layer(emb_out), min=1e-8)
    rate = torch.clamp(ds.rate_layer(emb_out), min=1e-8)
    g.update(emb_out=emb_out.numpy(), enc_out=enc_out.numpy(), sigma=sigma.numpy(), conc=conc.flatten(1).numpy(),
             rate=rate.flatten(1).numpy())

    gen = torch.Generator().manual_seed(seed)
    sg = torch._standard_gamma(conc, generator=gen)
    # the recipe's dwell is ~11 samples per k-mer: scale each chunk's draws to 0.4 .. 1.8 x max_signal_len in all
    u = 0.4 + 1.4 * torch.rand(B, generator=gen)
    sg *= (u * ts / (11.0 * te))[:, None, None]
    sg[1] *= 2.5                                          # crop: sum(dur) > max_signal_len
    sg[2] *= 0.05 / float(u[2] * ts / (11.0 * te))        # clamp(1.0) / min_duration floor
    z = torch.randn(B, ts, generator=gen).half().float()
    zdw = torch.randn(B, te, generator=gen).half().float()
    g.update(sg=sg.flatten(1).numpy(), z01=z.numpy().astype(np.float16), zdw=zdw.numpy().astype(np.float16))

    with MG.Inject(sg=sg):
        g_samp, _ = ds(emb_out)
    g["g"] = g_samp.numpy()
    with MG.Inject(sg=sg):
        lr_out, dpo, _, _, _ = m.length_regulator(emb_out=emb_out, x=enc_out, target=None, noise_std_prediction=sigma[:, :, None],
                                                  max_length=ts, dwell_mean=12.5, dwell_std=0.0, duration_sampling=True,
                                                  min_length=3)
    g["dur_gamma"] = torch.round(dpo).int().numpy()
    g["y_scaled_gamma"] = m.decoders(lr_out, None).squeeze(-1).numpy()
    with MG.Inject(sg=sg, z_normal=[z]):
        g["y_gamma_nsamp"] = MG.run_predict_step(m, names, x16, **KW).numpy()
    with MG.Inject(sg=sg, z_normal=[z]):
        g["y_gamma_nconst"] = MG.run_predict_step(m, names, x16, **dict(KW, noise_sampling=False)).numpy()
    g["y_ideal"] = MG.run_predict_step(m, names, x16, **dict(KW, noise_std=0.0, noise_sampling=False, duration_sampling=False)).numpy()
    with MG.Inject(z_normal=[zdw, z]):
        g["y_normal_nsamp"] = MG.run_predict_step(m, names, x16, **dict(KW, duration_sampling=False, dwell_std=4.0)).numpy()
    g["dur_normal"] = torch.round(torch.clamp(torch.full((B, te), 12.5) + zdw * torch.full((B, te), 4.0), min=3)).int().numpy()

    # the reference's 16-mixed arithmetic on the same chunks and variates (tools/make_geometry_mixed16_goldens.py)
    with torch.autocast("cpu", dtype=torch.float16):
        with MG.Inject(sg=sg, z_normal=[z]):
            y16 = MG.run_predict_step(m, names, x16, **KW).float()
        enc16, emb16 = m.encoders(x16.reshape(B, te, -1))
        sigma16 = m.noise_sampler(emb16)
        with MG.Inject(sg=sg):
            _, dpo16, _, _, _ = m.length_regulator(emb_out=emb16, x=enc16, target=None, noise_std_prediction=sigma16[:, :, None],
                                                   max_length=ts, dwell_mean=12.5, dwell_std=0.0, duration_sampling=True, min_length=3)
    y32 = torch.from_numpy(g["y_gamma_nsamp"])
    d = (y16 - y32).abs()
    same = (y16 == 0) == (y32 == 0)
    dur16 = torch.round(dpo16.float()).int().numpy()
    # a dwell index that rounds the other way under fp16 shifts every later sample of its chunk: the distance on the chunks whose
    # indices all agree is the arithmetic's own
    agree = torch.from_numpy((dur16 == g["dur_gamma"]).all(1))
    m16 = {f"y_gamma_nsamp_16mixed_{tag}": y16.numpy(), f"dur_gamma_16mixed_{tag}": dur16,
           f"mae_vs_fp32_{tag}": np.float64(d.mean()), f"max_vs_fp32_{tag}": np.float64(d.max()),
           f"zero_pattern_equal_share_{tag}": np.float64(same.float().mean()),
           f"dwell_indices_differing_{tag}": np.int64((dur16 != g["dur_gamma"]).sum()),
           f"mae_vs_fp32_where_dwell_equal_{tag}": np.float64(d[agree].mean()),
           f"max_vs_fp32_where_dwell_equal_{tag}": np.float64(d[agree].max())}
    sums = g["dur_gamma"].sum(1)
    print(tag, "chunks", B, "n_valid", sorted(set(nvalid.tolist())), "| sum(dur_gamma)", int(sums.min()), "..", int(sums.max()), "ts", ts,
          "| non-zero share", " ".join(f"{(g[k_] != 0).mean():.2f}" for k_ in ("y_gamma_nsamp", "y_gamma_nconst", "y_ideal", "y_normal_nsamp")),
          "| 16-mixed: dwell differing", int((dur16 != g["dur_gamma"]).sum()), "agreeing chunks", int(agree.sum()),
          f"MAE {float(d[agree].mean()):.4f} max {float(d[agree].max()):.3f} zero pattern equal {float(same.float().mean()):.4f}")
    return g, m16


def main():
    tags = sys.argv[1:] or list(EM.CASES)
    fasta = MG.read_fasta(os.path.join(MG.REF, "example/test.fasta"))
    mixed, total = {}, 0
    for tag in tags:
        cfg = EM.envelope_config(tag, MG.base_config(EM.CASES[tag]["seq_kmer"]))
        sd = EM.envelope_state_dict(tag)
        m = MG.RM.seq2squiggle(config=cfg)
        m.load_state_dict(sd, strict=True)
        m.eval()
        with torch.no_grad():
            g, m16 = record(tag, m, cfg, case_reads(tag, cfg, fasta), seed=300 + EM.CASES[tag]["seed"])
        sha = EM.weights_sha256(sd, cfg)
        g["weights_sha256"] = np.array(sha)
        m16[f"weights_sha256_{tag}"] = np.array(sha)
        mixed.update(m16)
        path = os.path.join(MG.OUT, f"envelope_{tag}.npz")
        save_npz(path, g)
        total += os.path.getsize(path)
        print(tag, "npz bytes", os.path.getsize(path))
    if tags == list(EM.CASES):
        path = os.path.join(MG.OUT, "envelope_mixed16.npz")
        save_npz(path, mixed)
        total += os.path.getsize(path)
        print("envelope_mixed16.npz bytes", os.path.getsize(path))
    print("total bytes", total)


if __name__ == "__main__":
    main()
