#!/usr/bin/env python
"""Golden vectors at chunk geometries other than 16 / 250, by IMPORTING the reference (build container only).

For the cases of tests/_geometry_models.py: the case's weights are loaded into the reference's own seq2squiggle(config=...) -- whose
Encoder, Decoder, length regulator and predict_step then run at the case's max_dna_len / max_signal_len -- and recorded as
tests/golden/geometry_<tag>.npz:
  codes, n_valid, names       the reference's split_sequence at that max_dna_len (utils.py:350-356), per chunk
  emb_out .. rate, g          stage outputs (Encoder, NoiseSampler, DurationSampler with injected standard-gamma draws)
  dur_gamma, y_scaled_gamma   the length regulator at max_length = max_signal_len and the Decoder on its output
  y_*                         predict_step signals with injected gamma / normal / z01 draws (make_goldens.stage_goldens' modes,
                              with its crop and floor stress rows scaled to the case's geometry)
  export_pa, export_offsets   export_and_clear_results' zero-stripped signal per read (y_gamma_nsamp's draws), read order
  weights_sha256              of the weight blob the vectors were made with.
The injected normals are fp16-representable (stored as float16) to keep the fixtures small.  make_goldens.py is not changed.

    python tools/make_geometry_goldens.py [tag ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_goldens as MG        # noqa: E402  (stubs the reference's third-party imports, imports the reference)
import _geometry_models as GM    # noqa: E402


def case_reads(tag):
    reads = MG.read_fasta(os.path.join(MG.REF, "example/test.fasta"))
    rng = np.random.default_rng(5)
    rand = ("".join(rng.choice(list("ACGTN"), 150, p=[.24, .24, .24, .24, .04])), "rand150_with_N")
    if tag == "d512x288":                  # two short reads: the dmodel-512 stage vectors are large
        return [(reads[0][0][:20], reads[0][1]), (rand[0][:30], rand[1])]
    n = {"r16x500": 1, "g12x300": 2, "g5x37": 7, "g64x1024": 2}[tag]
    return reads[:n] + [rand]


def record(tag, m, cfg, reads, seed):
    te, ts = cfg["max_dna_len"], cfg["max_signal_len"]
    names, chunks = [], []
    for seq, name in reads:
        for c in MG.RU.split_sequence(seq, cfg):
            names.append(name)
            chunks.append(c)
    x = np.stack(chunks)                                  # [B,te,k,5] fp16
    B = x.shape[0]
    codes = MG.codes_from_onehot(x)
    x16 = torch.from_numpy(x)
    nvalid = (~(codes == 0).all(-1)).sum(-1).astype(np.uint8)     # the pad k-mers ("_" * k, add_remainder) trail the chunk
    g = {"codes": codes, "n_valid": nvalid, "names": np.array(names)}

    data = x16.reshape(B, te, -1)
    enc_out, emb_out = m.encoders(data)
    sigma = m.noise_sampler(emb_out)
    ds = m.length_regulator.duration_sampler
    conc = torch.clamp(ds.conc_layer(emb_out), min=1e-8)
    rate = torch.clamp(ds.rate_layer(emb_out), min=1e-8)
    g.update(emb_out=emb_out.numpy(), enc_out=enc_out.numpy(), sigma=sigma.numpy(), conc=conc.flatten(1).numpy(),
             rate=rate.flatten(1).numpy())

    gen = torch.Generator().manual_seed(seed)
    sg = torch._standard_gamma(conc, generator=gen)
    sg[1] *= max(2.5, 1.5 * ts / (11.0 * te))            # crop: sum(dur) > max_signal_len
    sg[2] *= 0.05                                         # clamp(1.0) / min_duration floor
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
    common = dict(dwell_mean=12.5, dwell_std=0.0, min_duration=3)
    with MG.Inject(sg=sg, z_normal=[z]):
        g["y_gamma_nsamp"] = MG.run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True, duration_sampling=True,
                                                 min_noise=0.0, **common).numpy()
    with MG.Inject(sg=sg, z_normal=[z]):
        g["y_gamma_nconst"] = MG.run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=False, duration_sampling=True,
                                                  min_noise=0.0, **common).numpy()
    g["y_ideal"] = MG.run_predict_step(m, names, x16, noise_std=0.0, noise_sampling=False, duration_sampling=False, min_noise=0.0,
                                       **common).numpy()
    with MG.Inject(z_normal=[zdw, z]):
        g["y_normal_nsamp"] = MG.run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True, duration_sampling=False,
                                                  min_noise=0.0, dwell_mean=12.5, dwell_std=4.0, min_duration=3).numpy()
    g["dur_normal"] = torch.round(torch.clamp(torch.full((B, te), 12.5) + zdw * torch.full((B, te), 4.0), min=3)).int().numpy()
    g["y_ideal_dwell31"] = MG.run_predict_step(m, names, x16, noise_std=0.0, noise_sampling=False, duration_sampling=False,
                                               min_noise=0.0, dwell_mean=4000 / 130, dwell_std=0.0, min_duration=3).numpy()
    # export_and_clear_results (model.py:253-302) after one predict_step of the y_gamma_nsamp draws
    fw = MG.FakeWriter()
    for k_, v in dict(noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, **common).items():
        setattr(m, k_, v)
    m.results, m.total_samples, m.out_writer = [], 0, fw
    with MG.Inject(sg=sg, z_normal=[z]):
        m.predict_step((tuple(names), x16))
    m.on_predict_epoch_end()
    order = list(fw.saved[0].keys())
    sigs = [fw.saved[0][r].numpy() for r in order]
    g["export_reads"] = np.array(order)
    g["export_offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    g["export_pa"] = np.concatenate(sigs).astype(np.float32)
    print(tag, "chunks", B, "dur_gamma sums", int(g["dur_gamma"].sum(1).min()), int(g["dur_gamma"].sum(1).max()), "ts", ts,
          "zeros in y_ideal", int((g["y_ideal"] == 0).sum()))
    return g


def main():
    tags = sys.argv[1:] or list(GM.CASES)
    for tag in tags:
        cfg = GM.geometry_config(tag, MG.base_config(GM.CASES[tag]["seq_kmer"]))
        cfg.update({k: v for k, v in GM.CASES[tag].items() if k != "seed"})
        sd = GM.geometry_state_dict(tag)
        m = MG.RM.seq2squiggle(config=cfg)
        m.load_state_dict(sd, strict=True)
        m.eval()
        with torch.no_grad():
            g = record(tag, m, cfg, case_reads(tag), seed=200 + GM.CASES[tag]["seed"])
        g["weights_sha256"] = np.array(GM.weights_sha256(sd, cfg))
        path = os.path.join(MG.OUT, f"geometry_{tag}.npz")
        np.savez_compressed(path, **g)
        print(tag, "npz bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
