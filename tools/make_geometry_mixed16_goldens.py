#!/usr/bin/env python
"""The reference's 16-mixed arithmetic at the chunk geometries of tests/_geometry_models.py, by IMPORTING the reference (build
container only).

tools/make_sized_mixed16_goldens.py records what the reference's own GPU path (inference.py:403-404: Lightning "16-mixed" whenever a
GPU is present) gives at the model-size cases.  This does the same for the geometry cases: each case's weights (the seeded recipe of
tests/_geometry_models.py) are loaded into the reference's seq2squiggle(config=...), the fp32 run is checked to reproduce
tests/golden/geometry_<tag>.npz's y_gamma_nsamp bit for bit, and predict_step runs under torch.autocast("cpu", dtype=torch.float16)
on that file's chunks with the same injected standard-gamma and normal variates, the length regulator at max_length =
max_signal_len.  -> tests/golden/geometry_mixed16.npz, with the keys of sized_mixed16.npz: per case the 16-mixed signal rows, the
dwell indices under 16-mixed, their distance to the fp32 golden (all chunks, and the chunks whose dwell indices agree with fp32's)
and the weights' SHA-256.  The bar the opt-in reduced-precision geometry mode (S2S_MODE_GENERIC_GEOMETRY_F16) is held to
(tests/test_gpu_geometry_f16.py).  The existing fixtures are not touched.

    python tools/make_geometry_mixed16_goldens.py
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


def mixed16(tag):
    cfg = GM.geometry_config(tag, MG.base_config(GM.CASES[tag]["seq_kmer"]))
    sd = GM.geometry_state_dict(tag)
    g = dict(np.load(os.path.join(MG.OUT, f"geometry_{tag}.npz"), allow_pickle=False))
    sha = GM.weights_sha256(sd, cfg)
    assert sha == str(g["weights_sha256"]), tag
    te, ts = cfg["max_dna_len"], cfg["max_signal_len"]
    m = MG.RM.seq2squiggle(config=cfg)
    m.load_state_dict(sd, strict=True)
    m.eval()
    codes = g["codes"]
    x = np.zeros(codes.shape + (5,), np.float16)
    known = codes < 5
    x[known] = np.eye(5, dtype=np.float16)[codes[known]]
    x16 = torch.from_numpy(x)
    names = [str(n) for n in g["names"]]
    B = len(names)
    sg = torch.from_numpy(g["sg"]).reshape(B, te, 1)
    z = torch.from_numpy(g["z01"].astype(np.float32))
    kw = dict(noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, dwell_mean=12.5, dwell_std=0.0, min_duration=3)
    with torch.no_grad():
        with MG.Inject(sg=sg, z_normal=[z]):          # sanity: the fp32 run reproduces the committed golden bit for bit
            y32 = MG.run_predict_step(m, names, x16, **kw)
        assert np.array_equal(y32.numpy(), g["y_gamma_nsamp"]), tag
        with torch.autocast("cpu", dtype=torch.float16):
            with MG.Inject(sg=sg, z_normal=[z]):
                y16 = MG.run_predict_step(m, names, x16, **kw).float()
            enc_out, emb_out = m.encoders(x16.reshape(B, te, -1))
            sigma = m.noise_sampler(emb_out)
            with MG.Inject(sg=sg):
                _, dpo, _, _, _ = m.length_regulator(emb_out=emb_out, x=enc_out, target=None, noise_std_prediction=sigma[:, :, None],
                                                     max_length=ts, dwell_mean=12.5, dwell_std=0.0, duration_sampling=True, min_length=3)
    d = (y16 - y32).abs()
    same = (y16 == 0) == (y32 == 0)
    dur16 = torch.round(dpo.float()).int().numpy()
    # a dwell index that rounds the other way under fp16 shifts every later sample of its chunk: the distance on the chunks whose
    # indices all agree is the arithmetic's own
    agree = torch.from_numpy((dur16 == g["dur_gamma"]).all(1))
    out = {f"y_gamma_nsamp_16mixed_{tag}": y16.numpy(), f"dur_gamma_16mixed_{tag}": dur16,
           f"mae_vs_fp32_{tag}": np.float64(d.mean()), f"max_vs_fp32_{tag}": np.float64(d.max()),
           f"zero_pattern_equal_share_{tag}": np.float64(same.float().mean()),
           f"dwell_indices_differing_{tag}": np.int64((dur16 != g["dur_gamma"]).sum()),
           f"mae_vs_fp32_where_dwell_equal_{tag}": np.float64(d[agree].mean()),
           f"max_vs_fp32_where_dwell_equal_{tag}": np.float64(d[agree].max()),
           f"weights_sha256_{tag}": np.array(sha)}
    print(tag, "dwell indices differing:", int(out[f"dwell_indices_differing_{tag}"]), "of", dur16.size, "| on the", int(agree.sum()),
          "of", B, "chunks whose indices agree: MAE", float(d[agree].mean()), "max", float(d[agree].max()),
          "| all chunks: MAE", float(d.mean()), "max", float(d.max()), "zero pattern equal", float(same.float().mean()))
    return out


def main():
    out = {}
    for tag in GM.CASES:
        out.update(mixed16(tag))
    path = os.path.join(MG.OUT, "geometry_mixed16.npz")
    np.savez_compressed(path, **out)
    print("npz bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
