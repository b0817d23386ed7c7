#!/usr/bin/env python
"""Golden vectors for model sizes outside the shipped family, by IMPORTING the reference (build container only).

Like tools/make_goldens.py (whose stubs and helpers it reuses), for the size cases of tests/_sized_models.py: the case's weights
(a seeded recipe there -- a d512 checkpoint is too large to keep in the repository, so the tests rebuild the checkpoints from the
same recipe) are loaded into the reference's own seq2squiggle(config=...), and its stage outputs and predict_step signals with
injected standard-gamma / normal draws are recorded (make_goldens.stage_goldens) as tests/golden/sized_<tag>.npz, together with
the SHA-256 of the weight blob they were made with.  The existing fixtures are not touched.

    python tools/make_sized_goldens.py [tag ...]
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_goldens as MG      # noqa: E402  (stubs the reference's third-party imports, imports the reference)
import _sized_models as SM     # noqa: E402

READS = {"d512": 2}            # the first two reads only: keeps the d512 fixture small


def main():
    tags = sys.argv[1:] or list(SM.CASES)
    reads = MG.read_fasta(os.path.join(MG.REF, "example/test.fasta"))
    rng = np.random.default_rng(5)
    reads_x = reads + [("".join(rng.choice(list("ACGTN"), 150, p=[.24, .24, .24, .24, .04])), "rand150_with_N")]
    out_dir = MG.OUT
    for tag in tags:
        cfg = SM.sized_config(tag, MG.base_config(SM.CASES[tag]["seq_kmer"]))
        sd = SM.sized_state_dict(tag)
        m = MG.RM.seq2squiggle(config=cfg)
        m.load_state_dict(sd, strict=True)
        m.eval()
        with tempfile.TemporaryDirectory() as tmp:
            MG.OUT = tmp                        # stage_goldens writes stages_<tag>.npz into MG.OUT
            with torch.no_grad():
                MG.stage_goldens(tag, m, cfg, reads_x[:READS[tag]] if tag in READS else reads_x, seed=100 + SM.CASES[tag]["seed"])
            g = dict(np.load(os.path.join(tmp, f"stages_{tag}.npz"), allow_pickle=False))
            MG.OUT = out_dir
        g["weights_sha256"] = np.array(SM.weights_sha256(sd, cfg))
        path = os.path.join(out_dir, f"sized_{tag}.npz")
        np.savez_compressed(path, **g)
        print(tag, "npz bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
