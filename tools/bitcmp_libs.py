"""Are two builds of the library bit-identical?  python tools/bitcmp_libs.py libA.so libB.so [case ...]
Each library is loaded in a process of its own (S2S_HIP_LIB), runs every case and prints one hash per output; the parent
compares them line by line and ends with IDENTICAL or DIFFERENT (exit status 0 / 1).  A case is
  a mode alone ("f16x3", the default without cases): the shipped checkpoint, predict_chunks on 6,000 chunks, signal + dur;
  tag:mode[:B]: case `tag` of tests/_envelope_models.py (envelope_state_dict / envelope_config) on B chunks (default 37; "slice+13":
    the generic workspace's slice_max + 13, the slice loop entered twice):
    (a) predict_chunks with the built-in samplers, seed 42: signal, dur;
    (b) evaluate_chunks on seeded teacher inputs: loss, y, sigma, conc, rate;
    (c) mode generic-geometry, B not "slice+13": Trainer.gradients, then two Trainer.step calls and Trainer.weights, at 7 chunks
        under the budget that splits them into micro-batches of 3, 3 and 1 (tests/_train_classes.budget_for): the tape carved
        more than once.
  "seam": the cases that between them take every branch of the generic launch side (s2s_generic_host.h)."""
import hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRY = ("generic-geometry", "generic-geometry-f16")
SEAM = ([f"hd64:{m}" for m in ("generic", "generic-f16") + GEOMETRY]            # short staged, the f16 250-key instance, one pre-net layer
        + [f"{t}:{m}" for t in ("hd24",                                         # the f16 any-T instance at 255 keys, two pre-net layers
                                "un40",                                         # short unstaged
                                "hd96s",                                        # staged encoder, unstaged decoder, 4 / 4 / 4 layers
                                "hd6", "hd40", "hd136",                         # long <1>, <8>, <32>
                                "hd1")                                          # one row per chunk, no pre-net
           for m in GEOMETRY]
        + ["hd208:generic-geometry:slice+13"])


def sha(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def shipped(mode):
    import numpy as np, torch
    import seq2squiggle_amd as S
    sd, cfg = S.load_checkpoint(os.path.join(ROOT, "tests", "golden", "synthetic_k9.ckpt"))
    eng = S.Engine(sd, cfg, mode=mode)
    rng = np.random.default_rng(7)
    reads = ["".join(rng.choice(list("ACGT"), int(n))) for n in rng.integers(9, 3000, size=70)]
    bases, nv, _ = S.encode_reads(reads, 9)
    out = eng.predict_chunks(torch.from_numpy(bases).cuda(), torch.from_numpy(nv).cuda(), S.PredictParams(seed=42))
    print("HASH", mode, f"predict[{bases.shape[0]}]", sha(out["signal"], out["dur"]), flush=True)
    eng.close()


def envelope(case):
    import numpy as np, torch
    import seq2squiggle_amd as S
    from seq2squiggle_amd import train as T
    import _envelope_models as EM
    import _train_classes as TC
    tag, mode, size = (case.split(":") + ["37"])[:3]
    sd, cfg = EM.envelope_state_dict(tag), EM.envelope_config(tag)
    k, te, ts = (int(cfg[n]) for n in ("seq_kmer", "max_dna_len", "max_signal_len"))
    B = TC.slice_max(cfg) + 13 if size == "slice+13" else int(size)
    rng = np.random.default_rng(11)
    letters = np.frombuffer(b"ACGT", np.uint8)
    bases = letters[rng.integers(0, 4, (B, te + k - 1))]
    nv = np.full(B, te, np.uint8)
    nv[::7] = rng.integers(1, te + 1, len(nv[::7]))                            # every 7th chunk short
    teacher = [letters[rng.integers(0, 4, (B, te, k))], rng.poisson(ts / te, (B, te)).astype(np.int32),
               rng.random((B, ts), np.float32), rng.random((B, te), np.float32) * 0.02]      # kmers, dwell, target, stdev
    eng = S.Engine(sd, cfg, mode=mode)
    dev = eng.device
    out = eng.predict_chunks(torch.from_numpy(bases).to(dev), torch.from_numpy(nv).to(dev), S.PredictParams(seed=42))
    for n in ("signal", "dur"):
        print("HASH", case, f"predict[{B}].{n}", sha(out[n]), flush=True)
    teacher = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in teacher]
    out = eng.evaluate_chunks(*teacher, want_y=True, debug=True)
    for n in ("loss", "y", "sigma", "conc", "rate"):
        print("HASH", case, f"evaluate[{B}].{n}", sha(out[n]), flush=True)
    eng.close()
    if mode != "generic-geometry" or size == "slice+13":
        return
    tr = T.Trainer(sd, cfg, 0)
    tr.set_memory(TC.budget_for(cfg, 7, 3))
    assert TC.split(7, tr.micro_batch(7)) == [3, 3, 1]
    batch = [t[:7].contiguous() for t in teacher]
    out = tr.gradients(*batch)
    for n in ("loss", "grad"):
        print("HASH", case, f"gradients[3,3,1].{n}", sha(out[n]), flush=True)
    stats = [tr.step(*batch, lr=1e-3, step=i, clip=1.0).clone() for i in (1, 2)]
    print("HASH", case, "step,step.stats", sha(*stats), flush=True)
    print("HASH", case, "step,step.weights", sha(tr.weights()), flush=True)
    tr.close()


if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    for case in sys.argv[2:]:
        (envelope if ":" in case else shipped)(case)
    sys.exit(0)

cases = [c for a in (sys.argv[3:] or ["f16x3"]) for c in (SEAM if a == "seam" else [a])]
res = []
for lib in sys.argv[1:3]:
    r = subprocess.run([sys.executable, __file__, "--child", *cases], env=dict(os.environ, S2S_HIP_LIB=os.path.abspath(lib)),
                       capture_output=True, text=True)
    res.append([l.split(" ", 1)[1] for l in r.stdout.splitlines() if l.startswith("HASH ")])
    if r.returncode:                          # nothing more is started on a GPU that a library may have faulted
        print(f"FAILED in {lib} (exit status {r.returncode}) after {len(res[-1])} outputs: {r.stderr[-600:]}")
        sys.exit(2)
same = True
for i in range(max(len(res[0]), len(res[1]))):
    a, b = (r[i] if i < len(r) else "(missing)" for r in res)
    ok = a == b and not a.startswith("FAILED") and a != "(missing)"
    same &= ok
    print("IDENTICAL" if ok else "DIFFERENT", a if ok else f"{a} | {b}")
same &= bool(res[0])
print("IDENTICAL" if same else "DIFFERENT")
sys.exit(0 if same else 1)
