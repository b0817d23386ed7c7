#!/usr/bin/env python
"""Generate golden vectors by IMPORTING the reference (build container only).

Runs only where /root/reference exists.  It stubs the third-party modules the
reference imports but this image lacks, forces true-fp32
matmuls (the reference sets "medium" at import, model.py:22), builds synthetic
checkpoints in the Lightning .ckpt layout, and drives the reference's own
modules / predict_step / export / BLOW5Writer.save with *injected* random
variates.  Outputs (data only -- inputs and expected outputs) go to
tests/golden/.  Nothing of the reference's source text is written.

    python tools/make_goldens.py [pod5 | mixed16 | wide | preprocess]
"""
import os
import sys
import types
import math

import numpy as np
import torch
import yaml

REF = "/root/reference"
OUT = os.environ.get("S2S_GOLDEN_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


# ----------------------------------------------------------------------------- stubs
def _stub(name, **a):
    m = types.ModuleType(name)
    m.__dict__.update(a)
    sys.modules[name] = m
    return m


class _LM(torch.nn.Module):
    def save_hyperparameters(self, *a, **k):
        pass


class _FakeS5:
    """Captures what BLOW5Writer.save hands to pyslow5 (signal_io.py:88-172)."""
    captured = []          # list of dict(mode, header, records, auxs)

    def __init__(self, path, mode):
        self.path, self.mode, self.header = path, mode, None
        open(path, "a").close()            # so the next save() sees an existing file -> append mode

    def get_empty_header(self, aux=False):
        return {}, ["unknown", "partial", "mux_change", "unblock_mux_change", "data_service_unblock_mux_change",
                    "signal_positive", "signal_negative"]

    def write_header(self, header, end_reason_labels=None):
        self.header = dict(header)
        return 0

    def get_empty_record(self, aux=False):
        return {}, {}

    def write_record_batch(self, records, threads=1, batchsize=1, aux=None):
        _FakeS5.captured.append(dict(mode=self.mode, header=self.header,
                                     records={k: dict(v) for k, v in records.items()},
                                     auxs={k: dict(v) for k, v in aux.items()}))
        return 0

    def close(self):
        pass


_stub("numba", jit=lambda *a, **k: (lambda f: f))
_stub("pytorch_lightning", LightningModule=_LM, LightningDataModule=object, Trainer=object, __version__="stub")
_stub("pytorch_lightning.loggers", WandbLogger=object)
_stub("pytorch_lightning.strategies", DDPStrategy=object)
_stub("pytorch_lightning.callbacks", LearningRateMonitor=object, ModelCheckpoint=object)
_stub("pysam", FastxFile=object)
_stub("prettytable", PrettyTable=object)
_stub("pyslow5", Open=_FakeS5)
_stub("pod5")
sys.path.insert(0, os.path.join(REF, "src"))
import seq2squiggle.model as RM          # noqa: E402  (sets matmul precision "medium", model.py:22)
import seq2squiggle.utils as RU          # noqa: E402
import seq2squiggle.signal_io as RS      # noqa: E402

torch.set_float32_matmul_precision("highest")      # true fp32 goldens (SURVEY.md section 0 finding 3)
torch.set_grad_enabled(False)


def read_fasta(path):
    name, seq, out = None, [], []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            if name is not None:
                out.append(("".join(seq), name))
            name, seq = line[1:].split()[0], []
        elif line:
            seq.append(line)
    if name is not None:
        out.append(("".join(seq), name))
    return out


def base_config(k):
    cfg = yaml.safe_load(open(os.path.join(REF, "src/seq2squiggle/config.yaml")))
    cfg["seq_kmer"] = k
    return cfg


def make_model(seed, k):
    """Synthetic checkpoint: seeded default init, sharpened attention, calibrated head biases."""
    cfg = base_config(k)
    torch.manual_seed(seed)
    m = RM.seq2squiggle(config=cfg)
    sd = m.state_dict()
    for name, t in sd.items():
        if name.endswith(("w_qs.weight", "w_ks.weight")):
            t.mul_(3.0)                               # non-degenerate softmax rows
        if "layer_norm.weight" in name:
            t.add_(0.25 * torch.randn_like(t))       # non-trivial affine
        if "layer_norm.bias" in name:
            t.add_(0.1 * torch.randn_like(t))
    sd["length_regulator.duration_sampler.conc_layer.3.bias"].fill_(9.0)     # Gamma(~9, ~0.8): dwell ~ 11
    sd["length_regulator.duration_sampler.rate_layer.3.bias"].fill_(math.log(math.exp(0.8) - 1.0))
    sd["length_regulator.duration_sampler.conc_layer.3.weight"].mul_(4.0)
    sd["noise_sampler.stdv_layer.3.bias"].fill_(math.log(math.exp(0.01) - 1.0))  # sigma ~ 0.01 scaled
    sd["noise_sampler.stdv_layer.3.weight"].mul_(4.0)
    sd["decoders.out_linear.bias"].fill_(0.5)                                # ~ 80 pA, some ReLU zeros
    m.load_state_dict(sd)
    m.eval()
    return m, cfg


def save_ckpt(m, cfg, path):
    ckpt = {
        "epoch": 0, "global_step": 0, "pytorch-lightning_version": "2.5.1.post0",
        "state_dict": {k: v.clone() for k, v in m.state_dict().items()},
        "hyper_parameters": {"config": dict(cfg), "save_valid_plots": True, "out_writer": None,
                             "dwell_mean": 9.0, "dwell_std": 0.0, "noise_std": -1, "noise_sampling": False,
                             "duration_sampling": False, "export_every_n_samples": 2000000, "min_noise": 0.5,
                             "min_duration": 1},
        "loops": {}, "callbacks": {}, "optimizer_states": [], "lr_schedulers": [],
    }
    torch.save(ckpt, path)


def codes_from_onehot(x):
    """[C,16,k,5] one-hot -> uint8 codes, 255 for an all-zero row."""
    c = x.argmax(-1).astype(np.uint8)
    c[x.sum(-1) == 0] = 255
    return c


class Inject:
    """Replace the reference's RNG draws with recorded/injected variates."""

    def __init__(self, sg=None, z_normal=None):
        self.sg, self.z = sg, list(z_normal or [])
        self.used = []

    def __enter__(self):
        self._g, self._n = torch._standard_gamma, torch.normal
        inj = self

        def std_gamma(conc, generator=None):
            assert inj.sg is not None and inj.sg.shape == conc.shape, (conc.shape,)
            return inj.sg.clone()

        def normal(mean=0.0, std=1.0, size=None, **kw):
            z = inj.z.pop(0)
            inj.used.append(z)
            if isinstance(std, torch.Tensor) and isinstance(mean, torch.Tensor):
                return mean + z * std              # at::normal(Tensor, Tensor)
            if isinstance(std, torch.Tensor):
                return z * std + mean              # at::normal(double, Tensor)
            return z * std + mean                  # at::normal(double, double, size)
        torch._standard_gamma, torch.normal = std_gamma, normal
        return self

    def __exit__(self, *a):
        torch._standard_gamma, torch.normal = self._g, self._n


class FakeWriter:
    def __init__(self):
        self.signals, self.saved = None, []

    def save(self):
        self.saved.append({k: v.clone() for k, v in self.signals.items()})


def run_predict_step(m, names, x16, **over):
    """One reference predict_step on a fresh results list; returns [B,250] prediction rows."""
    for k, v in over.items():
        setattr(m, k, v)
    m.results, m.total_samples, m.out_writer = [], 0, None
    m.predict_step((tuple(names), x16))
    rows = []
    d = m.results[0]
    it = {k: iter(v) for k, v in d.items()}
    for n in names:
        rows.append(next(it[n]))
    return torch.stack(rows)


def stage_goldens(tag, m, cfg, reads, seed):
    k = cfg["seq_kmer"]
    names, chunks = [], []
    for seq, name in reads:
        br = RU.split_sequence(seq, cfg)
        for c in br:
            names.append(name)
            chunks.append(c)
    x = np.stack(chunks)                                  # [B,16,k,5] fp16
    codes = codes_from_onehot(x)
    B = x.shape[0]
    x16 = torch.from_numpy(x)
    g = {"codes": codes, "names": np.array(names)}

    data = x16.reshape(B, 16, -1)
    enc_out, emb_out = m.encoders(data)
    sigma = m.noise_sampler(emb_out)
    ds = m.length_regulator.duration_sampler
    conc = torch.clamp(ds.conc_layer(emb_out), min=1e-8)
    rate = torch.clamp(ds.rate_layer(emb_out), min=1e-8)
    g.update(emb_out=emb_out.numpy(), enc_out=enc_out.numpy(), sigma=sigma.numpy(),
             conc=conc.flatten(1).numpy(), rate=rate.flatten(1).numpy())

    gen = torch.Generator().manual_seed(seed)
    sg = torch._standard_gamma(conc, generator=gen)      # realistic draws, then stress cases
    sg[1] *= 2.5                                          # crop: sum(dur) > 250
    sg[2] *= 0.05                                         # clamp(1.0)/min_duration floor
    sg[3, 5:] *= 3.0
    z250 = torch.randn(B, 250, generator=gen)
    z16 = torch.randn(B, 16, generator=gen)
    g.update(sg=sg.flatten(1).numpy(), z01=z250.numpy(), zdw=z16.numpy())

    # -- gamma mode: duration sampler output (post clamp 1.0) == injected g
    with Inject(sg=sg):
        g_samp, _ = ds(emb_out)
    g["g"] = g_samp.numpy()
    with Inject(sg=sg):
        lr_out, dpo, _, sig_ext, _ = m.length_regulator(emb_out=emb_out, x=enc_out, target=None,
                                                        noise_std_prediction=sigma[:, :, None], max_length=250,
                                                        dwell_mean=12.5, dwell_std=0.0, duration_sampling=True,
                                                        min_length=3)
    dur = torch.round(dpo).int()
    g["dur_gamma"] = dur.numpy()
    g["sigma_ext_gamma"] = sig_ext.squeeze(-1).numpy()
    g["lr_rowsum_gamma"] = lr_out.sum(-1).numpy()         # compact check of the gather
    y_scaled = m.decoders(lr_out, None).squeeze(-1)
    g["y_scaled_gamma"] = y_scaled.numpy()
    common = dict(dwell_mean=12.5, dwell_std=0.0, min_duration=3)
    # full predict_step, default samplers (noise_sampling + duration_sampling), min_noise 0
    with Inject(sg=sg, z_normal=[z250]):
        g["y_gamma_nsamp"] = run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True,
                                              duration_sampling=True, min_noise=0.0, **common).numpy()
    with Inject(sg=sg, z_normal=[z250]):
        g["y_gamma_nsamp_minnoise"] = run_predict_step(m, names, x16, noise_std=1.5, noise_sampling=True,
                                                       duration_sampling=True, min_noise=0.02, **common).numpy()
    with Inject(sg=sg, z_normal=[z250]):
        g["y_gamma_nconst"] = run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=False,
                                               duration_sampling=True, min_noise=0.0, **common).numpy()
    with Inject(sg=sg):
        g["y_gamma_nonoise"] = run_predict_step(m, names, x16, noise_std=0.0, noise_sampling=True,
                                                duration_sampling=True, min_noise=0.0, **common).numpy()
    # ideal dwell (config 1 of BASELINE.json): everything deterministic
    g["y_ideal"] = run_predict_step(m, names, x16, noise_std=0.0, noise_sampling=False, duration_sampling=False,
                                    min_noise=0.0, **common).numpy()
    with Inject(z_normal=[z250]):
        g["y_ideal_nsamp"] = run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True,
                                              duration_sampling=False, min_noise=0.0, **common).numpy()
    # normal dwell (dwell_std > 0): torch.normal(mean, std) then clamp(min_duration)
    with Inject(z_normal=[z16, z250]):
        g["y_normal_nsamp"] = run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True,
                                               duration_sampling=False, min_noise=0.0, dwell_mean=12.5,
                                               dwell_std=4.0, min_duration=3).numpy()
    d_norm = torch.round(torch.clamp(torch.full((B, 16), 12.5) + z16 * torch.full((B, 16), 4.0), min=3)).int()
    g["dur_normal"] = d_norm.numpy()
    # rna-like long dwell: 16*31 = 496 > 250 -> every chunk cropped
    g["y_ideal_dwell31"] = run_predict_step(m, names, x16, noise_std=0.0, noise_sampling=False,
                                            duration_sampling=False, min_noise=0.0, dwell_mean=4000 / 130,
                                            dwell_std=0.0, min_duration=3).numpy()
    np.savez_compressed(os.path.join(OUT, f"stages_{tag}.npz"), **g)
    print(tag, "chunks", B, "zeros in y_ideal:", int((g["y_ideal"] == 0).sum()),
          "dur_gamma sum range", int(dur.sum(1).min()), int(dur.sum(1).max()))
    return names, x16, sg, z250


def export_goldens(tag, m, cfg, names, x16, sg, z250, profile_name):
    """Emulated Lightning predict loop -> export_and_clear_results -> BLOW5Writer.save (reference code)."""
    profile = RU.get_profile(profile_name)
    path = os.path.join("/tmp", f"golden_{tag}.blow5")
    if os.path.exists(path):
        os.remove(path)
    _FakeS5.captured = []
    w = RS.BLOW5Writer(path, profile, ideal_mode=True, profile_name=profile_name, preserve_read_ids=True)
    for k, v in dict(noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, dwell_mean=12.5,
                     dwell_std=0.0, min_duration=3, export_every_n_samples=16).items():
        setattr(m, k, v)
    m.results, m.total_samples, m.out_writer = [], 0, w
    bs = 10
    B = x16.shape[0]
    for s in range(0, B, bs):
        e = min(B, s + bs)
        with Inject(sg=sg[s:e], z_normal=[z250[s:e]]):
            m.predict_step((tuple(names[s:e]), x16[s:e]))
    m.on_predict_epoch_end()
    out = {"profile_name": np.array(profile_name), "batch_size": np.array(bs), "export_every": np.array(16)}
    order = []
    for si, cap in enumerate(_FakeS5.captured):
        for rid, rec in cap["records"].items():
            key = f"s{si}__{rid}"
            order.append(key)
            out[key + "__raw"] = np.asarray(rec["signal"])
            out[key + "__meta"] = np.array([rec["digitisation"], rec["offset"], rec["range"], rec["sampling_rate"],
                                            rec["len_raw_signal"], cap["auxs"][rid]["median_before"],
                                            cap["auxs"][rid]["start_time"], cap["auxs"][rid]["read_number"]],
                                           dtype=np.float64)
    out["order"] = np.array(order)
    hdr = _FakeS5.captured[0]["header"]
    out["header_keys"] = np.array(sorted(k for k in hdr if k != "exp_start_time"))
    out["header_vals"] = np.array([str(hdr[k]) for k in sorted(hdr) if k != "exp_start_time"])
    np.savez_compressed(os.path.join(OUT, f"export_{tag}.npz"), **out)
    os.remove(path)
    print(tag, "export saves:", len(_FakeS5.captured), "records:", len(order))

    # pA float signals per read (FakeWriter) with one final export
    fw = FakeWriter()
    m.results, m.total_samples, m.out_writer = [], 0, fw
    with Inject(sg=sg, z_normal=[z250]):
        m.predict_step((tuple(names), x16))
    m.on_predict_epoch_end()
    sig = {f"sig__{k}": v.numpy() for k, v in fw.saved[0].items()}
    sig["read_order"] = np.array(list(fw.saved[0].keys()))
    np.savez_compressed(os.path.join(OUT, f"signals_{tag}.npz"), **sig)


def chunker_goldens():
    rng = np.random.default_rng(7)
    reads = read_fasta(os.path.join(REF, "example/test.fasta"))
    extra = [("ACGTA", "short_lt_k"), ("ACGTACGTA", "exact_k"),
             ("".join(rng.choice(list("ACGT"), 9 + 15)), "exact_16_kmers"),
             ("".join(rng.choice(list("ACGT"), 9 + 16)), "17_kmers"),
             ("ACGTNNACGTacgtACGTRYACGTACGTACGTACGTAC_GT", "unknown_letters"),
             ("".join(rng.choice(list("ACGT"), 333)), "rand333")]
    out = {}
    for k in (9, 6):
        cfg = base_config(k)
        for seq, name in reads + extra:
            br = RU.split_sequence(seq, cfg)
            c = codes_from_onehot(br) if br.size else np.zeros((0, 16, k), np.uint8)
            out[f"k{k}__{name}"] = c
    out["names"] = np.array([n for _, n in reads + extra])
    out["seqs"] = np.array([s for s, _ in reads + extra])
    np.savez_compressed(os.path.join(OUT, "chunker.npz"), **out)


def profile_goldens():
    names = ["dna-r10-prom", "dna-r10-min", "dna-r9-prom", "dna-r9-min", "rna-004-prom", "rna-004-min"]
    rng = np.random.default_rng(11)
    sig = np.concatenate([rng.uniform(0, 200, 500), [0.0, 1e-3, 164.999, 400.0, 2000.0, 5000.0]]).astype(np.float32)
    out = {"signal": sig, "names": np.array(names)}
    for n in names:
        p = RU.get_profile(n)
        out[n + "__profile"] = np.array([p["digitisation"], p["sample_rate"], p["bps"], p["range"], p["offset_mean"],
                                         p["offset_std"], p["median_before_mean"], p["median_before_std"]], np.float64)
        path = f"/tmp/golden_prof_{n}.blow5"
        if os.path.exists(path):
            os.remove(path)
        _FakeS5.captured = []
        w = RS.BLOW5Writer(path, p, ideal_mode=True, profile_name=n, preserve_read_ids=False)
        w.signals = {"r0": torch.from_numpy(sig)}
        with np.errstate(all="ignore"):
            w.save()
        rec = list(_FakeS5.captured[0]["records"].items())
        out[n + "__read_id"] = np.array(rec[0][0])
        out[n + "__raw"] = np.asarray(rec[0][1]["signal"])
        hdr = _FakeS5.captured[0]["header"]
        out[n + "__header_keys"] = np.array(sorted(k for k in hdr if k != "exp_start_time"))
        out[n + "__header_vals"] = np.array([str(hdr[k]) for k in sorted(hdr) if k != "exp_start_time"])
        os.remove(path)
    np.savez_compressed(os.path.join(OUT, "profiles.npz"), **out)


def sampler_goldens():
    """Read sets drawn by the reference's own sampler for fixed seeds (utils.py:415-582)."""
    import random, hashlib
    genome = read_fasta(os.path.join(REF, "example/lamda_genome.fasta"))
    seqs, lens = zip(*[RU.process_genome(s) for s, _ in genome])
    # a two-contig reference with N runs and lower case, to cover the genome lookup and N handling
    rng = np.random.default_rng(3)
    c2 = "".join(rng.choice(list("ACGTN"), 20000, p=[.24, .24, .24, .24, .04])) + "acgtnnacgt" * 50
    seqs2, lens2 = zip(*[RU.process_genome(s) for s in (genome[0][0][:30000], c2)])
    out = {}
    cases = [("lambda_expon_dna", seqs, lens, 25, 5000, -1, "expon", "dna-r10-prom", 42),
             ("lambda_beta_dna", seqs, lens, 15, 3000, -1, "beta", "dna-r9-min", 7),
             ("lambda_gamma_rna", seqs, lens, 15, 2000, -1, "gamma", "rna-004-prom", 11),
             ("two_contigs_cov", seqs2, lens2, -1, 4000, 2, "expon", "dna-r10-min", 5)]
    for name, gs, gl, n, r, c, distr, prof, seed in cases:
        random.seed(seed)
        reads, total_l = RU.sample_reads_from_reference(list(gs), list(gl), n, r, c, base_config(9), "x.fasta", seed,
                                                        False, distr, prof, 30)
        reads = [rd for rd, _ in reads]
        out[name + "__lens"] = np.array([len(x) for x in reads])
        out[name + "__sha"] = np.array([hashlib.sha1(x.encode()).hexdigest() for x in reads])
        out[name + "__total_l"] = np.array(total_l)
        out[name + "__args"] = np.array([n, r, c, seed])
        out[name + "__distr_profile"] = np.array([distr, prof])
        print(name, len(reads), "reads, mean len", np.mean([len(x) for x in reads]) if reads else 0)
    out["two_contigs__seq1"] = np.array(c2)
    np.savez_compressed(os.path.join(OUT, "sampler.npz"), **out)


class _Rec:
    """Stands in for pod5.RunInfo / Pore / Calibration / EndReason / Read: keeps the keyword arguments."""
    def __init__(self, **kw):
        self.kw = kw


class _FakePod5Writer:
    captured = []          # list of (path, [Read kwargs])

    def __init__(self, path):
        self.path, self.reads = str(path), []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        _FakePod5Writer.captured.append((self.path, self.reads))

    def add_read(self, read):
        self.reads.append(read)


def pod5_goldens():
    """What the reference's POD5Writer.save (signal_io.py:201-287) hands to the pod5 library, for the per-read pA
    signals of signals_{k9,k6}.npz: the pod5 module is a recorder (the real library is not in the image)."""
    import enum
    import json
    P5 = sys.modules["pod5"]
    P5.RunInfo = P5.Pore = P5.Calibration = P5.EndReason = P5.Read = _Rec
    P5.EndReasonEnum = enum.Enum("EndReasonEnum", "UNKNOWN MUX_CHANGE UNBLOCK_MUX_CHANGE DATA_SERVICE_UNBLOCK_MUX_CHANGE "
                                                  "SIGNAL_POSITIVE SIGNAL_NEGATIVE", start=0)
    P5.Writer = _FakePod5Writer
    out = {}
    cases = [("k9", "dna-r10-prom", True, True), ("k9", "dna-r10-prom", True, False), ("k6", "rna-004-min", True, True)]
    for ci, (tag, prof, ideal, preserve) in enumerate(cases):
        sig = np.load(os.path.join(OUT, f"signals_{tag}.npz"))
        order = [str(x) for x in sig["read_order"]]
        _FakePod5Writer.captured = []
        w = RS.POD5Writer(f"/tmp/golden_{ci}.pod5", RU.get_profile(prof), ideal, prof, preserve)
        w.signals = {rid: torch.from_numpy(sig["sig__" + rid]) for rid in order}
        w.save()
        (path, reads), = _FakePod5Writer.captured
        key = f"case{ci}"
        out[key + "__args"] = np.array([tag, prof, str(ideal), str(preserve)])
        ri = reads[0].kw["run_info"].kw
        out[key + "__run_info"] = np.array(json.dumps({k: (v if isinstance(v, (str, int, float, dict)) else "<datetime>")
                                                        for k, v in ri.items()}, sort_keys=True))
        out[key + "__read_ids"] = np.array([str(r.kw["read_id"]) for r in reads])
        out[key + "__meta"] = np.array([[r.kw["calibration"].kw["offset"], r.kw["calibration"].kw["scale"],
                                         r.kw["median_before"], r.kw["read_number"], r.kw["start_sample"],
                                         r.kw["pore"].kw["channel"], r.kw["pore"].kw["well"],
                                         int(r.kw["end_reason"].kw["reason"].value), int(r.kw["end_reason"].kw["forced"])]
                                        for r in reads], np.float64)
        out[key + "__pore_type"] = np.array(reads[0].kw["pore"].kw["pore_type"])
        out[key + "__end_reason"] = np.array(reads[0].kw["end_reason"].kw["reason"].name)
        for i, r in enumerate(reads):
            out[f"{key}__raw{i}"] = np.asarray(r.kw["signal"])
            assert r.kw["run_info"] is reads[0].kw["run_info"]
        print(key, tag, prof, len(reads), "pod5 reads captured")
    np.savez_compressed(os.path.join(OUT, "pod5_records.npz"), **out)


def mixed16_goldens():
    """What the reference's OWN GPU arithmetic gives for the golden chunks: inference.py:403-404 selects precision "16-mixed" whenever a
    GPU is present, i.e. Lightning runs predict_step under torch.autocast(device, dtype=torch.float16).  No GPU build of the
    reference can run here, so the same predict_step (same committed checkpoints, same injected variates as y_gamma_nsamp) runs
    under torch.autocast("cpu", dtype=torch.float16): the CPU autocast policy casts the same Linear / matmul / bmm inputs to
    fp16 and keeps softmax / layer_norm in fp32 as the CUDA policy does; accumulation order differs from a GPU's, which is noise
    two orders below the fp16 rounding this measures.  -> tests/golden/mixed16.npz: per checkpoint the 16-mixed signal rows, the
    dwell indices under 16-mixed, and its MAE / max distance to the fp32 golden -- the bar the engine's opt-in reduced-precision
    mode (S2S_MODE_F16) is held to (tests/test_gpu_parity.py: test_reduced_precision_f16_mode)."""
    out = {}
    for tag in ("k9", "k6"):
        ck = torch.load(os.path.join(OUT, f"synthetic_{tag}.ckpt"), map_location="cpu", weights_only=True)
        cfg = ck["hyper_parameters"]["config"]
        m = RM.seq2squiggle(config=cfg)
        m.load_state_dict(ck["state_dict"])
        m.eval()
        g = dict(np.load(os.path.join(OUT, f"stages_{tag}.npz")))
        codes = g["codes"]
        x = np.zeros(codes.shape + (5,), np.float16)
        known = codes < 5
        x[known] = np.eye(5, dtype=np.float16)[codes[known]]
        x16 = torch.from_numpy(x)
        names = [str(n) for n in g["names"]]
        B = len(names)
        sg = torch.from_numpy(g["sg"]).reshape(B, 16, 1)
        z250 = torch.from_numpy(g["z01"])
        common = dict(dwell_mean=12.5, dwell_std=0.0, min_duration=3)
        with Inject(sg=sg, z_normal=[z250]):                 # sanity: the fp32 run reproduces the committed golden bit for bit
            y32 = run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, **common)
        assert np.array_equal(y32.numpy(), g["y_gamma_nsamp"]), tag
        with torch.autocast("cpu", dtype=torch.float16):
            with Inject(sg=sg, z_normal=[z250]):
                y16 = run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0,
                                       **common).float()
            enc_out, emb_out = m.encoders(x16.reshape(B, 16, -1))
            sigma = m.noise_sampler(emb_out)
            with Inject(sg=sg):
                _, dpo, _, _, _ = m.length_regulator(emb_out=emb_out, x=enc_out, target=None, noise_std_prediction=sigma[:, :, None],
                                                     max_length=250, dwell_mean=12.5, dwell_std=0.0, duration_sampling=True, min_length=3)
        d = (y16 - y32).abs()
        same = (y16 == 0) == (y32 == 0)
        out[f"y_gamma_nsamp_16mixed_{tag}"] = y16.numpy()
        out[f"dur_gamma_16mixed_{tag}"] = torch.round(dpo.float()).int().numpy()
        out[f"mae_vs_fp32_{tag}"] = np.float64(d.mean())
        out[f"max_vs_fp32_{tag}"] = np.float64(d.max())
        out[f"zero_pattern_equal_share_{tag}"] = np.float64(same.float().mean())
        # a dwell index that rounds the other way under fp16 shifts every later sample of its chunk: the distance on the chunks
        # whose indices all agree is the arithmetic's own
        agree = torch.from_numpy((out[f"dur_gamma_16mixed_{tag}"] == g["dur_gamma"]).all(1))
        out[f"dwell_indices_differing_{tag}"] = np.int64((out[f"dur_gamma_16mixed_{tag}"] != g["dur_gamma"]).sum())
        out[f"mae_vs_fp32_where_dwell_equal_{tag}"] = np.float64(d[agree].mean())
        out[f"max_vs_fp32_where_dwell_equal_{tag}"] = np.float64(d[agree].max())
        print(tag, "dwell indices differing:", int(out[f"dwell_indices_differing_{tag}"]), "of", g["dur_gamma"].size, "| on the", int(agree.sum()),
              "chunks whose indices agree: MAE", float(d[agree].mean()), "max", float(d[agree].max()))
        print(tag, "16-mixed vs fp32 golden: MAE", float(d.mean()), "max", float(d.max()), "zero pattern equal", float(same.float().mean()),
              "dwell indices equal", bool(np.array_equal(out[f"dur_gamma_16mixed_{tag}"], g["dur_gamma"])))
    np.savez_compressed(os.path.join(OUT, "mixed16.npz"), **out)


def wide_goldens():
    """More chunks through the reference itself (round 6: the stage goldens hold 51 / 56 chunks per chemistry; everything wider was
    checked through the oracle only).  The committed checkpoints, ~256 chunks per chemistry of REAL sequence -- windows of the
    reference's lambda genome example -- plus the edge reads of the test suites (homopolymers, a dinucleotide repeat, an N-rich read,
    reads that end in a short tail), the reference's predict_step with injected variates in two configurations (the default
    samplers: Gamma dwell + sampled noise; ideal dwell + constant noise), and the dwell indices of the Gamma run.
    -> tests/golden/wide_{k9,k6}.npz: codes, sg (injected standard-gamma draws), g (the duration sampler's output for them), z01
    (injected normals), y_gamma_nsamp, dur_gamma, y_ideal_nconst.  The normals are stored as float16-exact values (drawn, then rounded to float16 and used as such) to halve
    the fixture; they are injected variates, any values do."""
    lam = read_fasta(os.path.join(REF, "example", "lamda_genome.fasta"))[0][0].upper()        # (the reference's own spelling)
    for tag, seed in (("k9", 31), ("k6", 32)):
        ck = torch.load(os.path.join(OUT, f"synthetic_{tag}.ckpt"), map_location="cpu", weights_only=True)
        cfg = ck["hyper_parameters"]["config"]
        m = RM.seq2squiggle(config=cfg)
        m.load_state_dict(ck["state_dict"])
        m.eval()
        rng = np.random.default_rng(seed)
        reads = []
        for i, start in enumerate(rng.integers(0, len(lam) - 700, size=6)):
            L = int(rng.integers(380, 640))
            reads.append((lam[int(start):int(start) + L], f"lambda_{i}"))
        reads += [("A" * 90, "homopolymer_A"), ("T" * 57, "homopolymer_T"), ("ACACACACAC" * 11, "dinucleotide"),
                  ("".join(rng.choice(list("ACGTN"), 130, p=[.2, .2, .2, .2, .2])), "n_rich"),
                  (lam[1000:1000 + 16 * 3 + cfg["seq_kmer"]], "ends_on_a_chunk_boundary"),
                  (lam[5000:5000 + 16 * 2 + cfg["seq_kmer"] + 5], "short_tail")]
        names, chunks = [], []
        for seq, name in reads:
            for c in RU.split_sequence(seq, cfg):
                names.append(name)
                chunks.append(c)
        x = np.stack(chunks)
        B = x.shape[0]
        x16 = torch.from_numpy(x)
        gen = torch.Generator().manual_seed(1000 + seed)
        enc_out, emb_out = m.encoders(x16.reshape(B, 16, -1))
        sigma = m.noise_sampler(emb_out)
        ds = m.length_regulator.duration_sampler
        conc = torch.clamp(ds.conc_layer(emb_out), min=1e-8)
        sg = torch._standard_gamma(conc, generator=gen)
        z250 = torch.randn(B, 250, generator=gen).half().float()
        common = dict(dwell_mean=12.5, dwell_std=0.0, min_duration=3)
        with Inject(sg=sg, z_normal=[z250]):
            y = run_predict_step(m, names, x16, noise_std=2.0, noise_sampling=True, duration_sampling=True, min_noise=0.0, **common)
        with Inject(sg=sg):
            _, dpo, _, _, _ = m.length_regulator(emb_out=emb_out, x=enc_out, target=None, noise_std_prediction=sigma[:, :, None],
                                                 max_length=250, dwell_mean=12.5, dwell_std=0.0, duration_sampling=True, min_length=3)
        with Inject(z_normal=[z250]):
            yi = run_predict_step(m, names, x16, noise_std=1.0, noise_sampling=False, duration_sampling=False, min_noise=0.0, **common)
        with Inject(sg=sg):
            g_samp, _ = ds(emb_out)                          # the duration sampler's output for these draws: what the engine takes as inject_g
        out = {"codes": codes_from_onehot(x), "names": np.array(names), "sg": sg.flatten(1).numpy(), "g": g_samp.numpy(), "z01": z250.half().numpy(),
               "y_gamma_nsamp": y.numpy(), "dur_gamma": torch.round(dpo).int().numpy(), "y_ideal_nconst": yi.numpy()}
        np.savez_compressed(os.path.join(OUT, f"wide_{tag}.npz"), **out)
        print(tag, "wide:", B, "chunks from", len(reads), "reads; zeros in y:", int((out["y_gamma_nsamp"] == 0).sum()),
              "bytes", os.path.getsize(os.path.join(OUT, f"wide_{tag}.npz")))


# ----------------------------------------------------------------------------- preprocess
TABLE_HEAD = "read_name\tposition\tmodel_kmer\tstart_idx\tend_idx\tevent_level_mean\tevent_stdv\tsamples"


def save_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def preprocess_table(te, ts, k):
    """-> (the table's text, the name of the read laid with falling positions, the largest sample total of a chunk): the reads of one
    golden.  Why every choice is what it is:
      * one frame per read (partition_by=True): the reference's route that cuts chunks inside a read, the one our entry follows;
      * positions are unique inside a read and have gaps: the reference's sort by position has no ties to break (the stand-in's
        tie order cannot show), and a position is never usable as an index;
      * sample texts are multiples of 0.125 printed %.3f, event_stdv a multiple of 0.0625 printed %.4f: exact in fp32, so polars'
        cast, the stand-in's and the package's double-then-fp32 parse give the same bits;
      * end_idx - start_idx is the row's sample count and >= 1 (a row without samples is undefined in the reference: its samples
        text is empty while its length is not counted; it is left out); start_idx has gaps, which nothing may read;
      * a chunk holds fewer than 32,768 samples: pad_lengths' int16 lengths neither wrap nor (numpy 2) raise;
      * no read has only all-N rows: the reference would run process_df on an empty frame, where the stand-in, not polars, would
        decide what an empty column is.
    The reads: 1, te - 1, te, te + 1 and 3 te rows; a chunk of exactly ts samples and one of ts + 1; a row alone longer than ts;
    k-mers with some N, all-N rows at both ends and in the middle of a read; one read listed with position falling while start_idx
    rises (the reverse strand of `predict --events`); one read listed in shuffled order; the reads' lines interleaved, first
    appearances not in name order.  Chunks are made to pass or miss ts in turn, so that both kinds are many."""
    rng = np.random.default_rng([31, te, ts, k])
    b = max(1, ts // te)

    def group(m, keep=True, total=None):
        """The lengths of m rows that share a chunk with te - m pads: at most ts samples in all, more than ts, or exactly `total`."""
        if total is None and keep:
            return rng.integers(1, b + 1, m)
        total = ts + int(rng.integers(1, 4)) if total is None else total
        ln = np.ones(m, np.int64)
        np.add.at(ln, rng.integers(0, m, total - (te - m) - m), 1)
        return ln

    def kmers(n, some_n=()):
        out = rng.choice(list("ACGT"), (n, k))
        for j in some_n:
            out[j, rng.integers(0, k, max(1, k // 3))] = "N"
        return ["".join(r) for r in out]

    reads = {"solo": group(1), "full": group(te, total=ts), "full_and_one": np.concatenate([group(te, total=ts + 1), group(1)]),
             "three": np.concatenate([group(te, False), group(te), group(te, False)]),
             "long_row": np.array([1, ts + 1 + int(rng.integers(0, 3)), 1]),
             "falling": np.concatenate([group(te), group(te, False), group(1)])}
    if te > 1:
        reads["short"] = group(te - 1, False)
    rows = {name: list(zip(kmers(len(ln)), ln.tolist())) for name, ln in reads.items()}
    ln = group(te, False)                            # te rows between and around three all-N rows; some N in two of the rows
    real = list(zip(kmers(te, some_n=sorted({0, te - 1}) if k > 1 else ()), ln.tolist()))
    mid = (te + 1) // 2
    n_row = lambda: ("N" * k, int(rng.integers(1, b + 2)))      # noqa: E731
    rows["with_n"] = [n_row()] + real[:mid] + [n_row()] + real[mid:] + [n_row()]
    biggest = 0
    lines = {}
    for name, rs in rows.items():
        pos = int(rng.integers(0, 1000)) + np.cumsum(rng.integers(1, 4, len(rs)))
        order = list(range(len(rs)))
        if name == "falling":
            order = order[::-1]
        if name == "three":
            order = [int(i) for i in rng.permutation(len(rs))]
        at, mine = int(rng.integers(0, 50)), []
        for i in order:
            kmer, n = rs[i]
            x = rng.integers(320, 1200, n) / 8.0
            at += int(rng.integers(0, 3))
            mine.append(f"{name}\t{pos[i]}\t{kmer}\t{at}\t{at + n}\t{x.mean():.4f}\t{rng.integers(1, 200) / 16.0:.4f}\t" +
                        ",".join("%.3f" % v for v in x))
            at += n
        lines[name] = mine
        real_ln = [n for kmer, n in rs if kmer != "N" * k]
        biggest = max([biggest] + [sum(real_ln[a:a + te]) + te for a in range(0, len(real_ln), te)])
    names = sorted(lines, key=lambda s: rng.random())
    left = {name: list(lines[name]) for name in names}
    table = [TABLE_HEAD]
    while left:
        name = names[int(rng.integers(0, len(names)))]
        if name in left:
            table.append(left[name].pop(0))
            if not left[name]:
                del left[name]
    return "\n".join(table) + "\n", "falling", biggest


def preprocess_goldens():
    """The reference's own chunk cutting -> tests/golden/preprocess_<te>x<ts>x<k>.npz.  polars is not in the image: the reference's
    preprocess.py is imported over tools/polars_standin.py, and its split_eventtable_in_chunks(partition_by=True) (process_df,
    get_dna2signal_idxs, get_chunks, regular_break_points, one_hot_encode, pad_lengths, ChunkDataSet) -> typical_indices -> filter_chunks
    -> save_chunks run unmodified.  process_events is not used (it passes `parition_by=`, a TypeError), and typical_indices' result goes
    to filter_chunks as it is, where process_events would permute it at random.  Per file: the table's bytes, the reads in order of
    first appearance with the chunks the reference cuts from each alone, the unfiltered t_lengths, the kept indices, and for rna in
    (False, True) the five arrays as save_chunks writes them, dtypes and shapes untouched."""
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.join(os.path.dirname(here), "tests"))
    import polars_standin as PS
    sys.modules["polars"] = PS
    import seq2squiggle.preprocess as RP
    from _preprocess_cases import GEOMETRIES
    for te, ts, k in GEOMETRIES:
        text, falling, biggest = preprocess_table(te, ts, k)
        assert biggest < 32768, biggest
        cfg = dict(max_dna_len=te, max_signal_len=ts, seq_kmer=k)
        body = text.split("\n")[1:-1]
        names = list(dict.fromkeys(line.split("\t")[0] for line in body))
        assert names != sorted(names) and any(a.split("\t")[0] != b.split("\t")[0] for a, b in zip(body, body[1:]))
        per_read = [len(RP.split_eventtable_in_chunks(PS.from_table_text("\n".join([TABLE_HEAD] + [x for x in body if x.split("\t")[0] == n]) + "\n"),
                                                      cfg, None, partition_by=True, rna=False)) for n in names]
        out = {"table": np.frombuffer(text.encode("ascii"), np.uint8), "geometry": np.array([te, ts, k], np.int64), "names": np.array(names),
               "falling_read": np.array(falling), "chunks_per_read": np.array(per_read, np.int64)}
        for rna in (False, True):
            ds = RP.split_eventtable_in_chunks(PS.from_table_text(text), cfg, None, partition_by=True, rna=rna)
            t_all = np.array(ds.t_lengths)
            idx = RP.typical_indices(ds.t_lengths, ts)
            kept = RP.filter_chunks(ds, idx, ts)
            with tempfile.TemporaryDirectory() as d:
                RP.save_chunks(kept, d)
                for kind in ("chunks", "chunks_lengths", "targets", "targets_lengths", "stdevs"):
                    out[("rna_" if rna else "dna_") + kind] = np.load(os.path.join(d, kind + ".npy"))
            if rna:
                assert np.array_equal(out["t_lengths"], t_all) and np.array_equal(out["kept"], idx)
            out["t_lengths"], out["kept"] = t_all, np.asarray(idx)
        N, n_kept = len(out["t_lengths"]), len(out["kept"])
        assert N == sum(per_read) and 4 * n_kept >= N and 4 * (N - n_kept) >= N, (N, n_kept)      # both kinds: a quarter at least
        assert ts in out["t_lengths"] and ts + 1 in out["t_lengths"]
        assert ts == 1 or not np.array_equal(out["dna_targets"], out["rna_targets"])     # (at ts = 1 a kept row has one sample to reverse)
        path = os.path.join(OUT, f"preprocess_{te}x{ts}x{k}.npz")
        save_npz(path, out)
        print(f"preprocess {te}/{ts}/{k}: {len(body)} rows of {len(names)} reads, {N} chunks, {n_kept} kept; stdevs",
              out["dna_stdevs"].shape, out["dna_stdevs"].dtype, "targets_lengths", out["dna_targets_lengths"].dtype, "chunks_lengths",
              out["dna_chunks_lengths"].dtype, "bytes", os.path.getsize(path))


def main():
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:] == ["preprocess"]:    # only the chunk-cutting goldens (the reference's preprocess.py over tools/polars_standin.py)
        preprocess_goldens()
        return
    if sys.argv[1:] == ["wide"]:          # only the wide goldens (they read the committed checkpoints)
        wide_goldens()
        return
    if sys.argv[1:] == ["pod5"]:          # only the POD5 record goldens (they read the committed signals_*.npz)
        pod5_goldens()
        return
    if sys.argv[1:] == ["mixed16"]:       # only the reference-under-fp16-autocast vectors (they read the committed checkpoints and stages_*.npz)
        mixed16_goldens()
        return
    sampler_goldens()
    chunker_goldens()
    profile_goldens()
    reads = read_fasta(os.path.join(REF, "example/test.fasta"))
    rng = np.random.default_rng(5)
    reads_x = reads + [("".join(rng.choice(list("ACGTN"), 150, p=[.24, .24, .24, .24, .04])), "rand150_with_N")]
    for tag, seed, k, prof in (("k9", 1, 9, "dna-r10-prom"), ("k6", 2, 6, "dna-r9-min")):
        m, cfg = make_model(seed, k)
        save_ckpt(m, cfg, os.path.join(OUT, f"synthetic_{tag}.ckpt"))
        names, x16, sg, z250 = stage_goldens(tag, m, cfg, reads_x, seed=100 + k)
        export_goldens(tag, m, cfg, names, x16, sg, z250, prof)
    pe = {"enc": RM.Encoder(base_config(9)).position_enc.numpy(), "dec": RM.Decoder(base_config(9)).position_enc.numpy()}
    np.savez_compressed(os.path.join(OUT, "position_enc.npz"), **pe)
    pod5_goldens()
    mixed16_goldens()
    wide_goldens()
    print("goldens written to", OUT)


if __name__ == "__main__":
    main()
