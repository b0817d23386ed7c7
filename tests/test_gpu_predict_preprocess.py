"""`predict`, `preprocess` and `evaluate` closed into one chain on the six lambda reads of tests/test_gpu_predict_resquiggle.py: one
small `predict --events --events-samples` run from the committed synthetic checkpoint, `preprocess` of the table it wrote, `evaluate`
of the directory with the same checkpoint.  Asserted: the chunk count equals the restatement's (every k-mer of predict's table is a
row), the GPU's files equal --cpu's in every byte, the four losses are finite -- PRINTED, no bar: the checkpoint is untrained.  And
`resquiggle --chunks` of the signal predict wrote equals `--cpu --chunks` in every byte."""
import math

import numpy as np
import pytest

from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import evaluate as EV
from seq2squiggle_amd import preprocess as PP
from seq2squiggle_amd import resquiggle as RSQ
from seq2squiggle_amd import utils as U
from test_gpu_kmer_model import CKPT, LAMBDA, PROFILE, SEED

pytestmark = pytest.mark.gpu
GEOMETRY = (9, 16, 250)


def predict_run(d):
    """The module's one `predict --events --events-samples` run, into the directory d (also the data of tests/_trained.py's k9
    students)."""
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    genome = next(iter(U.read_fasta(LAMBDA)))[0].upper()
    (d / "reads.fasta").write_text("".join(f">lambda_{i}\n{genome[3000 * i + 100:3000 * i + 320 + 40 * i]}\n" for i in range(6)))
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=str(d / "reads.fasta"), read_input=True, n=-1, r=400, c=-1,
                  out=str(d / "p.blow5"), profile=PROFILE, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True,
                  duration_sampling=True, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None,
                  digitisation=None, range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None,
                  min_noise=0.0, min_duration=3, min_read_len=30, preserve_read_ids=True, seed=SEED, events=str(d / "truth.tsv"),
                  events_samples=True, kmer_table=None, kmer_model=str(d / "p.model"))
    return d


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return predict_run(tmp_path_factory.mktemp("predict_preprocess"))


def files_of(d):
    return {kind: np.concatenate([np.load(f[kind]) for f in EV.discover(str(d))]) for kind in EV.KINDS}


def test_predict_preprocess_evaluate(run):
    d = run
    gpu = PP.preprocess_table(d / "truth.tsv", d / "gpu", *GEOMETRY, chunks_per_file=7)
    cpu = PP.preprocess_table(d / "truth.tsv", d / "cpu", *GEOMETRY, cpu=True)
    a, b = files_of(d / "gpu"), files_of(d / "cpu")
    for kind in EV.KINDS:
        assert a[kind].dtype == b[kind].dtype and a[kind].shape == b[kind].shape and a[kind].tobytes() == b[kind].tobytes(), kind
    keys = PP.COUNTERS + ("chunks_written",)
    assert [gpu[k] for k in keys] == [cpu[k] for k in keys] and gpu["files"] == -(-gpu["chunks_kept"] // 7) and cpu["files"] == 1
    # the restatement: per read n rows (one per row of the table), floor(n / 16) + 1 chunks, kept iff their samples fit 250
    table = CMP.read_events(str(d / "truth.tsv"))
    formed = kept = 0
    for rows in table.values():
        lens = [e - s for _, _, s, e in sorted(rows, key=lambda r: int(r[0]))]
        lens += [1] * (16 - len(lens) % 16)
        sums = [sum(lens[i:i + 16]) for i in range(0, len(lens), 16)]
        formed += len(sums)
        kept += sum(v <= 250 for v in sums)
    assert gpu["reads"] == len(table) == 6 and gpu["rows"] == sum(len(v) for v in table.values()) and gpu["all_n_rows"] == 0
    assert (gpu["chunks_formed"], gpu["chunks_kept"]) == (formed, kept) and kept == len(a["targets"]) > 0
    import seq2squiggle_amd as S
    sd, cfg = S.load_checkpoint(CKPT)
    assert (cfg["seq_kmer"], cfg["max_dna_len"], cfg["max_signal_len"]) == GEOMETRY
    data = EV.EvalData(str(d / "gpu"), cfg)
    assert data.n == kept
    eng = S.Engine(sd, cfg, device=0)
    r, _, _ = EV.evaluate(eng, data)
    eng.close()
    losses = {k: float(r[k]) for k in ("valid_signal_loss", "valid_duration_loss", "valid_noise_loss", "valid_total_loss")}
    print(f"\npredict -> preprocess -> evaluate on six lambda reads: {gpu['rows']} rows, {formed} chunks formed, {kept} kept; {losses}")
    assert all(math.isfinite(v) for v in losses.values()), losses


def test_resquiggle_chunks_gpu_bytes_equal_cpu_bytes(run):
    d = run
    fasta = str(d / "reads.fasta")
    gpu = RSQ.resquiggle_files(fasta, d / "p.blow5", d / "p.model", d / "gpu.tsv", chunks=(d / "rq_gpu",) + GEOMETRY)
    cpu = RSQ.resquiggle_files(fasta, d / "p.blow5", d / "p.model", d / "cpu.tsv", chunks=(d / "rq_cpu",) + GEOMETRY, cpu=True,
                               max_samples=1)
    plain = RSQ.resquiggle_files(fasta, d / "p.blow5", d / "p.model", d / "plain.tsv")
    assert (d / "gpu.tsv").read_bytes() == (d / "cpu.tsv").read_bytes() == (d / "plain.tsv").read_bytes() and "chunks" not in plain
    a, b = files_of(d / "rq_gpu"), files_of(d / "rq_cpu")
    for kind in EV.KINDS:
        assert a[kind].dtype == b[kind].dtype and a[kind].shape == b[kind].shape and a[kind].tobytes() == b[kind].tobytes(), kind
    keys = PP.COUNTERS + ("chunks_written", "files")
    assert [gpu["chunks"][k] for k in keys] == [cpu["chunks"][k] for k in keys]
    assert gpu["chunks"]["reads"] == 6 and gpu["chunks"]["rows"] == gpu["events"] and len(a["targets"]) == gpu["chunks"]["chunks_kept"] > 0
