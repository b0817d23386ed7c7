"""`predict` and `segment` against each other: the `predict --read-input --preserve-read-ids --events` run of
tests/test_gpu_predict_resquiggle.py (six reads cut from the committed lambda genome, the committed synthetic checkpoint), then
`segment` of the signal it wrote.  Asserted: the GPU, --cpu and a three-batch --max-samples run write equal bytes; every row's level
and deviation are the restatement's (tests/_segment_ref.py) on the stored samples; the events of every record abut and cover it.
MEASURED AND PRINTED, not asserted: the share of the run's true k-mer boundaries (its own event table) with a detected boundary within
+-2 samples, and the detected boundaries per true one.  The synthetic checkpoints are untrained -- neighbouring k-mers need not differ
in level -- and the defaults are choices, so no bar is set."""
import numpy as np
import pytest

import _segment_ref as REF
from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import signal_batch as SB
from seq2squiggle_amd import segment as SEG
from seq2squiggle_amd import utils as U
from test_gpu_kmer_model import CKPT, LAMBDA, PROFILE, SEED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    d = tmp_path_factory.mktemp("predict_segment")
    genome = next(iter(U.read_fasta(LAMBDA)))[0].upper()
    (d / "reads.fasta").write_text("".join(f">lambda_{i}\n{genome[3000 * i + 100:3000 * i + 320 + 40 * i]}\n" for i in range(6)))
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=str(d / "reads.fasta"), read_input=True, n=-1, r=400, c=-1,
                  out=str(d / "p.blow5"), profile=PROFILE, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True,
                  duration_sampling=True, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None,
                  digitisation=None, range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None,
                  min_noise=0.0, min_duration=3, min_read_len=30, preserve_read_ids=True, seed=SEED, events=str(d / "truth.tsv"),
                  events_samples=False, kmer_table=None, kmer_model=None)
    records = [(r["read_id"], np.asarray(r["signal"], np.int16), (float(r["digitisation"]), float(r["offset"]), float(r["range"])))
               for r in SB.open_records(str(d / "p.blow5"))]
    lens = [len(x) for _, x, _ in records]

    def batches(m):                                  # the batching rule of segment_files
        count, held = 1, 0
        for n in lens:
            if held and held + n > m:
                count, held = count + 1, 0
            held += n
        return count
    three = next(m for m in range(max(lens), sum(lens) + 1, 16) if batches(m) == 3)
    gpu = SEG.segment_files(d / "p.blow5", d / "gpu.tsv", summary_out=d / "gpu.sum")
    cpu = SEG.segment_files(d / "p.blow5", d / "cpu.tsv", summary_out=d / "cpu.sum", cpu=True)
    cut = SEG.segment_files(d / "p.blow5", d / "cut.tsv", summary_out=d / "cut.sum", max_samples=three)
    return d, records, gpu, cpu, cut


def test_gpu_cpu_and_batched_runs_write_equal_bytes(run):
    d, records, gpu, cpu, cut = run
    assert (d / "gpu.tsv").read_bytes() == (d / "cpu.tsv").read_bytes() == (d / "cut.tsv").read_bytes()
    assert (d / "gpu.sum").read_bytes() == (d / "cpu.sum").read_bytes() == (d / "cut.sum").read_bytes()
    keys = ("records", "samples", "events", "refused", "mean_samples_per_event")
    assert [gpu[k] for k in keys] == [cpu[k] for k in keys] == [cut[k] for k in keys]
    assert gpu["records"] == 6 and gpu["refused"] == 0 and gpu["batches"] == 1 and cut["batches"] == 3 and gpu["events"] > 6


def test_rows_are_the_restatements_and_partition_each_record(run):
    d, records, gpu, _, _ = run
    text = (d / "gpu.tsv").read_text()
    want, want_summary = REF.table(records, 3, 6, REF.threshold_int(1.4), REF.threshold_int(9.0))
    assert text == want and (d / "gpu.sum").read_text() == want_summary       # every level and deviation, from the stored samples
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    for rid, x, _ in records:
        mine = [r for r in rows if r[0] == rid]
        REF.check_consequences(len(x), [int(r[2]) for r in mine], [int(r[3]) - int(r[2]) for r in mine], 3)
        assert [int(r[1]) for r in mine] == list(range(len(mine)))


def test_measure_the_recovery_of_the_true_boundaries(run):
    d, records, gpu, _, _ = run
    truth = CMP.read_events(str(d / "truth.tsv"))
    rows = [l.split("\t") for l in (d / "gpu.tsv").read_text().splitlines()[1:]]
    true_n = hit = found = 0
    for rid, x, _ in records:
        det = np.array(sorted(int(r[2]) for r in rows if r[0] == rid and int(r[2]) > 0), np.int64)
        tb = sorted({s for _, _, s, _ in truth[rid] if 0 < s < len(x)})
        found += len(det)
        true_n += len(tb)
        hit += sum(1 for b in tb if len(det) and np.abs(det - b).min() <= 2)
    print(f"\nsegment of predict's own output ({gpu['records']} reads, {gpu['samples']} samples, {gpu['events']} events, "
          f"{gpu['mean_samples_per_event']:.3f} samples per event): {hit} of {true_n} true k-mer boundaries have a detected boundary within "
          f"+-2 samples = {hit / max(true_n, 1):.4f}; {found} detected boundaries = {found / max(true_n, 1):.4f} per true one "
          f"(untrained checkpoint: neighbouring k-mers need not differ in level)")
    assert true_n > 0
