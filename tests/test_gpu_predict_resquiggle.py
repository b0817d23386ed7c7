"""`predict` and `resquiggle` against each other: one small `predict --read-input --preserve-read-ids` run with --events and
--kmer-model from the committed synthetic checkpoint, on six reads of 220 to 420 bases cut from the committed lambda genome (the
committed example reads are GAC repeats with 45 distinct 9-mers, which no aligner can place), then `resquiggle` of the signal it
wrote with the model it wrote.  Asserted: the
GPU's bytes equal --cpu's, every row's k-mer is the FASTA's at that position, and the intervals partition each record.  MEASURED AND
PRINTED, not asserted: the share of samples that come back on their true k-mer (the run's own event table), beside the same share for
a ruler that deals n / K samples to every k-mer.  The synthetic checkpoints are untrained -- how k-mer specific their levels are was
never measured -- and there is no f5c / uncalled4 to compare against, so no bar is set."""
import numpy as np
import pytest

from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import signal_batch as SB
from seq2squiggle_amd import resquiggle as RSQ
from seq2squiggle_amd import utils as U
from test_gpu_kmer_model import CKPT, LAMBDA, PROFILE, SEED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    d = tmp_path_factory.mktemp("predict_resquiggle")
    genome = next(iter(U.read_fasta(LAMBDA)))[0].upper()
    (d / "reads.fasta").write_text("".join(f">lambda_{i}\n{genome[3000 * i + 100:3000 * i + 320 + 40 * i]}\n" for i in range(6)))
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=str(d / "reads.fasta"), read_input=True, n=-1, r=400, c=-1,
                  out=str(d / "p.blow5"), profile=PROFILE, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True,
                  duration_sampling=True, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None,
                  digitisation=None, range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None,
                  min_noise=0.0, min_duration=3, min_read_len=30, preserve_read_ids=True, seed=SEED, events=str(d / "truth.tsv"),
                  events_samples=False, kmer_table=None, kmer_model=str(d / "p.model"))
    fasta = str(d / "reads.fasta")
    gpu = RSQ.resquiggle_files(fasta, d / "p.blow5", d / "p.model", d / "gpu.tsv", summary_out=d / "gpu.sum")
    cpu = RSQ.resquiggle_files(fasta, d / "p.blow5", d / "p.model", d / "cpu.tsv", summary_out=d / "cpu.sum", cpu=True)
    return d, gpu, cpu


def test_gpu_bytes_equal_cpu_bytes(run):
    d, gpu, cpu = run
    assert (d / "gpu.tsv").read_bytes() == (d / "cpu.tsv").read_bytes() and (d / "gpu.sum").read_bytes() == (d / "cpu.sum").read_bytes()
    keys = ("records", "solved", "unreached", "refused", "no_sequence", "no_known_level", "events", "skipped_kmers", "mean_cost_per_sample")
    assert [gpu[k] for k in keys] == [cpu[k] for k in keys]
    assert gpu["solved"] == gpu["records"] == 6 and gpu["k"] == 9 and gpu["refused"] == 0 and gpu["no_sequence"] == 0


def test_rows_match_the_fasta_and_partition_each_record(run):
    d, gpu, _ = run
    seqs = {name: RSQ.clean_sequence(seq) for seq, name in U.read_fasta(str(d / "reads.fasta"))}
    lengths = {r["read_id"]: len(r["signal"]) for r in SB.open_records(str(d / "p.blow5"))}
    table = CMP.read_events(str(d / "gpu.tsv"))
    assert len(table) == gpu["solved"] and sum(len(v) for v in table.values()) == gpu["events"]
    for rid, rows in table.items():
        at = 0
        assert int(rows[0][0]) == 0 and int(rows[-1][0]) == len(seqs[rid]) - 9       # the first and the last k-mer are never skipped
        for pos, kmer, s, e in rows:
            assert kmer == seqs[rid][int(pos):int(pos) + 9] and s == at and e > s
            at = e
        assert at == lengths[rid]
        assert (np.diff([int(r[0]) for r in rows]) <= 2).all() and (np.diff([int(r[0]) for r in rows]) >= 1).all()


def test_measure_the_share_of_samples_on_their_true_kmer(run):
    d, gpu, _ = run
    truth, got = CMP.read_events(str(d / "truth.tsv")), CMP.read_events(str(d / "gpu.tsv"))
    seqs = {name: seq for seq, name in U.read_fasta(str(d / "reads.fasta"))}
    lengths = {r["read_id"]: len(r["signal"]) for r in SB.open_records(str(d / "p.blow5"))}
    total = hit = ruler = 0
    for rid, rows in truth.items():
        if rid not in got:
            continue
        n, K = lengths[rid], len(seqs[rid]) - 9 + 1
        mine = np.full(n, -1, np.int64)
        for pos, _, s, e in got[rid]:
            mine[s:e] = int(pos)
        dealt = np.minimum(np.arange(n) * K // n, K - 1)
        for pos, _, s, e in rows:
            total += e - s
            hit += int((mine[s:e] == int(pos)).sum())
            ruler += int((dealt[s:e] == int(pos)).sum())
    print(f"\nresquiggle of predict's own output ({gpu['solved']} reads, {gpu['events']} events, {gpu['skipped_kmers']} skipped k-mers, mean "
          f"cost {gpu['mean_cost_per_sample']:.4f} MAD per sample): {hit} of {total} samples on their true k-mer = {hit / max(total, 1):.4f}; "
          f"a ruler that deals n / K samples to every k-mer: {ruler / max(total, 1):.4f}")
    assert total > 0
