"""`predict`, `eventalign` and `resquiggle` against each other: the six lambda reads of tests/test_gpu_predict_resquiggle.py simulated
from the committed synthetic checkpoint with --events and --kmer-model, then every stored signal gets 400 samples of ANOTHER record
in front -- an untrimmed read -- and goes through `eventalign` with the model the run wrote.  Asserted: the GPU's bytes equal
--cpu's, and the consequences of the definition hold on the rows (the k-mers are the FASTA's, positions ascend, the intervals of the
rows abut and lie inside the record).  MEASURED AND PRINTED, not asserted: the share of samples that come back on their true k-mer, the
error of the head trim, and beside them the share `resquiggle` reaches on the untouched records.  The synthetic checkpoints are
untrained and there is no f5c / nanopolish / uncalled4 to compare against, so no bar is set."""
import numpy as np
import pytest

from seq2squiggle_amd import compare as CMP
from seq2squiggle_amd import eventalign as EA
from seq2squiggle_amd import resquiggle as RSQ
from seq2squiggle_amd import signal_batch as SB
from seq2squiggle_amd import utils as U
from test_compare_cpu import write_file
from test_gpu_kmer_model import CKPT, LAMBDA, PROFILE, SEED

pytestmark = pytest.mark.gpu

HEAD = 400


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from seq2squiggle_amd.cli import set_config
    from seq2squiggle_amd.inference import inference_run
    d = tmp_path_factory.mktemp("predict_eventalign")
    genome = next(iter(U.read_fasta(LAMBDA)))[0].upper()
    (d / "reads.fasta").write_text("".join(f">lambda_{i}\n{genome[3000 * i + 100:3000 * i + 320 + 40 * i]}\n" for i in range(6)))
    U.set_seeds(SEED)
    inference_run(config=set_config(None), saved_weights=CKPT, fasta=str(d / "reads.fasta"), read_input=True, n=-1, r=400, c=-1,
                  out=str(d / "p.blow5"), profile=PROFILE, dwell_mean=20.0, dwell_std=0.0, noise_std=2.0, noise_sampling=True,
                  duration_sampling=True, distr="expon", predict_batch_size=1024, export_every_n_samples=1000000, sample_rate=None, bps=None,
                  digitisation=None, range_val=None, offset_mean=None, offset_std=None, median_before_mean=None, median_before_std=None,
                  min_noise=0.0, min_duration=3, min_read_len=30, preserve_read_ids=True, seed=SEED, events=str(d / "truth.tsv"),
                  events_samples=False, kmer_table=None, kmer_model=str(d / "p.model"))
    recs = [(r["read_id"], np.asarray(r["signal"], np.int16)) for r in SB.open_records(str(d / "p.blow5"))]
    junked = [np.concatenate([recs[(i + 1) % len(recs)][1][-HEAD:], sig]) for i, (_, sig) in enumerate(recs)]
    write_file(d / "j.blow5", [rid for rid, _ in recs], junked)
    fasta = str(d / "reads.fasta")
    gpu = EA.eventalign_files(fasta, d / "j.blow5", d / "p.model", d / "gpu.tsv", summary_out=d / "gpu.sum")
    cpu = EA.eventalign_files(fasta, d / "j.blow5", d / "p.model", d / "cpu.tsv", summary_out=d / "cpu.sum", cpu=True)
    rsq = RSQ.resquiggle_files(fasta, d / "p.blow5", d / "p.model", d / "rsq.tsv")
    return d, gpu, cpu, rsq, {rid: len(x) for (rid, _), x in zip(recs, junked)}


def test_gpu_bytes_equal_cpu_bytes(run):
    d, gpu, cpu, _, _ = run
    assert (d / "gpu.tsv").read_bytes() == (d / "cpu.tsv").read_bytes() and (d / "gpu.sum").read_bytes() == (d / "cpu.sum").read_bytes()
    keys = ("records", "solved", "unreached", "refused", "no_sequence", "no_known_level", "events", "aligned_events", "skipped_kmers",
            "trimmed_head_samples", "trimmed_tail_samples", "mean_cost_per_event")
    assert [gpu[k] for k in keys] == [cpu[k] for k in keys]
    assert gpu["records"] == 6 and gpu["solved"] + gpu["unreached"] == 6 and gpu["k"] == 9 and gpu["refused"] == 0


def test_rows_keep_the_consequences(run):
    d, gpu, _, _, lengths = run
    seqs = {name: RSQ.clean_sequence(seq) for seq, name in U.read_fasta(str(d / "reads.fasta"))}
    table = CMP.read_events(str(d / "gpu.tsv"))
    assert len(table) == gpu["solved"] and sum(len(v) for v in table.values()) == gpu["events"]
    summary = {l.split("\t")[0]: l.rstrip("\n").split("\t") for l in (d / "gpu.sum").read_text().splitlines()[1:]}
    for rid, rows in table.items():
        pos = [int(r[0]) for r in rows]
        assert pos[0] == 0 and (np.diff(pos) >= 1).all() and pos[-1] <= len(seqs[rid]) - 9       # the first assigned event is on k-mer 0
        at = rows[0][2]
        for p, kmer, s, e in rows:
            assert kmer == seqs[rid][int(p):int(p) + 9] and s == at and e > s
            at = e
        assert 0 <= rows[0][2] and at <= lengths[rid]
        assert int(summary[rid][9]) == rows[0][2] and int(summary[rid][10]) == lengths[rid] - at and summary[rid][3] == "solved"
        assert int(summary[rid][8]) == len(seqs[rid]) - 9 + 1 - len(rows)


def share_on_truth(truth, got, lengths, shift):
    total = hit = 0
    for rid, rows in truth.items():
        if rid not in got:
            continue
        mine = np.full(lengths[rid], -1, np.int64)
        for pos, _, s, e in got[rid]:
            mine[s:e] = int(pos)
        for pos, _, s, e in rows:
            total += e - s
            hit += int((mine[s + shift:e + shift] == int(pos)).sum())
    return hit, total


def test_measure_the_share_of_samples_on_their_true_kmer(run):
    d, gpu, _, rsq, lengths = run
    truth = CMP.read_events(str(d / "truth.tsv"))
    hit, total = share_on_truth(truth, CMP.read_events(str(d / "gpu.tsv")), lengths, HEAD)
    rhit, rtotal = share_on_truth(truth, CMP.read_events(str(d / "rsq.tsv")), {k: v - HEAD for k, v in lengths.items()}, 0)
    heads = [int(l.split("\t")[9]) - HEAD for l in (d / "gpu.sum").read_text().splitlines()[1:] if l.split("\t")[3] == "solved"]
    tails = [int(l.split("\t")[10]) for l in (d / "gpu.sum").read_text().splitlines()[1:] if l.split("\t")[3] == "solved"]
    print(f"\neventalign of predict's own output behind {HEAD} samples of another record ({gpu['solved']} of 6 reads solved, {gpu['events']} "
          f"rows of {gpu['aligned_events']} aligned events, {gpu['skipped_kmers']} skipped k-mers, mean cost {gpu['mean_cost_per_event'] or 0:.4f} "
          f"MAD per event): {hit} of {total} samples on their true k-mer = {hit / max(total, 1):.4f}; head trim error per read {heads}, "
          f"samples trimmed at the tail {tails}; resquiggle on the untouched records: {rhit} of {rtotal} = {rhit / max(rtotal, 1):.4f}")
    assert total > 0 and rtotal > 0
