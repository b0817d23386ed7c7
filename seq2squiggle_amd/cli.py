"""`seq2squiggle predict` command line (reference: seq2squiggle.py:43-84, 230-456, 458-599) on plain click.
Same option names and defaults; the other commands of the reference (preprocess, train, sweep) are training
and out of scope."""
import logging
import os
import pathlib
import sys

import click
import yaml

from . import __version__

logger = logging.getLogger("seq2squiggle")


def set_config(config_path) -> dict:
    """YAML config loader (seq2squiggle.py:640-657)."""
    default_config_path = pathlib.Path(__file__).parent / "config.yaml"
    path_to_use = default_config_path if config_path is None else config_path
    try:
        with open(path_to_use, "r") as f_in:
            config = yaml.safe_load(f_in)
    except FileNotFoundError:
        logger.error(f"Configuration file not found: {path_to_use}")
        raise
    except yaml.YAMLError as exc:
        logger.error(f"Error parsing YAML file: {path_to_use} - {exc}")
        raise
    if config_path is None:
        logger.info("Config file was not specified. Default config will be used.")
    return config


@click.group(context_settings=dict(help_option_names=["-h", "--help"]))
def main():
    """seq2squiggle (MI355X engine): predicts nanopore sequencing signals with a feed-forward transformer."""


@main.command()
def version():
    """Print the version."""
    click.echo(__version__)


@main.command(context_settings={"ignore_unknown_options": True})
@click.argument("fasta", required=False, type=click.Path(exists=False, file_okay=True, dir_okay=False, path_type=pathlib.Path))
@click.option("--read-input", default=False, is_flag=True, show_default=True,
              help="Read mode: simulate signals directly from the reads of a FASTA/FASTQ file.")
@click.option("-n", "--num-reads", type=int, default=-1, help="Number of generated reads.")
@click.option("-r", "--read-length", type=int, default=1000, show_default=True, help="Average read length.")
@click.option("-c", "--coverage", type=int, default=-1, help="Genome coverage.")
@click.option("-o", "--out", required=False, type=click.Path(file_okay=True, dir_okay=False, path_type=pathlib.Path),
              help="Output POD5/SLOW5/BLOW5 file.")
@click.option("--profile", default="dna-r10-prom", show_default=True,
              type=click.Choice(["dna-r10-prom", "dna-r10-min", "dna-r9-prom", "dna-r9-min", "rna-004-prom", "rna-004-min"]))
@click.option("--show-advanced-options", is_flag=True, default=False, help="Show advanced options.")
@click.option("--noise-sampler", default=True, type=bool, show_default=True, hidden=True)
@click.option("--duration-sampler", default=True, type=bool, show_default=True, hidden=True)
@click.option("--dwell-mean", default=None, type=float, hidden=True)
@click.option("--dwell-std", default=0.0, type=float, hidden=True)
@click.option("--noise-std", default=2.0, type=float, hidden=True)
@click.option("--distr", default="expon", type=click.Choice(["expon", "beta", "gamma"]), hidden=True)
@click.option("--predict-batch-size", default=1024, type=int, hidden=True)
@click.option("--export-every-n-samples", default=1000000, type=int, hidden=True)
@click.option("--sample-rate", default=None, type=int, hidden=True)
@click.option("--bps", default=None, type=int, hidden=True)
@click.option("--digitisation", default=None, type=int, hidden=True)
@click.option("--range_val", default=None, type=float, hidden=True)
@click.option("--offset_mean", default=None, type=float, hidden=True)
@click.option("--offset_std", default=None, type=float, hidden=True)
@click.option("--median_before_mean", default=None, type=float, hidden=True)
@click.option("--median_before_std", default=None, type=float, hidden=True)
@click.option("--min_noise", default=0.0, type=float, hidden=True)
@click.option("--min_duration", default=3, type=int, hidden=True)
@click.option("--min_read_len", default=30, type=int, hidden=True)
@click.option("--preserve-read-ids", is_flag=True, default=False,
              help="Keep the input read ids instead of generated ones.")
@click.option("-s", "--seed", type=int, default=0, help="Seed for reproducibility (0 = random).")
@click.option("-m", "--model", type=click.Path(exists=False, dir_okay=False), help="Model weights (.ckpt).")
@click.option("-y", "--config", help="YAML configuration file overriding the defaults.")
@click.option("-v", "--verbosity", type=click.Choice(["debug", "info", "warning", "error"], case_sensitive=False), default="info")
@click.option("--compute-mode", default=None,
              type=click.Choice(["f16x3", "f32", "f16", "generic", "generic-f16", "generic-geometry", "generic-geometry-f16"]),
              hidden=True, help="Decoder arithmetic of the MI355X engine (default: f16x3 for the shipped model sizes, generic for any "
                                "other; generic-f16: any size, reduced precision; generic-geometry: any size and any "
                                "max_dna_len / max_signal_len, the default for a geometry other than 16 / 250; "
                                "generic-geometry-f16: the same at reduced precision, opt-in only).")
@click.option("--attention-path", default="auto", type=click.Choice(["auto", "fast", "exact"]), hidden=True,
              help="Softmax path of the split-f16 decoder: auto = chosen per checkpoint by the engine's calibration launch "
                   "(include/s2s_hip.h: s2s_set_attention_path); exact = the same time whatever the weights.")
@click.option("--alignment", default=None, type=click.Path(dir_okay=False), hidden=True,
              help="Also write the ground-truth base-to-signal alignment: one PAF line per record of OUT with the samples of every "
                   "k-mer in the signal as stored (ss:Z: tag; include/s2s_hip.h: s2s_paf_format). Off by default.")
@click.option("--events", default=None, type=click.Path(dir_okay=False), hidden=True,
              help="Also write the per-k-mer event table of the simulated reads: one tab-separated row per k-mer with samples "
                   "(read_name, position, model_kmer, start_idx, end_idx, event_level_mean, event_stdv; include/s2s_hip.h: "
                   "s2s_events_format). Off by default.")
@click.option("--events-samples", is_flag=True, hidden=True,
              help="With --events: add the samples column (every stored sample of the event in pA, comma separated).")
@click.option("--kmer-table", default=None, type=click.Path(dir_okay=False), hidden=True,
              help="Also write the k-mer table of the run: one tab-separated row per k-mer that occurred (kmer, n_occ, n_events, "
                   "n_samples, level_mean, level_stdv, dwell_mean, dwell_stdv; include/s2s_hip.h: s2s_kmer_table_format), summed on "
                   "the GPU over all reads. Off by default.")
@click.option("--kmer-model", default=None, type=click.Path(dir_okay=False), hidden=True,
              help="Also write the k-mer model of the run: a nanopolish-style pore model with one tab-separated row per ACGT k-mer "
                   "that got events (kmer, level_mean, level_stdv, sd_mean, sd_stdv, n_events: statistics of EVENT means, "
                   "include/s2s_hip.h: s2s_kmer_model_format), summed on the GPU over all reads. Off by default.")
@click.option("--gpus", default=1, type=int, hidden=True,
              help="Run on this many GPUs of the node: one process per GPU, the read set sharded, one OUT.rankN file per process "
                   "(the same as starting the command under torchrun --nproc-per-node N).")
@click.option("--keep-shards", is_flag=True, hidden=True,
              help="With --gpus N: leave the OUT.rankN files as they are instead of merging them into OUT.")
@click.option("--join", "join_mode", default="after", type=click.Choice(["after", "live"]), hidden=True,
              help="With --gpus N: after = the rank files are joined in rank order once the ranks are done (the layout of a single-process "
                   "file); live = the parent copies complete records / signal batches into OUT while the ranks run (round robin over the "
                   "ranks: same reads, another record order; .blow5 and .pod5).")
@click.pass_context
def predict(ctx, fasta, read_input, num_reads, read_length, coverage, out, profile, show_advanced_options, noise_sampler,
            duration_sampler, dwell_mean, dwell_std, noise_std, distr, predict_batch_size, export_every_n_samples,
            sample_rate, bps, digitisation, range_val, offset_mean, offset_std, median_before_mean, median_before_std,
            min_noise, min_duration, min_read_len, preserve_read_ids, seed, model, config, verbosity, compute_mode, attention_path,
            alignment, events, events_samples, kmer_table, kmer_model, gpus, keep_shards, join_mode):
    """Generate nanopore signals from a reference genome (default) or from reads (--read-input)."""
    import os
    if events_samples and not events:
        raise click.UsageError("--events-samples needs --events OUT.tsv")
    if gpus > 1 and "WORLD_SIZE" not in os.environ:
        # The reference leaves multi-GPU runs to Lightning (devices="auto", DDP: inference.py:430-445); here the command starts its
        # own ranks as CHILD processes -- before anything in this process has touched the GPU -- and returns their exit code.
        if fasta is None or out is None:
            click.echo("FASTA and -o/--out are required")
            ctx.exit(1)
        if str(out).endswith(".pod5") and os.path.exists(out) and not keep_shards:
            raise FileExistsError(f"{out} exists (the POD5 writer refuses to overwrite, like pod5.Writer)")
        import time
        t0 = time.time()
        live, make_live = None, None
        ext_a = os.path.splitext(str(alignment))[1] if alignment else ""
        align_shards = [f"{str(alignment)[:len(str(alignment)) - len(ext_a)]}.rank{r}{ext_a}" for r in range(gpus)] if alignment else []
        ext_e = os.path.splitext(str(events))[1] if events else ""
        events_shards = [f"{str(events)[:len(str(events)) - len(ext_e)]}.rank{r}{ext_e}" for r in range(gpus)] if events else []
        if events and os.environ.get("S2S_DRY_LAUNCH"):
            import json
            click.echo(json.dumps({"events_rank_files": events_shards}))
        model_shards = [f"{os.path.splitext(str(kmer_model))[0]}.rank{r}.npz" for r in range(gpus)] if kmer_model else []
        if kmer_model and os.environ.get("S2S_DRY_LAUNCH"):
            import json
            click.echo(json.dumps({"kmer_model_rank_files": model_shards}))
        table_shards = [f"{os.path.splitext(str(kmer_table))[0]}.rank{r}.npz" for r in range(gpus)] if kmer_table else []
        if kmer_table and os.environ.get("S2S_DRY_LAUNCH"):
            import json
            click.echo(json.dumps({"kmer_table_rank_files": table_shards}))
        if join_mode == "live" and not keep_shards and not os.environ.get("S2S_DRY_LAUNCH"):
            if not str(out).endswith((".blow5", ".pod5")):
                raise click.UsageError("--join live handles .blow5 and .pod5 outputs")
            ext = os.path.splitext(str(out))[1]
            base_name = str(out)[:len(str(out)) - len(ext)]
            partial = base_name + ".partial" + ext
            shard_paths = [f"{base_name}.rank{r}{ext}" for r in range(gpus)]       # (parallel.rank_output_path, without its imports)
            for stale in [partial] + shard_paths + align_shards + events_shards + table_shards + model_shards:   # (a rank file left by an earlier run must not be mistaken for this run's)
                if os.path.exists(stale):
                    os.remove(stale)
            holder = {}

            def make_live():                                # (called once the ranks are started: numpy loads beside their start-up, not before it)
                from .merge import LiveJoin
                holder["live"] = LiveJoin(shard_paths, partial)
                return holder["live"]
        try:
            rc, timing, reap = _launch_ranks(gpus, make_live)
        except BaseException:
            if make_live is not None and holder.get("live") is not None:
                holder["live"].abort()          # (a rank file the live join could not make sense of: no partial output stays behind)
            raise
        live = holder.get("live") if make_live is not None else None
        try:
            timing["ranks_seconds"] = time.time() - t0
            if live is not None:
                if rc == 0:
                    t1 = time.time()
                    try:
                        n, st = live.finish(consume=True)
                        os.replace(live.out, str(out))
                    except BaseException:
                        live.abort()
                        raise
                    timing.update(merge_seconds=time.time() - t1, merge_bytes=st["bytes"], merge_bytes_copied=st["bytes"], reads=n, join="live",
                                  live_bytes=st["live_bytes"], live_copy_seconds=st["copy_seconds"], join_order=st["order"])
                    click.echo(f"{n} reads from {gpus} ranks -> {out}  [launch {round(timing.get('launch_seconds', 0), 2)} s, ranks "
                               f"{timing['ranks_seconds']:.2f} s in all with {st['live_bytes'] / 1e9:.2f} of {st['bytes'] / 1e9:.2f} GB joined meanwhile, "
                               f"{timing['merge_seconds']:.2f} s to finish the file; {st['order']}]")
                else:
                    live.abort()
            elif rc == 0 and not keep_shards and not os.environ.get("S2S_DRY_LAUNCH"):
                # one output file, as the reference writes (inference.py:65-79): the first rank's file becomes OUT, the payload of the
                # others moves in as byte ranges on copy threads (merge.py), the rank files are gone afterwards
                from .parallel import rank_output_path
                from .signal_io import merge_shards as _merge
                shards = [rank_output_path(str(out), r, gpus) for r in range(gpus)]
                t1 = time.time()
                n = _merge(shards, str(out), consume=True)
                timing["merge_seconds"] = time.time() - t1
                timing["merge_bytes"] = _merge.last.get("bytes", 0)
                timing["merge_bytes_copied"] = _merge.last.get("bytes_copied", 0)
                timing["reads"] = n
                launch = timing.get("launch_seconds")
                click.echo(f"{n} reads from {gpus} ranks -> {out}  [launch {launch if launch is None else round(launch, 2)} s, "
                           f"ranks {timing['ranks_seconds']:.2f} s in all, merge {timing['merge_seconds']:.2f} s for "
                           f"{timing['merge_bytes'] / 1e9:.2f} GB]")
            if alignment and rc == 0 and not keep_shards and not os.environ.get("S2S_DRY_LAUNCH"):
                # the ranks own contiguous shares of the reads: their alignment files in rank order are the single-process file
                from .alignment import join_rank_files
                join_rank_files(align_shards, str(alignment))
            if events and rc == 0 and not keep_shards and not os.environ.get("S2S_DRY_LAUNCH"):
                from .events import join_rank_files as join_event_files     # (the header of rank 0 only)
                join_event_files(events_shards, str(events))
            if kmer_table and rc == 0 and not os.environ.get("S2S_DRY_LAUNCH"):
                # integer counts: their sum over the ranks is the single-process table (--keep-shards leaves the .npz beside it)
                from .kmer_table import join_rank_files as join_table_files
                join_table_files(table_shards, str(kmer_table), keep=keep_shards)
            if kmer_model and rc == 0 and not os.environ.get("S2S_DRY_LAUNCH"):
                from .kmer_model import join_rank_files as join_model_files
                join_model_files(model_shards, str(kmer_model), keep=keep_shards)
            late = reap()                                       # (the merge did not wait for the ranks' teardown: see _launch_ranks)
            rc = rc or late
            timing["total_seconds"] = time.time() - t0
            try:
                import resource
                # (the peak counts the tmpfs pages of the output while they are mapped for the fill -- one shard's span, shared memory that
                #  belongs to the file, not to this process; what the process itself holds is the anonymous part)
                timing["parent_peak_rss_mb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
                for line in open("/proc/self/status"):
                    if line.startswith("RssAnon:"):
                        timing["parent_anon_rss_mb"] = int(line.split()[1]) / 1024.0
            except (ImportError, OSError):
                pass
            if os.environ.get("S2S_TIMING_JSON") and not os.environ.get("S2S_DRY_LAUNCH"):
                import json
                with open(os.environ["S2S_TIMING_JSON"], "w") as f:
                    json.dump(timing, f)
        except BaseException:
            reap(force=True)                    # (a failed join: no rank process and no s2s-ranks-* directory stays behind)
            raise
        ctx.exit(rc)
    # a rank of a multi-process run binds itself to its share of its GPU's socket FIRST: before torch starts its thread pools,
    # before the first page of a pinned staging buffer is touched (placement.pin_rank; S2S_NO_PIN=1 opts out)
    from .placement import pin_rank
    pinned = pin_rank()
    from .inference import inference_run
    from .utils import set_seeds, setup_logging

    if show_advanced_options:
        for p in ctx.command.params:
            p.hidden = False
        click.echo(ctx.get_help())
        ctx.exit()
    if not fasta or not out:
        logger.error("FASTA file and Output file are required for prediction.")
        ctx.exit(1)
    setup_logging(verbosity)
    logger.info("seq2squiggle (MI355X engine) version %s", str(__version__))
    if pinned:
        logger.debug(f"rank {os.environ.get('RANK', '0')}: bound to CPUs {pinned['cpus']} ({pinned['source']}"
                     + (f": NUMA node {pinned['numa_node']} of GPU {pinned['bdf']}" if pinned["source"] == "sysfs" else "") + ")")
    cfg = set_config(config)
    import time
    t_ready = time.time()                      # interpreter, torch and the library are loaded: what a rank pays before its first read
    from .parallel import shared_seed
    seed = set_seeds(shared_seed(seed))        # --seed 0 under torchrun: rank 0's fresh seed, for every rank
    inference_run(config=cfg, saved_weights=model, fasta=str(fasta), read_input=read_input, n=num_reads, r=read_length,
                  c=coverage, out=str(out), profile=profile, dwell_mean=dwell_mean, dwell_std=dwell_std, noise_std=noise_std,
                  noise_sampling=noise_sampler, duration_sampling=duration_sampler, distr=distr,
                  predict_batch_size=predict_batch_size, export_every_n_samples=export_every_n_samples,
                  sample_rate=sample_rate, bps=bps, digitisation=digitisation, range_val=range_val,
                  offset_mean=offset_mean, offset_std=offset_std, median_before_mean=median_before_mean,
                  median_before_std=median_before_std, min_noise=min_noise, min_duration=min_duration,
                  min_read_len=min_read_len, preserve_read_ids=preserve_read_ids, seed=seed, mode=compute_mode,
                  attention_path=attention_path, alignment=alignment, events=events, events_samples=events_samples,
                  kmer_table=kmer_table, kmer_model=kmer_model)
    logger.info("Prediction finished.")
    if os.environ.get("S2S_TIMING_DIR"):       # a rank of `predict --gpus N`: when it was ready and when it was done, for the parent's summary
        import json
        stamp = os.path.join(os.environ["S2S_TIMING_DIR"], f"rank{os.environ.get('RANK', '0')}.json")
        with open(stamp + ".tmp", "w") as f:
            json.dump({"ready": t_ready, "done": time.time()}, f)
        os.replace(stamp + ".tmp", stamp)      # (appears whole: the parent starts the merge when it sees every rank's)
        # The file is closed and the parent has been told: leave without the interpreter's and torch's teardown (0.3 - 0.5 s per
        # rank that the parent would wait for before it may return; the driver reclaims the device memory of a process that ends)
        logging.shutdown()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


def _launch_ranks(gpus: int, make_live=None, cmd=None):
    """`predict --gpus N` outside torchrun: the same command line once per GPU, as N CHILD processes of this one (which never touches
    the GPU) with the environment torchrun would give them (RANK, LOCAL_RANK, WORLD_SIZE, LOCAL_WORLD_SIZE, MASTER_ADDR = 127.0.0.1,
    MASTER_PORT) -- started directly: the elastic agent of torch.distributed.run costs an import of torch in the parent and a
    rendezvous before the first rank starts, and there is nothing here for it to supervise.  The first rank that fails ends the
    others (by their pids).  S2S_DRY_LAUNCH=1 prints the child command and environment instead of running it.
    -> (exit code, {"launch_seconds": spawn -> the slowest rank is ready to read its input, "predict_seconds": ... -> the slowest is
    done}, reap): returns as soon as every rank's output file is complete and closed; reap() collects the processes afterwards.
    make_live() -> merge.LiveJoin, called once the ranks are started: its step() runs in the waiting loop, so that the rank files are
    joined while they grow."""
    import json
    import os
    import shutil
    import socket
    import subprocess
    import tempfile
    import time
    argv, skip = [], False
    for a in sys.argv[1:]:
        if skip:
            skip = False
            continue
        if a == "--gpus":
            skip = True
            continue
        if a.startswith("--gpus=") or a == "--keep-shards":
            continue
        argv.append(a)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = cmd or [sys.executable, "-m", "seq2squiggle_amd"] + argv       # (cmd: the supervision tests start stand-in ranks)
    from .placement import rank_visibility, visible_list
    parent_visible = visible_list()

    def rank_env(r):
        # one device per rank (HIP_VISIBLE_DEVICES = the r-th device this process may see): a rank cannot place anything on a
        # neighbour's GPU, whatever a call site passes; S2S_PARENT_VISIBLE lets every rank work out the same CPU table (placement.pin_rank)
        return {"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(gpus), "LOCAL_WORLD_SIZE": str(gpus),
                "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                "S2S_PARENT_VISIBLE": ",".join(parent_visible) if parent_visible is not None else "", **rank_visibility(r)}
    if os.environ.get("S2S_DRY_LAUNCH"):
        click.echo(json.dumps({"dry_launch": cmd, "rank_env": [rank_env(r) for r in range(gpus)]}))
        return 0, {}, lambda force=False: 0
    timing_dir = tempfile.mkdtemp(prefix="s2s-ranks-")
    base = dict(os.environ, S2S_TIMING_DIR=timing_dir)
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    t0 = time.time()
    import signal

    class _Ended(BaseException):
        """SIGTERM / SIGHUP to the launcher: unwinds through the handlers below, which end the ranks."""

    def _on_signal(signum, frame):
        raise _Ended(signum)
    old_handlers = {}
    for sig in (signal.SIGTERM, signal.SIGHUP):
        try:                                     # (only the main thread may install handlers: tests call this from there too)
            old_handlers[sig] = signal.signal(sig, _on_signal)
        except (ValueError, OSError):
            pass
    procs = []
    try:
        for r in range(gpus):
            procs.append(subprocess.Popen(cmd, env=dict(base, **rank_env(r))))
    except BaseException:
        for p_ in procs:
            p_.kill()
        raise
    rc = 0

    def end_ranks(which, grace=float(os.environ.get("S2S_RANK_GRACE", "10"))):
        """terminate(), then kill() for whoever has not left after `grace` seconds (a rank stuck in a HIP call ignores SIGTERM)."""
        alive = [procs[q] for q in which if procs[q].poll() is None]
        for p_ in alive:
            p_.terminate()
        deadline = time.time() + grace
        for p_ in alive:
            try:
                p_.wait(timeout=max(0.0, deadline - time.time()))
            except subprocess.TimeoutExpired:
                p_.kill()
        for p_ in alive:
            try:
                p_.wait(timeout=30)
            except subprocess.TimeoutExpired:
                pass

    def stamps():
        try:
            names = os.listdir(timing_dir)
            return [json.load(open(os.path.join(timing_dir, f))) for f in names if f.endswith(".json")]
        except (OSError, ValueError):
            return []

    def reap(force: bool = False) -> int:
        """Waits for the ranks that are still shutting down (interpreter, torch and HIP teardown: ~0.3 s each, which the merge
        does not have to wait for) -> the first non-zero exit code, or 0.  force: the command is failing -- end them now.
        Idempotent; also gives the signal handlers back and removes the stamp directory."""
        code = 0
        if force:
            end_ranks(range(len(procs)))
        for p_ in procs:
            try:
                code = code or p_.wait(timeout=120)
            except subprocess.TimeoutExpired:
                p_.kill()
                code = code or 1
        for sig, h in old_handlers.items():
            try:
                signal.signal(sig, h)
            except (ValueError, OSError):
                pass
        old_handlers.clear()
        shutil.rmtree(timing_dir, ignore_errors=True)
        return code
    live = None
    try:
        if make_live is not None:
            live = make_live()
        try:                                    # the merge's imports (numpy, pyarrow, the library) load while the ranks work
            from . import merge, pod5_io, signal_io  # noqa: F401
            pod5_io._pa()
            from ._lib import lib
            lib()
        except Exception:                       # (reported by the merge itself, if it comes to that)
            pass
        left = set(range(gpus))
        # a rank writes its stamp when its output file is complete and closed (end of `predict`): once every rank has, the files
        # can be joined -- the processes may still be tearing down
        while left:
            stamped = {f for f in os.listdir(timing_dir) if f.endswith(".json")}
            if len(stamped) >= gpus:
                break
            moved = live is not None and live.step([f"rank{r}.json" in stamped for r in range(gpus)])   # (--join live: copy what is complete)
            for r in sorted(left):
                code = procs[r].poll()
                if code is None:
                    continue
                left.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    logger.error(f"rank {r} exited with code {code}; ending the other ranks")
                    end_ranks(sorted(left))
            if left and not moved:
                time.sleep(0.005)
    except BaseException:
        reap(force=True)
        raise
    timing = {}
    rows = stamps() if rc == 0 else []
    if len(rows) < gpus and rc == 0 and not left:      # every rank exited cleanly; a stamp may have been written a moment ago
        rows = stamps()
    if len(rows) == gpus:
        timing = {"launch_seconds": max(x["ready"] for x in rows) - t0,
                  "predict_seconds": max(x["done"] for x in rows) - max(x["ready"] for x in rows)}
    elif rc == 0:
        rc = reap() or 1                              # a rank ended without its stamp: not a complete set of files
    return rc, timing, reap


@main.command("merge-shards")
@click.argument("shards", nargs=-1, required=True, type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--out", required=True, type=click.Path(dir_okay=False), help="Merged .blow5 / .slow5 / .pod5 file.")
@click.option("--threads", default=None, type=int, help="Copy threads (default: this process's CPU share).")
@click.option("--consume", is_flag=True, help="Turn the first shard into the output and delete the others (moves 1/N fewer bytes).")
def merge_shards(shards, out, threads, consume):
    """Join the OUT.rankN.blow5 (or .slow5 / .pod5) shard files of a multi-GPU run, in the order given, into one file: raw byte
    ranges on copy threads, nothing is decompressed.  (Read ids and read numbers already continue across the shards of one run.)"""
    from .signal_io import merge_shards as _merge
    n = _merge(list(shards), out, threads=threads, consume=consume)
    st = _merge.last
    click.echo(f"{n} records -> {out}  [{st.get('bytes', 0) / 1e9:.3f} GB in {st.get('seconds', 0):.2f} s]")



MODES = ["f16x3", "f32", "f16", "generic", "generic-f16", "generic-geometry", "generic-geometry-f16"]


@main.command()
@click.argument("data_dir", type=click.Path(file_okay=False, path_type=pathlib.Path))
@click.option("-m", "--model", "models", multiple=True, required=True, type=click.Path(dir_okay=False),
              help="Checkpoint (.ckpt); repeat for several (one row each).")
@click.option("--compute-mode", default=None, type=click.Choice(MODES),
              help="Engine instance, as for predict (default: f16x3 for the shipped sizes, generic for others, generic-geometry for a "
                   "chunk geometry other than 16 / 250).")
@click.option("--max-chunks", default=0, type=int, show_default=True,
              help="Evaluate the first N chunks in file order (the reference's valid_limit); 0 = all.")
@click.option("--batch-size", default=65536, type=int, show_default=True, help="Chunks per GPU call.")
@click.option("--per-chunk", "per_chunk", default=None, type=click.Path(dir_okay=False),
              help="Write the per-chunk sums (signal, duration NLL, noise) of every checkpoint to this .npz.")
@click.option("--json", "as_json", is_flag=True, help="Print one JSON object per checkpoint instead of the table.")
def evaluate(data_dir, models, compute_mode, max_chunks, batch_size, per_chunk, as_json):
    """Teacher-forced validation losses (valid_signal / duration / noise / total_loss of the reference's validation_step) of
    one or more checkpoints on a preprocess directory (chunks-NNNN.npy ... or chunks.npy ...), on the GPU."""
    if batch_size < 1:
        raise click.BadParameter("must be >= 1", param_hint="--batch-size")
    if max_chunks < 0:
        raise click.BadParameter("must be >= 0", param_hint="--max-chunks")
    if not data_dir.is_dir():
        raise click.BadParameter(f"{data_dir} is not a directory", param_hint="DATA_DIR")
    for m in models:
        if not os.path.isfile(m):
            raise click.BadParameter(f"{m} does not exist", param_hint="--model")
    import json
    import numpy as np
    import torch  # noqa: F401  (before the library: see engine.py)
    from .checkpoint import load_checkpoint
    from .engine import Engine
    from .evaluate import EvalData, evaluate as run
    arrays = {}
    for i, m in enumerate(models):
        sd, cfg = load_checkpoint(m)
        try:
            data = EvalData(str(data_dir), cfg, max_chunks)
        except ValueError as e:
            raise click.ClickException(f"{m}: {e}")
        eng = Engine(sd, cfg, mode=compute_mode)
        losses, sums, secs = run(eng, data, batch_size)
        eng.close()
        row = dict(model=str(m), mode=eng.mode, chunks=int(data.n), chunks_per_s=data.n / secs if secs > 0 else None, **losses)
        arrays[f"model{i}"] = sums
        if as_json:
            click.echo(json.dumps(row))
        else:
            click.echo(f"{m}  [{eng.mode}, {data.n} chunks, {row['chunks_per_s']:,.0f} chunks/s]  signal {losses['valid_signal_loss']:.6g}  "
                       f"duration {losses['valid_duration_loss']:.6g}  noise {losses['valid_noise_loss']:.6g}  "
                       f"total {losses['valid_total_loss']:.6g}")
    if per_chunk:
        np.savez(per_chunk, models=np.array([str(m) for m in models]), **arrays)


def _signal_files(command: str, *paths) -> None:
    """The signal-analysis commands read .blow5 / .slow5 only: refuse anything else by its name, before any work."""
    for p in paths:
        if str(p).endswith(".pod5"):
            raise click.UsageError(f"{p}: {command} reads .blow5 and .slow5 files; reading POD5 is not supported")
        if not str(p).endswith((".blow5", ".slow5")):
            raise click.UsageError(f"{p}: {command} reads .blow5 and .slow5 files")


@main.command()
@click.argument("a", type=click.Path(dir_okay=False))
@click.argument("b", type=click.Path(dir_okay=False))
@click.option("-o", "--out", required=True, type=click.Path(dir_okay=False), help="Output table (.tsv), one row per pair of records.")
@click.option("--band", default=512, type=int, show_default=True,
              help="Half width of the DTW band in samples of the shorter signal.  The default is a choice, not a measurement: the dwell "
                   "drift over a 5 kb read is a few hundred samples.")
@click.option("--normalise", "normalise", default="mad", type=click.Choice(["mad", "none"]), show_default=True,
              help="mad: (x - median) / MAD per record, in integer steps of 1/64 MAD; none: the stored samples as they are.")
@click.option("--by-order", is_flag=True, help="Pair the k-th record of A with the k-th of B instead of pairing by read id.")
@click.option("--max-samples", default=1 << 27, type=int, show_default=True, help="Samples of both files per batch.")
@click.option("--cpu", is_flag=True, help="Compute on host threads instead of the GPU (the same integers).")
@click.option("--json", "as_json", is_flag=True, help="Print the summary as one JSON object.")
@click.option("--path", "path_out", default=None, type=click.Path(dir_okay=False),
              help="Also trace the warping path of every pair and write it here (.paths.tsv): read_id, n_a, n_b, band, dtw, steps, path; "
                   "path is run-length encoded (12M3A1M2B: M both signals step, A only A's, B only B's; * for no steps).")
@click.option("--events-a", default=None, type=click.Path(dir_okay=False, exists=True),
              help="The event table `predict --events` wrote for file A; needs --events-out.")
@click.option("--events-out", default=None, type=click.Path(dir_okay=False),
              help="Write A's events carried through the warping path onto B's samples: start_idx / end_idx in B, level and deviation "
                   "of B's stored samples with the offset, range and digitisation of B's record; events that map to no sample are dropped.")
@click.option("--path-memory", default=8 << 30, type=int, show_default=True,
              help="Bytes of decision scratch per batch with --path / --events-out; a pair that needs more is refused.  With "
                   "--open-ends a pair is refused when its interval of B is known, in front of its batch: the rows of earlier batches "
                   "are already written then.")
@click.option("--open-ends", is_flag=True,
              help="B may carry samples in front of and behind what A holds (adapter, stall, open pore, trailing samples): locate the "
                   "first and the last --anchor samples of A inside the first and the last --anchor-window samples of B by subsequence "
                   "DTW and compare A with that interval of B only.  OUT gains b_start, b_end, head_cost, tail_cost, the path rows "
                   "b_start, b_end; carried events come out in B's own coordinates.  To trim A instead, swap the files.")
@click.option("--anchor", default=None, type=int,
              help="Samples of A's head and tail that are located in B (--open-ends).  [default: 1024]  A choice, not a measurement: "
                   "long enough to be unmistakable, short enough to sit inside one window.")
@click.option("--anchor-window", default=None, type=int,
              help="Samples of B's head and tail the anchors are searched in (--open-ends).  [default: 16384]  A choice, not a "
                   "measurement: a DNA adapter is on the order of a thousand samples, and the window must cover the adapter plus the anchor.")
def compare(a, b, out, band, normalise, by_order, max_samples, cpu, as_json, path_out, events_a, events_out, path_memory, open_ends,
            anchor, anchor_window):
    """Banded dynamic-time-warping distance between the signals of two .blow5 / .slow5 files, record against record (paired by read
    id, in A's order): OUT gets read_id, n_a, n_b, med_a, mad_a, med_b, mad_b, band, dtw, dtw_per_sample.  Everything is computed in
    integers on the stored int16 samples; dtw_per_sample = dtw / (n_a + n_b) / 64, in MADs per step with --normalise mad.
    The alignment is global: a record of B that carries samples A lacks (a real read against a simulated one) needs --open-ends."""
    _signal_files("compare", a, b)
    if max_samples < 1:
        raise click.BadParameter("must be >= 1", param_hint="--max-samples")
    if path_memory < 1:
        raise click.BadParameter("must be >= 1", param_hint="--path-memory")
    if (events_a is None) != (events_out is None):
        raise click.UsageError("--events-a and --events-out go together")
    if not open_ends and (anchor is not None or anchor_window is not None):
        raise click.UsageError("--anchor and --anchor-window need --open-ends")
    import json
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    from . import compare as C, signal_batch as SB
    if not 1 <= band <= SB.max_band():
        raise click.BadParameter(f"must be 1..{SB.max_band()}", param_hint="--band")
    open_kw = {}
    if open_ends:
        anchor = C.DEFAULT_ANCHOR if anchor is None else anchor
        anchor_window = C.DEFAULT_ANCHOR_WINDOW if anchor_window is None else anchor_window
        if not 1 <= anchor <= C.max_query():
            raise click.BadParameter(f"must be 1..{C.max_query()}", param_hint="--anchor")
        if not 1 <= anchor_window <= SB.MAX_SAMPLES:
            raise click.BadParameter(f"must be 1..{SB.MAX_SAMPLES}", param_hint="--anchor-window")
        open_kw = dict(open_ends=True, anchor=anchor, anchor_window=anchor_window)
    s = C.compare_files(a, b, out, band=band, normalise=normalise, by_order=by_order, max_samples=max_samples, cpu=cpu,
                        path_out=path_out, events_a=events_a, events_out=events_out, path_memory=path_memory, **open_kw)
    if as_json:
        click.echo(json.dumps(s))
    else:
        if events_out is not None:
            click.echo(f"{s['events_written']} events -> {events_out}  [{s['events_dropped']} dropped: no sample of B; "
                       f"{s['events_unpaired']} of reads without a pair]")
        fmt = lambda v: "nan" if v is None else f"{v:.6f}"      # noqa: E731
        if open_ends:
            click.echo(f"open ends: anchor {anchor} in windows of {anchor_window}; {s['anchors_crossed']} pair(s) with crossed anchors "
                       f"compared against all of B")
        click.echo(f"{s['pairs']} pairs -> {out}  [band {band}, normalise {normalise}; unpaired: {s['unpaired_a']} of {s['records_a']} in "
                   f"{a}, {s['unpaired_b']} of {s['records_b']} in {b}]  dtw_per_sample mean {fmt(s['mean_dtw_per_sample'])}  "
                   f"median {fmt(s['median_dtw_per_sample'])}")


def _options(*decorators):
    """Several click decorators as one; --help lists their options in the order given."""
    def stack(f):
        for d in reversed(decorators):
            f = d(f)
        return f
    return stack


def _in_range(value, lo, hi, hint, lo_name=None) -> None:
    """A BadParameter that names the option `hint` unless lo <= value <= hi (hi None: no upper end)."""
    if value < lo or (hi is not None and value > hi):
        raise click.BadParameter(f"must be >= {lo}" if hi is None else f"must be {lo_name or lo}..{hi}", param_hint=hint)


def _echo_summary(s: dict, as_json: bool, text: str) -> None:
    """The end of a signal command: the summary as one JSON object with --json, else the text line."""
    import json
    click.echo(json.dumps(s) if as_json else text)


def _detector_options(detector: str, short_tail: str, long_tail: str):
    """The four options of segment's event detector, for `segment` and `eventalign`."""
    return _options(
        click.option("--window-short", default=3, type=int, show_default=True, help=f"Window of the short {detector} in samples (1..32)."),
        click.option("--window-long", default=6, type=int, show_default=True, help=f"Window of the long {detector} in samples (short..32)."),
        click.option("--threshold-short", default=1.4, type=float, show_default=True, help=f"Threshold t of the short detector{short_tail}"),
        click.option("--threshold-long", default=9.0, type=float, show_default=True, help=f"Threshold t of the long detector{long_tail}"))


def _check_detector(window_short, window_long, threshold_short, threshold_long) -> None:
    from . import segment as SEG
    _in_range(window_short, 1, SEG.MAX_WINDOW, "--window-short")
    _in_range(window_long, window_short, SEG.MAX_WINDOW, "--window-long", "--window-short")
    for hint, t in (("--threshold-short", threshold_short), ("--threshold-long", threshold_long)):
        try:
            SEG.threshold_int(t)
        except ValueError as e:
            raise click.BadParameter(str(e), param_hint=hint)


def _aligner_options(rows: str, unit: str, trace_memory: str, band, after_skip=(), after_rna=()):
    """The options of the commands that align reads to a pore model (pore_align.align_files), in --help's order.  rows / unit / trace_memory:
    the command's own words in the help of --samples, of --skip-penalty and --unknown-cost, and of --trace-memory; band, after_skip,
    after_rna: its own options."""
    return _options(
        click.argument("seqs", type=click.Path(dir_okay=False, exists=True)),
        click.argument("signals", type=click.Path(dir_okay=False)),
        click.option("--kmer-model", "model", required=True, type=click.Path(dir_okay=False, exists=True),
                     help="Pore model: the file `predict --kmer-model` writes, or a nanopolish-style table with the columns kmer and level_mean."),
        click.option("-o", "--out", required=True, type=click.Path(dir_okay=False), help="Output event table (.events.tsv)."),
        click.option("--samples", "with_samples", is_flag=True, help=f"Add the `samples` column: every {rows} samples in pA."),
        band,
        click.option("--skip-penalty", default=128, type=int, show_default=True,
                     help=f"Cost of a k-mer that gets no {unit}, in 1/64 MAD.  The default, two MADs, is a choice, not a measurement."),
        *after_skip,
        click.option("--unknown-cost", default=64, type=int, show_default=True,
                     help=f"Cost per {unit} on a k-mer the model has no level for (or with a letter outside ACGT), in 1/64 MAD.  The "
                          "default, one MAD, is a choice, not a measurement."),
        click.option("--rna", is_flag=True, help="The stored signal is reversed (RNA profiles): read the levels back to front; position stays in "
                                                 "read coordinates and start_idx falls as it rises, as in predict --events."),
        *after_rna,
        click.option("--cpu", is_flag=True, help="Compute on host threads instead of the GPU (the same bytes)."),
        click.option("--json", "as_json", is_flag=True, help="Print the summary as one JSON object."),
        click.option("--summary", "summary_out", default=None, type=click.Path(dir_okay=False), help="Also write one row per read here (.tsv)."),
        click.option("--max-samples", default=1 << 27, type=int, show_default=True, help="Samples per batch."),
        click.option("--trace-memory", default=8 << 30, type=int, show_default=True, help=trace_memory),
        click.option("--chunks", "chunks_out", default=None, type=click.Path(file_okay=False),
                     help="Also write the training chunks of the solved reads under this directory (what `preprocess` makes of the table, "
                          "cut on the device from the alignment itself; no text in between)."),
        click.option("-y", "--config", default=None, type=click.Path(dir_okay=False, exists=True),
                     help="With --chunks: YAML configuration file with seq_kmer, max_dna_len and max_signal_len."),
        click.option("--seq-kmer", default=None, type=int, help="k of the chunks' k-mers (default: seq_kmer of the config)."),
        click.option("--max-dna-len", default=None, type=int, help="k-mers per chunk, 1..64 (default: max_dna_len of the config)."),
        click.option("--max-signal-len", default=None, type=int, help="Samples per chunk, 1..1024 (default: max_signal_len of the config)."),
        click.option("--kmer-model-out", "model_out", default=None, type=click.Path(dir_okay=False),
                     help="Also write the pore model re-estimated from this run's alignments: per k-mer the statistics of its events' means "
                          "in pA, summed on the device from the alignment itself.  A file --kmer-model reads: a second round is the same "
                          "command with it."),
        click.option("--kmer-model-min-events", "model_min_events", default=None, type=int,
                     help="With --kmer-model-out: leave out k-mers with fewer events.  [default: 1, a choice, not a measurement]"))


def _model_out(model_out, model_min_events):
    """(NEW.model, min_events) of --kmer-model-out, or None; --kmer-model-min-events alone is a UsageError."""
    if model_out is None:
        if model_min_events is not None:
            raise click.UsageError("--kmer-model-min-events requires --kmer-model-out")
        return None
    if model_min_events is not None:
        _in_range(model_min_events, 1, None, "--kmer-model-min-events")
    return str(model_out), 1 if model_min_events is None else int(model_min_events)


def _aligner_start(command: str, signals, max_samples, trace_memory, cpu) -> None:
    """The checks both aligners begin with, and torch before the library."""
    _signal_files(command, signals)
    _in_range(max_samples, 1, None, "--max-samples")
    _in_range(trace_memory, 1, None, "--trace-memory")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)


@main.command()
@_aligner_options(
    "event's", "sample", "Bytes of decision scratch per batch; a read that needs more on its own is refused by its id.",
    click.option("--band", default=512, type=int, show_default=True,
                 help="Half width of the band in k-mers around the diagonal.  A choice, not a measurement."),
    after_rna=[click.option("--intervals", default=None, type=click.Path(dir_okay=False, exists=True),
                            help="A table of compare --open-ends: restrict every record to its [b_start, b_end) (an untrimmed real read); "
                                 "rows come out in the record's own coordinates.")])
def resquiggle(seqs, signals, model, out, with_samples, band, skip_penalty, unknown_cost, rna, intervals, cpu, as_json, summary_out,
               max_samples, trace_memory, chunks_out, config, seq_kmer, max_dna_len, max_signal_len, model_out, model_min_events):
    """Align every record of a .blow5 / .slow5 file to the levels a pore model expects for the k-mers of its sequence (SEQS: FASTA or
    FASTQ, record names = read ids) and write the event table predict --events writes: read_name, position, model_kmer, start_idx,
    end_idx, event_level_mean, event_stdv.  Both ends are pinned: the first sample belongs to the first k-mer, the last to the last.
    Exact integers on median / MAD normalised samples and levels; unvalidated against f5c / uncalled4."""
    _aligner_start("resquiggle", signals, max_samples, trace_memory, cpu)
    from . import resquiggle as R, signal_batch as SB
    _in_range(band, 1, SB.max_band(), "--band")
    _in_range(skip_penalty, 0, R.MAX_SKIP_PENALTY, "--skip-penalty")
    _in_range(unknown_cost, 0, R.MAX_UNKNOWN_COST, "--unknown-cost")
    new_model = _model_out(model_out, model_min_events)
    chunks = None if chunks_out is None else (chunks_out,) + _chunk_geometry(config, seq_kmer, max_dna_len, max_signal_len)
    s = R.resquiggle_files(seqs, signals, model, out, band=band, skip_penalty=skip_penalty, unknown_cost=unknown_cost, rna=rna,
                           intervals=intervals, with_samples=with_samples, cpu=cpu, summary_out=summary_out, max_samples=max_samples,
                           trace_memory=trace_memory, chunks=chunks, model_out=new_model)
    per = "nan" if s["mean_cost_per_sample"] is None else f"{s['mean_cost_per_sample']:.4f}"
    _echo_summary(s, as_json,
                  f"{s['events']} events of {s['solved']} reads -> {out}  [k {s['k']}, band {band}, skip penalty {skip_penalty}, unknown "
                  f"cost {unknown_cost}; of {s['records']} records {s['unreached']} unreached, {s['refused']} refused, "
                  f"{s['no_sequence']} without a sequence, {s['no_known_level']} without a known level; {s['skipped_kmers']} skipped "
                  f"k-mers]  mean cost per sample {per} MAD")


@main.command()
@click.argument("signals", type=click.Path(dir_okay=False))
@click.option("-o", "--out", required=True, type=click.Path(dir_okay=False), help="Output event table (.events.tsv).")
@_detector_options("detector", " on Welch's t between the two windows.  A choice, not a measurement.", ".  A choice, not a measurement.")
@click.option("--cpu", is_flag=True, help="Compute on host threads instead of the GPU (the same bytes).")
@click.option("--json", "as_json", is_flag=True, help="Print the summary as one JSON object.")
@click.option("--summary", "summary_out", default=None, type=click.Path(dir_okay=False), help="Also write one row per read here (.tsv).")
@click.option("--max-samples", default=1 << 27, type=int, show_default=True, help="Samples per batch.")
def segment(signals, out, window_short, window_long, threshold_short, threshold_long, cpu, as_json, summary_out, max_samples):
    """Cut every record of a .blow5 / .slow5 file into events -- runs of constant level -- without its sequence, and write one row per
    event: read_name, event_index, start_idx, end_idx, event_level_mean, event_stdv.  A boundary is a peak of a windowed t-statistic,
    short window or long; exact integers.  Not scrappie's detector; unvalidated against scrappie / f5c / uncalled4."""
    _signal_files("segment", signals)
    _in_range(max_samples, 1, None, "--max-samples")
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    from . import segment as SEG
    _check_detector(window_short, window_long, threshold_short, threshold_long)
    s = SEG.segment_files(signals, out, window_short=window_short, window_long=window_long, threshold_short=threshold_short,
                          threshold_long=threshold_long, cpu=cpu, summary_out=summary_out, max_samples=max_samples)
    per = "nan" if s["mean_samples_per_event"] is None else f"{s['mean_samples_per_event']:.3f}"
    _echo_summary(s, as_json,
                  f"{s['events']} events of {s['records'] - s['refused']} records -> {out}  [windows {window_short} / {window_long}, "
                  f"thresholds {threshold_short} / {threshold_long}; {s['samples']} samples, {s['refused']} record(s) refused: too long]  "
                  f"mean samples per event {per}")


@main.command()
@_aligner_options(
    "row's", "event", "Bytes of decision scratch per batch, counted by the most events a record can have; a read that may need more on "
                      "its own is refused by its id.",
    click.option("--band-width", default=128, type=int, show_default=True,
                 help="Cells of the adaptive band, a multiple of 64 in 64..1024.  A choice, not a measurement."),
    after_skip=[click.option("--trim-penalty", default=64, type=int, show_default=True,
                             help="Cost of an event trimmed at either end, in 1/64 MAD.  The default, one MAD, is a choice, not a measurement.")],
    after_rna=[_detector_options("event detector", " (see segment).", " (see segment).")])
def eventalign(seqs, signals, model, out, with_samples, band_width, skip_penalty, trim_penalty, unknown_cost, rna, window_short,
               window_long, threshold_short, threshold_long, cpu, as_json, summary_out, max_samples, trace_memory, chunks_out, config,
               seq_kmer, max_dna_len, max_signal_len, model_out, model_min_events):
    """Align the detected events of every UNTRIMMED record of a .blow5 / .slow5 file to the levels a pore model expects for the k-mers
    of its sequence (SEQS: FASTA or FASTQ, record names = read ids) and write the event table predict --events writes, one row per
    k-mer that got events.  Events come from the detector of `segment`; their means are median / MAD normalised over the whole record;
    the alignment runs in an adaptive band with free ends, so adapter, stall and trailing samples are trimmed.  Exact integers;
    unvalidated against f5c / nanopolish / uncalled4.  Junk beyond half of a record's events defeats the normalisation."""
    _aligner_start("eventalign", signals, max_samples, trace_memory, cpu)
    from . import eventalign as EA
    if not 64 <= band_width <= EA.MAX_WIDTH or band_width % 64:
        raise click.BadParameter(f"must be a multiple of 64 in 64..{EA.MAX_WIDTH}", param_hint="--band-width")
    _in_range(skip_penalty, 0, EA.MAX_SKIP_PENALTY, "--skip-penalty")
    _in_range(trim_penalty, 0, EA.MAX_TRIM_PENALTY, "--trim-penalty")
    _in_range(unknown_cost, 0, EA.MAX_UNKNOWN_COST, "--unknown-cost")
    _check_detector(window_short, window_long, threshold_short, threshold_long)
    new_model = _model_out(model_out, model_min_events)
    chunks = None if chunks_out is None else (chunks_out,) + _chunk_geometry(config, seq_kmer, max_dna_len, max_signal_len)
    s = EA.eventalign_files(seqs, signals, model, out, band_width=band_width, skip_penalty=skip_penalty, trim_penalty=trim_penalty,
                            unknown_cost=unknown_cost, rna=rna, window_short=window_short, window_long=window_long,
                            threshold_short=threshold_short, threshold_long=threshold_long, with_samples=with_samples, cpu=cpu,
                            summary_out=summary_out, max_samples=max_samples, trace_memory=trace_memory, chunks=chunks,
                            model_out=new_model)
    per = "nan" if s["mean_cost_per_event"] is None else f"{s['mean_cost_per_event']:.4f}"
    _echo_summary(s, as_json,
                  f"{s['events']} rows of {s['solved']} reads -> {out}  [k {s['k']}, band width {band_width}, skip penalty {skip_penalty}, "
                  f"trim penalty {trim_penalty}, unknown cost {unknown_cost}; of {s['records']} records {s['unreached']} unreached, "
                  f"{s['refused']} refused, {s['no_sequence']} without a sequence, {s['no_known_level']} without a known level; "
                  f"{s['aligned_events']} aligned events, {s['skipped_kmers']} skipped k-mers; {s['trimmed_head_samples']} / "
                  f"{s['trimmed_tail_samples']} samples trimmed at head / tail]  mean cost per aligned event {per} MAD")


def _chunk_geometry(config, seq_kmer, max_dna_len, max_signal_len):
    """(k, te, ts) of the training chunks: the three keys of the config (the packaged config.yaml by default), each overridden by
    its option; a value outside the limits of s2s_chunk_pack is a BadParameter that names the option."""
    from . import preprocess as PP
    cfg = set_config(config)
    given = (("--seq-kmer", "seq_kmer", seq_kmer, PP.MAX_K), ("--max-dna-len", "max_dna_len", max_dna_len, PP.MAX_TE),
             ("--max-signal-len", "max_signal_len", max_signal_len, PP.MAX_TS))
    out = []
    for hint, key, value, most in given:
        value = int(cfg[key]) if value is None else int(value)
        _in_range(value, 1, most, hint)
        out.append(value)
    return tuple(out)


@main.command()
@click.argument("events", type=click.Path(dir_okay=False, exists=True))
@click.argument("outdir", type=click.Path(file_okay=False))
@click.option("-y", "--config", default=None, type=click.Path(dir_okay=False, exists=True),
              help="YAML configuration file with seq_kmer, max_dna_len and max_signal_len (default: the packaged config.yaml).")
@click.option("--seq-kmer", default=None, type=int, help="k of the chunks' k-mers (default: seq_kmer of the config).")
@click.option("--max-dna-len", default=None, type=int, help="k-mers per chunk, 1..64 (default: max_dna_len of the config).")
@click.option("--max-signal-len", default=None, type=int, help="Samples per chunk, 1..1024 (default: max_signal_len of the config).")
@click.option("--rna", is_flag=True, help="The stored signal is reversed (RNA profiles): read every row's samples back to front.")
@click.option("--chunks-per-file", default=100_000, type=int, show_default=True, help="Chunks per numbered file set.  A choice.")
@click.option("--max-chunks", default=None, type=int, help="Stop after this many kept chunks.")
@click.option("--max-samples", default=1 << 27, type=int, show_default=True, help="Samples per batch.")
@click.option("--cpu", is_flag=True, help="Compute on host threads instead of the GPU (the same bytes).")
@click.option("--json", "as_json", is_flag=True, help="Print the summary as one JSON object.")
def preprocess(events, outdir, config, seq_kmer, max_dna_len, max_signal_len, rna, chunks_per_file, max_chunks, max_samples, cpu, as_json):
    """Cut an event table with a `samples` column (predict --events --events-samples, resquiggle --samples, eventalign --samples) into
    the training chunks the reference's preprocess writes -- chunks-NNNN.npy, chunks_lengths-, targets-, targets_lengths-, stdevs-
    under OUTDIR, the directory `evaluate` reads.  Per read, in the table's order; no random permutation."""
    if max_samples < 1:
        raise click.BadParameter("must be >= 1", param_hint="--max-samples")
    if chunks_per_file < 1:
        raise click.BadParameter("must be >= 1", param_hint="--chunks-per-file")
    if max_chunks is not None and max_chunks < 0:
        raise click.BadParameter("must be >= 0", param_hint="--max-chunks")
    import json
    if not cpu:
        import torch  # noqa: F401  (before the library: see engine.py)
    from . import preprocess as PP
    k, te, ts = _chunk_geometry(config, seq_kmer, max_dna_len, max_signal_len)
    s = PP.preprocess_table(events, outdir, k, te, ts, rna=rna, chunks_per_file=chunks_per_file, max_chunks=max_chunks,
                            max_samples=max_samples, cpu=cpu)
    if as_json:
        click.echo(json.dumps(s))
    else:
        click.echo(f"{s['chunks_written']} chunks in {s['files']} file set(s) -> {outdir}  [k {k}, {te} k-mers, {ts} samples; "
                   f"{s['reads']} reads, {s['rows']} rows, {s['all_n_rows']} all-N rows dropped, {s['pad_rows']} pad rows; "
                   f"{s['chunks_formed']} chunks formed, {s['chunks_kept']} kept, {s['chunks_too_long']} dropped as too long]")


@main.command()
@click.argument("train_dir", type=click.Path(file_okay=False, path_type=pathlib.Path))
@click.argument("valid_dir", type=click.Path(file_okay=False, path_type=pathlib.Path))
@click.option("-o", "--out", required=True, type=click.Path(dir_okay=False), help="MODEL_DIR/MODEL.ckpt, written after every epoch.")
@click.option("-y", "--config", default=None, type=click.Path(dir_okay=False, exists=True),
              help="YAML configuration file (default: the packaged config.yaml).")
@click.option("--init", default=None, type=click.Path(dir_okay=False, exists=True),
              help="Checkpoint to fine-tune; its geometry and sizes must be the config's (default: torch's default initialisation).")
@click.option("--seed", default=0, type=int, show_default=True, help="Seed of the initialisation and of the per-epoch permutations.")
@click.option("--max-steps", default=None, type=int, help="Stop after this many optimizer steps (default: max_epochs epochs).")
@click.option("--train-memory", default=None, type=int,
              help="Bytes of tape and backward scratch per micro-batch; a larger batch runs as micro-batches (default 2 GiB: a choice).")
@click.option("--keep-epochs", is_flag=True, help="Also keep a MODEL-epoch=N.ckpt copy per epoch.")
@click.option("--json", "as_json", is_flag=True, help="Log one JSON object per step and per epoch instead of the text lines.")
def train(train_dir, valid_dir, out, config, init, seed, max_steps, train_memory, keep_epochs, as_json):
    """Fit a checkpoint to a preprocess directory on one GPU: the reference's training_step, get_loss and configure_optimizers for
    Adam / AdamW in exact fp32 (no dropout, no mixed precision); after every epoch the four valid_* losses of `evaluate` on
    VALID_DIR and the checkpoint."""
    if not str(out).endswith(".ckpt"):
        raise click.BadParameter("must end in .ckpt", param_hint="--out")
    if not os.path.dirname(str(out)):
        raise click.BadParameter("needs a directory part: MODEL_DIR/MODEL.ckpt", param_hint="--out")
    for d, hint in ((train_dir, "TRAIN_DIR"), (valid_dir, "VALID_DIR")):
        if not d.is_dir():
            raise click.BadParameter(f"{d} is not a directory", param_hint=hint)
    if max_steps is not None:
        _in_range(max_steps, 1, 1 << 31, "--max-steps")
    if train_memory is not None:
        _in_range(train_memory, 1, 1 << 46, "--train-memory")
    cfg = set_config(config)
    from . import train as TR
    try:
        TR.check_config(cfg)
    except ValueError as e:
        raise click.BadParameter(str(e), param_hint="--config")
    for key, lo, hi in (("train_batch_size", 1, 1 << 20), ("max_epochs", 1, 1 << 20)):
        if not lo <= int(cfg.get(key, 0)) <= hi:
            raise click.BadParameter(f"{key} must be {lo}..{hi}", param_hint="--config")
    if not float(cfg.get("lr", 0)) > 0:
        raise click.BadParameter("lr must be positive", param_hint="--config")
    import torch  # noqa: F401  (before the library: see engine.py)
    try:
        TR.train_run(str(train_dir), str(valid_dir), str(out), cfg, init=init, seed=seed, max_steps=max_steps, train_memory=train_memory,
                     keep_epochs=keep_epochs, json_log=as_json, log=click.echo)
    except ValueError as e:
        raise click.ClickException(str(e))


if __name__ == "__main__":
    main()
