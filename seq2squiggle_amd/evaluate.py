"""Teacher-forced validation losses of a checkpoint on a preprocessed dataset, on the GPU.

The reference logs four numbers in `validation_step` (model.py:107-143, `get_loss` :419-480) -- only inside `train`, under
Lightning.  This module computes the same numbers for any checkpoint the engine runs:

* `discover` / `EvalData` read a directory in the reference's `preprocess` layout (`chunks-NNNN.npy`, `chunks_lengths-`, `targets-`,
  `targets_lengths-`, `stdevs-`, paired by number as `load_numpy` / `sort_files` / `check_file_order` do, dataloader.py:456-611; or
  the single-file `chunks.npy` ... that `save_chunks` writes), memory-mapped;
* `onehot_to_kmers` turns the reference's one-hot chunk tensor into the k-mer letters `Engine.evaluate_chunks` takes;
* `evaluate` streams super-batches to the engine, scaling targets and stdevs by `scaling_max_value` as
  `ChunkDataSetMemmap.__getitem__` does, and `finalize` turns the per-chunk sums into the four dataset losses.

The dataset losses are the reference's epoch-level `valid_*` values: per-chunk sums accumulated in float64, divided by N * ts,
N * te and N * te (x 0.0005 for the duration loss).  Lightning's epoch value of a metric logged per batch is the batch-size weighted
mean of the per-batch means, and every batch mean here has a fixed denominator per chunk, so the two agree for any batch size.
"""
import os
import re
import time
import warnings
from typing import Dict, List, Optional

import numpy as np
import torch

KINDS = ("chunks", "chunks_lengths", "targets", "targets_lengths", "stdevs")
DURATION_SCALE = 0.0005                     # get_loss: duration_loss * 0.0005 (model.py:465)
UNKNOWN = ord("N")                          # the letter of an all-zero one-hot row (any byte outside "_ACGT" embeds as zeros)
_LETTERS = torch.tensor([ord(c) for c in "_ACGT"], dtype=torch.uint8)


def onehot_to_kmers(data: torch.Tensor, k: int, name: str = "chunks", first_chunk: int = 0) -> torch.Tensor:
    """The reference's chunk tensor, one-hot [B,te,k,5] or [B,te,5k] of any float dtype (utils.py:56-89), -> the letters of every
    k-mer, uint8 [B,te,k] on the same device.  An all-zero letter row becomes UNKNOWN (the reference embeds it as zeros); a row
    with more than one hot entry is an error naming `name` and the row (chunk index offset by first_chunk)."""
    if data.dim() == 3:
        if data.shape[2] != 5 * k:
            raise ValueError(f"{name}: expected [chunks, k-mers, {5 * k}] (seq_kmer {k}), got {list(data.shape)}")
        data = data.reshape(data.shape[0], data.shape[1], k, 5)
    if data.dim() != 4 or data.shape[2] != k or data.shape[3] != 5:
        raise ValueError(f"{name}: expected [chunks, k-mers, {k}, 5] or [chunks, k-mers, {5 * k}] (seq_kmer {k}), got {list(data.shape)}")
    hot = data != 0
    n_hot = hot.sum(-1)
    if bool((n_hot > 1).any()):
        b, c, j = (int(v) for v in (n_hot > 1).nonzero()[0])
        raise ValueError(f"{name}: chunk {first_chunk + b}, k-mer {c}, letter {j} has {int(n_hot[b, c, j])} hot entries "
                         "(a one-hot row has at most one)")
    code = hot.to(torch.uint8).argmax(-1)
    letters = _LETTERS.to(data.device)[code]
    return torch.where(n_hot == 0, torch.full((), UNKNOWN, dtype=torch.uint8, device=data.device), letters).contiguous()


def _number(path: str) -> int:
    return int(os.path.basename(path).split("-")[-1].split(".")[0])       # dataloader.py: extract_number


def discover(data_dir: str) -> List[Dict[str, str]]:
    """The files of a preprocess directory -> one {kind: path} per file number, in number order.  The batched layout
    (`<kind>-NNNN.npy`, save_chunks_in_batches) wins over the single-file one (`<kind>.npy`, save_chunks)."""
    if not os.path.isdir(data_dir):
        raise ValueError(f"{data_dir}: not a directory")
    names = os.listdir(data_dir)
    per = {}
    for kind in KINDS:
        pat = re.compile(re.escape(kind) + r"-(\d+)\.npy$")
        per[kind] = sorted((os.path.join(data_dir, n) for n in names if pat.fullmatch(n)), key=_number)
    if any(per.values()):
        counts = {kind: len(v) for kind, v in per.items()}
        if len(set(counts.values())) != 1:
            raise ValueError(f"{data_dir}: every kind needs the same number of <kind>-NNNN.npy files, found "
                             + ", ".join(f"{k} {n}" for k, n in counts.items()))
        for i in range(counts["chunks"]):
            nums = {kind: _number(per[kind][i]) for kind in KINDS}
            if len(set(nums.values())) != 1:                      # dataloader.py: check_file_order
                raise ValueError(f"{data_dir}: file numbers do not pair up at position {i}: {nums}")
        return [{kind: per[kind][i] for kind in KINDS} for i in range(counts["chunks"])]
    single = {kind: os.path.join(data_dir, f"{kind}.npy") for kind in KINDS}
    missing = [k for k, p in single.items() if not os.path.exists(p)]
    if len(missing) == len(KINDS):
        raise ValueError(f"{data_dir}: no preprocess output (expected chunks-NNNN.npy ... or chunks.npy ...)")
    if missing:
        raise ValueError(f"{data_dir}: missing " + ", ".join(f"{k}.npy" for k in missing))
    return [single]


class EvalData:
    """A preprocess directory, memory-mapped and checked against a checkpoint's config (seq_kmer, max_dna_len, max_signal_len)."""

    def __init__(self, data_dir: str, config: dict, max_chunks: Optional[int] = None):
        self.k, self.te, self.ts = int(config["seq_kmer"]), int(config["max_dna_len"]), int(config["max_signal_len"])
        self.scale = float(config["scaling_max_value"])
        self.files = discover(data_dir)
        self.parts = []
        for f in self.files:
            a = {kind: np.load(f[kind], mmap_mode="r") for kind in KINDS}
            n = a["chunks"].shape[0]
            want = {"chunks": [(n, self.te, 5 * self.k), (n, self.te, self.k, 5)], "chunks_lengths": [(n, self.te)],
                    "targets": [(n, self.ts), (n, self.ts, 1)], "targets_lengths": [(n,), (n, 1)], "stdevs": [(n, self.te)]}
            for kind, shapes in want.items():
                if tuple(a[kind].shape) not in shapes:
                    raise ValueError(f"{f[kind]}: shape {list(a[kind].shape)}, expected "
                                     + " or ".join(str(list(s)) for s in shapes)
                                     + f" for this checkpoint (seq_kmer {self.k}, max_dna_len {self.te}, max_signal_len {self.ts})")
            lens = np.asarray(a["chunks_lengths"])
            if (lens < 0).any():
                i = np.argwhere(lens < 0)[0]
                raise ValueError(f"{f['chunks_lengths']}: negative length {int(lens[tuple(i)])} at chunk {int(i[0])}, k-mer {int(i[1])} "
                                 "(lengths are samples per k-mer, >= 0)")
            self.parts.append(a)
        total = sum(p["chunks"].shape[0] for p in self.parts)
        self.n = total if max_chunks is None or max_chunks <= 0 else min(total, int(max_chunks))   # valid_limit: the first N

    def batches(self, batch_size: int):
        """-> (first chunk, chunks [b,te,...] array, dwell int32 [b,te], target fp32 [b,ts] scaled, stdev fp32 [b,te] scaled), in file
        order, at most batch_size chunks each (a batch does not straddle two files)."""
        start = 0
        for a in self.parts:
            n = a["chunks"].shape[0]
            for i in range(0, n, batch_size):
                if start + i >= self.n:
                    return
                j = min(n, i + batch_size, self.n - start)
                tgt = np.asarray(a["targets"][i:j]).reshape(j - i, self.ts)
                # ChunkDataSetMemmap.__getitem__: targets / scaling_max_value, stdevs / scaling_max_value, then float32
                yield (start + i, np.asarray(a["chunks"][i:j]), np.asarray(a["chunks_lengths"][i:j]).astype(np.int32),
                       (tgt / self.scale).astype(np.float32), (np.asarray(a["stdevs"][i:j]) / self.scale).astype(np.float32))
            start += n


def finalize(per_chunk: np.ndarray, te: int, ts: int) -> Dict[str, float]:
    """Per-chunk sums [N,3] (signal, duration NLL, noise) -> the four dataset losses of get_loss (model.py:458-479)."""
    s = np.asarray(per_chunk, dtype=np.float64).sum(0)
    n = per_chunk.shape[0]
    if n == 0:
        raise ValueError("no chunks to evaluate")
    out = {"valid_signal_loss": s[0] / (n * ts), "valid_duration_loss": DURATION_SCALE * s[1] / (n * te),
           "valid_noise_loss": s[2] / (n * te)}
    out["valid_total_loss"] = out["valid_signal_loss"] + out["valid_duration_loss"] + out["valid_noise_loss"]
    return out


def evaluate_batch(engine, chunks, dwell, target, stdev, first_chunk: int = 0, want_y: bool = False, debug: bool = False):
    """One batch of host or device arrays -> Engine.evaluate_chunks' dict (the one-hot converted on the device)."""
    dev = engine.device
    with warnings.catch_warnings():          # a read-only memory map: the tensor is only copied to the device, never written
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        x = torch.as_tensor(chunks).to(dev, non_blocking=True)
    kmers = onehot_to_kmers(x, engine.k, first_chunk=first_chunk)
    if kmers.shape[1] != engine.t_enc:
        raise ValueError(f"chunks have {kmers.shape[1]} k-mers, the checkpoint's max_dna_len is {engine.t_enc}")
    dw = torch.as_tensor(dwell).to(dev, torch.int32).contiguous()
    if bool((dw < 0).any()):
        raise ValueError("negative k-mer length (lengths are samples per k-mer, >= 0)")
    tg = torch.as_tensor(target).to(dev, torch.float32).reshape(x.shape[0], engine.t_dec).contiguous()
    sd = torch.as_tensor(stdev).to(dev, torch.float32).contiguous()
    return engine.evaluate_chunks(kmers, dw, tg, sd, want_y=want_y, debug=debug)


def evaluate(engine, data: EvalData, batch_size: int = 65536):
    """-> (the four dataset losses, per-chunk sums float32 [N,3], seconds on the wall from first read to last sum)."""
    t0 = time.perf_counter()
    out = np.empty((data.n, 3), dtype=np.float32)
    pending = []
    for first, chunks, dwell, target, stdev in data.batches(batch_size):
        r = evaluate_batch(engine, chunks, dwell, target, stdev, first_chunk=first)
        pending.append((first, r["loss"].to("cpu", non_blocking=True)))
        if len(pending) > 2:
            torch.cuda.current_stream(engine.device).synchronize()
            for f, t in pending:
                out[f:f + t.shape[0]] = t.numpy()
            pending = []
    torch.cuda.current_stream(engine.device).synchronize()
    for f, t in pending:
        out[f:f + t.shape[0]] = t.numpy()
    return finalize(out, data.te, data.ts), out, time.perf_counter() - t0
