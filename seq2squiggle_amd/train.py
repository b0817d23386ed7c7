"""Training on the GPU: the reference's `training_step`, `get_loss` and `configure_optimizers` (model.py:65-105, 419-480) for the
Adam / AdamW case, in exact fp32 on one device (include/s2s_hip.h: s2s_trainer_*).

* `Trainer`: the ctypes wrapper -- `gradients()` (forward + backward), `step()` (+ clip + optimizer), `state_dict()`.
* `lr_at`: the `transformers` schedules `warmup_cosine`, `warmup_constant`, `constant` as closed forms of the step.
* `TrainData`: a preprocess directory (evaluate.EvalData's discovery) dealt out in per-epoch permutations
  `numpy.random.default_rng([seed, epoch]).permutation(N)`, `train_batch_size` chunks a batch, the short last batch kept.
* `default_init`: torch's default initialisation of the reference's modules, drawn on the CPU from one seeded generator in
  state-dict order.
* `train_run`: the loop -- epochs, the `valid_*` losses by `evaluate` after every epoch, the checkpoint `load_checkpoint` reads.

Deviations from the reference, all deliberate: fp32 only (the reference trains in 16-mixed); dropout is NOT applied (the three
rates are read, and a non-zero one is logged once); Adam / AdamW only, eps 1e-7, betas 0.9 / 0.999; one GPU; no W&B, plots or
Lightning; optimizer state is not stored in the checkpoint.
"""
import ctypes as C
import math
import os
import shutil
import sys
import warnings
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .checkpoint import blob_names, config_to_c, load_checkpoint, state_dict_to_blob
from .evaluate import EvalData, onehot_to_kmers

OPTIMIZERS = ("Adam", "AdamW")
SCHEDULES = ("warmup_cosine", "warmup_constant", "constant")
ADAM_EPS, ADAM_BETAS = 1e-7, (0.9, 0.999)
STAT_NAMES = ("train_signal_loss", "train_duration_loss", "train_noise_loss", "train_total_loss", "grad_norm")
# the geometry and size keys a checkpoint given as --init must share with the config
SHAPE_KEYS = ("seq_kmer", "max_dna_len", "max_signal_len", "dmodel", "dff", "encoder_heads", "decoder_heads", "encoder_layers",
              "decoder_layers", "pre_layers")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------ schedules
def lr_at(schedule: str, step: int, total_steps: int, warmup_ratio: float, base_lr: float) -> float:
    """The learning rate of optimizer step `step` (0-based: the value LambdaLR holds while that step runs).  transformers'
    get_cosine_schedule_with_warmup / get_constant_schedule_with_warmup / get_constant_schedule with
    num_warmup_steps = int(total_steps * warmup_ratio)."""
    if schedule not in SCHEDULES:
        raise ValueError(f"lr_schedule {schedule!r} is not supported (one of {', '.join(SCHEDULES)})")
    if schedule == "constant":
        return base_lr
    warm = int(total_steps * warmup_ratio)
    if step < warm:
        return base_lr * step / max(1, warm)
    if schedule == "warmup_constant":
        return base_lr
    progress = (step - warm) / max(1, total_steps - warm)
    return base_lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


# ------------------------------------------------------------------------------------------------------------ weights
def state_shapes(cfg: dict) -> Dict[str, tuple]:
    """name -> shape of every tensor of the reference's state_dict, in blob order (checkpoint.blob_names)."""
    d, f, k = int(cfg["dmodel"]), int(cfg["dff"]), int(cfg["seq_kmer"])
    te, ts = int(cfg["max_dna_len"]), int(cfg["max_signal_len"])
    out = {}
    for n in blob_names(cfg):
        if n == "encoders.position_enc":
            s = (1, te, d)
        elif n == "decoders.position_enc":
            s = (1, ts, d)
        elif n == "encoders.src_emb.weight":
            s = (d, 5 * k)
        elif n.endswith("pos_ffn.w_1.weight"):
            s = (f, d)
        elif n.endswith("pos_ffn.w_1.bias"):
            s = (f,)
        elif n.endswith("pos_ffn.w_2.weight"):
            s = (d, f)
        elif n.endswith("_layer.3.weight") or n == "decoders.out_linear.weight":      # the heads' Linear(d, 1)
            s = (1, d)
        elif n.endswith("_layer.3.bias") or n == "decoders.out_linear.bias":
            s = (1,)
        elif n.endswith("layer_norm.weight") or n.endswith(".bias"):
            s = (d,)
        else:
            s = (d, d)
        out[n] = s
    return out


def sinusoid_table(n_position: int, d_hid: int) -> torch.Tensor:
    """get_sinusoid_encoding_table (layers.py:145-165) -> [1, n_position, d_hid] float32: the angles in Python floats, rounded to
    fp32, then sin / cos in fp32."""
    tab = torch.tensor([[pos / 10000 ** (2 * (j // 2) / d_hid) for j in range(d_hid)] for pos in range(n_position)])
    tab[:, 0::2] = torch.sin(tab[:, 0::2])
    tab[:, 1::2] = torch.cos(tab[:, 1::2])
    return tab.float().unsqueeze(0)


def default_init(cfg: dict, seed: int) -> Dict[str, torch.Tensor]:
    """torch's default initialisation of the reference's modules: nn.Linear kaiming-uniform with a = sqrt(5), i.e. weight and bias
    both U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)); LayerNorm 1 / 0; the two sinusoid position tables.  Drawn on the CPU from
    torch.Generator().manual_seed(seed) in state-dict order."""
    gen = torch.Generator().manual_seed(int(seed))
    sd = {}
    shapes = state_shapes(cfg)
    for n, s in shapes.items():
        if n.endswith("position_enc"):
            sd[n] = sinusoid_table(s[1], s[2])
        elif n.endswith("layer_norm.weight"):
            sd[n] = torch.ones(s)
        elif n.endswith("layer_norm.bias"):
            sd[n] = torch.zeros(s)
        else:
            w = shapes[n[:-len("bias")] + "weight"] if n.endswith(".bias") else s
            bound = 1.0 / math.sqrt(w[1])
            sd[n] = (torch.rand(s, generator=gen) * 2.0 - 1.0) * bound
    return sd


def check_init(sd: Dict[str, torch.Tensor], init_cfg: dict, cfg: dict) -> None:
    """--init: the checkpoint's geometry and sizes must be the config's; the error names the key that differs."""
    for key in SHAPE_KEYS:
        if int(init_cfg[key]) != int(cfg[key]):
            raise ValueError(f"--init: {key} is {init_cfg[key]} in the checkpoint and {cfg[key]} in the config")
    for n, s in state_shapes(cfg).items():
        if n not in sd:
            raise ValueError(f"--init: the checkpoint lacks {n}")
        if tuple(sd[n].shape) != s:
            raise ValueError(f"--init: {n} is {list(sd[n].shape)} in the checkpoint, {list(s)} for the config")


# ------------------------------------------------------------------------------------------------------------ Trainer
class Trainer:
    """fp32 weights, gradient, Adam moments and the tape on one GPU (s2s_trainer_*)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: dict, device: Optional[int] = None,
                 train_memory: Optional[int] = None):
        self._t = None
        L = _lib.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("seq2squiggle_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.config = dict(config)
        self.k, self.t_enc, self.t_dec = int(config["seq_kmer"]), int(config["max_dna_len"]), int(config["max_signal_len"])
        ccfg = config_to_c(config, "generic-geometry")
        blob = np.ascontiguousarray(state_dict_to_blob(state_dict, config))
        self.n_floats = int(blob.size)
        t = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            rc = L.s2s_trainer_create(C.byref(ccfg), blob.ctypes.data_as(C.c_void_p), blob.nbytes, self.device_index, C.byref(t))
        if rc != 0:
            raise ValueError(f"s2s_trainer_create failed ({rc}): {L.s2s_trainer_last_error(None).decode()}")
        self._t = t
        if train_memory is not None:
            self.set_memory(train_memory)

    def close(self):
        if self._t is not None:
            _lib.lib().s2s_trainer_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {_lib.lib().s2s_trainer_last_error(self._t).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _inputs(self, kmers, dwell, target, stdev):
        B = int(kmers.shape[0])
        for name, t, dt, shape in (("kmers", kmers, torch.uint8, (B, self.t_enc, self.k)), ("dwell", dwell, torch.int32, (B, self.t_enc)),
                                   ("target", target, torch.float32, (B, self.t_dec)), ("stdev", stdev, torch.float32, (B, self.t_enc))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name} must be contiguous {dt} {shape} on {self.device}")
        return B

    def set_memory(self, nbytes: int):
        """The bytes of tape + backward scratch a micro-batch may use (one chunk always runs)."""
        self._check(_lib.lib().s2s_trainer_set_memory(self._t, int(nbytes)), "s2s_trainer_set_memory")

    def micro_batch(self, B: int) -> int:
        """Chunks per micro-batch of a batch of B under the memory budget."""
        return int(_lib.lib().s2s_trainer_micro_batch(self._t, int(B)))

    def gradients(self, kmers, dwell, target, stdev):
        """Forward and backward only (no weight changes) -> dict(loss float32 [B,3]: the per-chunk sums of evaluate_chunks;
        grad float32 [n_floats]: the gradient of the total loss in blob order), both on the device."""
        B = self._inputs(kmers, dwell, target, stdev)
        f = dict(dtype=torch.float32, device=self.device)
        out = {"loss": torch.empty(B, 3, **f), "grad": torch.empty(self.n_floats, **f)}
        with torch.cuda.device(self.device):
            rc = _lib.lib().s2s_trainer_gradients(self._t, self._stream(), _ptr(kmers), _ptr(dwell), _ptr(target), _ptr(stdev), B,
                                                  _ptr(out["loss"]), _ptr(out["grad"]))
        self._check(rc, "s2s_trainer_gradients")
        return out

    def step(self, kmers, dwell, target, stdev, lr: float, step: int, optimizer: str = "Adam", weight_decay: float = 0.0,
             clip: float = 0.0, betas=ADAM_BETAS, eps: float = ADAM_EPS, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimizer step (`step` counts from 1) -> float32 [5] on the device: STAT_NAMES of this step's forward pass and the
        gradient norm before clipping.  Nothing is read back: the caller decides when to look."""
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer {optimizer!r} is not supported (one of {', '.join(OPTIMIZERS)})")
        B = self._inputs(kmers, dwell, target, stdev)
        stats = out if out is not None else torch.empty(5, dtype=torch.float32, device=self.device)
        hyper = _lib.S2SAdam(lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps), weight_decay=float(weight_decay),
                             clip=float(clip or 0.0), decoupled=int(optimizer == "AdamW"), step=int(step))
        with torch.cuda.device(self.device):
            rc = _lib.lib().s2s_trainer_step(self._t, self._stream(), _ptr(kmers), _ptr(dwell), _ptr(target), _ptr(stdev), B,
                                             C.byref(hyper), _ptr(stats))
        self._check(rc, "s2s_trainer_step")
        return stats

    def weights(self) -> torch.Tensor:
        """The weights in blob order, float32 [n_floats] on the device."""
        out = torch.empty(self.n_floats, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _lib.lib().s2s_trainer_weights(self._t, self._stream(), _ptr(out))
        self._check(rc, "s2s_trainer_weights")
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's state_dict (CPU float32), both position tables included."""
        return blob_to_state_dict(self.weights().cpu(), self.config)


def blob_to_state_dict(blob: torch.Tensor, cfg: dict) -> Dict[str, torch.Tensor]:
    sd, at = {}, 0
    for n, s in state_shapes(cfg).items():
        num = int(np.prod(s))
        sd[n] = blob[at:at + num].reshape(s).clone()
        at += num
    if at != blob.numel():
        raise ValueError(f"blob holds {blob.numel()} values, the config's state_dict {at}")
    return sd


def split_blob(blob, cfg: dict) -> Dict[str, np.ndarray]:
    """A blob-ordered vector (weights or gradient) -> {name: array of the tensor's shape}."""
    return {n: t.numpy() for n, t in blob_to_state_dict(torch.as_tensor(np.asarray(blob)), cfg).items()}


# ------------------------------------------------------------------------------------------------------------ data
class TrainData(EvalData):
    """A preprocess directory dealt out in seeded per-epoch permutations."""

    def __init__(self, data_dir: str, config: dict, max_chunks: Optional[int] = None, seed: int = 0):
        super().__init__(data_dir, config, max_chunks)
        self.seed = int(seed)
        self._starts = np.cumsum([0] + [p["chunks"].shape[0] for p in self.parts])

    def order(self, epoch: int) -> np.ndarray:
        return np.random.default_rng([self.seed, int(epoch)]).permutation(self.n)

    def steps_per_epoch(self, batch_size: int) -> int:
        return (self.n + batch_size - 1) // batch_size

    def rows(self, idx: np.ndarray):
        """-> (chunks, dwell int32, target fp32 scaled, stdev fp32 scaled) of the chunks `idx` (global numbers), in that order."""
        idx = np.asarray(idx, dtype=np.int64)
        part = np.searchsorted(self._starts, idx, side="right") - 1
        out = {k: [None] * len(idx) for k in ("chunks", "chunks_lengths", "targets", "stdevs")}
        for p in np.unique(part):
            sel = np.nonzero(part == p)[0]
            local = idx[sel] - self._starts[p]
            o = np.argsort(local, kind="stable")
            for k in out:
                got = np.asarray(self.parts[p][k][local[o]])
                for pos, row in zip(sel[o], got):
                    out[k][pos] = row
        chunks = np.stack(out["chunks"])
        dwell = np.stack(out["chunks_lengths"]).astype(np.int32)
        target = (np.stack(out["targets"]).reshape(len(idx), self.ts) / self.scale).astype(np.float32)
        stdev = (np.stack(out["stdevs"]) / self.scale).astype(np.float32)
        return chunks, dwell, target, stdev

    def epoch(self, epoch: int, batch_size: int):
        order = self.order(epoch)
        for i in range(0, self.n, batch_size):
            yield self.rows(order[i:i + batch_size])


def to_device(trainer, chunks, dwell, target, stdev):
    """One host batch -> the trainer's device inputs.  The one-hot is decoded and the dwells are checked on the HOST, before the
    copies, so that nothing is read back from the device inside a step."""
    dev = trainer.device
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        kmers = onehot_to_kmers(torch.as_tensor(chunks), trainer.k)
    if kmers.shape[1] != trainer.t_enc:
        raise ValueError(f"chunks have {kmers.shape[1]} k-mers, the config's max_dna_len is {trainer.t_enc}")
    if (np.asarray(dwell) < 0).any():
        raise ValueError("negative k-mer length (lengths are samples per k-mer, >= 0)")
    dw = torch.as_tensor(np.ascontiguousarray(dwell)).to(dev, torch.int32).contiguous()
    tg = torch.as_tensor(target).to(dev, torch.float32).reshape(kmers.shape[0], trainer.t_dec).contiguous()
    sd = torch.as_tensor(stdev).to(dev, torch.float32).contiguous()
    return kmers.to(dev).contiguous(), dw, tg, sd


# ------------------------------------------------------------------------------------------------------------ the loop
def check_config(cfg: dict) -> None:
    if cfg.get("optimizer", "Adam") not in OPTIMIZERS:
        raise ValueError(f"optimizer {cfg.get('optimizer')!r} is not supported (one of {', '.join(OPTIMIZERS)})")
    if cfg.get("lr_schedule", "constant") not in SCHEDULES:
        raise ValueError(f"lr_schedule {cfg.get('lr_schedule')!r} is not supported (one of {', '.join(SCHEDULES)})")


def save_checkpoint(path: str, sd: Dict[str, torch.Tensor], cfg: dict, epoch: int, global_step: int) -> None:
    """The layout load_checkpoint reads (ModelCheckpoint(save_weights_only=True)): plain tensors and containers only."""
    tmp = path + ".tmp"
    torch.save({"epoch": int(epoch), "global_step": int(global_step), "state_dict": {k: v.contiguous() for k, v in sd.items()},
                "hyper_parameters": {"config": dict(cfg)}}, tmp)
    os.replace(tmp, path)


def train_run(train_dir: str, valid_dir: str, out_path: str, cfg: dict, init: Optional[str] = None, seed: int = 0,
              max_steps: Optional[int] = None, train_memory: Optional[int] = None, keep_epochs: bool = False, json_log: bool = False,
              device: Optional[int] = None, log=None, log_every: int = 1):
    """-> list of per-epoch records.  One log line per step (every `log_every`) and per epoch, or JSON objects."""
    import json as _json
    from .engine import Engine
    from .evaluate import evaluate
    log = log or (lambda s: print(s, file=sys.stderr, flush=True))
    check_config(cfg)
    if init:
        sd, init_cfg = load_checkpoint(init)
        check_init(sd, init_cfg, cfg)
    else:
        sd = default_init(cfg, seed)
    drops = {k: cfg.get(k, 0) for k in ("encoder_dropout", "decoder_dropout", "duration_dropout") if float(cfg.get(k, 0) or 0) != 0.0}
    if drops:
        log("train: dropout is not applied (" + ", ".join(f"{k} {v}" for k, v in drops.items()) + " ignored)")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    bs = int(cfg["train_batch_size"])
    data = TrainData(train_dir, cfg, cfg.get("max_chunks_train"), seed)
    valid = EvalData(valid_dir, cfg, cfg.get("max_chunks_valid"))
    spe = data.steps_per_epoch(bs)
    epochs = int(cfg["max_epochs"])
    total_steps = spe * epochs if not max_steps else min(spe * epochs, int(max_steps))
    tr = Trainer(sd, cfg, device, train_memory)
    opt, wd = cfg.get("optimizer", "Adam"), float(cfg.get("weight_decay", 0.0) or 0.0)
    clip = float(cfg.get("gradient_clip_val", 0.0) or 0.0)
    base_lr, sched, ratio = float(cfg["lr"]), cfg.get("lr_schedule", "constant"), float(cfg.get("warmup_ratio", 0.0) or 0.0)
    records, step = [], 0
    for epoch in range(epochs):
        if step >= total_steps:
            break
        pending = []
        for batch in data.epoch(epoch, bs):
            if step >= total_steps:
                break
            lr = lr_at(sched, step, total_steps, ratio, base_lr)
            step += 1
            st = tr.step(*to_device(tr, *batch), lr=lr, step=step, optimizer=opt, weight_decay=wd, clip=clip)
            if log_every and step % log_every == 0:
                pending.append((step, lr, st))
        for s, lr, st in pending:                         # read back once per epoch, not once per step
            rec = {"step": s, "lr": lr, **{n: float(v) for n, v in zip(STAT_NAMES, st.cpu().numpy())}}
            log(_json.dumps(rec) if json_log else
                f"step {s} lr {lr:.6g} " + " ".join(f"{n} {rec[n]:.9g}" for n in STAT_NAMES))
        sd_now = tr.state_dict()
        save_checkpoint(out_path, sd_now, cfg, epoch, step)
        if keep_epochs:
            shutil.copyfile(out_path, out_path[:-len(".ckpt")] + f"-epoch={epoch}.ckpt")
        eng = Engine(sd_now, cfg, tr.device_index, "generic-geometry")
        losses, _, _ = evaluate(eng, valid)
        eng.close()
        rec = {"epoch": epoch, "global_step": step, **{k: float(v) for k, v in losses.items()}}
        records.append(rec)
        log(_json.dumps(rec) if json_log else f"epoch {epoch} step {step} " + " ".join(f"{k} {v:.9g}" for k, v in losses.items()))
    tr.close()
    return records
