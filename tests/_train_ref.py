"""The reference gradient and optimizer trajectory of `train`, from the differentiable torch oracle (oracle/s2s_oracle.py: encoder,
noise_sampler, duration_params, length_regulate, decoder -- each held to the reference's goldens by the oracle's own tests).

The loss is training_step + get_loss (model.py:65-105, 419-480): the three heads read emb_out.detach(), the length regulator runs
on the measured dwell, and
    total = mean (y - target)^2 + 0.0005 mean -Gamma(conc, rate).log_prob(max(|dwell|, 1)) + mean (stdev - sigma)^2.
float64 is the truth; float32 on the CPU is the yardstick the device is measured against."""
import numpy as np
import torch

from oracle import s2s_oracle as O

POSITION_TABLES = ("encoders.position_enc", "decoders.position_enc")
DURATION_SCALE = 0.0005


def head_input(sd, cfg, codes, dtype=torch.float64):
    """emb_out.detach(): what the three heads read."""
    with torch.no_grad():
        return O.encoder(sd, dict(cfg, encoder_layers=0), O.one_hot(codes, dtype))[1]


def total_loss(sd, cfg, codes, lengths, target, stdev, dtype=torch.float64, heads_read=None):
    """-> (total, (signal, duration x 0.0005, noise)) as torch scalars of `dtype`, differentiable in sd's tensors.  heads_read: a
    fixed tensor in place of emb_out.detach() -- with it the value is a function whose true gradient is the one training uses
    (a finite difference that moved the heads' input with the pre-net would measure another function)."""
    enc_out, emb_out = O.encoder(sd, cfg, O.one_hot(codes, dtype))
    emb_d = emb_out.detach() if heads_read is None else heads_read
    sigma = O.noise_sampler(sd, emb_d)
    conc, rate = O.duration_params(sd, emb_d)
    dur = torch.as_tensor(np.ascontiguousarray(lengths).astype(np.int64))
    h, _ = O.length_regulate(enc_out, sigma, dur, cfg["max_signal_len"])
    y = O.decoder(sd, cfg, h)
    x = torch.as_tensor(np.asarray(lengths)).abs().clamp(min=1).to(dtype)
    signal = ((y - torch.as_tensor(np.asarray(target)).to(dtype)) ** 2).mean()
    duration = DURATION_SCALE * (-torch.distributions.Gamma(conc, rate, validate_args=False).log_prob(x)).mean()
    noise = ((torch.as_tensor(np.asarray(stdev)).to(dtype) - sigma) ** 2).mean()
    return signal + duration + noise, (signal, duration, noise)


def leaves(sd, dtype):
    """A copy of the state dict in `dtype`, every tensor but the position tables a leaf that requires grad."""
    out = {}
    for k, v in sd.items():
        t = v.detach().to(dtype).clone()
        if k not in POSITION_TABLES:
            t.requires_grad_(True)
        out[k] = t
    return out


def loss_and_grads(sd, cfg, codes, lengths, target, stdev, dtype=torch.float64):
    """-> (total float, (signal, duration, noise) floats, {name: gradient numpy array of `dtype`}); the position tables get zeros."""
    p = leaves(sd, dtype)
    total, parts = total_loss(p, cfg, codes, lengths, target, stdev, dtype)
    total.backward()
    grads = {k: (np.zeros(tuple(v.shape), v.numpy().dtype) if v.grad is None else v.grad.numpy().copy()) for k, v in p.items()}
    return float(total.detach()), tuple(float(t.detach()) for t in parts), grads


def adam_run(sd, cfg, batches, dtype=torch.float64, optimizer="Adam", lr=5e-4, weight_decay=0.0, clip=1.0, eps=1e-7,
             betas=(0.9, 0.999), lrs=None):
    """torch.optim.Adam / AdamW with clip_grad_norm_ over `batches` (an iterable of (codes, lengths, target, stdev)) ->
    (per-step total losses, per-step gradient norms before clipping, the final state dict as numpy arrays of `dtype`).
    lrs: the learning rate of every step, written into the param group before that step (what LambdaLR does); default: `lr`
    throughout."""
    p = leaves(sd, dtype)
    params = [v for v in p.values() if v.requires_grad]
    cls = torch.optim.AdamW if optimizer == "AdamW" else torch.optim.Adam
    opt = cls(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    losses, norms = [], []
    for s, (codes, lengths, target, stdev) in enumerate(batches):
        if lrs is not None:
            for group in opt.param_groups:
                group["lr"] = float(lrs[s])
        opt.zero_grad(set_to_none=True)
        total, _ = total_loss(p, cfg, codes, lengths, target, stdev, dtype)
        total.backward()
        norm = torch.nn.utils.clip_grad_norm_(params, clip if clip and clip > 0 else float("inf"))
        opt.step()
        losses.append(float(total.detach()))
        norms.append(float(norm))
    return losses, norms, {k: v.detach().numpy().copy() for k, v in p.items()}


def kmers_of(codes: np.ndarray) -> np.ndarray:
    """letter codes [B,te,k] (0-4 "_ACGT", 5 = unknown) -> the letters the device entries take, uint8."""
    return np.frombuffer(b"_ACGTN", dtype=np.uint8)[np.asarray(codes)]


def rows_with_every_kind(kind: np.ndarray, B: int) -> np.ndarray:
    """B chunk indices of a golden such that every `kind` it holds is among them: the first chunk of each kind, then the rest in
    index order."""
    first = [int(np.nonzero(kind == k)[0][0]) for k in sorted(set(kind.tolist()))]
    rest = [i for i in range(len(kind)) if i not in first]
    idx = (first + rest)[:B]
    assert len(idx) == B and set(kind[idx].tolist()) == set(kind.tolist())
    return np.asarray(idx, dtype=np.int64)
