"""The evaluation goldens (tests/golden/eval_<tag>.npz, tools/make_eval_goldens.py) turned back into the reference's preprocess
layout, and the checkpoints they belong to."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ("k9", "k6", "d32", "r16x500", "hd1", "g5x37", "hd24", "hd64", "hd96s", "g64x1024", "hd208")
ROW_KEYS = ("codes", "lengths", "targets", "stdevs", "kind", "prediction_ref", "sigma", "conc", "rate", "per_chunk", "per_chunk16")
LOSSES = ("valid_signal_loss", "valid_duration_loss", "valid_noise_loss", "valid_total_loss")


def load(tag: str) -> dict:
    return dict(np.load(os.path.join(HERE, "golden", f"eval_{tag}.npz"), allow_pickle=False))


def checkpoint(tag: str) -> str:
    if tag in ("k9", "k6"):
        return os.path.join(HERE, "golden", f"synthetic_{tag}.ckpt")
    if tag == "d32":
        import _sized_models as SM
        return SM.checkpoint_path(tag)
    import _envelope_models as EM
    if tag in EM.CASES:
        return EM.checkpoint_path(tag)
    import _geometry_models as GM
    return GM.checkpoint_path(tag)


def scaled(g: dict, scale: float):
    """-> (targets, stdevs) float32 as ChunkDataSetMemmap.__getitem__ hands them to the model: / scaling_max_value."""
    return (g["targets"].astype(np.float32) / scale).astype(np.float32), (g["stdevs"] / scale).astype(np.float32)


def draw_rows(g: dict, B: int, seed: int):
    """A dataset of B rows drawn from the golden's chunks -> (idx int64 [B], the golden's per-row arrays at idx).  idx is a chain of
    seeded permutations of the golden's chunks, so every window of N rows that starts at a multiple of N covers the golden exactly
    once, and no two adjacent rows come from the same golden chunk: a row swapped with its neighbour, or one that took another
    row's hand-off slot, disagrees with the reference's answer for its own chunk."""
    N = g["codes"].shape[0]
    assert N >= 3 and B >= 1
    rng = np.random.default_rng(seed)
    parts = []
    while sum(len(p) for p in parts) < B:
        p = rng.permutation(N)
        if parts and p[0] == parts[-1][-1]:
            p[[0, 1]] = p[[1, 0]]
        parts.append(p)
    idx = np.concatenate(parts)[:B].astype(np.int64)
    assert B == 1 or (idx[1:] != idx[:-1]).all()
    return idx, {k: g[k][idx] for k in ROW_KEYS}


def onehot(codes: np.ndarray) -> np.ndarray:
    """letter codes [N,te,k] (0-4 "_ACGT", 5 = unknown) -> the reference's one-hot chunks [N,te,5k] float16 (an all-zero row for 5)."""
    x = np.zeros(codes.shape + (5,), np.float16)
    known = codes < 5
    x[known] = np.eye(5, dtype=np.float16)[codes[known]]
    return x.reshape(codes.shape[0], codes.shape[1], -1)


def arrays(g: dict) -> dict:
    """-> {kind: array} as preprocess writes them (chunks [N,te,5k], chunks_lengths [N,te], targets [N,ts], targets_lengths [N],
    stdevs [N,te])."""
    N, ts = g["targets"].shape
    return {"chunks": onehot(g["codes"]), "chunks_lengths": g["lengths"].astype(np.int64), "targets": g["targets"].astype(np.float32),
            "targets_lengths": np.full(N, ts, np.int64), "stdevs": g["stdevs"].astype(np.float32)}


def write_dir(g: dict, path: str, per_file: int = 0, numbers=None) -> str:
    """Write the golden's dataset under `path`: batched files <kind>-NNNN.npy of per_file chunks each (numbers: the file numbers,
    default 0, 1, ...), or the single-file layout <kind>.npy when per_file == 0."""
    os.makedirs(path, exist_ok=True)
    a = arrays(g)
    N = a["chunks"].shape[0]
    if per_file <= 0:
        for kind, v in a.items():
            np.save(os.path.join(path, f"{kind}.npy"), v)
        return path
    starts = list(range(0, N, per_file))
    numbers = list(numbers) if numbers is not None else list(range(len(starts)))
    for num, i in zip(numbers, starts):
        for kind, v in a.items():
            np.save(os.path.join(path, f"{kind}-{num:04d}.npy"), v[i:i + per_file])
    return path
