"""The evaluation goldens (tests/golden/eval_<tag>.npz, tools/make_eval_goldens.py) turned back into the reference's preprocess
layout, and the checkpoints they belong to."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ("k9", "k6", "d32", "r16x500")
LOSSES = ("valid_signal_loss", "valid_duration_loss", "valid_noise_loss", "valid_total_loss")


def load(tag: str) -> dict:
    return dict(np.load(os.path.join(HERE, "golden", f"eval_{tag}.npz"), allow_pickle=False))


def checkpoint(tag: str) -> str:
    if tag in ("k9", "k6"):
        return os.path.join(HERE, "golden", f"synthetic_{tag}.ckpt")
    if tag == "d32":
        import _sized_models as SM
        return SM.checkpoint_path(tag)
    import _geometry_models as GM
    return GM.checkpoint_path(tag)


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
