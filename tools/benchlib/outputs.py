"""`--dump-outputs DIR`: what the timed path computed in its last timed region, as DIR/<name>.npy (float32; float64 stays float64),
so that two builds can be compared output for output. When the files would exceed MAX_BYTES in all, every array is replaced by a fixed,
seeded sample of its elements (the same indices for the same shapes in every run), written beside it as DIR/<name>.sample_index.npy (flat
indices, float64); values, indices and file headers together stay within MAX_BYTES."""
from pathlib import Path

import numpy as np
import torch

MAX_BYTES = 60_000_000  # every file written, headers included (the dump's limit is 64 MB)
NPY_HEADER_BYTES = 256  # an upper bound of np.save's header for these shapes (128 bytes in practice)
INDEX_BYTES = 8  # one float64 flat index per sampled element

# the rollout log RolloutEngine.buffer() hands to a caller (utils/rollout_engine.py), [n, A, T, ...] / [n_lights, L, T]
ROLLOUT_LOGS = ("out_pose", "out_valid", "out_motion", "out_action", "out_tl_state", "out_reward", "out_reward_valid", "out_tf",
                "out_tl_nll", "out_outside_map", "out_dest_reached")


def rollout_outputs(eng, n_steps):
    """The engine's rollout log over the first n_steps slots (W prime + K closed-loop steps of the last timed region)."""
    return {k: eng.S[k][:, :, :n_steps] for k in ROLLOUT_LOGS}


def train_outputs(metrics):
    """The metrics dict the training step returns to its caller (loss and its terms)."""
    return {k.replace("/", "."): v.detach() for k, v in metrics.items() if torch.is_tensor(v)}


def _item_bytes(t):
    return 8 if t.dtype == torch.float64 else 4


def collect(tensors, max_bytes=MAX_BYTES):
    """Device tensors -> {name: host numpy array}, sampled on the device when the .npy files would exceed max_bytes in all."""
    whole = sum(t.numel() * _item_bytes(t) for t in tensors.values()) + NPY_HEADER_BYTES * len(tensors)
    frac = 1.0
    if whole > max_bytes:
        # a sampled element costs its value and its index; every array then writes two files (a sample keeps at least one element:
        # the few bytes that floor adds are inside the header allowance, which is twice np.save's real header)
        per_element = sum(t.numel() * (_item_bytes(t) + INDEX_BYTES) for t in tensors.values())
        frac = max(0.0, max_bytes - 2 * NPY_HEADER_BYTES * len(tensors)) / max(per_element, 1)
    rng = np.random.default_rng(0)
    out = {}
    for name in sorted(tensors):
        t = tensors[name]
        dt = torch.float64 if t.dtype == torch.float64 else torch.float32
        if frac >= 1.0:
            out[name] = t.to(dt).cpu().numpy()
            continue
        n = t.numel()
        idx = np.unique(rng.integers(0, n, max(1, int(n * frac))))
        flat = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        out[name] = flat.to(dt).cpu().numpy()
        out[name + ".sample_index"] = idx.astype(np.float64)
    return out


def write(arrays, out_dir):
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(d / f"{name}.npy", a)
    return sorted(arrays)
