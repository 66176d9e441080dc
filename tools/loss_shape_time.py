"""What the loss shaping of the training objective (temporal_discount, p_loss_for_irrelevant, w_relevant_agent) costs on the device.

  python tools/loss_shape_time.py      tbx_loss_shape (hip.loss_shape: its two launches + the output allocations) at the training shape, 16
                                       scenes x 64 agents x 90 steps in the chain's [n, T, A] layout, against a torch restatement of the
                                       reference's models/metrics/training.py:90-138 on the same device tensors (the Python loop over time
                                       with 4 elementwise launches per step, the masks and reductions around it)

Same process, HIP events around `reps` back-to-back repetitions after `warmup` untimed ones; medians over `rounds` such measurements. One
JSON line."""
import json
import statistics
import sys
from importlib import import_module
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402


def timed(fn, warmup=5, reps=10, rounds=9):
    """Median ms per call of fn over `rounds` event-timed runs of `reps` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def torch_shaping(pred_valid, tf, reward_valid, reward, ag_role, pick, start, tf_loss, p, w_rel, discount):
    """training.py:90-138 on [n, A, T] tensors (the agent weight per (scene, agent), as the kernel applies it) -> (sum, counter)."""
    lv = pred_valid
    if p < 1.0:
        rel = ag_role.any(-1, keepdim=True)
        if p > 0.0:
            rel = rel | pick.unsqueeze(-1)
        lv = lv & rel
    if start > 0:
        lv = lv.clone()
        lv[:, :, :start] &= False
    if not tf_loss:
        lv = lv & ~tf
    w = lv.any(-1) + ag_role.any(-1) * w_rel if w_rel > 0 else None
    rv = lv & reward_valid
    err = reward.masked_fill(~rv, 0.0)
    if w is not None:
        err = err * w.unsqueeze(-1)
    if discount > 0:
        m = torch.ones_like(err)
        for i in range(1, m.shape[-1]):
            f = tf[:, :, i].type(m.dtype)
            m[:, :, i] = f + (1 - f) * m[:, :, i - 1] * discount
        err = err * m
    return err.sum(), rv.sum()


def main(n=16, A=64, T=90):
    load_package()
    hip = import_module("trafficbots_amd.hip")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    chain = lambda x: x.permute(0, 2, 1).contiguous().to(dev).permute(0, 2, 1)  # [n, A, T] views of [n, T, A] logs
    pred_valid, tf = chain(r(n, A, T) < 0.85), chain((torch.arange(T) < 10).expand(n, A, T) | (r(n, A, T) < 0.1))
    reward_valid, reward = chain(r(n, A, T) < 0.9), chain(-r(n, A, T))
    ag_role, pick = (r(n, A, 3) < 0.2).to(dev), (r(n, A) < 0.5).to(dev)
    relevant = ag_role.any(-1).contiguous()
    cfg = dict(start=10, tf_loss=True, p=0.5, w_rel=2.0, discount=0.9)

    def kernel():
        return hip.loss_shape(pred_valid, tf, cfg["start"], cfg["tf_loss"], reward=reward, reward_valid=reward_valid, relevant=relevant, pick=pick,
                              mask_irrelevant=True, w_relevant=cfg["w_rel"], discount=cfg["discount"], want_w=True)

    def reference():
        return torch_shaping(pred_valid, tf, reward_valid, reward, ag_role, pick, **cfg)

    acc, (s, c) = kernel()[3], reference()
    k_ms, t_ms = timed(kernel), timed(reference, warmup=3, reps=3, rounds=7)
    print(json.dumps({"what": "tbx_loss_shape vs torch restatement of training.py:90-138", "n": n, "A": A, "T": T, "layout": "[n, T, A]",
                      "kernel_ms": round(k_ms[0], 4), "kernel_ms_min_max": [round(k_ms[1], 4), round(k_ms[2], 4)],
                      "torch_ms": round(t_ms[0], 3), "torch_ms_min_max": [round(t_ms[1], 3), round(t_ms[2], 3)],
                      "ratio": round(t_ms[0] / k_ms[0], 1), "sum_kernel": float(acc[0]), "sum_torch": float(s), "count_kernel": float(acc[1]),
                      "count_torch": int(c)}), flush=True)


if __name__ == "__main__":
    main()
