"""Test-side reference of error-threshold teacher forcing (the reference's utils/teacher_forcing.py:128-151), restated in plain torch, and
the layout of tests/golden/tf_threshold.npz (written by tests/golden/make_golden_tf_threshold.py from the reference itself).

For a step s with 0 < s < Tg, per (row, agent), float32 throughout:
    inv   = ~(valid & gt_valid[s-1])
    e     = (pose - gt_pose[s-1]) with 0 where inv;   e_spd = (motion[0] - gt_motion[s-1][0]) with 0 where inv
    reset = (thr_xy > 0 & |e.xy| > thr_xy) | (thr_yaw > 0 & |rad2deg(cast_rad(e.yaw))| > thr_yaw) | (thr_spd > 0 & |e_spd| > thr_spd)
    table[:, :, s] |= reset                        (in place: the table keeps the bits)
Any other s: nothing happens and the agents' override is empty (all-zero valid, pose, motion)."""
import math
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"

# (rows, A, Tg, step): smallest (state == ground truth: nothing fires); generic; one past a wavefront, last column; workload sizes, last
# column; step >= Tg twice (the empty override)
CASES = [(1, 1, 3, 1), (2, 5, 8, 4), (3, 65, 12, 11), (2, 64, 91, 90), (2, 5, 8, 8), (2, 5, 8, 9)]
# (threshold_xy, threshold_yaw, threshold_spd): each alone - the xy and speed ones on both sides of the exactly representable edges (an
# offset of (3, 4) against 5.0 and 4.99; a speed offset of 1.5 against 1.5 and 1.25) - and all three together
SETTINGS = [(5.0, -1.0, -1.0), (4.99, -1.0, -1.0), (-1.0, 20.0, -1.0), (-1.0, -1.0, 1.5), (-1.0, -1.0, 1.25), (5.0, 20.0, 1.5)]
INPUT_KEYS = ("gt_valid", "gt_pose", "gt_motion", "tl_state", "pred_valid", "pred_pose", "pred_motion", "tf_init")


def case_name(rows, A, Tg, step):
    return f"r{rows}_a{A}_t{Tg}_s{step}"


def load_cases():
    """[(name, step, {inputs as torch tensors}, {"ov_valid" [n_set, rows, A], "ov_pose", "ov_motion" [rows, A, 3], "tf_after" [n_set, rows, A, Tg]})]"""
    z = np.load(GOLDEN / "tf_threshold.npz")
    assert [tuple(s) for s in z["settings"].tolist()] == SETTINGS
    out = []
    for rows, A, Tg, step in CASES:
        name = case_name(rows, A, Tg, step)
        t = lambda k: torch.from_numpy(z[f"{name}/{k}"])
        out.append((name, step, {k: t(k) for k in INPUT_KEYS}, {k: t(k) for k in ("ov_valid", "ov_pose", "ov_motion", "tf_after")}))
    return out


def cast_rad(a: torch.Tensor) -> torch.Tensor:
    return torch.remainder(a + math.pi, 2 * math.pi) - math.pi


def resets(thresholds, step, pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion) -> torch.Tensor:
    """[rows, A] bool: this step's resets (all False outside 0 < step < Tg)."""
    thr_xy, thr_yaw, thr_spd = thresholds
    out = torch.zeros_like(pred_valid, dtype=torch.bool)
    if not 0 < step < gt_valid.shape[-1]:
        return out
    inv = ~(pred_valid.bool() & gt_valid[:, :, step - 1].bool())
    e = torch.where(inv.unsqueeze(-1), torch.zeros((), dtype=torch.float32), pred_pose.float() - gt_pose[:, :, step - 1].float())
    e_spd = torch.where(inv, torch.zeros((), dtype=torch.float32), pred_motion[..., 0].float() - gt_motion[:, :, step - 1, 0].float())
    if thr_xy > 0:
        out |= torch.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2) > thr_xy
    if thr_yaw > 0:
        out |= torch.rad2deg(cast_rad(e[..., 2])).abs() > thr_yaw
    if thr_spd > 0:
        out |= e_spd.abs() > thr_spd
    return out


def apply(thresholds, step, table, pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion):
    """The step's override ({"valid", "pose", "motion"}) and the table after the call (a copy: `table` is left alone)."""
    table = table.clone()
    if 0 < step < table.shape[-1]:
        table[:, :, step] |= resets(thresholds, step, pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion)
        ov = {"valid": table[:, :, step].clone(), "pose": gt_pose[:, :, step], "motion": gt_motion[:, :, step]}
    else:
        ov = {"valid": torch.zeros_like(table[:, :, 0]), "pose": torch.zeros_like(gt_pose[:, :, 0]), "motion": torch.zeros_like(gt_motion[:, :, 0])}
    return ov, table
