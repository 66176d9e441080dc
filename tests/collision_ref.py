"""The relaxed five-circle collision term of the differentiable reward (w_collision > 0) and the reward dict of one step, restated as a
float64 torch expression (autograd gives the gradient). tests/test_collision_ref.py holds it against the reference's own outputs
(tests/golden/collision_reward.npz); the GPU tests compare tbx_collision_reward_fwd / _bwd and the layers above them with it.

Every agent is a row of five circles of radius w / 2 along its heading, spaced (l - w) / 4 apart (w / l = the smaller / larger of its
first two sizes). A pair's overlap is 1 - (smallest centre distance of the 5 x 5 circle pairs) / (sum of the two radii), clamped at 0; it is 0
for an agent with itself and when either agent is invalid. Per agent the overlaps are reduced over the partners by their maximum, or by
their sum (each capped at 1) over the number of valid agents. A scene without a valid agent gives 0 in sum mode (the project's stated
deviation: the reference divides 0 by 0 there). `EPS`, added to every radius and every distance, is float32's machine epsilon - the
constant of the float32 kernels - whatever the dtype this module computes in.
"""
from typing import Dict, Optional

import torch
from torch import Tensor

EPS = float(torch.finfo(torch.float32).eps)


def pair_overlap(valid: Tensor, pose: Tensor, ag_size: Tensor, dtype=torch.float64):
    """valid [n, A] bool, pose [n, A, 3] (x, y, yaw), ag_size [n, A, 3] -> (overlap [n, A, A] with the masked pairs at 0, the raw
    1 - dmin / r_sum [n, A, A] before clamp and mask, the 25 centre distances [n, A, A, 25] with the own circle major)."""
    pose, size = pose.to(dtype), ag_size.to(dtype)
    n, A = valid.shape
    short, long = size[..., :2].amin(-1), size[..., :2].amax(-1)
    heading = torch.stack([pose[..., 2].cos(), pose[..., 2].sin()], -1)                                   # [n, A, 2]
    offset = torch.arange(-2, 3, dtype=dtype, device=pose.device).view(1, 1, 5, 1)
    centre = pose[..., None, :2] + offset * heading[..., None, :] * ((long - short) / 4)[..., None, None]  # [n, A, 5, 2]
    diff = centre[:, :, None, :, None, :] - centre[:, None, :, None, :, :]                                 # [n, A(own), A(partner), 5, 5, 2]
    dist = torch.linalg.vector_norm(diff, dim=-1).reshape(n, A, A, 25) + EPS                               # (zero gradient at distance 0)
    radius = short / 2 + EPS
    raw = 1 - dist.min(-1).values / (radius[:, :, None] + radius[:, None, :])
    off = torch.eye(A, dtype=torch.bool, device=pose.device)[None] | ~valid[:, :, None] | ~valid[:, None, :]
    return raw.clamp(min=0).masked_fill(off, 0.0), raw, dist


def term(valid: Tensor, pose: Tensor, ag_size: Tensor, reduce_with_max: bool, dtype=torch.float64) -> Tensor:
    """The unweighted term c [n, A] in [0, 1]."""
    overlap = pair_overlap(valid, pose, ag_size, dtype)[0]
    if reduce_with_max:
        return overlap.amax(-1)
    return overlap.clamp(max=1).sum(-1) / valid.sum(-1, keepdim=True).clamp(min=1)


def term_log(valid: Tensor, pose: Tensor, ag_size: Tensor, reduce_with_max: bool, dtype=torch.float64) -> Tensor:
    """`term` for a log: valid [n, T, A], pose [n, T, A, 3], ag_size [n, A, 3] -> [n, T, A]."""
    n, T, A = valid.shape
    size = ag_size[:, None].expand(n, T, A, 3).reshape(n * T, A, 3)
    return term(valid.reshape(n * T, A), pose.reshape(n * T, A, 3), size, reduce_with_max, dtype).view(n, T, A)


def _smooth_l1(d: Tensor) -> Tensor:
    return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)


def get(w_collision: float, reduce_with_max: bool, use_il_loss: bool, w_pos: float, w_rot: float, w_spd: float, pred_valid: Tensor,
        pred_pose: Tensor, pred_motion: Tensor, gt_valid: Optional[Tensor], gt_pose: Optional[Tensor], gt_motion: Optional[Tensor],
        ag_size: Optional[Tensor], dtype=torch.float64) -> Dict[str, Tensor]:
    """The reward dict of one step ([n, A] tensors): three imitation terms on pred & gt valid (SmoothL1 position / speed, (1 - cos) / 2
    heading), the collision term on pred valid, their sum, and the mask the loss averages over."""
    pp, pm = pred_pose.to(dtype), pred_motion.to(dtype)
    zero = torch.zeros_like(pp[..., 0])
    out = {"diffbar_reward_valid": pred_valid, "diffbar_reward": zero, "r_imitation_pos": zero, "r_imitation_rot": zero, "r_imitation_spd": zero,
           "r_traffic_rule_approx": zero}
    if use_il_loss and gt_valid is not None:
        both = pred_valid & gt_valid
        gp, gm = gt_pose.to(dtype), gt_motion.to(dtype)
        out["diffbar_reward_valid"] = both
        out["r_imitation_pos"] = (-w_pos * _smooth_l1(gp[..., :2] - pp[..., :2]).sum(-1)).masked_fill(~both, 0.0)
        out["r_imitation_rot"] = (-w_rot * 0.5 * (1 - torch.cos(gp[..., 2] - pp[..., 2]))).masked_fill(~both, 0.0)
        out["r_imitation_spd"] = (-w_spd * _smooth_l1(gm[..., 0] - pm[..., 0])).masked_fill(~both, 0.0)
        out["diffbar_reward"] = out["r_imitation_pos"] + out["r_imitation_rot"] + out["r_imitation_spd"]
    if w_collision > 0:
        out["diffbar_reward_valid"] = pred_valid
        out["r_traffic_rule_approx"] = (-w_collision * term(pred_valid, pred_pose, ag_size, reduce_with_max, dtype)).masked_fill(~pred_valid, 0.0)
        out["diffbar_reward"] = out["diffbar_reward"] + out["r_traffic_rule_approx"]
    return out


def upstream_weight(n: int, A: int, device=None) -> Tensor:
    """The fixed non-uniform dL/dc [n, A] of the gradient comparisons: 0.5 .. 1.5, no two neighbours alike."""
    i = torch.arange(n * A, dtype=torch.float64, device=device).view(n, A)
    return 0.5 + ((i * 7) % 11) / 11


def grad(valid: Tensor, pose: Tensor, ag_size: Tensor, reduce_with_max: bool, weight: Optional[Tensor] = None, dtype=torch.float64) -> Tensor:
    """d(sum(weight * c)) / d(pose) [n, A, 3], weight = upstream_weight by default."""
    p = pose.detach().to(dtype).requires_grad_(True)
    w = upstream_weight(*valid.shape, device=pose.device) if weight is None else weight
    (term(valid, p, ag_size, reduce_with_max, dtype) * w.to(dtype)).sum().backward()
    return p.grad


def margins(valid: Tensor, pose: Tensor, ag_size: Tensor, reduce_with_max: bool) -> Dict[str, Tensor]:
    """Per agent [n, A], float64: how far the discrete decisions its gradient hangs on are from flipping (inf where none is taken).
      max_rel   the relative gap between the largest and second-largest overlap of a row, over the rows the agent is the owner, the
                winner or the runner-up of (max mode; inf in sum mode)
      min_gap   the gap [m] between the smallest and second-smallest of the 25 centre distances, over the pairs that carry gradient
                (max mode: a row's winning pair; sum mode: every pair with a positive overlap) and involve the agent
      clamp     |1 - dmin / r_sum| over the unmasked pairs that involve the agent"""
    overlap, raw, dist = pair_overlap(valid, pose, ag_size)
    n, A = valid.shape
    inf = torch.full((n, A), float("inf"), dtype=torch.float64)
    live = overlap > 0

    def spread(per_pair: Tensor, pairs: Tensor) -> Tensor:  # min over the pairs (i, j) in `pairs` of per_pair[i, j], to both i and j
        v = per_pair.masked_fill(~pairs, float("inf"))
        return torch.minimum(v.amin(2), v.amin(1))

    off = torch.eye(A, dtype=torch.bool)[None] | ~valid[:, :, None] | ~valid[:, None, :]
    out = {"clamp": spread(raw.abs(), ~off) if A > 1 else inf.clone(), "max_rel": inf.clone()}
    two = dist.topk(2, dim=-1, largest=False).values
    gap = two[..., 1] - two[..., 0]
    carrying = live
    if reduce_with_max and A > 1:
        top = overlap.topk(2, dim=-1)
        rel = ((top.values[..., 0] - top.values[..., 1]) / top.values[..., 0]).masked_fill(top.values[..., 0] <= 0, float("inf"))  # [n, A]
        m = rel.clone()
        for k in range(2):  # the winner and the runner-up of a row inherit the row's gap
            m = torch.minimum(m, torch.full_like(m, float("inf")).scatter_reduce(1, top.indices[..., k], rel, "amin"))
        out["max_rel"] = m
        carrying = torch.zeros_like(live).scatter_(2, top.indices[..., :1], True) & live
    out["min_gap"] = spread(gap, carrying) if A > 1 else inf.clone()
    return out


MARGIN_FLOOR = {"max_rel": 1e-5, "min_gap": 1e-4, "clamp": 1e-5}


def inside_margins(m: Dict[str, Tensor]) -> Tensor:
    """bool [n, A]: the agents whose gradient is compared (every decision margin at or above its floor)."""
    ok = torch.ones_like(m["clamp"], dtype=torch.bool)
    for k, floor in MARGIN_FLOOR.items():
        ok &= torch.as_tensor(m[k]) >= floor
    return ok
