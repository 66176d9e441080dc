"""Float64 restatement of the imitation terms of the differentiable reward for every criterion / angular type (include/tbx_hip_il.h;
utils/rewards.py:58-74 and models/metrics/loss.py:9-36 of the reference), with autograd for the gradients, and the seeded inputs the
fixture generator (tests/golden/make_golden_il_loss.py) and the tests (test_il_loss_ref.py, test_hip_il_loss.py) share.

With d = gt - pred: SmoothL1 / Huber |d| < 1 ? 0.5 d^2 : |d| - 0.5, MSE d^2, L1 |d| (torch's sign(0) = 0 at the kink).
e_rot: cosine 0.5 (1 - cos(gw - pw)); none crit(gw - pw); cast crit(wrap(gw - pw)), wrap(a) = (a + pi) mod 2 pi - pi (floor-mod);
vector crit(cos gw - cos pw) + crit(sin gw - sin pw). r_x = -w_x e_x, 0 where !(pred_valid && gt_valid) and where the slot's ground-truth
index t + gt_offset is past the ground truth; sum = (r_pos + r_rot) + r_spd."""
import math

import torch

WEIGHTS = (0.1, 10.0, 0.1)  # sim_agent.yaml's l_pos / l_rot / l_spd weights
CRITERIA = ("SmoothL1Loss", "MSELoss", "L1Loss", "HuberLoss")
# name -> (criterion of pos, of rot, of spd, angular_type)
CONFIGS = {}
for _c in CRITERIA:  # each criterion on pos and spd, cosine heading
    CONFIGS[f"{_c}_cosine"] = (_c, "SmoothL1Loss", _c, "cosine")
for _a in (None, "cast", "vector"):  # the three non-cosine angular types x three criteria on rot
    for _c in ("SmoothL1Loss", "MSELoss", "L1Loss"):
        CONFIGS[f"rot_{_a}_{_c}"] = ("SmoothL1Loss", _c, "SmoothL1Loss", _a)
CONFIGS["mixed"] = ("MSELoss", "SmoothL1Loss", "L1Loss", "cast")
# the two training configurations of tests/golden/train_c1_il.npz
TRAIN_CONFIGS = {"mse_l1_cast": ("MSELoss", "SmoothL1Loss", "L1Loss", "cast"), "huber_sl1_vector_mse": ("HuberLoss", "MSELoss", "SmoothL1Loss", "vector")}
GOLDEN_CASE = dict(rows=3, A=80, T=1, Tg=1, n_k=1, gt_offset=0, seed=1)  # the one-step inputs of tests/golden/il_loss.npz
MAX_EXCLUDED = 0.05  # of a case's elements
CAST_MARGIN, L1_MARGIN = 1e-3, 1e-6


def reward_cfg(cfg, weights=WEIGHTS):
    """The l_pos / l_rot / l_spd sections of a `differentiable_reward` configuration."""
    return dict(l_pos=dict(weight=weights[0], criterion=cfg[0]), l_rot=dict(weight=weights[1], criterion=cfg[1], angular_type=cfg[3]),
                l_spd=dict(weight=weights[2], criterion=cfg[2]))


def make_case(rows, A, T, Tg, n_k, gt_offset, seed):
    """Seeded float32 inputs: pred_valid [rows, T, A] bool, pred_pose / pred_motion [rows, T, A, 3], gt_valid [rows / n_k, A, Tg] bool,
    gt_pose / gt_motion [rows / n_k, A, Tg, 3], and `planted` [rows, T, A, 4] bool: where the x, y, yaw, speed of the prediction IS the
    ground truth's (d exactly 0). Where a slot has a ground truth, the prediction is the ground truth minus d with d drawn from a
    mixture - uniform in [-2, 2] (both sides of the SmoothL1 kink), uniform in [-100, 100] (metres: MSE's range), N(0, 0.3) - for x, y and
    the speed, and uniform in [-2 pi, 2 pi] for the yaw (ground-truth yaw uniform in [-pi, pi)); ~20 % of the predictions and of the
    ground truth are invalid."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + A + 13 * T)
    rnd = lambda *s: torch.rand(*s, generator=g)
    n_sc = rows // n_k
    gt_pose = torch.cat([(rnd(n_sc, A, Tg, 2) - 0.5) * 400.0, (rnd(n_sc, A, Tg, 1) - 0.5) * 2 * math.pi], -1)
    gt_motion = torch.cat([rnd(n_sc, A, Tg, 1) * 30.0, torch.randn(n_sc, A, Tg, 2, generator=g)], -1)
    gt_valid = rnd(n_sc, A, Tg) > 0.2
    pred_valid = rnd(rows, T, A) > 0.2
    pred_pose = torch.cat([(rnd(rows, T, A, 2) - 0.5) * 400.0, (rnd(rows, T, A, 1) - 0.5) * 4 * math.pi], -1)
    pred_motion = torch.cat([rnd(rows, T, A, 1) * 30.0, torch.randn(rows, T, A, 2, generator=g)], -1)
    kind = torch.randint(0, 3, (rows, T, A, 4), generator=g)
    d = torch.where(kind == 0, (rnd(rows, T, A, 4) - 0.5) * 4.0, torch.where(kind == 1, (rnd(rows, T, A, 4) - 0.5) * 200.0,
                                                                              torch.randn(rows, T, A, 4, generator=g) * 0.3))
    d[..., 2] = (rnd(rows, T, A) - 0.5) * 4 * math.pi
    planted = rnd(rows, T, A, 4) < 0.06
    d[planted] = 0.0
    for t in range(T):
        s = t + gt_offset
        if s >= Tg:
            continue
        gp = gt_pose[:, :, s].repeat_interleave(n_k, 0)  # [rows, A, 3]
        gv = gt_motion[:, :, s, 0].repeat_interleave(n_k, 0)
        pred_pose[:, t] = torch.where(planted[:, t, :, :3], gp, gp - d[:, t, :, :3])
        pred_motion[:, t, :, 0] = torch.where(planted[:, t, :, 3], gv, gv - d[:, t, :, 3])
    if T > Tg - gt_offset:
        planted[:, max(Tg - gt_offset, 0):] = False
    return dict(pred_valid=pred_valid, pred_pose=pred_pose, pred_motion=pred_motion, gt_valid=gt_valid, gt_pose=gt_pose, gt_motion=gt_motion,
                planted=planted, n_k=n_k, gt_offset=gt_offset)


def upstream_weight(rows, T, A, seed=5):
    """The fixed random dL/d(sum) [rows, T, A] (float64) the gradients are taken under."""
    return torch.randn(rows, T, A, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def crit(name, d):
    if name in ("SmoothL1Loss", "HuberLoss"):
        return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    if name == "MSELoss":
        return d * d
    assert name == "L1Loss", name
    return d.abs()


def wrap(a):
    return torch.remainder(a + math.pi, 2 * math.pi) - math.pi


def _aligned_gt(case, T):
    """(has_gt [T] bool list, gt_valid [rows, T, A], gt_pose [rows, T, A, 3], gt speed [rows, T, A]) aligned with the log's slots (zeros past the ground truth)."""
    n_k, off = case["n_k"], case["gt_offset"]
    Tg = case["gt_valid"].shape[2]
    idx = [min(t + off, Tg - 1) for t in range(T)]
    has = torch.tensor([t + off < Tg for t in range(T)])
    al = lambda x: x[:, :, idx].repeat_interleave(n_k, 0).transpose(1, 2)
    return has, al(case["gt_valid"]) & has[None, :, None], al(case["gt_pose"]), al(case["gt_motion"])[..., 0]


def errors(case, cfg, dtype=torch.float64, pred_pose=None, pred_spd=None):
    """(e_pos, e_rot, e_spd, mask) [rows, T, A] of a case under cfg = (crit_pos, crit_rot, crit_spd, angular_type); mask: the element counts."""
    pp = case["pred_pose"].to(dtype) if pred_pose is None else pred_pose
    pv = case["pred_motion"][..., 0].to(dtype) if pred_spd is None else pred_spd
    _, gvalid, gp, gs = _aligned_gt(case, pp.shape[1])
    gp, gs = gp.to(dtype), gs.to(dtype)
    e_pos = crit(cfg[0], gp[..., 0] - pp[..., 0]) + crit(cfg[0], gp[..., 1] - pp[..., 1])
    e_spd = crit(cfg[2], gs - pv)
    gw, pw = gp[..., 2], pp[..., 2]
    if cfg[3] == "cosine":
        e_rot = 0.5 * (1 - torch.cos(gw - pw))
    elif cfg[3] is None:
        e_rot = crit(cfg[1], gw - pw)
    elif cfg[3] == "cast":
        e_rot = crit(cfg[1], wrap(gw - pw))
    else:
        assert cfg[3] == "vector", cfg[3]
        e_rot = crit(cfg[1], torch.cos(gw) - torch.cos(pw)) + crit(cfg[1], torch.sin(gw) - torch.sin(pw))
    return e_pos, e_rot, e_spd, case["pred_valid"] & gvalid


def reward(case, cfg, weights=WEIGHTS, upstream=None, dtype=torch.float64):
    """-> dict(r4 [rows, T, A, 4] = r_pos, r_rot, r_spd, sum; valid [rows, T, A]; and, with `upstream` [rows, T, A] = dL/d(sum),
    d_pose [rows, T, A, 3] / d_spd [rows, T, A] = dL/d(prediction), by autograd)."""
    pp = case["pred_pose"].to(dtype).clone().requires_grad_(upstream is not None)
    pv = case["pred_motion"][..., 0].to(dtype).clone().requires_grad_(upstream is not None)
    e_pos, e_rot, e_spd, mask = errors(case, cfg, dtype, pp, pv)
    r = [(-w * e).masked_fill(~mask, 0.0) for w, e in zip(weights, (e_pos, e_rot, e_spd))]
    total = (r[0] + r[1]) + r[2]
    out = {"r4": torch.stack(r + [total], -1).detach(), "valid": mask}
    if upstream is not None:
        (total * upstream.to(dtype)).sum().backward()
        out["d_pose"], out["d_spd"] = pp.grad, pv.grad
    return out


def excluded(case, cfg):
    """[rows, T, A] bool: the elements left out of a GRADIENT comparison - the values are continuous there, the derivative is not:
    cast: |wrap(gw - pw)| within CAST_MARGIN of pi; an L1 criterion: an argument with 0 < |d| < L1_MARGIN."""
    pp, pv = case["pred_pose"].double(), case["pred_motion"][..., 0].double()
    _, _, gp, gs = _aligned_gt(case, pp.shape[1])
    gp, gs = gp.double(), gs.double()
    near0 = lambda d: (d.abs() > 0) & (d.abs() < L1_MARGIN)
    ex = torch.zeros(pp.shape[:3], dtype=torch.bool)
    if cfg[0] == "L1Loss":
        ex |= near0(gp[..., 0] - pp[..., 0]) | near0(gp[..., 1] - pp[..., 1])
    if cfg[2] == "L1Loss":
        ex |= near0(gs - pv)
    gw, pw = gp[..., 2], pp[..., 2]
    if cfg[3] == "cast":
        ex |= (wrap(gw - pw).abs() - math.pi).abs() < CAST_MARGIN
    if cfg[3] != "cosine" and cfg[1] == "L1Loss":
        if cfg[3] is None:
            ex |= near0(gw - pw)
        elif cfg[3] == "cast":
            ex |= near0(wrap(gw - pw))
        else:
            ex |= near0(torch.cos(gw) - torch.cos(pw)) | near0(torch.sin(gw) - torch.sin(pw))
    return ex
