"""ctypes wrappers of the rule-check / rollout-filter / post-processing entry points (tbx_rule_*, tbx_filter_futures, tbx_womd_modes,
tbx_pose_to_global, tbx_rollout_metrics). Re-exported by hip.py."""
import ctypes as C
import os
from typing import List, Optional, Sequence

import torch

from .abi import *  # noqa: F401,F403  (constants, structures, load, declared_symbols: the C-ABI mirror)
from .abi import load, load_aggr  # noqa: F401
from .hip_base import _check, _cptr, _ptr, stream_ptr


def rule_tables(mp_valid_u8, mp_type_idx_u8, mp_pos, mp_dir):
    """-> (seg [n,M*N,4], n_seg [n] i32, lane [n,M*N,2], n_lane [n] i32): compacted road-edge segments / lane-centre nodes."""
    n, M, N = mp_valid_u8.shape
    dev = mp_pos.device
    seg = torch.empty(n, M * N, 4, dtype=torch.float32, device=dev)
    lane = torch.empty(n, M * N, 2, dtype=torch.float32, device=dev)
    n_seg = torch.empty(n, dtype=torch.int32, device=dev)
    n_lane = torch.empty(n, dtype=torch.int32, device=dev)
    rc = load().tbx_rule_tables(_cptr(mp_valid_u8, torch.uint8), _cptr(mp_type_idx_u8, torch.uint8), _cptr(mp_pos, torch.float32),
                                _cptr(mp_dir, torch.float32), mp_pos.shape[-1], n, M, N, _ptr(seg), _ptr(n_seg), _ptr(lane),
                                _ptr(n_lane), stream_ptr())
    _check(rc, "tbx_rule_tables")
    return seg, n_seg, lane, n_lane


def rule_grid(seg, n_seg, lane, n_lane):
    """tbx_rule_grid: the tables of rule_tables sorted into a uniform raster -> dict(seg, lane: the sorted tables; seg_start, lane_start
    [n, cells + 1] i32; seg_grid, lane_grid [n, 4] f32) - what RuleCtx.seg / .lane / .seg_start / ... point at."""
    n, cap = seg.shape[:2]
    dev = seg.device
    cells = int(load().tbx_rule_grid_cells())
    out = dict(seg=torch.empty_like(seg), lane=torch.empty_like(lane), seg_start=torch.empty(n, cells + 1, dtype=torch.int32, device=dev),
               lane_start=torch.empty(n, cells + 1, dtype=torch.int32, device=dev), seg_grid=torch.empty(n, 4, dtype=torch.float32, device=dev),
               lane_grid=torch.empty(n, 4, dtype=torch.float32, device=dev))
    rc = load().tbx_rule_grid(_cptr(seg, torch.float32), _cptr(n_seg, torch.int32), _cptr(lane, torch.float32), _cptr(n_lane, torch.int32), n, cap,
                              _ptr(out["seg"]), _ptr(out["seg_start"]), _ptr(out["seg_grid"]), _ptr(out["lane"]), _ptr(out["lane_start"]),
                              _ptr(out["lane_grid"]), stream_ptr())
    _check(rc, "tbx_rule_grid")
    return out


def rule_check(ctx: RuleCtx, valid_u8, pose, motion, tl_state_u8, ld_t: int, t0: int, n_t: int, flags):
    rc = load().tbx_rule_check(C.byref(ctx), _cptr(valid_u8, torch.uint8), _cptr(pose, torch.float32), _cptr(motion, torch.float32),
                               _cptr(tl_state_u8, torch.uint8), ld_t, t0, n_t, _cptr(flags, torch.uint8), stream_ptr())
    _check(rc, "tbx_rule_check")


def rule_accumulate(raw, n_rows: int, ld_t: int, t0: int, n_t: int, acc_state, passive_counter, out_now, out_acc):
    rc = load().tbx_rule_accumulate(_cptr(raw, torch.uint8), n_rows, ld_t, t0, n_t, _cptr(acc_state, torch.uint8),
                                    _cptr(passive_counter, torch.float32), _cptr(out_now, torch.uint8), _cptr(out_acc, torch.uint8),
                                    stream_ptr())
    _check(rc, "tbx_rule_accumulate")


def rule_navi_check(valid_u8, pose, boundary, map_batch_div: int, dest: Optional[dict], goal, goal_thresh, acc, out_now):
    """tbx_rule_navi_check: outside-map / destination-reached / goal-reached of ONE step. dest = dict(invalid [n,A,N] u8, pos / dir
    [n,A,N,2] f32, kind [n,A] u8, thresh [n,A] f32) or None (no destinations); goal [n,A,4] + goal_thresh [n,A] or None; acc [3,n,A] u8
    (outside_map, dest_reached, goal_reached) updated in place; out_now [3,n,A] u8."""
    n, A = valid_u8.shape
    d = dest or {}
    rc = load().tbx_rule_navi_check(_cptr(valid_u8, torch.uint8), _cptr(pose, torch.float32), _cptr(boundary, torch.float32), map_batch_div,
                                    _cptr(d.get("invalid"), torch.uint8), _cptr(d.get("pos"), torch.float32), _cptr(d.get("dir"), torch.float32),
                                    _cptr(d.get("kind"), torch.uint8), _cptr(d.get("thresh"), torch.float32), _cptr(goal, torch.float32),
                                    _cptr(goal_thresh, torch.float32), n, A, d["invalid"].shape[2] if dest else 0, _cptr(acc, torch.uint8),
                                    _cptr(out_now, torch.uint8), stream_ptr())
    _check(rc, "tbx_rule_navi_check")


def filter_futures(flags, col_bit: int, ag_role_any, n_scene: int, n_k: int, t_start: int, w_road_edge: float, n_keep: int,
                   pred_pose=None):
    """flags [n_scene*n_k, A, T] u8 bits, ag_role_any [n_scene, A] u8 -> (score [n_scene,n_k], idx [n_scene,n_keep] i32,
    trajs [n_scene, n_keep, A, T - t_start, 3] or None)."""
    A, T = flags.shape[-2:]
    dev = flags.device
    score = torch.empty(n_scene, n_k, dtype=torch.float32, device=dev)
    idx = torch.empty(n_scene, n_keep, dtype=torch.int32, device=dev)
    trajs = None if pred_pose is None else torch.empty(n_scene, n_keep, A, T - t_start, 3, dtype=torch.float32, device=dev)
    rc = load().tbx_filter_futures(_cptr(flags, torch.uint8), col_bit, _cptr(ag_role_any, torch.uint8), n_scene, n_k, A, T, t_start,
                                   w_road_edge, n_keep, _ptr(score), _ptr(idx), _cptr(pred_pose, torch.float32), _ptr(trajs),
                                   stream_ptr())
    _check(rc, "tbx_filter_futures")
    return score, idx, trajs


def _thresh3(thresh: Optional[Sequence[float]], what: str):
    """[] / None -> NULL (the step is off), three floats (veh, ped, cyc) -> a host float[3]."""
    if thresh is None or len(thresh) == 0:
        return None
    if len(thresh) != 3:
        raise ValueError(f"{what}: expected [] or [veh, ped, cyc], got {len(thresh)} values")
    return (C.c_float * 3)(*[float(v) for v in thresh])


def log_row_steps(t) -> Optional[int]:
    """t [..., A, T, 3] float32: a rollout log or a time slice of one (every dimension dense but for the row length)? -> the steps per
    row of the underlying log, else None. Dimensions of size 1 carry no stride information and are not held against the view."""
    if t.dtype != torch.float32 or t.shape[-1] != 3 or t.stride(-1) != 1 or t.stride(-2) != 3:
        return None
    lead = [(n, st) for n, st in zip(t.shape[:-2], t.stride()[:-2]) if n > 1]  # innermost last
    if not lead:
        return t.shape[-2]
    ld3 = lead[-1][1] if t.shape[-3] > 1 else None  # stride of the agent dimension = 3 * steps per row
    want = None
    for n, st in reversed(lead):
        if want is None:
            if ld3 is None:  # one agent per row: the row length is whatever the next dimension's stride says
                ld3 = st
            want = st
        if st != want or st % 3:
            return None
        want = st * n
    return ld3 // 3 if ld3 // 3 >= t.shape[-2] else None


def womd_modes(pred_pose, log_prob, ag_type_u8, n_scene: int, n_k: int, t_start: int, n_step: int, k_pred: int, use_ade: bool,
               mtr_nms_thresh: Optional[Sequence[float]] = None, mpa_nms_thresh: Optional[Sequence[float]] = None,
               score_temperature: float = -1.0, sample_first: int = 4, sample_stride: int = 5, sample_end: Optional[int] = None):
    """tbx_womd_modes on the rollout log in place. pred_pose [n_scene*n_k, A, >= t_start + n_step, 3]: rows may be longer than what is
    read (the engine's log, or a time slice of it - only the last two strides are fixed), log_prob [n_scene*n_k, A] or None,
    ag_type_u8 [n_scene, A, 3] -> (trajs [n_scene, A, k, n_out, 3], scores [n_scene, A, k], idx [n_scene, A, k] i32)."""
    R, A, T_avail = pred_pose.shape[:3]
    ld_t = log_row_steps(pred_pose) if pred_pose.dim() == 4 else None
    if ld_t is None or R != n_scene * n_k or t_start + n_step > T_avail:
        raise RuntimeError("womd_modes: pred_pose must be [n_scene*n_k, A, T, 3] rows of the rollout log (dense but for the row length)")
    mtr, mpa = _thresh3(mtr_nms_thresh, "mtr_nms_thresh"), _thresh3(mpa_nms_thresh, "mpa_nms_thresh")
    sample_end = n_step if sample_end is None else min(sample_end, n_step)
    k, n_out = min(n_k, k_pred), len(range(sample_first, sample_end, sample_stride))
    dev = pred_pose.device
    trajs = torch.empty(n_scene, A, k, n_out, 3, dtype=torch.float32, device=dev)
    scores = torch.empty(n_scene, A, k, dtype=torch.float32, device=dev)
    idx = torch.empty(n_scene, A, k, dtype=torch.int32, device=dev)
    rc = load().tbx_womd_modes(_ptr(pred_pose, torch.float32), _cptr(log_prob, torch.float32), _cptr(ag_type_u8, torch.uint8), n_scene, n_k,
                               A, ld_t, t_start, n_step, k_pred, int(bool(use_ade)), mtr, mpa, float(score_temperature), sample_first,
                               sample_stride, sample_end, _ptr(trajs), _ptr(scores), _ptr(idx), stream_ptr())
    _check(rc, "tbx_womd_modes")
    return trajs, scores, idx


def womd_aggr(pred_pose, log_prob, ag_type_u8, n_scene: int, n_k: int, t_start: int, n_step: int, k_pred: int, use_ade: bool,
              aggr_thresh: Sequence[float], n_iter_em: int, mpa_nms_thresh: Optional[Sequence[float]] = None,
              score_temperature: float = -1.0, sample_first: int = 4, sample_stride: int = 5, sample_end: Optional[int] = None):
    """tbx_womd_aggr (include/tbx_hip_aggr.h, libtbx_aggr.so) on the rollout log in place: `womd_modes`' arguments and view checks, with
    aggr_thresh [veh, ped, cyc] and n_iter_em in place of mtr_nms_thresh; n_k > k_pred.
    -> (trajs [n_scene, A, k_pred, n_out, 3] the cluster means, scores [n_scene, A, k_pred], idx [n_scene, A, k_pred] i32 the seeds)."""
    R, A, T_avail = pred_pose.shape[:3]
    ld_t = log_row_steps(pred_pose) if pred_pose.dim() == 4 else None
    if ld_t is None or R != n_scene * n_k or t_start + n_step > T_avail:
        raise RuntimeError("womd_aggr: pred_pose must be [n_scene*n_k, A, T, 3] rows of the rollout log (dense but for the row length)")
    aggr, mpa = _thresh3(aggr_thresh, "aggr_thresh"), _thresh3(mpa_nms_thresh, "mpa_nms_thresh")
    if aggr is None:
        raise ValueError("aggr_thresh: expected [veh, ped, cyc], got none (without it the call is womd_modes)")
    sample_end = n_step if sample_end is None else min(sample_end, n_step)
    n_out = len(range(sample_first, sample_end, sample_stride))
    dev = pred_pose.device
    a = WomdAggr()
    a.pred_pose, a.log_prob, a.ag_type = _ptr(pred_pose, torch.float32), _cptr(log_prob, torch.float32), _cptr(ag_type_u8, torch.uint8)
    trajs = torch.empty(n_scene, A, k_pred, n_out, 3, dtype=torch.float32, device=dev)
    scores = torch.empty(n_scene, A, k_pred, dtype=torch.float32, device=dev)
    idx = torch.empty(n_scene, A, k_pred, dtype=torch.int32, device=dev)
    a.out_trajs, a.out_scores, a.out_idx = _ptr(trajs), _ptr(scores), _ptr(idx)
    a.n_scene, a.n_k, a.n_ag, a.ld_t, a.t_start, a.n_step, a.k_pred = n_scene, n_k, A, ld_t, t_start, n_step, k_pred
    a.use_ade, a.n_iter_em, a.has_mpa = int(bool(use_ade)), int(n_iter_em), int(mpa is not None)
    a.sample_first, a.sample_stride, a.sample_end = sample_first, sample_stride, sample_end
    a.aggr_thresh = aggr
    if mpa is not None:
        a.mpa_nms_thresh = mpa
    a.score_temperature = float(score_temperature)
    _check(load_aggr().tbx_womd_aggr(C.byref(a), stream_ptr()), "tbx_womd_aggr")
    return trajs, scores, idx


def pose_to_global(xy, ld_xy: int, yaw, ld_yaw: int, scenario_center, scenario_yaw, rows_per_scene: int, n_t: int, ld_t: int):
    """tbx_pose_to_global: xy / yaw are tensors whose data pointers address point (row 0, step 0) -> (pos [n_scene*rows, n_t, 2],
    yaw [n_scene*rows, n_t]) in the global frame."""
    n_scene = scenario_yaw.shape[0]
    pos = torch.empty(n_scene * rows_per_scene, n_t, 2, dtype=torch.float32, device=xy.device)
    out_yaw = torch.empty(n_scene * rows_per_scene, n_t, dtype=torch.float32, device=xy.device)
    rc = load().tbx_pose_to_global(_ptr(xy, torch.float32), ld_xy, _ptr(yaw, torch.float32), ld_yaw, _cptr(scenario_center, torch.float32),
                                   _cptr(scenario_yaw, torch.float32), n_scene, rows_per_scene, n_t, ld_t, _ptr(pos), _ptr(out_yaw),
                                   stream_ptr())
    _check(rc, "tbx_pose_to_global")
    return pos, out_yaw


def u8_row_steps(t, tail: int = 0) -> Optional[int]:
    """t [R, A, T] (+ `tail` dense trailing dimensions): rows of a log or a time slice of one -> the steps per row of the underlying
    log (what log_row_steps finds for the float logs), else None. Dimensions of size 1 carry no stride information."""
    shape, stride = t.shape, t.stride()
    inner = 1
    for d in range(t.dim() - 1, t.dim() - 1 - tail, -1):
        if shape[d] > 1 and stride[d] != inner:
            return None
        inner *= shape[d]
    R, A, T = shape[:3]
    if T > 1 and stride[2] != inner:
        return None
    ld = stride[1] if A > 1 else (stride[0] if R > 1 else T * inner)
    if ld % inner or ld // inner < T or (R > 1 and stride[0] != A * ld):
        return None
    return ld // inner


def rollout_metrics(acc, partials, pred_valid, n_k: int, ld_t: int, t0: int, n_t: int, pred_pose=None, pred_motion=None, gt_valid=None,
                    gt_pose=None, gt_motion=None, gt_t0: int = 0, flags=None, ld_flags: int = 0, outside_map=None, dest_reached=None,
                    goal_reached=None, ag_type=None):
    """tbx_rollout_metrics: the 13 sums of ErrorMetrics / TrafficRuleMetrics of a rollout log added into acc [METRICS_SLOTS] f64.
    pred_valid [R, A, ..] u8 and the other logs are given as tensors whose data pointers address (row 0, agent 0, step 0) of rows
    ld_t steps long - views are fine, only the pointers cross; the ground truth and ag_type are dense. partials
    [METRICS_PARTIAL_ROWS, METRICS_SLOTS] f64 workspace."""
    R, A = pred_valid.shape[:2]
    if acc.numel() < METRICS_SLOTS or partials.numel() < METRICS_PARTIAL_ROWS * METRICS_SLOTS:
        raise RuntimeError("rollout_metrics: acc needs METRICS_SLOTS, partials METRICS_PARTIAL_ROWS * METRICS_SLOTS float64 values")
    u8, f32 = torch.uint8, torch.float32
    rc = load().tbx_rollout_metrics(_ptr(pred_valid, u8), _ptr(pred_pose, f32), _ptr(pred_motion, f32), R, n_k, A, ld_t, t0, n_t,
                                    _cptr(gt_valid, u8), _cptr(gt_pose, f32), _cptr(gt_motion, f32),
                                    gt_valid.shape[-1] if gt_valid is not None else 0, gt_t0, _ptr(flags, u8), ld_flags,
                                    _ptr(outside_map, u8), _ptr(dest_reached, u8), _ptr(goal_reached, u8), _cptr(ag_type, u8),
                                    _cptr(acc, torch.float64), _cptr(partials, torch.float64), stream_ptr())
    _check(rc, "tbx_rollout_metrics")
