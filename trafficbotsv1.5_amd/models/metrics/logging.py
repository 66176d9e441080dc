"""`ErrorMetrics` and `TrafficRuleMetrics` with the reference's `update` / `compute` / `reset` (models/metrics/logging.py:10-119) on
`tbx_rollout_metrics`: an update is ONE reduction of the rollout log where it lies on the device, added into a float64 state vector
(`hip.METRICS_SLOTS` values, include/tbx_hip_metrics.h names the slots) - no host read, no `.item()`; `compute` divides on the device and hands
out float32 0-d tensors like the reference's. The reference's float32 states stop counting at 2^24 agent-steps; these do not.

Both accept the engine-filled `RolloutBuffer` (views of the u8 / f32 logs, time slices of them included: read in place) and one filled
step-wise through `add` / `finish` (dense tensors), as `[n_sc, n_joint_future, n_ag, n_step]` (after `flatten_joint_future`) or
`[n_rows, n_ag, n_step]`. `sync()` is the reference's `dist_reduce_fx="sum"`: one all_reduce of the state vector."""
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from ... import hip

_ERR = ("err_counter", "err_pos_meter", "err_rot_deg", "err_spd_m_per_s")  # state[0:4]
_RULE = ("counter_agent", "counter_veh", "outside_map", "collided", "run_road_edge", "run_red_light", "passive", "goal_reached",
         "dest_reached")  # state[4:13]
_SLOT = {k: i for i, k in enumerate(_ERR + _RULE)}
_FLAG_BITS = (("collided", hip.RULE_COLLIDED), ("run_road_edge", hip.RULE_RUN_ROAD_EDGE), ("run_red_light", hip.RULE_RUN_RED_LIGHT),
              ("passive", hip.RULE_PASSIVE))


def _u8(t: Tensor) -> Tensor:
    """bool / u8 of any strides -> u8, reinterpreted where it is bool (the logs hold 0 / 1)."""
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise TypeError(f"expected a bool or uint8 tensor, got {t.dtype}")
    return t


def _rows(t: Tensor, tail: int) -> Tensor:
    """[n_sc, K, A, T, ..] or [R, A, T, ..] -> [R, A, T, ..]: a view wherever the strides allow one (the engine's logs do)."""
    return t.flatten(0, 1) if t.dim() == 4 + tail else t


def _same_rows(u8s: List[Optional[Tensor]], f32s: List[Optional[Tensor]]) -> Tuple[List[Optional[Tensor]], List[Optional[Tensor]], int]:
    """Rows of one log layout: every tensor [R, A, T(, 3)] with the same steps per row -> (u8s, f32s, ld_t). Anything else (a
    transposed view, tensors of different logs) is copied dense; strides are host metadata, nothing here reads the device."""
    lds = {hip.u8_row_steps(t) for t in u8s if t is not None} | {hip.u8_row_steps(t, 1) for t in f32s if t is not None}
    if len(lds) == 1 and None not in lds:
        return u8s, f32s, lds.pop()
    dense = lambda ts: [None if t is None else t.contiguous() for t in ts]
    return dense(u8s), dense(f32s), u8s[0].shape[2]


class _LogMetrics(nn.Module):
    """State: one float64 vector (and tbx_rollout_metrics' workspace), on the CPU until the first update brings a device."""

    def __init__(self, prefix: str) -> None:
        super().__init__()
        self.prefix = prefix
        self.register_buffer("state", torch.zeros(hip.METRICS_SLOTS, dtype=torch.float64), persistent=False)
        self.register_buffer("_partials", torch.zeros(hip.METRICS_PARTIAL_ROWS * hip.METRICS_SLOTS, dtype=torch.float64), persistent=False)

    def reset(self) -> None:
        self.state.zero_()

    def forward(self, *a, **kw) -> Dict[str, Tensor]:  # torchmetrics' Metric.forward: this batch's value (as TrainingMetrics here)
        self.reset()
        self.update(*a, **kw)
        return self.compute()

    def sync(self, group=None) -> None:
        """Sum the state over the ranks of `group` (the reference's dist_reduce_fx="sum"); a no-op outside torch.distributed."""
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(self.state, op=torch.distributed.ReduceOp.SUM, group=group)

    def _on(self, dev) -> None:
        if self.state.device != dev:
            self.to(dev)

    def _ratio(self, num: str, den: str) -> Tensor:
        return (self.state[_SLOT[num]] / self.state[_SLOT[den]]).float()  # (0 / 0 = nan, as the reference's)


class ErrorMetrics(_LogMetrics):
    @torch.no_grad()
    def update(self, buffer, gt_valid: Tensor, gt_pose: Tensor, gt_motion: Tensor) -> None:
        """buffer.pred_valid [n_sc, 1, n_ag, n_step_buffer] (or [n_sc, n_ag, n_step_buffer]), pred_pose / pred_motion [.., 3]; gt_valid
        [n_sc, n_ag, n_step] bool, gt_pose / gt_motion [n_sc, n_ag, n_step, 3]: buffer step 0 is ground-truth step buffer.step_start."""
        pv = buffer.pred_valid
        if pv.dim() == 4 and pv.shape[1] != 1:
            raise ValueError(f"ErrorMetrics is defined for one joint future per scene (the reference squeezes that axis), got {pv.shape[1]}")
        self._on(pv.device)
        (v,), (pose, motion), ld_t = _same_rows([_u8(_rows(pv, 0))], [_rows(buffer.pred_pose, 1), _rows(buffer.pred_motion, 1)])
        T = v.shape[2]
        if tuple(gt_valid.shape[:2]) != tuple(v.shape[:2]) or pose.shape != (*v.shape, 3) or motion.shape != pose.shape \
                or gt_pose.shape != (*gt_valid.shape, 3) or gt_motion.shape != gt_pose.shape:
            raise ValueError(f"buffer rows {tuple(v.shape)} / ground truth {tuple(gt_valid.shape)}: scenes, agents or the [.., 3] logs do not match")
        if buffer.step_start + T > gt_valid.shape[-1]:
            raise ValueError(f"the buffer's {T} steps from step {buffer.step_start} on run past the {gt_valid.shape[-1]} ground-truth steps")
        hip.rollout_metrics(self.state, self._partials, v, 1, ld_t, 0, T, pred_pose=pose, pred_motion=motion,
                            gt_valid=_u8(gt_valid.contiguous()), gt_pose=gt_pose.float().contiguous(),
                            gt_motion=gt_motion.float().contiguous(), gt_t0=buffer.step_start)

    def compute(self) -> Dict[str, Tensor]:
        p = self.prefix
        return {f"{p}/err/pos_meter": self._ratio("err_pos_meter", "err_counter"),
                f"{p}/err/rot_deg": self._ratio("err_rot_deg", "err_counter"),
                f"{p}/err/spd_m_per_s": self._ratio("err_spd_m_per_s", "err_counter")}


class TrafficRuleMetrics(_LogMetrics):
    """n_agent_violating / n_agent_valid; violating = the flag is set at any step at which the agent is valid."""

    @torch.no_grad()
    def update(self, buffer, ag_type: Tensor) -> None:
        """buffer.pred_valid / buffer.violation[..] [n_sc, n_joint_future, n_ag, n_step] (or [n_rows, n_ag, n_step], n_rows a multiple
        of n_sc) bool; ag_type [n_sc, n_ag, 3] bool one-hot. A buffer without "goal_reached" (navi_mode "dest") counts none."""
        pv, vio = buffer.pred_valid, buffer.violation
        self._on(pv.device)
        n_sc = ag_type.shape[0]
        goal = vio.get("goal_reached")
        logs = [_u8(_rows(t, 0)) for t in (pv, vio["outside_map"], vio["dest_reached"])] + [None if goal is None else _u8(_rows(goal, 0))]
        (v, outside, dest, goal), _, ld_t = _same_rows(logs, [])
        R, _, T = v.shape
        if R % n_sc or tuple(ag_type.shape[1:]) != (v.shape[1], 3):
            raise ValueError(f"buffer rows {tuple(v.shape)} are no whole number of rollouts of ag_type {tuple(ag_type.shape)}")
        if any(t is not None and t.shape != v.shape for t in (outside, dest, goal)) or any(_rows(vio[k], 0).shape != v.shape for k, _ in _FLAG_BITS):
            raise ValueError("buffer.violation entries must have buffer.pred_valid's shape")
        # the four metric-only checks as TBX_RULE_* bits of one byte per step (the dict holds them as separate bool tensors)
        four = torch.stack([_rows(vio[k], 0) for k, _ in _FLAG_BITS]).view(torch.uint8)
        flags = four[0]
        for i, (_, bit) in enumerate(_FLAG_BITS[1:], 1):
            flags = flags | (four[i] << (bit.bit_length() - 1))
        hip.rollout_metrics(self.state, self._partials, v, R // n_sc, ld_t, 0, T, flags=flags, ld_flags=T, outside_map=outside,
                            dest_reached=dest, goal_reached=goal, ag_type=_u8(ag_type.contiguous()))

    def compute(self) -> Dict[str, Tensor]:
        p = self.prefix
        return {f"{p}/traffic_rule/outside_map": self._ratio("outside_map", "counter_agent"),
                f"{p}/traffic_rule/collided": self._ratio("collided", "counter_agent"),
                f"{p}/traffic_rule/run_road_edge": self._ratio("run_road_edge", "counter_veh"),
                f"{p}/traffic_rule/run_red_light": self._ratio("run_red_light", "counter_veh"),
                f"{p}/traffic_rule/passive": self._ratio("passive", "counter_veh"),
                f"{p}/traffic_rule/goal_reached": self._ratio("goal_reached", "counter_agent"),
                f"{p}/traffic_rule/dest_reached": self._ratio("dest_reached", "counter_agent")}
