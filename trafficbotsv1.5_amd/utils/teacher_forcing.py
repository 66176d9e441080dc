"""`TeacherForcing` (utils/teacher_forcing.py:8-168): which agents are overridden by ground truth at which step.
The whole [n_sc, n_ag, n_step] mask is built once per rollout on the device; `tbx_sim_step` indexes it by the device
step counter, so there is no per-step host work.

Error thresholds (threshold_xy [m], threshold_yaw [deg], threshold_spd [m/s]; <= 0: off) are the one schedule that reacts to the
rollout: an agent whose state at entry of step s is farther from the ground truth at s - 1 than a threshold is forced at step s. As in
the reference (:129-145) the decision is ORed IN PLACE into column s of the table before the step reads it, so the table keeps the bits
and the logged flag contains them. On device tensors that is one tbx_tf_threshold launch (include/tbx_hip_tf.h), on CPU tensors the
torch expression `threshold_resets` below. Two properties of the reference are kept: a reset does not ask for ag_valid[:, :, s] (an
agent whose track ends at s - 1 is overridden with whatever the ground truth holds at s), and the resets count as teacher forcing for
RolloutBuffer, loss_for_teacher_forcing = False and the loss shaping."""
import math
from typing import Dict, Tuple

import torch
from torch import Tensor


def threshold_resets(thresholds, pred_valid: Tensor, pred_pose: Tensor, pred_motion: Tensor, gt_valid: Tensor, gt_pose: Tensor,
                     gt_motion: Tensor) -> Tensor:
    """[n_sc, n_ag] bool: the agents a threshold puts back on the ground truth, from the state at entry of a step (pred_*) and the
    ground truth one step earlier (gt_* [n_sc, n_ag(, 3)]). float32, strict comparisons; thresholds = (xy, yaw [deg], spd), <= 0 off."""
    thr_xy, thr_yaw, thr_spd = thresholds
    ok = pred_valid.bool() & gt_valid.bool()
    reset = torch.zeros_like(ok)
    if thr_xy > 0 or thr_yaw > 0:
        e = (pred_pose - gt_pose).masked_fill(~ok.unsqueeze(-1), 0.0)
        if thr_xy > 0:
            reset |= (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]).sqrt() > thr_xy
        if thr_yaw > 0:
            yaw = torch.remainder(e[..., 2] + math.pi, 2 * math.pi) - math.pi  # transform_utils.py:9-11
            reset |= (yaw * (180.0 / math.pi)).abs() > thr_yaw
    if thr_spd > 0:
        reset |= (pred_motion[..., 0] - gt_motion[..., 0]).masked_fill(~ok, 0.0).abs() > thr_spd
    return reset


class TeacherForcing:
    def __init__(self, step_spawn_agent: int = 10, step_warm_start: int = 10, step_horizon: int = 0,
                 step_horizon_decrease_per_epoch: int = 0, prob_forcing_agent: float = 0,
                 prob_forcing_agent_decrease_per_epoch: float = 0, prob_scheduled_sampling: float = 0,
                 prob_scheduled_sampling_decrease_per_epoch: float = 0, gt_sdc: bool = False, threshold_xy: float = -1.0,
                 threshold_yaw: float = -1.0, threshold_spd: float = -1.0) -> None:
        self.threshold_xy, self.threshold_yaw, self.threshold_spd = float(threshold_xy), float(threshold_yaw), float(threshold_spd)
        self.step_spawn_agent, self.step_warm_start = step_spawn_agent, step_warm_start
        self.step_horizon, self.step_horizon_decrease_per_epoch = step_horizon, step_horizon_decrease_per_epoch
        self.prob_forcing_agent, self.prob_forcing_agent_decrease_per_epoch = prob_forcing_agent, prob_forcing_agent_decrease_per_epoch
        self.prob_scheduled_sampling = prob_scheduled_sampling
        self.prob_scheduled_sampling_decrease_per_epoch = prob_scheduled_sampling_decrease_per_epoch
        self.gt_sdc = gt_sdc

    @property
    def thresholds(self) -> Tuple[float, float, float]:
        return self.threshold_xy, self.threshold_yaw, self.threshold_spd

    @property
    def has_threshold(self) -> bool:
        """An error threshold is on: the table is written during the rollout (one tbx_tf_threshold launch per step)."""
        return self.threshold_xy > 0 or self.threshold_yaw > 0 or self.threshold_spd > 0

    @torch.no_grad()
    def init(self, ag_valid: Tensor, ag_pose: Tensor, ag_motion: Tensor, tl_state: Tensor, current_epoch: int) -> None:
        self.ag_valid, self.ag_pose, self.ag_motion, self.tl_state = ag_valid, ag_pose, ag_motion, tl_state
        self.tl_teacher_forcing = torch.ones_like(tl_state[..., 0], dtype=torch.bool)
        tf = torch.zeros_like(ag_valid)
        if self.has_threshold:  # written in place per step: a dense table and the float32 ground truth tbx_tf_threshold reads
            tf = torch.zeros(ag_valid.shape, dtype=ag_valid.dtype, device=ag_valid.device)
            self._gt_dev = None
        tf[:, :, 0] |= ag_valid[:, :, 0]
        if self.step_spawn_agent > 0:
            spawn = (~ag_valid[:, :, :-1]) & ag_valid[:, :, 1:]
            spawn[:, :, self.step_spawn_agent:] = False
            tf[:, :, 1:] |= spawn
        if self.step_warm_start >= 0:
            tf[:, :, : self.step_warm_start + 1] |= ag_valid[:, :, : self.step_warm_start + 1]
        horizon = int(self.step_horizon - self.step_horizon_decrease_per_epoch * current_epoch)
        if horizon > 0:
            tf[:, :, :horizon] |= ag_valid[:, :, :horizon]
        p_agent = self.prob_forcing_agent - self.prob_forcing_agent_decrease_per_epoch * current_epoch
        if p_agent > 0:
            pick = torch.bernoulli(torch.full_like(ag_valid[:, :, 0], p_agent, dtype=torch.float32)).bool()
            tf |= pick.unsqueeze(-1) & ag_valid
        p_ss = self.prob_scheduled_sampling - self.prob_scheduled_sampling_decrease_per_epoch * current_epoch
        if p_ss > 0:
            tf |= torch.bernoulli(torch.full_like(ag_valid, p_ss, dtype=torch.float32)).bool() & ag_valid
        if self.gt_sdc:
            tf[:, 0] |= ag_valid[:, 0]
        self.ag_teacher_forcing = tf

    @torch.no_grad()
    def get(self, step: int, pred_valid: Tensor, pred_pose: Tensor, pred_motion: Tensor) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
        if 0 < step < self.ag_teacher_forcing.shape[-1]:
            if self.has_threshold:
                self._decide(step, pred_valid, pred_pose, pred_motion)
            ag = {"valid": self.ag_teacher_forcing[:, :, step], "pose": self.ag_pose[:, :, step], "motion": self.ag_motion[:, :, step]}
        else:
            ag = {"valid": torch.zeros_like(self.ag_teacher_forcing[:, :, 0]), "pose": torch.zeros_like(self.ag_pose[:, :, 0]),
                  "motion": torch.zeros_like(self.ag_motion[:, :, 0])}
        if 0 < step < self.tl_teacher_forcing.shape[-1]:
            tl = {"valid": self.tl_teacher_forcing[:, :, step], "state": self.tl_state[:, :, step]}
        else:
            tl = {"valid": torch.zeros_like(self.tl_teacher_forcing[:, :, 0]), "state": torch.zeros_like(self.tl_state[:, :, 0])}
        return ag, tl

    def _decide(self, step: int, pred_valid: Tensor, pred_pose: Tensor, pred_motion: Tensor) -> None:
        """This step's resets into self.ag_teacher_forcing[:, :, step], in place (0 < step < n_step)."""
        tf = self.ag_teacher_forcing
        if not tf.is_cuda:
            tf[:, :, step] |= threshold_resets(self.thresholds, pred_valid, pred_pose.float(), pred_motion.float(), self.ag_valid[:, :, step - 1],
                                               self.ag_pose[:, :, step - 1].float(), self.ag_motion[:, :, step - 1].float())
            return
        from .. import hip

        if self._gt_dev is None:  # once per rollout
            self._gt_dev = (self.ag_valid.contiguous(), self.ag_pose.float().contiguous(), self.ag_motion.float().contiguous())
        hip.tf_threshold(self.thresholds, int(step), pred_valid.contiguous(), pred_pose.float().contiguous(), pred_motion.float().contiguous(),
                         *self._gt_dev, tf)
