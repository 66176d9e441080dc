"""`DifferentiableReward` with the reference's constructor and `get` (utils/rewards.py:9-154): the three imitation terms - position, heading,
speed, each with the criterion the configuration names (SmoothL1Loss, MSELoss, L1Loss, HuberLoss) and the heading with its angular type
(cosine, null, cast, vector; models/metrics/loss.py:9-36) - and, with `w_collision > 0`, the relaxed five-circle collision term that
couples the agents of a scene. One step per call. With every term at its default (SmoothL1 position / speed, cosine heading) the imitation
terms go through tbx_diffbar_reward - the expressions tbx_sim_step logs for every step of a rollout (`RolloutBuffer.diffbar_reward`) and
tbx_train_chain_fwd / _bwd differentiates inside the training step; with any other configuration through tbx_il_reward_fwd, the launch
the rollout engine runs once over its finished log (rollout_engine.add_imitation_terms) and train_ops.TrainChainFn differentiates. The
collision term goes through tbx_collision_reward_fwd (the launch the rollout engine runs once over its finished pose log and
train_ops.CollisionRewardFn differentiates); this stand-alone call is forward-only."""
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from .. import hip
from ..models.metrics.loss import TORCH_CRITERIA, AngularError, criterion_code


class DifferentiableReward:
    il_codes: Tuple[int, int, int, int] = (0, 0, 0, 0)  # (criterion of pos, rot, spd; angular type): TBX_IL_* / TBX_IL_ANG_* of include/tbx_hip_il.h
    il_default: bool = True  # SmoothL1 position / speed, cosine heading: the terms written into tbx_sim_step / tbx_train_chain

    def __init__(self, l_pos, l_rot, l_spd, w_collision: float, use_il_loss: bool, reduce_collsion_with_max: bool, is_enabled: bool = True):
        self.w_collision, self.reduce_collsion_with_max, self.is_enabled, self.use_il_loss = w_collision, reduce_collsion_with_max, is_enabled, use_il_loss
        if use_il_loss:
            self.il_l_rot = AngularError(l_rot["criterion"], l_rot.get("angular_type"))
            self.il_criteria = (l_pos["criterion"], l_rot["criterion"], l_spd["criterion"])
            self.il_codes = (criterion_code(l_pos["criterion"], "differentiable_reward.l_pos"), self.il_l_rot.criterion_code,
                             criterion_code(l_spd["criterion"], "differentiable_reward.l_spd"), self.il_l_rot.angular_code)
            self.il_default = self.il_codes[0] == hip.IL_SMOOTH_L1 and self.il_codes[2] == hip.IL_SMOOTH_L1 and self.il_codes[3] == hip.IL_ANG_COSINE
            self.il_w_pos, self.il_w_rot, self.il_w_spd = float(l_pos["weight"]), float(l_rot["weight"]), float(l_spd["weight"])

    @property
    def il_weights(self) -> Tuple[float, float, float]:
        return self.il_w_pos, self.il_w_rot, self.il_w_spd

    @property
    def il_config(self):
        """(il_codes, il_weights) of a reward whose imitation terms are NOT the ones written into tbx_sim_step / tbx_train_chain, else None
        - then nothing of libtbx_il.so is launched."""
        return None if (not self.use_il_loss or self.il_default) else (self.il_codes, self.il_weights)

    def torch_errors(self, gt_pose: Tensor, gt_motion: Tensor, pred_pose: Tensor, pred_motion: Tensor):
        """(e_pos, e_rot, e_spd) of rewards.py:60-62 as torch expressions (autograd; any device): what the torch state machine of the
        training step differentiates - the checked reference of the fused path."""
        e_pos = TORCH_CRITERIA[self.il_criteria[0]](gt_pose[..., :2], pred_pose[..., :2]).sum(-1)
        e_rot = self.il_l_rot.compute_torch(gt_pose[..., 2], pred_pose[..., 2])
        e_spd = TORCH_CRITERIA[self.il_criteria[2]](gt_motion[..., 0], pred_motion[..., 0])
        return e_pos, e_rot, e_spd

    @torch.no_grad()
    def imitation(self, pred_valid: Tensor, pred_pose: Tensor, pred_motion: Tensor, gt_valid: Tensor, gt_pose: Tensor, gt_motion: Tensor) -> Tensor:
        """The imitation terms of ONE step with this configuration's criteria, [n_sc, n_ag, 4] = r_pos, r_rot, r_spd, their sum
        (tbx_il_reward_fwd on one-step views: gt_offset 0)."""
        c = lambda t: t.float().contiguous()
        u8 = lambda t: t.to(torch.uint8).contiguous()
        n, A = pred_valid.shape
        out4 = torch.empty(n, A, 4, dtype=torch.float32, device=pred_pose.device)
        hip.il_reward_fwd(u8(pred_valid).view(n, 1, A), c(pred_pose).view(n, 1, A, 3), c(pred_motion).view(n, 1, A, 3), u8(gt_valid).view(n, A, 1),
                          c(gt_pose).view(n, A, 1, 3), c(gt_motion).view(n, A, 1, 3), self.il_codes, self.il_weights, gt_offset=0, out4=out4.view(n, 1, A, 4))
        return out4

    @torch.no_grad()
    def get(self, pred_valid: Tensor, pred_pose: Tensor, pred_motion: Tensor, gt_valid: Optional[Tensor], gt_pose: Optional[Tensor],
            gt_motion: Optional[Tensor], ag_size: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """[n_sc, n_ag] / [n_sc, n_ag, 3] tensors of ONE step -> the reference's reward dict."""
        if not self.is_enabled:
            return {}
        if self.w_collision > 0 and ag_size is None:
            raise ValueError("DifferentiableReward.get: w_collision > 0 needs ag_size [n_sc, n_ag, 3]")
        c = lambda t: t.float().contiguous()
        u8 = lambda t: t.to(torch.uint8).contiguous()
        il = self.use_il_loss and gt_valid is not None
        if il and not self.il_default:
            out4, valid = self.imitation(pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion), pred_valid.bool() & gt_valid.bool()
        else:  # today's path, untouched
            w = (self.il_w_pos, self.il_w_rot, self.il_w_spd) if il else (0.0, 0.0, 0.0)
            out4, valid = hip.diffbar_reward(u8(pred_valid), c(pred_pose), c(pred_motion), u8(gt_valid) if il else None,
                                             c(gt_pose) if il else None, c(gt_motion) if il else None, *w)
        out = {"diffbar_reward_valid": valid.bool(), "diffbar_reward": out4[..., 3], "r_imitation_pos": out4[..., 0],
               "r_imitation_rot": out4[..., 1], "r_imitation_spd": out4[..., 2], "r_traffic_rule_approx": torch.zeros_like(out4[..., 0])}
        if self.w_collision > 0:
            # one step = a log of T = 1: [n_sc, 1, n_ag(, 3)] views; the term is 0 on invalid agents by construction
            term, _ = hip.collision_reward_fwd(c(pred_pose).unsqueeze(1), u8(pred_valid).unsqueeze(1), c(ag_size), self.reduce_collsion_with_max,
                                               want_arg=False)
            out["diffbar_reward_valid"] = pred_valid.bool()
            out["r_traffic_rule_approx"] = (-1.0 * self.w_collision * term[:, 0]).masked_fill_(~out["diffbar_reward_valid"], 0.0)
            out["diffbar_reward"] = out["diffbar_reward"] + out["r_traffic_rule_approx"]
        return out
