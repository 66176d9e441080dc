"""`WOSACPostProcessing._filter_futures` (data_modules/wosac_post_processing.py:12-64 of the reference): of the K joint
futures simulated per scene keep the 32 with the fewest collisions / road-edge crossings among the agents that carry a
role. The step right after the rollout and its rule checks; scoring, ranking and the gather of the
kept trajectories are one C-ABI call (`tbx_filter_futures`) on the device-resident rollout log.

`forward` (:66-105) continues on the device: the kept futures and the not-simulated agents' histories are moved from the scenario
frame to the global frame by `tbx_pose_to_global`; the records keep the reference's names and shapes. `get_joint_scenes` builds what
`get_scenario_rollouts` (:103-202) fills its protobuf messages with - compaction by validity, constant-velocity extrapolation - as
device arrays in one launch (`tbx_wosac_joint_scenes`); the messages themselves need `waymo_open_dataset` and are out of scope.
"""
from typing import Dict

import torch
from torch import Tensor, nn

from .. import hip
from ..utils.buffer import RolloutBuffer
from ..utils.submission import scenario_id_codes


class WOSACPostProcessing(nn.Module):
    def __init__(self, step_gt: int, step_current: int, const_vel_z_sim: bool, const_vel_no_sim: bool, w_road_edge: float,
                 use_wosac_col: bool) -> None:
        super().__init__()
        self.step_gt, self.step_current = step_gt, step_current
        self.const_vel_z_sim, self.const_vel_no_sim = const_vel_z_sim, const_vel_no_sim
        self.n_joint_future = 32  # from the WOSAC challenge (wosac_post_processing.py:28)
        self.w_road_edge, self.use_wosac_col = w_road_edge, use_wosac_col
        self.last_idx = None   # [n_sc, 32] i32 rollouts kept by the last call, ascending (score, index)
        self.last_score = None  # [n_sc, K] f32

    @torch.no_grad()
    def _filter_futures(self, buffer: RolloutBuffer, ag_role: Tensor) -> Tensor:
        """buffer.pred_pose [n_sc, K, A, T, 3], buffer.violation[*] [n_sc, K, A, T] bool, ag_role [n_sc, A, 3] bool
        -> trajs [n_sc, min(K, 32), A, T - step_future_start, 3]. Ties between equally bad rollouts go to the lower index
        (the reference's topk leaves them unspecified)."""
        start = buffer.step_future_start
        n_sc, K, A, T = buffer.pred_pose.shape[:4]
        if K <= self.n_joint_future:
            return buffer.pred_pose[:, :, :, start:]
        col = buffer.violation["collided_wosac" if self.use_wosac_col else "collided"]
        bit = hip.RULE_COLLIDED_WOSAC if self.use_wosac_col else hip.RULE_COLLIDED
        flags = (col.to(torch.uint8) * bit + buffer.violation["run_road_edge"].to(torch.uint8) * hip.RULE_RUN_ROAD_EDGE)
        self.last_score, self.last_idx, trajs = hip.filter_futures(
            flags.reshape(n_sc * K, A, T).contiguous(), bit, ag_role.any(-1).to(torch.uint8).contiguous(), n_sc, K, start,
            float(self.w_road_edge), self.n_joint_future, pred_pose=buffer.pred_pose.reshape(n_sc * K, A, T, 3).float().contiguous())
        return trajs

    @torch.no_grad()
    def forward(self, batch: Dict[str, Tensor], buffer: RolloutBuffer) -> Dict[str, Tensor]:
        """wosac_post_processing.py:66-105. pos_sim / yaw_sim [n_sc, min(K, 32), n_ag, n_step_future, 2 / 1] and pos_no_sim / yaw_no_sim
        [n_sc, n_ag_no_sim, n_step_history, 2 / 1] in the global frame, scenario_id [n_sc, 16] i32 (characters, padded with -1), the
        other keys passed through."""
        trajs = self._filter_futures(buffer, batch["ref/ag_role"])  # dense, or (K <= 32) a time slice of the log - read in place
        n_sc, K, A, T = trajs.shape[:4]
        ld_t = hip.log_row_steps(trajs)
        if ld_t is None:
            trajs, ld_t = trajs.float().contiguous(), T
        center, yaw = batch["scenario_center"].float().contiguous(), batch["scenario_yaw"].float().contiguous()
        pos_sim, yaw_sim = hip.pose_to_global(trajs, 3, trajs[..., 2], 3, center, yaw, K * A, T, ld_t)
        pos_ns, yaw_ns = batch["history/agent_no_sim/pos"].float().contiguous(), batch["history/agent_no_sim/yaw_bbox"].float().contiguous()
        N, Th = pos_ns.shape[1:3]
        pos_no_sim, yaw_no_sim = hip.pose_to_global(pos_ns, pos_ns.shape[-1], yaw_ns, 1, center, yaw, N, Th, Th)
        return {
            "scenario_id": scenario_id_codes(batch["scenario_id"], trajs.device),  # (wosac_post_processing.py:81-86)
            "valid_sim": batch["history/agent/valid"],
            "pos_sim": pos_sim.view(n_sc, K, A, T, 2),
            "z_sim": batch["history/agent/pos"][..., 2:3],
            "yaw_sim": yaw_sim.view(n_sc, K, A, T, 1),
            "valid_no_sim": batch["history/agent_no_sim/valid"],
            "object_id_sim": batch["history/agent/object_id"],
            "pos_no_sim": pos_no_sim.view(n_sc, N, Th, 2),
            "z_no_sim": batch["history/agent_no_sim/pos"][..., 2:3],
            "yaw_no_sim": yaw_no_sim.view(n_sc, N, Th, 1),
            "object_id_no_sim": batch["history/agent_no_sim/object_id"],
        }

    @torch.no_grad()
    def get_joint_scenes(self, wosac_data: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """What `get_scenario_rollouts` (wosac_post_processing.py:103-202) puts into its protobuf messages, as device arrays from ONE
        launch (`tbx_wosac_joint_scenes`): per scene the objects valid at `step_current`, packed to the front in index order.
        -> "scenario_id" (passed through), "traj_sim" [n_sc, K, n_ag, T, 4] (center_x, center_y, center_z, heading), "traj_no_sim"
        [n_sc, n_ag_no_sim, T, 4] - stored once per scene, where the reference copies it into each of the K joint scenes -,
        "object_id_sim" [n_sc, n_ag] / "object_id_no_sim" [n_sc, n_ag_no_sim] i64 (-1 past the count), "n_sim" / "n_no_sim" [n_sc] i32.
        T = step_gt - step_current must be pos_sim's step count (the reference silently builds trajectories of unequal length)."""
        pos_sim = wosac_data["pos_sim"]
        T = self.step_gt - self.step_current
        if pos_sim.shape[3] != T:
            raise ValueError(f"get_joint_scenes: pos_sim has {pos_sim.shape[3]} future steps, step_gt - step_current = {T}")
        dense = lambda k: wosac_data[k].squeeze(-1).contiguous()  # (z_* are column views of the batch's positions: [n_sc, n, Th] copies)
        traj_sim, traj_no_sim, id_sim, id_no_sim, count = hip.wosac_joint_scenes(
            pos_sim.contiguous(), dense("yaw_sim"), wosac_data["valid_sim"].contiguous(), dense("z_sim"), wosac_data["object_id_sim"].contiguous(),
            wosac_data["pos_no_sim"].contiguous(), dense("yaw_no_sim"), dense("z_no_sim"), wosac_data["valid_no_sim"].contiguous(),
            wosac_data["object_id_no_sim"].contiguous(), self.step_current, self.const_vel_z_sim, self.const_vel_no_sim)
        return {"scenario_id": wosac_data["scenario_id"], "traj_sim": traj_sim, "traj_no_sim": traj_no_sim, "object_id_sim": id_sim,
                "object_id_no_sim": id_no_sim, "n_sim": count[:, 0], "n_no_sim": count[:, 1]}

    def get_scenario_rollouts(self, wosac_data):
        raise NotImplementedError("the protobuf submission records need waymo_open_dataset (SURVEY.md §8f); "
                                  "get_joint_scenes(wosac_data) returns what they hold as arrays")
