"""`WOMDPostProcessing` (data_modules/womd_post_processing.py:8-278 of the reference): the K joint futures of every agent reduced to
`k_pred` scored modes at 2 Hz for the motion-prediction challenge. The reference runs `mpa_nms` as a Python loop over scenes x agents x
modes with a host branch per iteration, and `traj_aggr` as a Python loop with a host branch per empty cluster; here the whole `forward`
is one C-ABI call on the device-resident rollout log, read in the layout the engine wrote it: `tbx_womd_modes` (`traj_topk`, `mtr_nms`)
or, with `aggr_thresh` set and K > k_pred, `tbx_womd_aggr` (`traj_aggr`: greedy seeds, then `n_iter_em` rounds of k-means over whole
trajectories - each mode the mean of a cluster of futures, its score the mean of their probabilities).

Mode order (the reference's `topk(sorted=False)` leaves it unspecified): `traj_topk` in descending softmax score, ties to the lower
future index; `mtr_nms` and `traj_aggr` in pick order. `last_idx` holds the future each mode was taken from - for `traj_aggr` the seed
its cluster grew from.

`aggr_thresh` is the per-type list [veh, ped, cyc] of the other two thresholds (the reference's own `forward` hands the list to a
tensor comparison and raises TypeError). As there it wins over `mtr_nms_thresh` when both are set.
"""
from typing import Dict, Optional, Sequence

import torch
from torch import Tensor, nn

from .. import hip


class WOMDPostProcessing(nn.Module):
    def __init__(self, k_pred: int, score_temperature: float, mpa_nms_thresh: Sequence[float], mtr_nms_thresh: Sequence[float],
                 aggr_thresh: Sequence[float], n_iter_em: int, use_ade: bool, step_gt: int, step_current: int) -> None:
        super().__init__()
        self.k_pred, self.score_temperature = k_pred, score_temperature
        self.mpa_nms_thresh, self.mtr_nms_thresh, self.aggr_thresh = list(mpa_nms_thresh), list(mtr_nms_thresh), list(aggr_thresh)
        self.n_iter_em, self.use_ade = n_iter_em, use_ade
        self.track_future_samples = step_gt - step_current
        if len(self.aggr_thresh) not in (0, 3):
            raise NotImplementedError(f"aggr_thresh: expected [] or [veh, ped, cyc], got {self.aggr_thresh}; one threshold for all types "
                                      "is not implemented")
        if isinstance(n_iter_em, bool) or not isinstance(n_iter_em, int) or n_iter_em < 0:  # (checked with aggr_thresh=[] too)
            raise ValueError(f"n_iter_em = {n_iter_em!r}: expected an int >= 0")
        for name in ("mpa_nms_thresh", "mtr_nms_thresh"):
            if len(getattr(self, name)) not in (0, 3):
                raise ValueError(f"{name}: expected [] or [veh, ped, cyc], got {getattr(self, name)}")
        if not 0 < k_pred <= 8:
            raise ValueError(f"k_pred = {k_pred}: tbx_womd_modes keeps 1..8 modes")
        self.last_idx = None  # [n_sc, n_ag, k] i32: the futures kept by the last call (traj_aggr: the seeds), in output order

    @torch.no_grad()
    def forward(self, ag_type: Tensor, trajs: Tensor, scores: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """ag_type [n_sc, n_ag, 3] bool, trajs [n_sc, K, n_ag, n_step_future, 3] (x, y, yaw) - typically the view
        `buffer.pred_pose[:, :, :, step_future_start:]`, read in place -, scores [n_sc, K, n_ag] log-probabilities or None
        -> {"trajs": [n_sc, n_ag, k, n_step_2hz, 3], "scores": [n_sc, n_ag, k] normalised}, k = min(K, k_pred)."""
        n_sc, K, A, T = trajs.shape[:4]
        trajs = trajs.float()
        if hip.log_row_steps(trajs) is None:
            trajs = trajs.contiguous()  # a caller-made view that is not a time slice of a dense log
        ag_type = ag_type.contiguous()
        ag_type_u8 = ag_type.view(torch.uint8) if ag_type.dtype == torch.bool else ag_type.to(torch.uint8)  # (bool is a 0 / 1 byte: no launch)
        log_prob = None if scores is None else scores.float().contiguous().view(n_sc * K, A)
        if len(self.aggr_thresh) > 0 and K > self.k_pred:  # (:55-59; K <= k_pred: no reduction, as without it)
            out_trajs, out_scores, self.last_idx = hip.womd_aggr(
                trajs.flatten(0, 1), log_prob, ag_type_u8, n_sc, K, 0, T, self.k_pred, self.use_ade, self.aggr_thresh, self.n_iter_em,
                self.mpa_nms_thresh, self.score_temperature, 4, 5, self.track_future_samples)
        else:
            out_trajs, out_scores, self.last_idx = hip.womd_modes(
                trajs.flatten(0, 1), log_prob, ag_type_u8, n_sc, K, 0, T, self.k_pred, self.use_ade, self.mtr_nms_thresh,
                self.mpa_nms_thresh, self.score_temperature, 4, 5, self.track_future_samples)
        return {"trajs": out_trajs, "scores": out_scores}
