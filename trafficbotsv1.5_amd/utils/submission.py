"""`SubWOMD` / `SubWOSAC` (utils/submission.py:15-225 of the reference): the challenge records of the test loop, up to - not including -
the protobuf container. The reference keeps the post-processed tensors of every `update`, copies them to the host and walks scenes x
agents (x rollouts x objects) in Python to fill `waymo_open_dataset` messages. Here `update` builds the records on the device in one
launch (`tbx_womd_predictions` / `tbx_wosac_joint_scenes`: global frame, per-scene compaction, extrapolation), `aggregate_on_cpu`
makes one device-to-host copy per key and drops scenes it has already seen, and `records()` hands out the host arrays a writer would
serialise. `save_sub_file` raises: the messages need `waymo_open_dataset`.

Plain classes with the reference's method names: no torchmetrics, and no cross-rank gather (the reference's `dist_reduce_fx="cat"`) -
`compute()` returns the calling rank's records only."""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import hip


def scenario_id_codes(ids: Sequence[str], device) -> Tensor:
    """[n_sc, 16] int32: the characters of each id, padded with -1 (utils/submission.py:64-70; 16 = the longest id)."""
    code = torch.full((len(ids), 16), -1, dtype=torch.int32)
    for i, str_id in enumerate(ids):
        code[i, : len(str_id)] = torch.tensor([ord(c) for c in str_id], dtype=torch.int32)
    return code.to(device, non_blocking=True)


def scenario_id_strings(codes: np.ndarray) -> List[str]:
    """The inverse (utils/submission.py:85-86)."""
    return ["".join(chr(int(x)) for x in row if x > 0) for row in codes]


class _Sub:
    """What the two classes share: the reference's constructor arguments, device records per `update`, `compute` / `reset`, and the
    host side - scenes already seen are dropped (utils/submission.py:90,181)."""
    data_keys: List[str] = []

    def __init__(self, is_active: bool, wb_artifact: str = "", method_name: str = "", authors: Sequence[str] = (), affiliation: str = "",
                 description: str = "", method_link: str = "", account_name: str = "") -> None:
        self.is_active = bool(is_active)
        self.wb_artifact, self.method_name, self.authors = wb_artifact, method_name, list(authors)
        self.affiliation, self.description, self.method_link, self.account_name = affiliation, description, method_link, account_name
        self.submission_scenario_id: List[str] = []
        self._host: List[Dict[str, object]] = []
        self.reset()

    def reset(self) -> None:
        """Drops the device records of the updates since the last reset (what torchmetrics' reset does to the reference's states); the
        host records stay."""
        self._state: Dict[str, List[Tensor]] = {k: [] for k in self.data_keys}

    def _append(self, rec: Dict[str, Tensor]) -> None:
        for k in self.data_keys:
            self._state[k].append(rec[k])

    def compute(self) -> Optional[Dict[str, Tensor]]:
        """The records of the updates since the last reset, concatenated over scenes, on the device."""
        if not self._state[self.data_keys[0]]:
            return None
        return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in self._state.items()}

    def records(self) -> List[Dict[str, object]]:
        """One dict of host arrays per aggregated scene, in the order the scenes were first seen."""
        return self._host

    def save_sub_file(self, logger=None):
        raise NotImplementedError("the submission container (protobuf messages, tar.gz shards) needs waymo_open_dataset; "
                                  "records() returns the arrays it would hold")


class SubWOMD(_Sub):
    """Motion-prediction records: per scene the agents to predict (`ref/ag_role[..., 2]`), their k scored modes at 2 Hz in the global frame."""
    data_keys = ["trajs", "scores", "object_id", "n_pred", "scenario_id"]

    @torch.no_grad()
    def update(self, batch: Dict[str, Tensor], trajs: Tensor, scores: Tensor) -> Dict[str, Tensor]:
        """utils/submission.py:48-70 plus the selection of :94-96, one launch. trajs [n_sc, n_ag, k, n_step, 3] (x, y, yaw) and scores
        [n_sc, n_ag, k] as `WOMDPostProcessing.forward` returns them -> the appended record: "trajs" [n_sc, n_ag, k, n_step, 2] global,
        "scores", "object_id" [n_sc, n_ag] - the predicted agents first, in index order; zeros / -1 behind them -, "n_pred" [n_sc] i32,
        "scenario_id" [n_sc, 16] i32."""
        mask = batch["ref/ag_role"][..., 2].contiguous()
        pos, sc, oid, count = hip.womd_predictions(
            trajs.float().contiguous(), scores.float().contiguous(), batch["history/agent/object_id"].contiguous(), mask,
            batch["scenario_center"].float().contiguous(), batch["scenario_yaw"].float().contiguous())
        rec = {"trajs": pos, "scores": sc, "object_id": oid, "n_pred": count, "scenario_id": scenario_id_codes(batch["scenario_id"], pos.device)}
        self._append(rec)
        return rec

    def aggregate_on_cpu(self, gpu_dict_sync: Optional[Dict[str, Tensor]]) -> None:
        """utils/submission.py:75-110 up to the messages: one copy per key, then per NEW scene its predicted agents' arrays."""
        if gpu_dict_sync is None:
            return
        host = {k: gpu_dict_sync[k].cpu().numpy() for k in self.data_keys}
        for i, sid in enumerate(scenario_id_strings(host["scenario_id"])):
            if sid in self.submission_scenario_id:
                continue
            n = int(host["n_pred"][i])
            self._host.append({"scenario_id": sid, "object_id": host["object_id"][i, :n], "trajs": host["trajs"][i, :n],
                               "scores": host["scores"][i, :n]})
            self.submission_scenario_id.append(sid)


class SubWOSAC(_Sub):
    """Sim-agents records: per scene the K joint scenes' simulated trajectories and, once, the not-simulated objects' extrapolated ones."""
    data_keys = ["scenario_id", "traj_sim", "traj_no_sim", "object_id_sim", "object_id_no_sim", "n_sim", "n_no_sim"]

    @torch.no_grad()
    def update(self, wosac_data: Dict[str, Tensor], post_processing) -> Dict[str, Tensor]:
        """`post_processing.get_joint_scenes(wosac_data)` (WOSACPostProcessing: one launch) appended as a device record and returned.
        The reference keeps `wosac_data` itself here and builds the joint scenes on the host (utils/submission.py:172-174,
        wosac_post_processing.py:103-140)."""
        rec = post_processing.get_joint_scenes(wosac_data)
        self._append(rec)
        return rec

    def aggregate_on_cpu(self, gpu_dict_sync: Optional[Dict[str, Tensor]]) -> None:
        """utils/submission.py:179-185 on arrays: one copy per key, then per NEW scene "traj_sim" [K, n_sim, T, 4], "traj_no_sim"
        [n_no_sim, T, 4] (every joint scene of the scene carries these) and the two id vectors."""
        if gpu_dict_sync is None:
            return
        host = {k: gpu_dict_sync[k].cpu().numpy() for k in self.data_keys}
        for i, sid in enumerate(scenario_id_strings(host["scenario_id"])):
            if sid in self.submission_scenario_id:
                continue
            n_sim, n_ns = int(host["n_sim"][i]), int(host["n_no_sim"][i])
            self._host.append({"scenario_id": sid, "traj_sim": host["traj_sim"][i, :, :n_sim], "traj_no_sim": host["traj_no_sim"][i, :n_ns],
                               "object_id_sim": host["object_id_sim"][i, :n_sim], "object_id_no_sim": host["object_id_no_sim"][i, :n_ns]})
            self.submission_scenario_id.append(sid)
