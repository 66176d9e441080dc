#!/usr/bin/env python
"""Generate tests/golden/sub_records.npz by running the REFERENCE's submission code (the checkout make_golden.py imports) on seeded
inputs (`synthetic.make_sub_case`, `make_womd_sub_case` - ours, shipped): `WOSACPostProcessing.get_scenario_rollouts` unchanged, with
`sim_agents_submission_pb2` replaced by three plain record classes that only store their keyword arguments, `SubWOMD.update` called
unbound on a namespace with its five list states, and the `mask_pred` selection of `aggregate_on_cpu` (utils/submission.py:94-96)
restated as its three indexing statements. Container-only tooling, like make_golden.py whose shims it uses; the fixture holds the
reference's outputs only (plus, as a JSON string, the arguments each case was made with).

Layout per WOSAC case `c` (ragged lists padded to the object axis, zeros / -1 behind the count):
    c_n_sim, c_n_no_sim [n_sc] i32; c_id_sim [n_sc, A], c_id_no_sim [n_sc, N] i64
    c_sim_xyh   [n_sc, K, A, T, 3] f32  center_x, center_y, heading of every rollout: copies of the inputs (float32 in the reference)
    c_sim_z     [n_sc, A, T] f64        center_z: the same array in every rollout (asserted here), float64 in the reference under numpy 2
    c_ns_xyz    [n_sc, N, T, 3] f64     the extrapolated centre of the not-simulated objects; c_ns_heading [n_sc, N, T] f32
    (the not-simulated list is the same object in each of the K joint scenes: asserted)
`flags_off` has the inputs of `default`: its c_sim_xyh equals default's (asserted) and is not stored twice.
WOMD: womd_pos [n_sc, A, k, n, 2] f32, womd_scores [n_sc, A, k] f32, womd_id [n_sc, A] i64 (padded), womd_n [n_sc] i32.

    python tests/golden/make_golden_sub.py
"""
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import install_shims, npz, tb  # noqa: E402

STEP_CURRENT = 10
# name -> (make_sub_case arguments, step_gt, const_vel_z_sim, const_vel_no_sim)
WOSAC_CASES = {
    "default": (dict(n_sc=3, n_k=32, n_ag=12, n_no_sim=70, n_step=20, seed=0), 30, True, True),
    "flags_off": (dict(n_sc=3, n_k=32, n_ag=12, n_no_sim=70, n_step=20, seed=0), 30, False, False),
    "edge": (dict(n_sc=1, n_k=1, n_ag=65, n_no_sim=0, n_step=3, seed=1), 13, True, True),
}
WOMD_CASE = dict(n_sc=3, n_ag=12, k=6, n=16, seed=0)


class _Record:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class SimulatedTrajectory(_Record):
    pass


class JointScene(_Record):
    pass


class ScenarioRollouts(_Record):
    pass


def gen_wosac(out):
    import data_modules.wosac_post_processing as ref_mod

    ref_mod.sim_agents_submission_pb2 = SimpleNamespace(SimulatedTrajectory=SimulatedTrajectory, JointScene=JointScene,
                                                        ScenarioRollouts=ScenarioRollouts)
    for name, (case_kw, step_gt, cz, cn) in WOSAC_CASES.items():
        data = tb.synthetic.make_sub_case(step_current=STEP_CURRENT, **case_kw)
        n_sc, K, A, T = data["pos_sim"].shape[:4]
        N = data["pos_no_sim"].shape[1]
        assert T == step_gt - STEP_CURRENT
        pp = ref_mod.WOSACPostProcessing(step_gt=step_gt, step_current=STEP_CURRENT, const_vel_z_sim=cz, const_vel_no_sim=cn, w_road_edge=0.0,
                                         use_wosac_col=True)
        ids = ["".join(chr(int(x)) for x in row if x > 0) for row in data["scenario_id"]]
        rollouts = pp.get_scenario_rollouts({k: v.clone() for k, v in data.items()})
        assert len(rollouts) == n_sc and [r.scenario_id for r in rollouts] == ids
        n_sim, n_ns = np.zeros(n_sc, np.int32), np.zeros(n_sc, np.int32)
        id_sim, id_ns = np.full((n_sc, A), -1, np.int64), np.full((n_sc, N), -1, np.int64)
        sim_xyh, sim_z = np.zeros((n_sc, K, A, T, 3), np.float32), np.zeros((n_sc, A, T), np.float64)
        ns_xyz, ns_h = np.zeros((n_sc, N, T, 3), np.float64), np.zeros((n_sc, N, T), np.float32)
        valid_sim, valid_ns = data["valid_sim"][:, :, STEP_CURRENT].numpy(), data["valid_no_sim"][:, :, STEP_CURRENT].numpy()
        for s, r in enumerate(rollouts):
            assert len(r.joint_scenes) == K
            n_sim[s], n_ns[s] = valid_sim[s].sum(), valid_ns[s].sum()
            for k, scene in enumerate(r.joint_scenes):
                trajs = scene.simulated_trajectories
                assert len(trajs) == n_sim[s] + n_ns[s]
                for j, t in enumerate(trajs[:n_sim[s]]):
                    assert t.center_x.dtype == t.center_y.dtype == t.heading.dtype == np.float32 and t.center_z.dtype == np.float64
                    sim_xyh[s, k, j] = np.stack([t.center_x, t.center_y, t.heading], -1)
                    if k == 0:
                        sim_z[s, j], id_sim[s, j] = t.center_z, t.object_id
                    assert np.array_equal(sim_z[s, j], t.center_z) and id_sim[s, j] == t.object_id
                for j, t in enumerate(trajs[n_sim[s]:]):
                    assert t is r.joint_scenes[0].simulated_trajectories[n_sim[s] + j], "one not-simulated list per scene, shared by its rollouts"
                    if k == 0:
                        assert t.center_x.dtype == t.center_y.dtype == t.center_z.dtype == np.float64 and t.heading.dtype == np.float32
                        ns_xyz[s, j], ns_h[s, j], id_ns[s, j] = np.stack([t.center_x, t.center_y, t.center_z], -1), t.heading, t.object_id
        print(f"{name}: n_sim {n_sim.tolist()}, n_no_sim {n_ns.tolist()}")
        out.update({f"{name}_n_sim": n_sim, f"{name}_n_no_sim": n_ns, f"{name}_id_sim": id_sim, f"{name}_id_no_sim": id_ns, f"{name}_sim_z": sim_z,
                    f"{name}_ns_xyz": ns_xyz, f"{name}_ns_heading": ns_h})
        if name == "flags_off":
            assert np.array_equal(sim_xyh, out["default_sim_xyh"]), "copies of the same inputs"
        else:
            out[f"{name}_sim_xyh"] = sim_xyh
    # the test's case properties hold for what was generated
    v = tb.synthetic.make_sub_case(step_current=STEP_CURRENT, **WOSAC_CASES["default"][0])
    for key in ("valid_sim", "valid_no_sim"):
        assert bool((v[key][:, :, STEP_CURRENT] & ~v[key][:, :, STEP_CURRENT - 1]).any()), "some objects valid at 10 but not at 9"
    assert out["default_n_no_sim"][1] == 0 and out["default_n_sim"][2] == 0
    assert bool(v["valid_no_sim"][0, 64:, STEP_CURRENT].any()), "kept objects on both sides of the wave boundary"
    assert np.abs(out["default_sim_z"][0, 0, 1] - out["default_sim_z"][0, 0, 0]) > 0


def gen_womd(out):
    from utils.submission import SubWOMD

    c = tb.synthetic.make_womd_sub_case(**WOMD_CASE)
    state = SimpleNamespace(trajs=[], scores=[], object_id=[], mask_pred=[], scenario_id=[])
    SubWOMD.update(state, c, c["trajs"].clone(), c["scores"].clone())
    trajs, scores = state.trajs[0].cpu().numpy(), state.scores[0].cpu().numpy()
    mask_pred, object_id = state.mask_pred[0].cpu().numpy(), state.object_id[0].cpu().numpy()
    n_sc, A = object_id.shape
    pos, sc = np.zeros(trajs.shape, np.float32), np.zeros(scores.shape, np.float32)
    oid, n = np.full((n_sc, A), -1, np.int64), np.zeros(n_sc, np.int32)
    for i_batch in range(n_sc):
        agent_pos = trajs[i_batch, mask_pred[i_batch]]  # utils/submission.py:94-96
        agent_id = object_id[i_batch, mask_pred[i_batch]]
        agent_score = scores[i_batch, mask_pred[i_batch]]
        n[i_batch] = agent_pos.shape[0]
        pos[i_batch, : n[i_batch]], oid[i_batch, : n[i_batch]], sc[i_batch, : n[i_batch]] = agent_pos, agent_id, agent_score
    assert "".join(chr(int(x)) for x in state.scenario_id[0][0] if x > 0) == c["scenario_id"][0]
    assert n[1] == 0 and n[2] == A and 0 < n[0] < A
    print(f"womd: n_pred {n.tolist()}, pos {pos.shape} {pos.dtype}")
    out.update({"womd_pos": pos, "womd_scores": sc, "womd_id": oid, "womd_n": n})


if __name__ == "__main__":
    install_shims()
    out = {}
    gen_wosac(out)
    gen_womd(out)
    out["cases"] = json.dumps({"wosac": {n: dict(case=c, step_gt=g, step_current=STEP_CURRENT, const_vel_z_sim=cz, const_vel_no_sim=cn)
                                         for n, (c, g, cz, cn) in WOSAC_CASES.items()}, "womd": WOMD_CASE})
    npz("sub_records.npz", **out)
