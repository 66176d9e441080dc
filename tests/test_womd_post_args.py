"""Argument validation of the post-processing entry points (tbx_womd_modes, tbx_pose_to_global) and of their modules' constructors:
everything here is rejected before a kernel would be launched, so no GPU is needed."""
import ctypes as C
from importlib import import_module

import pytest
import torch

ERR_ARG, ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib(tb):
    return import_module("trafficbots_amd.hip").load()


def _womd(lib, **over):
    """A call that would be valid if its pointers addressed device memory (they are never dereferenced: each case fails validation)."""
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    thr = (C.c_float * 3)(2.0, 2.0, 2.0)
    a = dict(pred_pose=p, log_prob=p, ag_type=p, n_scene=1, n_k=32, n_ag=4, ld_t=90, t_start=10, n_step=80, k_pred=6, use_ade=1,
             mtr=None, mpa=thr, temperature=-1.0, s_first=4, s_stride=5, s_end=80, out_trajs=p, out_scores=p, out_idx=p)
    a.update(over)
    return lib.tbx_womd_modes(*a.values(), None)


def test_new_symbols_are_declared_and_exported(tb, lib):
    hip = import_module("trafficbots_amd.hip")
    for s in ("tbx_womd_modes", "tbx_pose_to_global"):
        assert s in hip.declared_symbols() and hasattr(lib, s) and getattr(lib, s).argtypes is not None
    assert lib.tbx_version() == 7  # (the entry points here were added without a bump; 7 = the closed-loop step family)
    assert callable(hip.womd_modes) and callable(hip.pose_to_global)


@pytest.mark.parametrize("over,code", [
    (dict(pred_pose=None), ERR_ARG), (dict(ag_type=None), ERR_ARG), (dict(out_trajs=None), ERR_ARG), (dict(out_scores=None), ERR_ARG),
    (dict(n_scene=0), ERR_ARG), (dict(n_k=0), ERR_ARG), (dict(k_pred=0), ERR_ARG), (dict(t_start=11), ERR_ARG), (dict(s_stride=0), ERR_ARG),
    (dict(s_end=81), ERR_ARG),
    (dict(n_k=129), ERR_UNSUPPORTED), (dict(k_pred=9), ERR_UNSUPPORTED), (dict(ld_t=120, n_step=92, s_end=92), ERR_UNSUPPORTED),
])
def test_womd_modes_rejects_before_launch(lib, over, code):
    assert _womd(lib, **over) == code


def test_pose_to_global_rejects_before_launch(lib):
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(xy=p, ld_xy=3, yaw=p, ld_yaw=3, center=p, scen_yaw=p, n_scene=1, rows=4, n_t=8, ld_t=8, out_pos=p, out_yaw=p)
    for over in (dict(xy=None), dict(yaw=None), dict(center=None), dict(scen_yaw=None), dict(out_pos=None), dict(out_yaw=None),
                 dict(n_scene=0), dict(rows=0), dict(n_t=0), dict(ld_t=7), dict(ld_xy=1), dict(ld_yaw=0)):
        assert lib.tbx_pose_to_global(*{**ok, **over}.values(), None) == ERR_ARG, over


def test_module_constructor_refuses_what_the_kernel_does_not_do(tb):
    P = import_module("trafficbots_amd.data_modules.womd_post_processing")
    hip = import_module("trafficbots_amd.hip")
    base = dict(k_pred=6, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0], mtr_nms_thresh=[], aggr_thresh=[], n_iter_em=3, use_ade=True,
                step_gt=90, step_current=10)
    pp = P.WOMDPostProcessing(**base)
    assert pp.track_future_samples == 80 and pp.mpa_nms_thresh == [2.0, 2.0, 2.0]
    with pytest.raises(NotImplementedError, match="aggr_thresh"):
        P.WOMDPostProcessing(**{**base, "aggr_thresh": [1.0]})
    for bad in (dict(mpa_nms_thresh=[2.0]), dict(mtr_nms_thresh=[1.0, 2.0]), dict(mpa_nms_thresh=[1.0] * 4), dict(k_pred=9), dict(k_pred=0)):
        with pytest.raises(ValueError):
            P.WOMDPostProcessing(**{**base, **bad})
    # the wrapper refuses a threshold list of the wrong length before it touches a tensor's device pointer
    pose, ty = torch.zeros(32, 4, 80, 3), torch.zeros(1, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="mtr_nms_thresh"):
        hip.womd_modes(pose, None, ty, 1, 32, 0, 80, 6, True, mtr_nms_thresh=[1.0, 2.0])
    with pytest.raises(RuntimeError, match="rollout log"):
        hip.womd_modes(pose.transpose(1, 2), None, ty, 1, 32, 0, 4, 6, True)
    with pytest.raises(RuntimeError, match="device tensors"):  # and there is no CPU path
        hip.womd_modes(pose, None, ty, 1, 32, 0, 80, 6, True)


def test_waymo_motion_builds_the_post_processing_modules_from_its_config(tb):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg()
    assert dict(scfg["womd_post_processing"]) == dict(k_pred=6, use_ade=True, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0],
                                                      mtr_nms_thresh=[], aggr_thresh=[], n_iter_em=3)
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    assert wm.womd_post_processing.k_pred == 6 and wm.womd_post_processing.track_future_samples == 80
    assert wm.wosac_post_processing.use_wosac_col is True and wm.wosac_post_processing.w_road_edge == 0.0
    assert wm.hparams.womd_post_processing.mpa_nms_thresh == [2.0, 2.0, 2.0]
    with pytest.raises(NotImplementedError):
        wm.wosac_post_processing.get_scenario_rollouts({})
    for k in ("womd_post_processing", "wosac_post_processing"):  # a configuration without the sections: as before, no module
        scfg.pop(k)
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    assert not hasattr(wm, "womd_post_processing") and not hasattr(wm, "wosac_post_processing")


def test_synthetic_helpers_are_seeded_and_leave_the_old_ones_alone(tb):
    S = tb.synthetic
    a, b = S.make_womd_case(2, 8, 5, 80, seed=3), S.make_womd_case(2, 8, 5, 80, seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert a["trajs"].shape == (2, 8, 5, 80, 3) and a["log_prob"].shape == (2, 8, 5) and a["ag_type"].shape == (2, 5, 3)
    assert (a["ag_type"].sum(-1) <= 1).all()
    big = S.make_womd_case(4, 32, 64, 80, seed=1)["ag_type"]
    assert 0 < int((~big.any(-1)).sum()) < 0.2 * big[..., 0].numel(), "a few agents without a type"
    w = S.make_wosac_keys(2, 5, seed=0)
    assert w["scenario_center"].shape == (2, 2) and w["scenario_yaw"].shape == (2,) and len(w["scenario_id"]) == 2
    assert all(isinstance(s, str) and 0 < len(s) <= 16 for s in w["scenario_id"])
    assert w["history/agent_no_sim/pos"].shape == (2, 256, 11, 3) and w["history/agent_no_sim/yaw_bbox"].shape == (2, 256, 11, 1)
    assert w["history/agent_no_sim/valid"].shape == (2, 256, 11) and w["history/agent_no_sim/object_id"].shape == (2, 256)
    assert w["history/agent/object_id"].shape == (2, 5)
    assert float(w["history/agent_no_sim/yaw_bbox"].abs().max()) > 3.1416 - 0.3


def test_log_row_steps_accepts_time_slices_of_a_dense_log_only(tb, golden_dir):
    """What decides whether the kernels read a tensor in place: a [..., A, T, 3] float32 log, or a slice of it along time."""
    import json

    f = import_module("trafficbots_amd.hip").log_row_steps
    log = torch.zeros(2, 32, 8, 90, 3)
    assert f(log) == 90 and f(log[:, :, :, 10:]) == 90 and f(log[:, :, :, 10:].flatten(0, 1)) == 90 and f(log[:, :, :, 10:50]) == 90
    assert f(log[:1, :1, :, 10:]) == 90 and f(torch.zeros(1, 1, 8, 90, 3)[:, :, :, 10:]) == 90  # (size-1 dimensions: any stride)
    assert f(log[:, :, :1, 10:]) == 8 * 90, "one agent of eight: rows 8 x 90 steps apart"
    assert f(log[:, :, ::2]) == 2 * 90, "every other agent: the same addresses as rows of 180 steps"
    for bad in (log.transpose(1, 2), log[:, :, :, ::2], log[:, ::2], log[:, :1], log[..., :2], log.double()):
        assert f(bad) is None
    # the not-simulated agents' sizes of make_wosac_keys are the reference's (tests/golden/womd_tensor_sizes.json)
    sizes = json.loads((golden_dir / "womd_tensor_sizes.json").read_text())["64"]["tensor_size_test"]
    w = tb.synthetic.make_wosac_keys(1, 64, seed=1)
    for k in ("history/agent/object_id", "history/agent_no_sim/object_id", "history/agent_no_sim/valid", "history/agent_no_sim/pos",
              "history/agent_no_sim/yaw_bbox"):
        assert list(w[k].shape[1:]) == sizes[k], k
