"""CPU-only checks of the test loop's submission records: the C ABI of libtbx_sub.so (header, exports, the ctypes mirrors' layout as gcc
lays out the header, every refusal before a launch), `WOSACPostProcessing.get_joint_scenes`' step-count check, what stays
unimplemented (`save_sub_file`, `get_scenario_rollouts`), `WaymoMotion`'s new entry points with unchanged hparams, the host side of
`SubWOMD` / `SubWOSAC`, and the seeded synthetic helpers. The kernels themselves: tests/test_hip_sub_records.py."""
import ctypes as C
import re
import subprocess
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
ARG, UNSUPPORTED, ALIGN = -1, -2, -3
ENTRY_POINTS = ["tbx_womd_predictions", "tbx_wosac_joint_scenes"]


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[2] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("tbx_"))


def test_entry_points_are_declared_exported_and_typed(hip):
    """libtbx_sub.so exports exactly the two tbx_* functions include/tbx_hip_sub.h declares, bound with argtypes by hip.load_sub();
    libtbx_hip.so / libtbx_grad.so and include/tbx_hip.h - ABI 7's closed list - carry neither."""
    lib = hip.load_sub()
    assert lib.tbx_wosac_joint_scenes.argtypes == [C.POINTER(hip.JointScenes), C.c_void_p] and lib.tbx_wosac_joint_scenes.restype is C.c_int
    assert lib.tbx_womd_predictions.argtypes == [C.POINTER(hip.WomdPred), C.c_void_p] and lib.tbx_womd_predictions.restype is C.c_int
    assert _exported(hip.SUB_LIB_PATH) == ENTRY_POINTS
    txt = (hip.HEADER_PATH.parent / "tbx_hip_sub.h").read_text()
    assert sorted(re.findall(r"^(?:int|int64_t|const char\*)\s+(tbx_\w+)\s*\(", txt, flags=re.M)) == ENTRY_POINTS
    for other in (hip.LIB_PATH, hip.GRAD_LIB_PATH):
        assert not set(ENTRY_POINTS) & set(_exported(other)), other
    assert not set(ENTRY_POINTS) & set(hip.declared_symbols()) and "tbx_hip_sub.h" not in hip.HEADER_PATH.read_text()
    assert not re.fullmatch(r"libtbx_hip_\w+\.so", hip.SUB_LIB_PATH.name)
    assert hip.load().tbx_version() == 7
    assert f"#define TBX_SUB_MAX_OBJECTS {hip.SUB_MAX_OBJECTS} " in txt


@pytest.mark.parametrize("c_name,cls", [("tbx_joint_scenes_t", "JointScenes"), ("tbx_womd_pred_t", "WomdPred")])
def test_ctypes_mirrors_have_the_layout_gcc_gives_the_header(hip, tmp_path, c_name, cls):
    """tbx_hip_sub.h included FIRST (it includes tbx_hip.h for the codes) compiles as C with -Wall -Werror; sizeof and every offsetof
    equal the ctypes classes'."""
    st = getattr(hip, cls)
    fields = [f[0] for f in st._fields_]
    src, exe = tmp_path / "sub.c", tmp_path / "sub"
    src.write_text(f'#include "tbx_hip_sub.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){{printf("%zu\\n", sizeof({c_name}));'
                   + "".join(f'printf("%zu\\n", offsetof({c_name}, {f}));' for f in fields) + "return 0;}\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(st)
    for f, off in zip(fields, out[1:]):
        assert getattr(st, f).offset == off, f


JS_SIM = ("pos_sim", "yaw_sim", "valid_sim", "z_sim", "object_id_sim", "traj_sim", "id_sim")
JS_NO_SIM = ("pos_no_sim", "yaw_no_sim", "z_no_sim", "valid_no_sim", "object_id_no_sim", "traj_no_sim", "id_no_sim")
JS_PTRS = ("pos_sim", "yaw_sim", "valid_sim", "z_sim", "object_id_sim", "pos_no_sim", "yaw_no_sim", "z_no_sim", "valid_no_sim", "object_id_no_sim",
           "traj_sim", "traj_no_sim", "id_sim", "id_no_sim", "count")
WP_PTRS = ("trajs", "scores", "object_id", "mask_pred", "scenario_center", "scenario_yaw", "out_pos", "out_scores", "out_object_id", "out_count")


def _joint_scenes(hip, **over):
    """A tbx_joint_scenes_t that passes every check, on stand-in pointers (never dereferenced: each call below is refused before a launch)."""
    a = hip.JointScenes()
    for i, name in enumerate(JS_PTRS):
        setattr(a, name, 0x10000 * (i + 1))
    a.n_sc, a.n_k, a.n_ag, a.n_no_sim, a.n_step, a.n_hist, a.step_current, a.const_vel_z_sim, a.const_vel_no_sim = 2, 4, 8, 16, 20, 11, 10, 1, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _womd_pred(hip, **over):
    a = hip.WomdPred()
    for i, name in enumerate(WP_PTRS):
        setattr(a, name, 0x10000 * (i + 1))
    a.n_sc, a.n_ag, a.n_mode, a.n_sample = 2, 8, 6, 16
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_bad_arguments_are_refused_before_any_launch(hip):
    lib = hip.load_sub()
    js = lambda **over: lib.tbx_wosac_joint_scenes(C.byref(_joint_scenes(hip, **over)), None)
    assert lib.tbx_wosac_joint_scenes(None, None) == ARG
    for k in JS_PTRS:  # a NULL array with a non-zero extent
        assert js(**{k: None}) == ARG, k
    # ... and with a zero extent it is no reason: the call gets past the pointer checks to the next refusal (an unaligned output)
    assert js(n_ag=0, traj_no_sim=0x10004, **{k: None for k in JS_SIM}) == ALIGN
    assert js(n_no_sim=0, traj_sim=0x10004, **{k: None for k in JS_NO_SIM}) == ALIGN
    assert js(n_ag=0, count=None, **{k: None for k in JS_SIM}) == ARG  # count has n_sc * 2 elements whatever the object counts
    for over in (dict(step_current=0), dict(step_current=-1), dict(step_current=11), dict(step_current=12), dict(n_step=0), dict(n_step=-3),
                 dict(n_k=0), dict(n_k=-1), dict(n_sc=0), dict(n_ag=-1), dict(n_no_sim=-1)):
        assert js(**over) == ARG, over
    assert js(n_ag=hip.SUB_MAX_OBJECTS + 1) == UNSUPPORTED and js(n_no_sim=hip.SUB_MAX_OBJECTS + 1) == UNSUPPORTED
    assert js(traj_sim=0x10008) == ALIGN and js(traj_no_sim=0x10004) == ALIGN and js(pos_sim=0x10004) == ALIGN
    wp = lambda **over: lib.tbx_womd_predictions(C.byref(_womd_pred(hip, **over)), None)
    assert lib.tbx_womd_predictions(None, None) == ARG
    for k in WP_PTRS:
        assert wp(**{k: None}) == ARG, k
    for over in (dict(n_sc=0), dict(n_ag=0), dict(n_mode=0), dict(n_sample=0), dict(n_ag=-2)):
        assert wp(**over) == ARG, over
    assert wp(n_ag=hip.SUB_MAX_OBJECTS + 1) == UNSUPPORTED and wp(out_pos=0x10004) == ALIGN
    assert hip.load().tbx_error_string(ARG) and hip.load().tbx_error_string(UNSUPPORTED) and hip.load().tbx_error_string(ALIGN)


def test_wrappers_take_device_tensors_only(tb, hip):
    """CPU tensors: no fallback path (as hip.womd_modes)."""
    d = tb.synthetic.make_sub_case(n_sc=1, n_k=2, n_ag=4, n_no_sim=3, n_step=5)
    sq = lambda k: d[k].squeeze(-1).contiguous()
    with pytest.raises(RuntimeError):
        hip.wosac_joint_scenes(d["pos_sim"], sq("yaw_sim"), d["valid_sim"], sq("z_sim"), d["object_id_sim"], d["pos_no_sim"], sq("yaw_no_sim"),
                               sq("z_no_sim"), d["valid_no_sim"], d["object_id_no_sim"], 10, True, True)
    w = tb.synthetic.make_womd_sub_case(n_sc=1, n_ag=4)
    with pytest.raises(RuntimeError):
        hip.womd_predictions(w["trajs"], w["scores"], w["history/agent/object_id"], w["ref/ag_role"][..., 2].contiguous(), w["scenario_center"],
                             w["scenario_yaw"])
    with pytest.raises(TypeError):  # a tensor's dtype and shape are checked before its pointer is taken
        hip.womd_predictions(w["trajs"].double(), w["scores"], w["history/agent/object_id"], w["ref/ag_role"][..., 2].contiguous(),
                             w["scenario_center"], w["scenario_yaw"])


def test_what_raises(tb):
    PP = import_module("trafficbots_amd.data_modules.wosac_post_processing")
    SUB = import_module("trafficbots_amd.utils.submission")
    post = PP.WOSACPostProcessing(step_gt=30, step_current=10, const_vel_z_sim=True, const_vel_no_sim=True, w_road_edge=0.0, use_wosac_col=True)
    d = tb.synthetic.make_sub_case(n_sc=1, n_k=2, n_ag=4, n_no_sim=3, n_step=19)
    with pytest.raises(ValueError, match="19 future steps"):  # before any device call: these are CPU tensors
        post.get_joint_scenes(d)
    with pytest.raises(NotImplementedError, match="get_joint_scenes"):
        post.get_scenario_rollouts({})
    for cls in (SUB.SubWOMD, SUB.SubWOSAC):
        sub = cls(is_active=True, wb_artifact="a:v0", method_name="m", authors=["x", "y"], affiliation="f", description="d", method_link="l",
                  account_name="n")
        assert sub.is_active and sub.authors == ["x", "y"] and sub.compute() is None and sub.records() == []
        with pytest.raises(NotImplementedError, match="waymo_open_dataset"):
            sub.save_sub_file(None)
        assert not cls(is_active=False).is_active


def test_aggregate_on_cpu_keeps_a_scene_once(tb):
    """The host side alone, on CPU tensors standing in for the device records: trimmed to the counts, the second sight of an id dropped."""
    SUB = import_module("trafficbots_amd.utils.submission")
    codes = SUB.scenario_id_codes(["abc123", "0123456789abcdef"], "cpu")
    assert codes.shape == (2, 16) and codes.dtype == torch.int32 and SUB.scenario_id_strings(codes.numpy()) == ["abc123", "0123456789abcdef"]
    sub = SUB.SubWOMD(is_active=True)
    rec = {"trajs": torch.arange(2 * 3 * 2 * 4 * 2, dtype=torch.float32).view(2, 3, 2, 4, 2), "scores": torch.ones(2, 3, 2),
           "object_id": torch.tensor([[7, 9, -1], [-1, -1, -1]]), "n_pred": torch.tensor([2, 0], dtype=torch.int32), "scenario_id": codes}
    sub._append(rec)
    sub._append(rec)
    both = sub.compute()
    assert both["trajs"].shape == (4, 3, 2, 4, 2)
    sub.aggregate_on_cpu(both)
    sub.reset()
    assert sub.compute() is None
    got = sub.records()
    assert [r["scenario_id"] for r in got] == ["abc123", "0123456789abcdef"] == sub.submission_scenario_id
    assert got[0]["object_id"].tolist() == [7, 9] and got[0]["trajs"].shape == (2, 2, 4, 2) and got[1]["trajs"].shape == (0, 2, 4, 2)
    assert np.array_equal(got[0]["trajs"], rec["trajs"][0, :2].numpy())
    wos = SUB.SubWOSAC(is_active=True)
    rec = {"scenario_id": codes, "traj_sim": torch.rand(2, 3, 4, 5, 4), "traj_no_sim": torch.rand(2, 6, 5, 4), "object_id_sim": torch.arange(8).view(2, 4),
           "object_id_no_sim": torch.arange(12).view(2, 6), "n_sim": torch.tensor([4, 1], dtype=torch.int32), "n_no_sim": torch.tensor([0, 6], dtype=torch.int32)}
    wos._append(rec)
    wos.aggregate_on_cpu(wos.compute())
    wos.aggregate_on_cpu(wos.compute())
    got = wos.records()
    assert len(got) == 2 and got[0]["traj_sim"].shape == (3, 4, 5, 4) and got[0]["traj_no_sim"].shape == (0, 5, 4)
    assert got[1]["traj_sim"].shape == (3, 1, 5, 4) and got[1]["object_id_no_sim"].tolist() == list(range(6, 12))


def test_waymo_motion_has_the_test_loop_and_the_hparams_it_had(tb):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    SUB = import_module("trafficbots_amd.utils.submission")
    import inspect

    assert list(inspect.signature(W.WaymoMotion.test_step).parameters) == ["self", "batch", "batch_idx"]
    assert list(inspect.signature(W.WaymoMotion.test_epoch_end).parameters) == ["self", "outputs"]
    scfg = tb.config.default_sim_cfg()
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    assert set(wm.hparams) == set(scfg) | {"model", "data_size"}  # nothing added by the submission sections' stand-ins
    assert isinstance(wm.sub_wosac, SUB.SubWOSAC) and isinstance(wm.sub_womd_joint_future_pred, SUB.SubWOMD)
    assert not wm.sub_wosac.is_active and not wm.sub_womd_joint_future_pred.is_active  # a missing section means inactive
    assert wm.last_joint_scenes is None
    sec = dict(_target_="utils.submission.SubWOSAC", is_active=True, wb_artifact="a:v0", method_name="m", authors=["x"], affiliation="f",
               description="d", method_link="l", account_name="n")
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, sub_wosac=sec,
                       sub_womd_joint_future_pred=dict(sec, is_active=False), **scfg)
    assert wm.sub_wosac.is_active and wm.sub_wosac.method_name == "m" and not wm.sub_womd_joint_future_pred.is_active
    assert set(wm.hparams) == set(scfg) | {"model", "data_size", "sub_wosac", "sub_womd_joint_future_pred"}  # (as every unnamed argument)
    assert not any("sub_" in k for k in wm.state_dict())


def test_synthetic_helpers_are_seeded(tb):
    S = tb.synthetic
    for make, kw in ((S.make_sub_case, dict(n_sc=3, n_k=2, n_ag=5, n_no_sim=7, n_step=4)), (S.make_womd_sub_case, dict(n_sc=3, n_ag=5))):
        a, b, c = make(seed=3, **kw), make(seed=3, **kw), make(seed=4, **kw)
        assert list(a) == list(b)
        assert all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)
        assert any(not torch.equal(a[k], c[k]) for k in a if torch.is_tensor(a[k]) and a[k].is_floating_point())
    d = S.make_sub_case()
    assert list(d) == ["scenario_id", "valid_sim", "pos_sim", "z_sim", "yaw_sim", "valid_no_sim", "object_id_sim", "pos_no_sim", "z_no_sim",
                       "yaw_no_sim", "object_id_no_sim"]  # the reference's wosac_data keys, in its order
    assert d["pos_sim"].shape == (3, 32, 12, 20, 2) and d["z_no_sim"].shape == (3, 70, 11, 1) and d["valid_sim"].dtype == torch.bool
    assert not d["valid_no_sim"][1, :, 10].any() and not d["valid_sim"][2, :, 10].any()
    assert float(d["pos_sim"].abs().max()) > 1e3
    w = S.make_womd_sub_case()
    assert not w["ref/ag_role"][1, :, 2].any() and w["ref/ag_role"][2, :, 2].all() and len(w["scenario_id"]) == 3
