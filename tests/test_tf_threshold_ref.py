"""CPU checks of error-threshold teacher forcing (TeacherForcing's threshold_xy / threshold_yaw / threshold_spd): the torch restatement
tests/tf_threshold_ref.py and `TeacherForcing.get` on CPU tensors against the reference's own results (tests/golden/tf_threshold.npz), the
C ABI of tbx_tf_threshold (header, argtypes, every refusal before a launch; the export list and the ctypes mirror's layout:
tests/test_abi_and_host.py) and the constructor that used to refuse the thresholds."""
import ctypes as C
import subprocess
import sys
from importlib import import_module
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tf_threshold_ref as TR  # noqa: E402


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def TF(tb):
    return import_module("trafficbots_amd.utils.teacher_forcing")


@pytest.fixture(scope="module")
def cases():
    return TR.load_cases()


def test_fixture_holds_the_cases_and_settings_the_issue_lists(cases):
    assert [(c[0], c[1]) for c in cases] == [(TR.case_name(*c), c[3]) for c in TR.CASES]
    assert TR.CASES == [(1, 1, 3, 1), (2, 5, 8, 4), (3, 65, 12, 11), (2, 64, 91, 90), (2, 5, 8, 8), (2, 5, 8, 9)]
    for (name, step, inp, want), (rows, A, Tg, _) in zip(cases, TR.CASES):
        assert inp["gt_valid"].shape == (rows, A, Tg) and want["tf_after"].shape == (len(TR.SETTINGS), rows, A, Tg)
        new = want["tf_after"] & ~inp["tf_init"]
        if A >= 5 and 0 < step < Tg:
            # each term alone resets someone; the edges: agent 0 is reset by 4.99 / 1.25 only; a reset onto invalid ground truth (agent 3)
            assert new[0].any() and new[2].any() and new[3].any()
            assert new[1][:, 0, step].all() and new[4][:, 0, step].all() and not new[0][:, 0].any() and not new[3][:, 0].any() and not new[5][:, 0].any()
            assert new[5][:, 3, step].all() and not inp["gt_valid"][:, 3, step].any()
            assert not new[:, :, :, :step].any() and not new[:, :, :, step + 1:].any()
        else:
            assert not new.any()


def test_restatement_equals_the_reference_exactly(cases):
    for name, step, inp, want in cases:
        for i, thr in enumerate(TR.SETTINGS):
            ov, table = TR.apply(thr, step, inp["tf_init"], inp["pred_valid"], inp["pred_pose"], inp["pred_motion"], inp["gt_valid"], inp["gt_pose"],
                                 inp["gt_motion"])
            assert torch.equal(table, want["tf_after"][i]), (name, thr)
            assert torch.equal(ov["valid"], want["ov_valid"][i]), (name, thr)
            assert torch.equal(ov["pose"], want["ov_pose"]) and torch.equal(ov["motion"], want["ov_motion"]), (name, thr)


def _tf(TF, inp, thr):
    """A TeacherForcing with the fixture's table (init's draw of scheduled sampling is the reference's: the table is put in its place)."""
    tf = TF.TeacherForcing(step_spawn_agent=10, step_warm_start=2, threshold_xy=thr[0], threshold_yaw=thr[1], threshold_spd=thr[2])
    tf.init(inp["gt_valid"].clone(), inp["gt_pose"].clone(), inp["gt_motion"].clone(), inp["tl_state"].clone(), 0)
    assert tf.ag_teacher_forcing.shape == inp["tf_init"].shape and tf.ag_teacher_forcing.dtype == torch.bool
    tf.ag_teacher_forcing.copy_(inp["tf_init"])
    return tf


def test_get_on_cpu_tensors_equals_the_reference_and_keeps_the_bits(cases, TF):
    for name, step, inp, want in cases:
        for i, thr in enumerate(TR.SETTINGS):
            tf = _tf(TF, inp, thr)
            assert tf.has_threshold and tf.thresholds == thr
            ag, tl = tf.get(step, inp["pred_valid"].clone(), inp["pred_pose"].clone(), inp["pred_motion"].clone())
            assert torch.equal(ag["valid"], want["ov_valid"][i]), (name, thr)
            assert torch.equal(ag["pose"], want["ov_pose"]) and torch.equal(ag["motion"], want["ov_motion"]), (name, thr)
            assert torch.equal(tf.ag_teacher_forcing, want["tf_after"][i]), (name, thr)  # the table itself holds the new bits
            Tt = inp["tl_state"].shape[2]
            assert tl["valid"].all() == (0 < step < Tt)


def test_constructor_accepts_thresholds_and_waymo_motion_builds_with_them(tb, TF):
    tf = TF.TeacherForcing(threshold_xy=2.0, threshold_yaw=15.0, threshold_spd=1.0)  # raised NotImplementedError before
    assert tf.has_threshold and tf.thresholds == (2.0, 15.0, 1.0)
    assert not TF.TeacherForcing().has_threshold and TF.TeacherForcing().thresholds == (-1.0, -1.0, -1.0)
    assert TF.TeacherForcing(threshold_spd=0.5).has_threshold and not TF.TeacherForcing(threshold_xy=0.0).has_threshold
    d = tb.config.default_sim_cfg()
    for k in ("teacher_forcing_training", "teacher_forcing_reactive_replay", "teacher_forcing_joint_future_pred"):
        assert all(d[k].get(t, -1) == -1 for t in ("threshold_xy", "threshold_yaw", "threshold_spd")), k  # config.py's defaults stay off
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg()
    scfg["teacher_forcing_reactive_replay"] = dict(scfg["teacher_forcing_reactive_replay"], threshold_xy=2.0)
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    assert wm.teacher_forcing_reactive_replay.has_threshold and not wm.teacher_forcing_training.has_threshold


def test_thresholds_off_leave_get_and_the_table_as_they_were(cases, TF):
    for name, step, inp, _ in cases:
        tf = _tf(TF, inp, (-1.0, -1.0, -1.0))
        assert not tf.has_threshold
        ag, _ = tf.get(step, inp["pred_valid"], inp["pred_pose"], inp["pred_motion"])
        assert torch.equal(tf.ag_teacher_forcing, inp["tf_init"]), name
        Tg = inp["tf_init"].shape[-1]
        if 0 < step < Tg:
            assert torch.equal(ag["valid"], inp["tf_init"][:, :, step]) and torch.equal(ag["pose"], inp["gt_pose"][:, :, step])
            assert torch.equal(ag["motion"], inp["gt_motion"][:, :, step])
        else:
            assert not ag["valid"].any() and not ag["pose"].any() and not ag["motion"].any()


def test_header_library_exports_and_argtypes_agree(hip):
    lib = hip.load()
    assert "tbx_tf_threshold" in hip.declared_symbols()
    assert lib.tbx_tf_threshold.argtypes == [C.POINTER(hip.TfThreshold), C.c_void_p] and lib.tbx_tf_threshold.restype is C.c_int
    assert '#include "tbx_hip_tf.h"' in hip.HEADER_PATH.read_text()
    assert lib.tbx_version() == 7


def test_the_header_alone_compiles(tmp_path):
    """tbx_hip_tf.h included first (it includes tbx_hip.h for the codes) compiles as C with -Wall -Werror. (sizeof / offsetof of
    tbx_tf_threshold_t against hip.TfThreshold: tests/test_abi_and_host.py.)"""
    root = Path(__file__).resolve().parent.parent
    alone = tmp_path / "alone.c"
    alone.write_text('#include "tbx_hip_tf.h"\nint main(void){return (int)sizeof(tbx_tf_threshold_t) == 0;}\n')
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(root / "include"), str(alone), "-o", str(tmp_path / "alone")], check=True)


def _stand_in(hip, **over):
    """A tbx_tf_threshold_t that passes every check, on stand-in pointers (never dereferenced: each call below is refused, or launches
    nothing: n_rows == 0, or a step_host outside (0, n_step_gt))."""
    a = hip.TfThreshold()
    for k in ("valid", "pose", "motion", "gt_valid", "gt_pose", "gt_motion", "tf_mask", "out_reset"):
        setattr(a, k, 0x1000)
    a.step_dev, a.step_host = None, 3
    a.n_rows, a.n_ag, a.n_step_gt = 0, 4, 8
    a.threshold_xy, a.threshold_yaw, a.threshold_spd = 2.0, -1.0, -1.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_every_refusal_returns_its_code_before_a_launch(hip):
    lib = hip.load()
    ARG, UNSUPPORTED = -1, -2  # TBX_ERR_ARG, TBX_ERR_UNSUPPORTED
    assert lib.tbx_tf_threshold(None, None) == ARG
    assert lib.tbx_tf_threshold(C.byref(_stand_in(hip)), None) == 0  # n_rows == 0: nothing to do, nothing launched
    for k in ("valid", "pose", "motion", "gt_valid", "gt_pose", "gt_motion", "tf_mask"):
        assert lib.tbx_tf_threshold(C.byref(_stand_in(hip, **{k: None})), None) == ARG, k
    for over in (dict(n_rows=-1), dict(n_ag=0), dict(n_ag=-3), dict(n_step_gt=0), dict(n_step_gt=-1),
                 dict(threshold_xy=-1.0), dict(threshold_xy=0.0)):  # no threshold on: a caller launches nothing then
        assert lib.tbx_tf_threshold(C.byref(_stand_in(hip, **over)), None) == ARG, over
    for over in (dict(out_reset=None), dict(threshold_xy=-1.0, threshold_yaw=10.0), dict(threshold_xy=-1.0, threshold_spd=1.0)):
        assert lib.tbx_tf_threshold(C.byref(_stand_in(hip, **over)), None) == 0, over
    # a host step outside (0, n_step_gt) is the empty override: no launch, whatever the row count
    for s in (0, 8, 9, -1):
        assert lib.tbx_tf_threshold(C.byref(_stand_in(hip, n_rows=2, step_host=s)), None) == 0, s
    assert lib.tbx_tf_threshold(C.byref(_stand_in(hip, n_rows=1 << 29, n_ag=4)), None) == UNSUPPORTED  # n_rows * n_ag == 2^31
    assert lib.tbx_tf_threshold(C.byref(_stand_in(hip, n_rows=(1 << 31) // 3 + 1, n_ag=3)), None) == UNSUPPORTED
    with pytest.raises(RuntimeError):  # host tensors: no CPU path through the wrapper
        z = torch.zeros
        hip.tf_threshold((2.0, -1.0, -1.0), 1, z(1, 2, dtype=torch.bool), z(1, 2, 3), z(1, 2, 3), z(1, 2, 4, dtype=torch.bool), z(1, 2, 4, 3),
                         z(1, 2, 4, 3), z(1, 2, 4, dtype=torch.bool))
