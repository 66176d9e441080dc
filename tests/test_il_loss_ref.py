"""CPU-only checks of the configurable imitation terms of the differentiable reward (criteria MSE / L1 / Huber beside SmoothL1, angular
types null / cast / vector beside cosine): the float64 restatement (tests/il_loss_ref.py) against the reference's float64 outputs in
tests/golden/il_loss.npz, the constructors of `DifferentiableReward`, `AngularError` and `WaymoMotion`, the torch expressions the CPU /
autograd paths use, and the C ABI of libtbx_il.so (header, exports, the ctypes mirror's layout as gcc lays out the header, every refusal
before a launch). The kernels themselves: tests/test_hip_il_loss.py."""
import ctypes as C
import re
import subprocess
import sys
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import il_loss_ref as IL  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
ARG, UNSUPPORTED = -1, -2
ENTRY_POINTS = ["tbx_il_reward_bwd", "tbx_il_reward_fwd", "tbx_train_chain_bwd_state"]
PTRS = ("pred_valid", "pred_pose", "pred_motion", "gt_valid", "gt_pose", "gt_motion", "out_pos", "out_rot", "out_spd", "out_sum", "g",
        "d_pred_pose", "d_pred_spd")


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "il_loss.npz")


def _golden_case(golden):
    case = {k: torch.from_numpy(golden[k]) for k in ("pred_valid", "pred_pose", "pred_motion", "gt_valid", "gt_pose", "gt_motion", "planted")}
    case.update(n_k=IL.GOLDEN_CASE["n_k"], gt_offset=IL.GOLDEN_CASE["gt_offset"])
    return case


def test_fixture_has_the_issues_configurations_and_inputs(golden):
    assert len(IL.CONFIGS) == 14 and all(f"{name}/r4" in golden.files for name in IL.CONFIGS)
    for c in IL.CRITERIA:
        assert IL.CONFIGS[f"{c}_cosine"] == (c, "SmoothL1Loss", c, "cosine")
    assert {(cfg[1], cfg[3]) for n, cfg in IL.CONFIGS.items() if n.startswith("rot_")} == {(c, a) for c in ("SmoothL1Loss", "MSELoss", "L1Loss")
                                                                                            for a in (None, "cast", "vector")}
    assert IL.CONFIGS["mixed"] == ("MSELoss", "SmoothL1Loss", "L1Loss", "cast")
    case, made = _golden_case(golden), IL.make_case(**IL.GOLDEN_CASE)
    for k, v in case.items():
        if torch.is_tensor(v):
            assert torch.equal(v, made[k]), k  # the seeded inputs are the stored ones
    d = case["gt_pose"][:, :, 0] - case["pred_pose"][:, 0]
    live = case["pred_valid"][:, 0] & case["gt_valid"][:, :, 0]
    assert bool(((d[..., 0].abs() < 1) & live).any()) and bool(((d[..., 0].abs() > 1) & (d[..., 0].abs() < 2) & live).any())  # the SmoothL1 kink
    assert bool(((d == 0) & live.unsqueeze(-1)).any(0).any(0).all()) and bool(case["planted"].any())  # exact zeros in x, y and yaw
    assert float(d[..., :2].abs().max()) > 90  # MSE's range
    assert float(d[..., 2].min()) < -1.8 * np.pi and float(d[..., 2].max()) > 1.8 * np.pi  # wrapped and unwrapped angles
    assert not bool(case["pred_valid"].all()) and not bool(case["gt_valid"].all())
    for name, cfg in IL.CONFIGS.items():
        assert float(IL.excluded(case, cfg).double().mean()) <= IL.MAX_EXCLUDED, name
        assert 0 < float(golden[f"{name}/bound_r"]) < 1e-5 and 0 < float(golden[f"{name}/bound_g"]) < 1e-5, name


@pytest.mark.parametrize("name", list(IL.CONFIGS))
def test_restatement_equals_the_reference_in_float64(golden, name):
    cfg, case = IL.CONFIGS[name], _golden_case(golden)
    w = IL.upstream_weight(*case["pred_valid"].shape)
    got = IL.reward(case, cfg, tuple(golden["weights"]), upstream=w)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    close(got["r4"][:, 0], torch.from_numpy(golden[f"{name}/r4"]))
    assert torch.equal(got["valid"][:, 0], torch.from_numpy(golden[f"{name}/valid"]))
    keep = ~IL.excluded(case, cfg)[:, 0]
    close(got["d_pose"][:, 0][keep], torch.from_numpy(golden[f"{name}/d_pose"])[keep])
    close(got["d_spd"][:, 0][keep], torch.from_numpy(golden[f"{name}/d_spd"])[keep])
    # the planted exact zeros give gradient exactly 0 (L1: sign(0) = 0)
    live = got["valid"][:, 0].unsqueeze(-1) & case["planted"][:, 0]
    grads = torch.cat([got["d_pose"][:, 0], got["d_spd"][:, 0].unsqueeze(-1)], -1)
    assert bool(live.any(0).any(0).all()) and not bool(grads[live].any())


@pytest.mark.parametrize("name", list(IL.CONFIGS))
def test_torch_expressions_equal_the_reference_in_float64(tb, golden, name):
    """`AngularError.compute` on CPU tensors and `DifferentiableReward.torch_errors` - what the torch state machine of the training step
    differentiates - against the reference's float64 outputs."""
    L = import_module("trafficbots_amd.models.metrics.loss")
    R = import_module("trafficbots_amd.utils.rewards")
    cfg, case = IL.CONFIGS[name], _golden_case(golden)
    gw, pw = case["gt_pose"][:, :, 0, 2].double(), case["pred_pose"][:, 0, :, 2].double()
    torch.testing.assert_close(L.AngularError(cfg[1], cfg[3]).compute(gw, pw), torch.from_numpy(golden[f"{name}/ang"]), rtol=1e-12, atol=1e-12)
    dr = R.DifferentiableReward(**IL.reward_cfg(cfg, tuple(golden["weights"])), w_collision=0, use_il_loss=True, reduce_collsion_with_max=True)
    e = dr.torch_errors(case["gt_pose"][:, :, 0].double(), case["gt_motion"][:, :, 0].double(), case["pred_pose"][:, 0].double(), case["pred_motion"][:, 0].double())
    valid = torch.from_numpy(golden[f"{name}/valid"])
    for i, w in enumerate(dr.il_weights):
        torch.testing.assert_close((-w * e[i]).masked_fill(~valid, 0.0), torch.from_numpy(golden[f"{name}/r4"])[..., i], rtol=1e-12, atol=1e-12)


def test_huber_at_delta_1_is_smooth_l1_at_beta_1():
    d = torch.cat([torch.linspace(-3, 3, 601, dtype=torch.float64), torch.tensor([0.0, 1.0, -1.0], dtype=torch.float64)]).requires_grad_(True)
    z = torch.zeros_like(d)
    a, b = torch.nn.HuberLoss(reduction="none")(d, z), torch.nn.SmoothL1Loss(reduction="none")(d, z)
    ga, gb = torch.autograd.grad(a.sum(), d)[0], torch.autograd.grad(b.sum(), d)[0]
    assert torch.equal(a, b) and torch.equal(ga, gb)
    s = torch.zeros(3, dtype=torch.float64, requires_grad=True)  # torch's L1 gradient at 0 is 0
    assert not bool(torch.autograd.grad(torch.nn.L1Loss(reduction="none")(s, torch.zeros(3, dtype=torch.float64)).sum(), s)[0].any())


# ------------------------------------------------------------------------------------------------------------------ constructors
def _sim_cfg(tb, cfg=None, **dr_over):
    scfg = tb.config.default_sim_cfg()
    if cfg is not None:
        scfg["differentiable_reward"].update(IL.reward_cfg(cfg))
    scfg["differentiable_reward"].update(dr_over)
    return scfg


@pytest.mark.parametrize("name", list(IL.CONFIGS) + list(IL.TRAIN_CONFIGS))
def test_constructors_accept_every_configuration(tb, hip, name):
    L = import_module("trafficbots_amd.models.metrics.loss")
    R = import_module("trafficbots_amd.utils.rewards")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    cfg = {**IL.CONFIGS, **IL.TRAIN_CONFIGS}[name]
    ang = L.AngularError(cfg[1], cfg[3])
    assert ang.angular_type == cfg[3] and ang.angular_code == hip.IL_ANGULAR[cfg[3]]
    dr = R.DifferentiableReward(**IL.reward_cfg(cfg), w_collision=0, use_il_loss=True, reduce_collsion_with_max=True)
    assert dr.il_codes == (hip.IL_CRITERIA[cfg[0]], hip.IL_CRITERIA[cfg[1]], hip.IL_CRITERIA[cfg[2]], hip.IL_ANGULAR[cfg[3]])
    default = cfg[0] == cfg[2] == "SmoothL1Loss" and cfg[3] == "cosine"
    assert dr.il_default == default and (dr.il_config is None) == default
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **_sim_cfg(tb, cfg))
    assert wm.diffbar_reward.il_codes == dr.il_codes and wm.diffbar_reward.il_weights == IL.WEIGHTS


def test_constructors_refuse_what_is_not_implemented(tb):
    L = import_module("trafficbots_amd.models.metrics.loss")
    R = import_module("trafficbots_amd.utils.rewards")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    mk = lambda **kw: W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **kw)
    sl1 = ("SmoothL1Loss",) * 3
    for cfg in (("CrossEntropyLoss", "SmoothL1Loss", "SmoothL1Loss", "cosine"), ("SmoothL1Loss", "SmoothL1Loss", "CrossEntropyLoss", "cosine"),
                ("SmoothL1Loss", "CrossEntropyLoss", "SmoothL1Loss", "cast"), sl1 + ("foo",)):
        with pytest.raises(NotImplementedError, match="accepted: ") as e:
            R.DifferentiableReward(**IL.reward_cfg(cfg), w_collision=0, use_il_loss=True, reduce_collsion_with_max=True)
        if cfg[3] != "foo":
            assert all(c in str(e.value) for c in IL.CRITERIA)
        with pytest.raises(NotImplementedError):
            mk(**_sim_cfg(tb, cfg))
    with pytest.raises(NotImplementedError):
        L.AngularError("SmoothL1Loss", "foo")
    with pytest.raises(NotImplementedError):
        L.AngularError("CrossEntropyLoss", None)
    # with the cosine heading the rotation criterion is not looked up, as in the reference
    dr = R.DifferentiableReward(**IL.reward_cfg(("SmoothL1Loss", "CrossEntropyLoss", "SmoothL1Loss", "cosine")), w_collision=0, use_il_loss=True,
                                reduce_collsion_with_max=True)
    assert dr.il_default and dr.il_config is None
    assert L.AngularError("CrossEntropyLoss", "cosine").angular_type == "cosine"
    # out of scope, still refused
    with pytest.raises(NotImplementedError):
        mk(**_sim_cfg(tb, use_il_loss=False))
    with pytest.raises(NotImplementedError):
        mk(**_sim_cfg(tb, is_enabled=False))


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[2] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("tbx_"))


def test_entry_points_are_declared_exported_and_typed(hip):
    """libtbx_il.so exports exactly the three tbx_* functions include/tbx_hip_il.h declares, bound with argtypes by hip.load_il(); the
    other libraries and include/tbx_hip.h - ABI 7's closed list - do not carry them."""
    lib = hip.load_il()
    assert lib.tbx_il_reward_fwd.argtypes == lib.tbx_il_reward_bwd.argtypes == [C.POINTER(hip.IlReward), C.c_void_p]
    assert len(lib.tbx_train_chain_bwd_state.argtypes) == 9 and lib.tbx_train_chain_bwd_state.argtypes[0] == C.POINTER(hip.TrainChainArgs)
    assert all(getattr(lib, s).restype is C.c_int for s in ENTRY_POINTS)
    assert _exported(hip.IL_LIB_PATH) == ENTRY_POINTS == sorted(hip.IL_SYMBOLS)
    txt = (hip.HEADER_PATH.parent / "tbx_hip_il.h").read_text()
    assert sorted(re.findall(r"^(?:int|int64_t|const char\*)\s+(tbx_\w+)\s*\(", txt, flags=re.M)) == ENTRY_POINTS
    for other in (hip.LIB_PATH, hip.GRAD_LIB_PATH, hip.SUB_LIB_PATH, hip.AGGR_LIB_PATH):
        assert not set(ENTRY_POINTS) & set(_exported(other)), other
    main = hip.HEADER_PATH.read_text()
    assert not set(ENTRY_POINTS) & set(hip.declared_symbols()) and "tbx_hip_il.h" not in main and not any(s in main for s in ENTRY_POINTS)
    assert hip.load().tbx_version() == 7
    for name, v in list(hip.IL_CRITERIA.items()) + list(hip.IL_ANGULAR.items()):
        macro = {"SmoothL1Loss": "SMOOTH_L1", "MSELoss": "MSE", "L1Loss": "L1", "HuberLoss": "HUBER", "cosine": "ANG_COSINE", None: "ANG_NONE",
                 "cast": "ANG_CAST", "vector": "ANG_VECTOR"}[name]
        assert re.search(rf"^#define TBX_IL_{macro} {v}\s", txt, flags=re.M), name
    assert hip.IL_CRITERIA["SmoothL1Loss"] == hip.IL_ANGULAR["cosine"] == 0  # an all-zero tbx_il_reward_t is the default loss


def test_ctypes_mirror_has_the_layout_gcc_gives_the_header(hip, tmp_path):
    """tbx_hip_il.h included FIRST (it includes tbx_hip.h for the codes and tbx_train_chain_t) compiles as C with -Wall -Werror; sizeof
    and every offsetof equal the ctypes class's."""
    st = hip.IlReward
    fields = [f[0] for f in st._fields_]
    assert fields[:13] == list(PTRS) and fields[-3:] == ["w_pos", "w_rot", "w_spd"] and len(fields) == 31
    src, exe = tmp_path / "il.c", tmp_path / "il"
    src.write_text('#include "tbx_hip_il.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu\\n", sizeof(tbx_il_reward_t));'
                   + "".join(f'printf("%zu\\n", offsetof(tbx_il_reward_t, {f}));' for f in fields) + "return 0;}\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(st) == 280
    for f, off in zip(fields, out[1:]):
        assert getattr(st, f).offset == off, f


def _args(hip, **over):
    """A tbx_il_reward_t that passes every check of both entry points, on stand-in pointers (never dereferenced: each call below is
    refused before a launch)."""
    a = hip.IlReward()
    for i, name in enumerate(PTRS):
        setattr(a, name, 0x10000 * (i + 1))
    a.rows, a.n_k, a.n_ag, a.n_step, a.n_step_gt, a.gt_offset = 4, 2, 8, 5, 6, 1
    for name in ("valid_stride", "pose_stride", "motion_stride", "out_stride", "g_stride"):
        setattr(a, name, (C.c_int64 * 3)(40, 8, 1))
    a.w_pos, a.w_rot, a.w_spd = IL.WEIGHTS
    for k, v in over.items():
        setattr(a, k, v)
    return a


_NEG = lambda: (C.c_int64 * 3)(40, -8, 1)
BOTH = [(dict(pred_valid=None), ARG), (dict(pred_pose=None), ARG), (dict(pred_motion=None), ARG), (dict(gt_valid=None), ARG),
        (dict(gt_pose=None), ARG), (dict(gt_motion=None), ARG), (dict(rows=0), ARG), (dict(rows=-2), ARG), (dict(n_k=0), ARG), (dict(n_ag=0), ARG),
        (dict(n_step=0), ARG), (dict(n_step_gt=0), ARG), (dict(gt_offset=-1), ARG), (dict(n_k=3), ARG), (dict(rows=5), ARG),
        (dict(pose_stride=_NEG()), ARG), (dict(valid_stride=_NEG()), ARG), (dict(motion_stride=_NEG()), ARG),
        (dict(crit_pos=4), UNSUPPORTED), (dict(crit_rot=-1), UNSUPPORTED), (dict(crit_spd=7), UNSUPPORTED), (dict(angular=4), UNSUPPORTED),
        (dict(angular=-1), UNSUPPORTED)]
FWD = [(dict(out_sum=None), ARG), (dict(out_pos=None), ARG), (dict(out_rot=None, out_spd=None), ARG), (dict(out_stride=_NEG()), ARG)]
BWD = [(dict(g=None), ARG), (dict(d_pred_pose=None), ARG), (dict(d_pred_spd=None), ARG), (dict(g_stride=_NEG()), ARG)]


@pytest.mark.parametrize("fn,over,code", [("tbx_il_reward_fwd", o, c) for o, c in BOTH + FWD] + [("tbx_il_reward_bwd", o, c) for o, c in BOTH + BWD],
                         ids=lambda v: v if isinstance(v, str) else (",".join(v) if isinstance(v, dict) else str(v)))
def test_bad_arguments_are_refused_before_any_launch(hip, fn, over, code):
    lib = hip.load_il()
    assert getattr(lib, fn)(C.byref(_args(hip, **over)), None) == code
    assert hip.load().tbx_error_string(code)


def test_null_structs_are_refused(hip):
    lib = hip.load_il()
    assert lib.tbx_il_reward_fwd(None, None) == ARG and lib.tbx_il_reward_bwd(None, None) == ARG
    assert lib.tbx_train_chain_bwd_state(None, 0x1000, 8, 2, 0x2000, None, None, 0x3000, None) == ARG
    c = hip.TrainChainArgs()  # all-zero: non-positive sizes, NULL pointers
    assert lib.tbx_train_chain_bwd_state(C.byref(c), 0x1000, 8, 2, 0x2000, None, None, 0x3000, None) == ARG


def test_wrappers_need_device_tensors(tb, hip):
    """The rollout / training paths are HIP kernels: the one-step call on CPU tensors is an error, not a fall-back."""
    R = import_module("trafficbots_amd.utils.rewards")
    dr = R.DifferentiableReward(**IL.reward_cfg(IL.CONFIGS["mixed"]), w_collision=0, use_il_loss=True, reduce_collsion_with_max=True)
    case = IL.make_case(**IL.GOLDEN_CASE)
    with pytest.raises(RuntimeError, match="device tensors"):
        dr.get(case["pred_valid"][:, 0], case["pred_pose"][:, 0], case["pred_motion"][:, 0], case["gt_valid"][:, :, 0], case["gt_pose"][:, :, 0],
               case["gt_motion"][:, :, 0])
