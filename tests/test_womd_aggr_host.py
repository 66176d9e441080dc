"""CPU-only checks of the trajectory aggregation of the WOMD post-processing: the float64 restatement (tests/womd_aggr_ref.py) against the
reference's outputs in tests/golden/womd_aggr.npz, the C ABI of libtbx_aggr.so (header, exports, the ctypes mirror's layout as gcc lays
out the header, every refusal before a launch), `WOMDPostProcessing`'s constructor, the wrapper's view checks and the seeded synthetic
helper. The kernel itself: tests/test_hip_womd_aggr.py."""
import ctypes as C
import json
import re
import subprocess
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

import womd_aggr_ref as R

ROOT = Path(__file__).resolve().parent.parent
ARG, UNSUPPORTED = -1, -2
ENTRY_POINTS = ["tbx_womd_aggr"]
CASES = ("ade32", "fde48", "k7", "k128", "iter0", "temp_type", "t91", "repair_ade", "repair_fde")
PTRS = ("pred_pose", "log_prob", "ag_type", "out_trajs", "out_scores", "out_idx")
BASE = dict(k_pred=6, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0], mtr_nms_thresh=[], aggr_thresh=[], n_iter_em=3, use_ade=True,
            step_gt=90, step_current=10)


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "womd_aggr.npz")


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[2] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("tbx_"))


def test_fixture_has_the_issues_cases(golden):
    spec = json.loads(str(golden["cases"]))
    assert tuple(spec) == CASES
    for name, s in spec.items():
        assert s["cfg"]["k_pred"] == 6 and len(s["cfg"]["aggr_thresh"]) == 3 and s["cfg"]["mtr_nms_thresh"] == [], name
        safe = R.safe_agents(golden[f"{name}_margin_d"], golden[f"{name}_margin_s"], golden[f"{name}_margin_c"])
        assert 1.0 - safe.mean() <= 0.05, name
    assert spec["k128"]["case"]["n_k"] == 128 and spec["t91"]["case"]["n_step"] == 91 and spec["k7"]["case"]["n_k"] == 7
    assert spec["iter0"]["cfg"]["n_iter_em"] == 0 and not spec["fde48"]["cfg"]["use_ade"] and not spec["repair_fde"]["cfg"]["use_ade"]
    assert float(golden["iter0_bound_trajs"]) == 0.0, "n_iter_em = 0 is a gather in every precision"


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(tb, golden, name):
    """The float64 restatement against the reference's FLOAT32 outputs, on the agents with safe margins, within the reference's own
    float32 - float64 difference; the decision margins it reports are the fixture's."""
    spec = json.loads(str(golden["cases"]))[name]
    c = getattr(tb.synthetic, spec["helper"])(**spec["case"])
    n_step = c["trajs"].shape[3]
    out = R.aggr_case(c["trajs"].double().numpy(), c["log_prob"].double().numpy(), c["ag_type"].numpy(), spec["cfg"], n_step)
    safe = R.safe_agents(golden[f"{name}_margin_d"], golden[f"{name}_margin_s"], golden[f"{name}_margin_c"])
    assert out["trajs"].shape == golden[f"{name}_trajs"].shape and out["trajs"].shape[3] == len(range(4, n_step, 5))
    dt = np.abs(out["trajs"] - golden[f"{name}_trajs"])[safe].max()
    ds = np.abs(out["scores"] - golden[f"{name}_scores"])[safe].max()
    print(f"{name}: restatement - float32 reference {dt:.3e} m (bound {float(golden[f'{name}_bound_trajs']):.3e}), scores {ds:.3e} "
          f"(bound {float(golden[f'{name}_bound_scores']):.3e}), repairs {int(out['n_repair'].sum())}")
    # |restatement - ref32| <= |restatement - ref64| + |ref64 - ref32|: the generator asserted the first below 1e-9 m / 1e-12 (numpy and
    # torch sum float64 in different orders), the second is the stored bound
    assert dt <= float(golden[f"{name}_bound_trajs"]) + 1e-9 and ds <= float(golden[f"{name}_bound_scores"]) + 1e-12
    assert np.array_equal(out["seeds"], golden[f"{name}_seeds"])
    for m in ("margin_d", "margin_s", "margin_c"):
        np.testing.assert_allclose(out[m], golden[f"{name}_{m}"], rtol=1e-9, atol=0)
    if name.startswith("repair"):
        assert (out["n_repair"] >= 1).all(), "the constructed case empties a cluster of every agent"
    np.testing.assert_allclose(out["scores"].sum(-1), 1.0, rtol=0, atol=1e-12)


def test_restatement_rules_on_a_hand_made_agent():
    """Six seeds 100 m apart, a seventh future next to seed 2: one round puts it there, the centre moves half way, the score is the mean;
    n_iter_em = 0 returns the picks."""
    T = 20
    tr = np.zeros((7, T, 3))
    tr[:, :, 0] = (np.arange(7) * 100.0)[:, None]
    tr[6, :, 0], tr[6, :, 1], tr[:, :, 2] = 200.0, 1.0, (0.1 * np.arange(7))[:, None]
    logp = np.log(np.array([7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0]))
    cfg = dict(k_pred=6, aggr_thresh=[0.5, 0.5, 0.5], n_iter_em=1, use_ade=True, mpa_nms_thresh=[], score_temperature=-1)
    out = R.aggr_agent(tr, logp, [True, False, False], cfg, T)
    assert out["seeds"].tolist() == [0, 1, 2, 3, 4, 5] and out["assign"].tolist() == [0, 1, 2, 3, 4, 5, 2] and out["n_repair"] == 0
    np.testing.assert_allclose(out["centres"][2, 0], [200.0, 0.5, 0.4])
    want = np.array([7.0, 6.0, (5.0 + 1.0) / 2, 4.0, 3.0, 2.0])
    np.testing.assert_allclose(out["scores"], want / want.sum())
    out0 = R.aggr_agent(tr, logp, [True, False, False], {**cfg, "n_iter_em": 0}, T)
    assert np.array_equal(out0["centres"], tr[:6]) and out0["assign"] is None
    assert R.type_thresh([False, False, False], [2.5, 1.0, 1.5]) == 0.0 and R.type_thresh([False, True, False], [2.5, 1.0, 1.5]) == 1.0


def test_entry_point_is_declared_exported_and_typed(hip):
    """libtbx_aggr.so exports exactly the one tbx_* function include/tbx_hip_aggr.h declares, bound with argtypes by hip.load_aggr();
    the other three libraries and include/tbx_hip.h - ABI 7's closed list - do not carry it."""
    lib = hip.load_aggr()
    assert lib.tbx_womd_aggr.argtypes == [C.POINTER(hip.WomdAggr), C.c_void_p] and lib.tbx_womd_aggr.restype is C.c_int
    assert _exported(hip.AGGR_LIB_PATH) == ENTRY_POINTS
    txt = (hip.HEADER_PATH.parent / "tbx_hip_aggr.h").read_text()
    assert sorted(re.findall(r"^(?:int|int64_t|const char\*)\s+(tbx_\w+)\s*\(", txt, flags=re.M)) == ENTRY_POINTS
    for other in (hip.LIB_PATH, hip.GRAD_LIB_PATH, hip.SUB_LIB_PATH):
        assert not set(ENTRY_POINTS) & set(_exported(other)), other
    assert not set(ENTRY_POINTS) & set(hip.declared_symbols()) and "tbx_hip_aggr.h" not in hip.HEADER_PATH.read_text()
    assert not re.fullmatch(r"libtbx_hip_\w+\.so", hip.AGGR_LIB_PATH.name)
    assert hip.load().tbx_version() == 7
    for name, v in (("MAX_K", hip.AGGR_MAX_K), ("MAX_KEEP", hip.AGGR_MAX_KEEP), ("MAX_T", hip.AGGR_MAX_T)):
        assert re.search(rf"^#define TBX_AGGR_{name} {v}\s", txt, flags=re.M), name
    assert callable(hip.womd_aggr)


def test_ctypes_mirror_has_the_layout_gcc_gives_the_header(hip, tmp_path):
    """tbx_hip_aggr.h included FIRST (it includes tbx_hip.h for the codes) compiles as C with -Wall -Werror; sizeof and every offsetof
    equal the ctypes class's."""
    st = hip.WomdAggr
    fields = [f[0] for f in st._fields_]
    assert fields[:6] == list(PTRS) and fields[-3:] == ["aggr_thresh", "mpa_nms_thresh", "score_temperature"] and len(fields) == 22
    src, exe = tmp_path / "aggr.c", tmp_path / "aggr"
    src.write_text('#include "tbx_hip_aggr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu\\n", sizeof(tbx_womd_aggr_t));'
                   + "".join(f'printf("%zu\\n", offsetof(tbx_womd_aggr_t, {f}));' for f in fields) + "return 0;}\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(st) == 128
    for f, off in zip(fields, out[1:]):
        assert getattr(st, f).offset == off, f


def _args(hip, **over):
    """A tbx_womd_aggr_t that passes every check, on stand-in pointers (never dereferenced: each call below is refused before a launch)."""
    a = hip.WomdAggr()
    for i, name in enumerate(PTRS):
        setattr(a, name, 0x10000 * (i + 1))
    a.n_scene, a.n_k, a.n_ag, a.ld_t, a.t_start, a.n_step, a.k_pred, a.use_ade, a.n_iter_em = 1, 32, 4, 90, 10, 80, 6, 1, 3
    a.sample_first, a.sample_stride, a.sample_end, a.has_mpa = 4, 5, 80, 1
    a.aggr_thresh, a.mpa_nms_thresh, a.score_temperature = (C.c_float * 3)(2.5, 1.0, 1.5), (C.c_float * 3)(2.0, 2.0, 2.0), -1.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over,code", [
    (dict(pred_pose=None), ARG), (dict(ag_type=None), ARG), (dict(out_trajs=None), ARG), (dict(out_scores=None), ARG),
    (dict(n_scene=0), ARG), (dict(n_k=0), ARG), (dict(n_ag=0), ARG), (dict(n_ag=-1), ARG), (dict(ld_t=0), ARG), (dict(n_step=0), ARG),
    (dict(k_pred=0), ARG), (dict(t_start=-1), ARG), (dict(t_start=11), ARG), (dict(n_iter_em=-1), ARG), (dict(sample_first=-1), ARG),
    (dict(sample_stride=0), ARG), (dict(sample_end=81), ARG), (dict(n_k=6), ARG), (dict(n_k=5), ARG), (dict(n_k=8, k_pred=8), ARG),
    (dict(n_k=129), UNSUPPORTED), (dict(n_k=16, k_pred=9), UNSUPPORTED), (dict(ld_t=120, n_step=92, sample_end=92), UNSUPPORTED),
    (dict(n_scene=1 << 16, n_ag=1 << 15), UNSUPPORTED),
])
def test_bad_arguments_are_refused_before_any_launch(hip, over, code):
    lib = hip.load_aggr()
    assert lib.tbx_womd_aggr(C.byref(_args(hip, **over)), None) == code
    assert hip.load().tbx_error_string(code)


def test_null_struct_is_refused(hip):
    assert hip.load_aggr().tbx_womd_aggr(None, None) == ARG


def test_constructor_accepts_the_per_type_list(tb):
    P = import_module("trafficbots_amd.data_modules.womd_post_processing")
    pp = P.WOMDPostProcessing(**{**BASE, "aggr_thresh": [2.5, 1.0, 1.5]})
    assert pp.aggr_thresh == [2.5, 1.0, 1.5] and pp.n_iter_em == 3 and pp.last_idx is None
    assert P.WOMDPostProcessing(**BASE).aggr_thresh == []
    assert P.WOMDPostProcessing(**{**BASE, "aggr_thresh": (2.5, 1.0, 1.5), "mtr_nms_thresh": [2.5, 1.0, 1.5], "n_iter_em": 0}).n_iter_em == 0
    for bad in ([1.0], [1.0, 2.0], [1.0, 2.0, 3.0, 4.0]):
        with pytest.raises(NotImplementedError, match=r"aggr_thresh.*\[veh, ped, cyc\]"):
            P.WOMDPostProcessing(**{**BASE, "aggr_thresh": bad})
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="n_iter_em"):
            P.WOMDPostProcessing(**{**BASE, "aggr_thresh": [2.5, 1.0, 1.5], "n_iter_em": bad})
        with pytest.raises(ValueError, match="n_iter_em"):  # ... and with the switch off as well (INTEGRATION.md states it)
            P.WOMDPostProcessing(**{**BASE, "n_iter_em": bad})
    assert tb.config.default_sim_cfg()["womd_post_processing"]["aggr_thresh"] == []


def test_wrapper_checks_the_view_and_takes_device_tensors_only(hip):
    pose, ty = torch.zeros(32, 4, 80, 3), torch.zeros(1, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="aggr_thresh"):
        hip.womd_aggr(pose, None, ty, 1, 32, 0, 80, 6, True, [1.0, 2.0], 3)
    with pytest.raises(ValueError, match="aggr_thresh"):
        hip.womd_aggr(pose, None, ty, 1, 32, 0, 80, 6, True, [], 3)
    with pytest.raises(ValueError, match="mpa_nms_thresh"):
        hip.womd_aggr(pose, None, ty, 1, 32, 0, 80, 6, True, [2.5, 1.0, 1.5], 3, mpa_nms_thresh=[2.0])
    with pytest.raises(RuntimeError, match="rollout log"):
        hip.womd_aggr(pose.transpose(1, 2), None, ty, 1, 32, 0, 4, 6, True, [2.5, 1.0, 1.5], 3)
    with pytest.raises(RuntimeError, match="rollout log"):
        hip.womd_aggr(pose, None, ty, 1, 32, 1, 80, 6, True, [2.5, 1.0, 1.5], 3)  # t_start + n_step past the view
    with pytest.raises(RuntimeError, match="device tensors"):  # and there is no CPU path
        hip.womd_aggr(pose, None, ty, 1, 32, 0, 80, 6, True, [2.5, 1.0, 1.5], 3)
    P = import_module("trafficbots_amd.data_modules.womd_post_processing")
    pp = P.WOMDPostProcessing(**{**BASE, "aggr_thresh": [2.5, 1.0, 1.5]})
    with pytest.raises(RuntimeError, match="device tensors"):
        pp(ty.bool(), pose.view(1, 32, 4, 80, 3))


def test_missing_library_is_an_import_error(hip, monkeypatch):
    abi = import_module("trafficbots_amd.abi")
    monkeypatch.setattr(abi, "_aggr_lib", None)
    monkeypatch.setattr(abi, "AGGR_LIB_PATH", ROOT / "no_such_dir" / "libtbx_aggr.so")
    with pytest.raises(ImportError, match="libtbx_aggr.so"):
        abi.load_aggr()


def test_repair_helper_is_seeded_and_old_helpers_are_unchanged(tb):
    S = tb.synthetic
    a, b, other = S.make_womd_repair_case(), S.make_womd_repair_case(n_ag=16, n_step=80, seed=0), S.make_womd_repair_case(seed=1)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["trajs"], other["trajs"])
    assert a["trajs"].shape == (1, 13, 16, 80, 3) and a["log_prob"].shape == (1, 13, 16) and a["ag_type"].shape == (1, 16, 3)
    assert a["ag_type"].dtype == torch.bool and (a["ag_type"].sum(-1) <= 1).all()
    assert a["ag_type"].any(-1)[0].tolist() == [i % 4 != 3 for i in range(16)], "every fourth agent without a type"
    top6 = a["log_prob"][0].argsort(0, descending=True)[:6]  # per agent: the futures that end at 0, 4, -40, 100, 200, 300 x scale
    ends = a["trajs"][0, :, :, -1, :2].norm(dim=-1).gather(0, top6)
    assert bool((ends[0] < 1.0).all()) and bool((ends[5] / ends[4] - 1.5).abs().max() < 0.01)
    small = S.make_womd_repair_case(n_ag=3, n_step=20, seed=2)
    assert small["trajs"].shape == (1, 13, 3, 20, 3)
    # make_womd_case draws what it drew before this helper existed (values taken from the parent commit; the log-probabilities are drawn
    # after the trajectories, so they pin the whole sequence of draws)
    c = S.make_womd_case(2, 8, 5, 80, seed=3)
    assert c["log_prob"][0, :4, 0].tolist() == [-3.9575142860412598, 0.7505622506141663, -1.044836163520813, -1.8824294805526733]
    assert c["ag_type"].int().flatten().tolist() == [1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0]
    assert abs(float(c["trajs"].double().sum()) - 242130.15863352377) < 1e-3 and abs(float(c["trajs"].abs().max()) - 118.59880828857422) < 1e-4
