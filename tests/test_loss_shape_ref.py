"""CPU checks of the training objective's loss shaping (temporal_discount, p_loss_for_irrelevant, w_relevant_agent): the float64
restatement tests/loss_shape_ref.py against the reference's own numbers (tests/golden/loss_shape.npz), the C ABI of tbx_loss_shape
(header, argtypes, every refusal before a launch; the export list and the ctypes mirror's layout: tests/test_abi_and_host.py) and the
constructors that used to refuse the switches."""
import ctypes as C
import inspect
import subprocess
import sys
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import loss_shape_ref as LR  # noqa: E402

CASES = ("r3_a5_t12", "r2_a64_t91", "r2_a65_t30", "r1_a1_t1", "r4_a33_t90", "r2_a1_t40")


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(golden_dir / "loss_shape.npz")


def case_settings(g, name):
    """[(index, dict of SETTING_FIELDS)] of a case."""
    return [(i, dict(zip(LR.SETTING_FIELDS, (float(row[0]), float(row[1]), bool(row[2]), int(row[3]), float(row[4])))))
            for i, row in enumerate(g[f"{name}/settings"])]


def restate(g, name, i, s):
    """loss_shape_ref.shape on a case's inputs under setting i."""
    return LR.shape(g[f"{name}/pred_valid"], g[f"{name}/tf"], g[f"{name}/ag_role"].any(-1), g[f"{name}/pick"][i], reward=g[f"{name}/reward"],
                    reward_valid=g[f"{name}/reward_valid"], **{k: s[k] for k in LR.SETTING_FIELDS})


def test_fixture_holds_the_cases_and_the_cross_the_issue_lists(fixture):
    for name in CASES:
        rows, A, T = (int(x[1:]) for x in name.split("_"))
        assert fixture[f"{name}/pred_valid"].shape == (rows, A, T)
        got = {tuple(r) for r in fixture[f"{name}/settings"].tolist()}
        want = {(d, p, float(tfl), float(start), w) for d in (-1.0, 0.9) for p in (1.0, 0.5, 0.0) for tfl in (True, False) for start in (0, 10, T + 1)
                for w in ((0.0, 2.0) if A == 1 else (0.0,))}
        assert got == want, name


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(fixture, name):
    """m bit-equal to the reference's float32 chain; the reward / KL / navigation sums within 1e-6 * sum |summand| (a summand's two float32
    roundings are at most 2^-23 relative each), the counters exact; the keys compute() leaves out are the zero counters'."""
    g = fixture
    m = LR.discount_chain(g[f"{name}/tf"], 0.9)
    assert m.dtype == np.float32 and np.array_equal(m.view(np.uint32), g[f"{name}/m"].view(np.uint32))
    worst = 0.0
    for i, s in case_settings(g, name):
        sh = restate(g, name, i, s)
        assert np.array_equal(sh["m"], m if s["temporal_discount"] > 0 else np.ones_like(m))
        sums = dict(zip(LR.SUM_KEYS, g[f"{name}/sums"][i]))
        out = dict(zip(LR.OUT_KEYS, g[f"{name}/out"][i]))
        weighted = s["w_relevant_agent"] > 0
        kl = LR.agent_term(g[f"{name}/kl_err"], g[f"{name}/post_valid"], sh, weighted)
        navi = LR.agent_term(g[f"{name}/navi_nll"], g[f"{name}/navi_valid"], sh, weighted)
        for key, (total, abs_total, count) in (("diffbar_reward", (sh["total"], sh["abs_total"], sh["count"])), ("vae_kl", kl), ("navi_loss", navi)):
            counter = key.replace("_loss", "") + "_counter"
            assert count == int(sums[counter]), (name, s, key)
            assert abs(total - sums[key]) <= 1e-6 * abs_total, (name, s, key, total, sums[key], abs_total)
            worst = max(worst, abs(total - sums[key]) / max(abs_total, 1e-30))
            assert np.isnan(out[key]) == (count == 0), (name, s, key)
            if count:
                assert abs(total / count - out[key]) <= 2e-6 * abs_total / count
    print(f"[{name}] restatement vs the reference's float32 sums: worst |d| / sum |summand| {worst:.3g} (bound 1e-6)")


def test_header_library_exports_and_argtypes_agree(hip):
    lib = hip.load()
    assert "tbx_loss_shape" in hip.declared_symbols()
    assert lib.tbx_loss_shape.argtypes == [C.POINTER(hip.LossShape), C.c_void_p] and lib.tbx_loss_shape.restype is C.c_int
    assert '#include "tbx_hip_loss.h"' in hip.HEADER_PATH.read_text()
    assert lib.tbx_version() == 7


def test_the_header_alone_compiles_and_defines_the_workspace_size(hip, tmp_path):
    """tbx_hip_loss.h included first (it includes tbx_hip.h for the codes) compiles as C with -Wall -Werror, and TBX_LOSS_PARTIALS is the
    ctypes module's LOSS_PARTIALS. (sizeof / offsetof of tbx_loss_shape_t against hip.LossShape: tests/test_abi_and_host.py.)"""
    root = Path(__file__).resolve().parent.parent
    src = tmp_path / "alone.c"
    src.write_text('#include "tbx_hip_loss.h"\n#include <stdio.h>\nint main(void){printf("%d\\n", TBX_LOSS_PARTIALS);'
                   'return (int)sizeof(tbx_loss_shape_t) == 0;}\n')
    exe = tmp_path / "alone"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == hip.LOSS_PARTIALS


def _stand_in(hip, **over):
    """A tbx_loss_shape_t that passes every check, on stand-in pointers (never dereferenced: each call below is refused, or rows == 0)."""
    a = hip.LossShape()
    for k in ("pred_valid", "tf", "reward_valid", "reward", "relevant", "pick", "any_valid", "w_agent", "w", "acc", "partials"):
        setattr(a, k, 0x1000)
    a.rows, a.n_ag, a.n_step, a.step_training_start = 0, 4, 8, 10
    a.mask_irrelevant, a.w_relevant, a.discount = 1, 2.0, 0.9
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_every_refusal_returns_its_code_before_a_launch(hip):
    lib = hip.load()
    ARG, UNSUPPORTED = -1, -2  # TBX_ERR_ARG, TBX_ERR_UNSUPPORTED
    assert lib.tbx_loss_shape(None, None) == ARG
    assert lib.tbx_loss_shape(C.byref(_stand_in(hip)), None) == 0  # rows == 0: nothing to do, nothing launched
    for k in ("pred_valid", "tf", "any_valid", "w_agent", "acc", "partials"):
        assert lib.tbx_loss_shape(C.byref(_stand_in(hip, **{k: None})), None) == ARG, k
    for over in (dict(rows=-1), dict(n_ag=0), dict(n_ag=-3), dict(n_step=0), dict(step_training_start=-1),
                 dict(relevant=None),                                  # both relevance switches on
                 dict(relevant=None, w_relevant=0.0),                   # mask_irrelevant alone
                 dict(relevant=None, mask_irrelevant=0),                # w_relevant alone
                 dict(reward=None), dict(reward_valid=None),            # exactly one of the pair
                 dict(reward=None, reward_valid=None)):                 # w without reward
        assert lib.tbx_loss_shape(C.byref(_stand_in(hip, **over)), None) == ARG, over
    # what is allowed to be NULL: pick; relevant with both switches off; the reward pair together with w, acc and partials (masks only)
    for over in (dict(pick=None), dict(relevant=None, mask_irrelevant=0, w_relevant=0.0), dict(w=None),
                 dict(reward=None, reward_valid=None, w=None, acc=None, partials=None)):
        assert lib.tbx_loss_shape(C.byref(_stand_in(hip, **over)), None) == 0, over
    assert lib.tbx_loss_shape(C.byref(_stand_in(hip, rows=1 << 29, n_ag=4)), None) == UNSUPPORTED  # rows * n_ag == 2^31
    assert lib.tbx_loss_shape(C.byref(_stand_in(hip, rows=(1 << 31) // 3 + 1, n_ag=3)), None) == UNSUPPORTED
    assert hip.load().tbx_error_string(UNSUPPORTED) and hip.load().tbx_error_string(ARG)
    with pytest.raises(RuntimeError):  # host tensors: no CPU path
        hip.loss_shape(torch.zeros(1, 2, 3, dtype=torch.bool), torch.zeros(1, 2, 3, dtype=torch.bool), 0, True)


def test_training_metrics_and_waymo_motion_construct_with_the_switches_on(tb):
    TM = import_module("trafficbots_amd.models.metrics.training")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    for over in (dict(temporal_discount=0.9), dict(p_loss_for_irrelevant=0.5), dict(p_loss_for_irrelevant=0.0), dict(w_relevant_agent=2.0),
                 dict(temporal_discount=0.9, p_loss_for_irrelevant=0.5, w_relevant_agent=2.0)):
        cfg = tb.config.default_sim_cfg()["training_metrics"]
        cfg.update(over)
        m = TM.TrainingMetrics(prefix="training", train_navi=True, train_latent=True, **cfg)
        assert all(getattr(m, k) == v for k, v in over.items())
        scfg = tb.config.default_sim_cfg()
        scfg["training_metrics"].update(over)
        wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
        assert all(getattr(wm.train_metrics_reactive_replay, k) == v for k, v in over.items())
        assert all(wm.hp.training_metrics[k] == v for k, v in over.items())


def test_training_loss_keeps_its_signature_and_update_gains_a_trailing_pick(tb):
    TG = import_module("trafficbots_amd.train_graph")
    TM = import_module("trafficbots_amd.models.metrics.training")
    p = list(inspect.signature(TG.training_loss).parameters.values())
    assert [q.name for q in p] == ["cfg", "ro", "navi_pred", "navi_gt", "post", "prior", "counts", "ag_role", "pick"]
    assert all(q.default is None for q in p[6:]) and all(q.default is inspect.Parameter.empty for q in p[:6])
    u = list(inspect.signature(TM.TrainingMetrics.update).parameters.values())
    assert [q.name for q in u] == ["self", "buffer", "ag_role", "navi_pred", "navi_gt", "latent_post", "latent_prior", "pick"] and u[-1].default is None
    assert TG.loss_shaping(tb.config.default_sim_cfg()["training_metrics"]) is None
