"""CPU-only checks of the validation metrics: `tbx_rollout_metrics` is declared, exported and bound, refuses bad arguments before any
launch, `ErrorMetrics` / `TrafficRuleMetrics` (models/metrics/logging.py) construct without a device and turn the reference's raw states
(tests/golden/val_metrics.npz, written by tests/golden/make_golden_val.py from the reference's classes) into the reference's keys and
ratios, `WaymoMotion` carries the validation entry points, and `sync()` sums the states of two gloo ranks."""
import json
import os
import sys
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
ERR_ARG, ERR_UNSUPPORTED = -1, -2
ERR_KEYS = ["err/pos_meter", "err/rot_deg", "err/spd_m_per_s"]
RULE_KEYS = ["traffic_rule/" + k for k in ("outside_map", "collided", "run_road_edge", "run_red_light", "passive", "goal_reached", "dest_reached")]


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "val_metrics.npz")


def test_rollout_metrics_is_declared_exported_and_bound(hip):
    """include/tbx_hip.h declares the entry point through the topical header it includes; it is bound with its 23 arguments, and the
    ctypes module mirrors the header's #defines. (The library's export list against the headers: tests/test_abi_and_host.py.)"""
    lib = hip.load()
    assert "tbx_rollout_metrics" in hip.declared_symbols()
    assert '#include "tbx_hip_metrics.h"' in hip.HEADER_PATH.read_text()
    assert hasattr(lib, "tbx_rollout_metrics")
    assert len(lib.tbx_rollout_metrics.argtypes) == 23 and lib.tbx_rollout_metrics.restype is not None
    assert lib.tbx_version() == 7  # (an added entry point changes no existing one: no bump)
    assert (hip.METRICS_SLOTS, hip.METRICS_PARTIAL_ROWS) == (16, 256)
    ext = (hip.HEADER_PATH.parent / "tbx_hip_metrics.h").read_text()
    assert "#define TBX_METRICS_SLOTS 16" in ext and "#define TBX_METRICS_PARTIAL_ROWS 256" in ext
    assert callable(hip.rollout_metrics) and callable(hip.u8_row_steps)


def test_the_header_compiles_as_c_with_the_extension(hip, tmp_path):
    """gcc on a C file that includes tbx_hip.h alone, and one that includes the topical header first: the declaration is visible."""
    import subprocess

    inc = hip.HEADER_PATH.parent
    for i, first in enumerate(("tbx_hip.h", "tbx_hip_metrics.h")):
        src = tmp_path / f"t{i}.c"
        src.write_text(f'#include "{first}"\n#include "tbx_hip.h"\nint main(void){{ int (*f)(const uint8_t*, const float*, const float*, int64_t, int, int, int, int, '
                       'int, const uint8_t*, const float*, const float*, int, int, const uint8_t*, int, const uint8_t*, const uint8_t*, '
                       'const uint8_t*, const uint8_t*, double*, double*, void*) = tbx_rollout_metrics; '
                       'return (f != 0 && TBX_METRICS_SLOTS == 16 && TBX_RULE_PASSIVE == 16 && TBX_ABI_VERSION == 7) ? 0 : 1; }\n')
        subprocess.run(["gcc", "-Wall", "-Werror", "-I", str(inc), "-c", str(src), "-o", str(tmp_path / f"t{i}.o")], check=True)


def _call(lib, **over):
    """A consistent call with both halves on (stand-in pointers: every variation below is refused before anything is launched)."""
    P = lambda i: 0x10000 * (i + 1)
    a = dict(pred_valid=P(0), pred_pose=P(1), pred_motion=P(2), n_rows=4, n_k=1, n_ag=5, ld_t=11, t0=1, n_t=7, gt_valid=P(3), gt_pose=P(4),
             gt_motion=P(5), n_step_gt=10, gt_t0=1, flags=P(6), ld_flags=7, outside_map=P(7), dest_reached=P(8), goal_reached=P(9),
             ag_type=P(10), acc=P(11), partials=P(12))
    assert set(over) <= set(a)
    a.update(over)
    return lib.tbx_rollout_metrics(*a.values(), None)


RULE_OFF = dict(flags=None, outside_map=None, dest_reached=None, goal_reached=None, ag_type=None)
ERR_OFF = dict(gt_valid=None, gt_pose=None, gt_motion=None)


@pytest.mark.parametrize("over,code", [
    (dict(pred_valid=None), ERR_ARG), (dict(acc=None), ERR_ARG), (dict(partials=None), ERR_ARG),
    ({**RULE_OFF, **ERR_OFF}, ERR_ARG),                                      # nothing to do
    (dict(gt_pose=None), ERR_ARG), (dict(gt_motion=None), ERR_ARG), (dict(pred_pose=None), ERR_ARG), (dict(pred_motion=None), ERR_ARG),
    ({**ERR_OFF, "gt_pose": 0x50000}, ERR_ARG),                              # a pointer of a half that is off
    (dict(outside_map=None), ERR_ARG), (dict(dest_reached=None), ERR_ARG), (dict(ag_type=None), ERR_ARG),
    ({**RULE_OFF, "ag_type": 0x50000}, ERR_ARG), ({**RULE_OFF, "goal_reached": 0x50000}, ERR_ARG),
    (dict(n_rows=0), ERR_ARG), (dict(n_ag=0), ERR_ARG), (dict(n_t=0), ERR_ARG), (dict(n_k=0), ERR_ARG), (dict(t0=-1), ERR_ARG),
    ({**ERR_OFF, "n_k": 3}, ERR_ARG),                                        # 4 rows are no whole number of 3 rollouts
    (dict(ld_t=7), ERR_ARG),                                                 # steps 1..7 of a 7-step row
    (dict(n_step_gt=7), ERR_ARG), (dict(gt_t0=4), ERR_ARG), (dict(gt_t0=-1), ERR_ARG),
    (dict(ld_flags=6), ERR_ARG),
    (dict(n_k=2), ERR_UNSUPPORTED),                                          # the error half with joint futures
    ({**ERR_OFF, "n_rows": 1 << 29}, ERR_UNSUPPORTED),                       # 5 * 2^29 pairs
])
def test_argument_checks_return_codes_without_a_gpu(hip, over, code):
    assert _call(hip.load(), **over) == code


def test_wrapper_refuses_cpu_tensors_and_short_vectors(hip):
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt)
    acc, part = z(16, dt=torch.float64), z(256 * 16, dt=torch.float64)
    with pytest.raises(RuntimeError, match="device tensors"):
        hip.rollout_metrics(acc, part, z(2, 3, 4), 1, 4, 0, 4, flags=z(2, 3, 4), ld_flags=4, outside_map=z(2, 3, 4), dest_reached=z(2, 3, 4),
                            ag_type=z(2, 3, 3))
    with pytest.raises(RuntimeError, match="METRICS_SLOTS"):
        hip.rollout_metrics(acc[:8], part, z(2, 3, 4), 1, 4, 0, 4)


def test_u8_row_steps_finds_the_log_behind_a_view(hip):
    log = torch.zeros(6, 5, 11, dtype=torch.uint8)
    f = torch.zeros(6, 5, 11, 3)
    assert hip.u8_row_steps(log) == 11 and hip.u8_row_steps(log[:, :, 1:8]) == 11 and hip.u8_row_steps(f[:, :, 1:8], 1) == 11
    assert hip.u8_row_steps(log.view(2, 3, 5, 11)[:, :, :, 2:].flatten(0, 1)) == 11
    assert hip.u8_row_steps(log[:, :, 1:8].contiguous()) == 7
    assert hip.u8_row_steps(log[:1, :1, 2:5]) == 3                       # size-1 dimensions carry no stride information
    assert hip.u8_row_steps(log[:, :1, 2:5]) == 55                       # one agent per row: the row stride is all there is
    assert hip.u8_row_steps(log.transpose(0, 1)) is None and hip.u8_row_steps(log[:, :, ::2]) is None
    assert hip.u8_row_steps(f[..., :2], 1) is None and hip.u8_row_steps(log[:, ::2]) is None


def test_classes_construct_and_compute_the_references_keys_and_ratios(tb, golden):
    L = import_module("trafficbots_amd.models.metrics.logging")
    cases = json.loads(str(golden["cases"]))
    for cls, keys in ((L.ErrorMetrics, ERR_KEYS), (L.TrafficRuleMetrics, RULE_KEYS)):
        m = cls("p")
        assert m.state.dtype == torch.float64 and m.state.shape == (16,) and float(m.state.abs().sum()) == 0 and not m.state.is_cuda
        assert not m.state_dict(), "metric states are no checkpoint entries"
        out = m.compute()
        assert list(out) == ["p/" + k for k in keys]
        assert all(v.dtype == torch.float32 and v.dim() == 0 and bool(torch.isnan(v)) for v in out.values()), "0 / 0 -> nan, as the reference"
    seen_nan = False
    for name, c in cases.items():
        rule = L.TrafficRuleMetrics("p")
        rule.state[4:13] = torch.from_numpy(golden[f"{name}_rule_state"])
        out = rule.compute()
        assert list(out) == c["rule_keys"]
        want = torch.from_numpy(golden[f"{name}_rule_compute"])
        torch.testing.assert_close(torch.stack(list(out.values())).double(), want, rtol=2.0 ** -23, atol=0, equal_nan=True)
        seen_nan |= bool(torch.isnan(want).any())
        if "err_keys" in c:
            err = L.ErrorMetrics("p")
            err.state[0:4] = torch.from_numpy(golden[f"{name}_err_state"])
            out = err.compute()
            assert list(out) == c["err_keys"]
            torch.testing.assert_close(torch.stack(list(out.values())).double(), torch.from_numpy(golden[f"{name}_err_compute"]), rtol=2.0 ** -23, atol=0)
            err.reset()
            assert float(err.state.abs().sum()) == 0
    assert seen_nan, "the fixture's counter_veh = 0 case"


def test_update_refuses_what_the_kernel_must_not_see(tb):
    """Shape errors are raised from host metadata before the wrapper is reached (the tensors are on the CPU: reaching it would raise
    'device tensors')."""
    from types import SimpleNamespace

    L = import_module("trafficbots_amd.models.metrics.logging")
    b = lambda *s: torch.zeros(*s, dtype=torch.bool)
    buf = SimpleNamespace(step_start=1, step_end=7, pred_valid=b(2, 3, 5, 7), pred_pose=torch.zeros(2, 3, 5, 7, 3), pred_motion=torch.zeros(2, 3, 5, 7, 3),
                          violation={k: b(2, 3, 5, 7) for k in ("outside_map", "dest_reached", "collided", "run_road_edge", "run_red_light", "passive")})
    with pytest.raises(ValueError, match="one joint future"):
        L.ErrorMetrics("p").update(buf, b(2, 5, 10), torch.zeros(2, 5, 10, 3), torch.zeros(2, 5, 10, 3))
    with pytest.raises(ValueError, match="whole number"):
        L.TrafficRuleMetrics("p").update(buf, b(4, 5, 3))
    with pytest.raises(ValueError, match="whole number"):
        L.TrafficRuleMetrics("p").update(buf, b(2, 6, 3))
    buf.violation["passive"] = b(2, 3, 5, 6)
    with pytest.raises(ValueError, match="pred_valid's shape"):
        L.TrafficRuleMetrics("p").update(buf, b(2, 5, 3))
    one = SimpleNamespace(step_start=4, step_end=10, pred_valid=b(2, 1, 5, 7), pred_pose=torch.zeros(2, 1, 5, 7, 3), pred_motion=torch.zeros(2, 1, 5, 7, 3))
    with pytest.raises(ValueError, match="run past"):
        L.ErrorMetrics("p").update(one, b(2, 5, 10), torch.zeros(2, 5, 10, 3), torch.zeros(2, 5, 10, 3))
    with pytest.raises(ValueError, match="do not match"):
        L.ErrorMetrics("p").update(one, b(2, 6, 12), torch.zeros(2, 6, 12, 3), torch.zeros(2, 6, 12, 3))


def test_waymo_motion_has_the_validation_entry_points(tb):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    L = import_module("trafficbots_amd.models.metrics.logging")
    TM = import_module("trafficbots_amd.models.metrics.training")
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg())
    assert isinstance(wm.train_metrics_reactive_replay, TM.TrainingMetrics) and wm.train_metrics_reactive_replay.prefix == "reactive_replay"
    assert wm.train_metrics_reactive_replay.train_navi and wm.train_metrics_reactive_replay.train_latent
    assert isinstance(wm.err_metrics_reactive_replay, L.ErrorMetrics) and wm.err_metrics_reactive_replay.prefix == "reactive_replay"
    assert isinstance(wm.rule_metrics_reactive_replay, L.TrafficRuleMetrics) and wm.rule_metrics_reactive_replay.prefix == "reactive_replay"
    assert isinstance(wm.rule_metrics_joint_future_pred, L.TrafficRuleMetrics) and wm.rule_metrics_joint_future_pred.prefix == "joint_future_pred"
    assert callable(wm.validation_step) and callable(wm.validation_epoch_end)
    assert not [k for k in wm.state_dict() if "metrics" in k], "the checkpoint layout is the reference's"
    with pytest.raises(NotImplementedError):
        wm.wosac_post_processing.get_scenario_rollouts({})


def _sync_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from __graft_entry__ import load_package

    load_package()
    L = import_module("trafficbots_amd.models.metrics.logging")
    err, rule = L.ErrorMetrics("p"), L.TrafficRuleMetrics("p")
    err.state[0:4] = torch.tensor([3.0, 1.5, 20.0, 0.25], dtype=torch.float64) * (rank + 1)
    rule.state[4:13] = torch.arange(9, dtype=torch.float64) + 10 * rank
    err.sync()
    rule.sync(group=dist.group.WORLD)
    torch.save({"err": err.state, "rule": rule.state, "compute": err.compute()}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_sync_sums_the_states_of_two_ranks(tmp_path, tb):
    L = import_module("trafficbots_amd.models.metrics.logging")
    alone = L.ErrorMetrics("p")
    alone.state[0] = 2.0
    alone.sync()  # no process group: a no-op
    assert float(alone.state[0]) == 2.0
    world, port = 2, 29553
    mp.spawn(_sync_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        got = torch.load(tmp_path / f"r{r}.pt")
        want_err = torch.zeros(16, dtype=torch.float64)
        want_err[0:4] = torch.tensor([9.0, 4.5, 60.0, 0.75], dtype=torch.float64)
        want_rule = torch.zeros(16, dtype=torch.float64)
        want_rule[4:13] = 2 * torch.arange(9, dtype=torch.float64) + 10
        assert torch.equal(got["err"], want_err) and torch.equal(got["rule"], want_rule), r
        assert float(got["compute"]["p/err/pos_meter"]) == 0.5
