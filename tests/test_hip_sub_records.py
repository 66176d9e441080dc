"""GPU tests of the submission-record kernels (include/tbx_hip_sub.h: tbx_wosac_joint_scenes, tbx_womd_predictions) against
tests/golden/sub_records.npz - the reference's `get_scenario_rollouts`, `SubWOMD.update` and `mask_pred` selection run on the seeded
cases of `synthetic.make_sub_case` / `make_womd_sub_case` (tests/golden/make_golden_sub.py) -, plus what the header promises beyond
values: every output element written by every call, a capturable call, the transform of tbx_pose_to_global bit for bit.

Tolerances. Counts, ids, scores and copied values (sim x / y / heading, no-sim heading): exact. Extrapolated values: |got - ref| <=
2^-23 |ref| - a correctly rounded float32 fmaf is within 2^-24 relative of the real value z + v t, the reference's float64 value within
2^-53 of it, the factor 2 is the margin - and exactly equal where the velocity is 0. WOMD positions against the fixture: 4 eps
(|center|_inf + |pos|_inf), the bound of test_wosac_forward_vs_reference for the same transform (a rounding each for the two products,
their sum and the translation)."""
import json
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23
WOSAC_CASES = ("default", "flags_off", "edge")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "sub_records.npz")


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load_sub()
    return h


def _post(tb, spec):
    PP = import_module("trafficbots_amd.data_modules.wosac_post_processing")
    return PP.WOSACPostProcessing(step_gt=spec["step_gt"], step_current=spec["step_current"], const_vel_z_sim=spec["const_vel_z_sim"],
                                  const_vel_no_sim=spec["const_vel_no_sim"], w_road_edge=0.0, use_wosac_col=True)


def _wosac(tb, golden, name):
    """-> (spec, the case's wosac_data on the host, on the device)."""
    spec = json.loads(str(golden["cases"]))["wosac"][name]
    data = tb.synthetic.make_sub_case(step_current=spec["step_current"], **spec["case"])
    return spec, data, {k: v.to(DEV) for k, v in data.items()}


def _kernel_inputs(d):
    sq = lambda k: d[k].squeeze(-1).contiguous()
    return (d["pos_sim"], sq("yaw_sim"), d["valid_sim"], sq("z_sim"), d["object_id_sim"], d["pos_no_sim"], sq("yaw_no_sim"), sq("z_no_sim"),
            d["valid_no_sim"], d["object_id_no_sim"])


def _within(got, ref, still, what):
    """got f32, ref f64 arrays of one shape; still: bool, broadcastable - where the velocity is 0."""
    got, err = got.astype(np.float64), np.abs(got.astype(np.float64) - ref)
    rel = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if ref.size else 0.0
    print(f"{what}: largest |got - ref| / |ref| = {rel:.3e} (bound {EPS:.3e}), {int(np.broadcast_to(still, ref.shape).sum())} of {ref.size} values at velocity 0")
    assert (err <= EPS * np.abs(ref)).all(), what
    assert (np.broadcast_to(still, ref.shape) <= (got == ref)).all(), f"{what}: a value at velocity 0 is not the value at step_current"


@pytest.mark.parametrize("name", WOSAC_CASES)
def test_joint_scenes_vs_reference(tb, golden, name):
    spec, data, dev = _wosac(tb, golden, name)
    out = {k: v.cpu().numpy() for k, v in _post(tb, spec).get_joint_scenes(dev).items()}
    assert list(out) == ["scenario_id", "traj_sim", "traj_no_sim", "object_id_sim", "object_id_no_sim", "n_sim", "n_no_sim"]
    n_sc, K, A, T = data["pos_sim"].shape[:4]
    N, c = data["pos_no_sim"].shape[1], spec["step_current"]
    assert out["traj_sim"].shape == (n_sc, K, A, T, 4) and out["traj_no_sim"].shape == (n_sc, N, T, 4), "no-sim rows are stored once per scene"
    assert out["traj_sim"].dtype == out["traj_no_sim"].dtype == np.float32 and out["object_id_sim"].dtype == np.int64 and out["n_sim"].dtype == np.int32
    assert np.array_equal(out["scenario_id"], data["scenario_id"].numpy())
    # counts and compacted ids: exact
    assert np.array_equal(out["n_sim"], golden[f"{name}_n_sim"]) and np.array_equal(out["n_no_sim"], golden[f"{name}_n_no_sim"])
    assert np.array_equal(out["object_id_sim"], golden[f"{name}_id_sim"]) and np.array_equal(out["object_id_no_sim"], golden[f"{name}_id_no_sim"])
    print(f"{name}: n_sim {out['n_sim'].tolist()}, n_no_sim {out['n_no_sim'].tolist()}")
    # copies: bit-equal (the fixture's padding is zeros, so this also covers the rows from the count on)
    xyh = golden["default_sim_xyh" if name == "flags_off" else f"{name}_sim_xyh"]
    assert np.array_equal(out["traj_sim"][..., [0, 1, 3]].view(np.int32), xyh.view(np.int32)), "sim x / y / heading"
    assert np.array_equal(out["traj_no_sim"][..., 3].view(np.int32), golden[f"{name}_ns_heading"].view(np.int32)), "no-sim heading"
    # extrapolated values; `still` = no velocity by the reference's rule, per compacted slot
    for key, n, flag in (("sim", A, spec["const_vel_z_sim"]), ("no_sim", N, spec["const_vel_no_sim"])):
        valid = data[f"valid_{key}"].numpy()
        still = np.ones((n_sc, n), bool)  # (slots past the count: zeros on both sides)
        for s in range(n_sc):
            kept = np.where(valid[s, :, c])[0]
            still[s, : len(kept)] = ~(flag & valid[s, kept, c - 1])
        if key == "sim":
            z = out["traj_sim"][..., 2]  # [n_sc, K, A, T]: the reference's center_z is the same array in every rollout
            assert np.array_equal(z.view(np.int32), np.broadcast_to(z[:, :1], z.shape).view(np.int32))
            _within(z[:, 0], golden[f"{name}_sim_z"], still[:, :, None], f"{name} sim z")
        else:
            _within(out["traj_no_sim"][..., :3], golden[f"{name}_ns_xyz"], still[:, :, None, None], f"{name} no-sim x / y / z")
        if flag and n:
            assert not still[np.arange(n)[None] < out[f"n_{key}"][:, None]].all(), "the case has objects with a velocity"
    # rows from the count on: zeros, ids -1
    for key, n in (("sim", A), ("no_sim", N)):
        past = np.arange(n)[None] >= out[f"n_{key}"][:, None]  # [n_sc, n]
        tr = out["traj_sim"].transpose(0, 2, 1, 3, 4) if key == "sim" else out["traj_no_sim"]
        assert not tr[past].any() and (out[f"object_id_{key}"][past] == -1).all() and (out[f"object_id_{key}"][~past] >= 0).all()


@pytest.mark.parametrize("name", ("default", "edge"))
def test_joint_scenes_write_every_element_and_capture(tb, golden, hip, name):
    """Two calls into buffers pre-filled with NaN / -7 give what a call into fresh buffers gives, bit for bit; one replay of a captured
    call equals the eager call."""
    spec, data, dev = _wosac(tb, golden, name)
    args = _kernel_inputs(dev) + (spec["step_current"], spec["const_vel_z_sim"], spec["const_vel_no_sim"])
    fresh = hip.wosac_joint_scenes(*args)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    for _ in range(2):
        out = tuple(torch.full_like(t, float("nan")) if t.is_floating_point() else torch.full_like(t, -7) for t in fresh)
        assert hip.wosac_joint_scenes(*args, out=out) is out
        for got, want in zip(out, fresh):
            assert torch.equal(bits(got), bits(want))
    assert not any(bool(torch.isnan(t).any()) for t in fresh[:2])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = hip.wosac_joint_scenes(*args)
    for t in cap:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip(cap, fresh):
        assert torch.equal(bits(got), bits(want))
    del g


@pytest.fixture(scope="module")
def womd(tb, golden, hip):
    spec = json.loads(str(golden["cases"]))["womd"]
    c = tb.synthetic.make_womd_sub_case(**spec)
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    args = (dev["trajs"], dev["scores"], dev["history/agent/object_id"], dev["ref/ag_role"][..., 2].contiguous(), dev["scenario_center"],
            dev["scenario_yaw"])
    return c, dev, args, hip.womd_predictions(*args)


def test_womd_predictions_vs_reference_and_pose_to_global(tb, golden, hip, womd):
    c, dev, args, (pos, scores, oid, count) = womd
    n_sc, A, k, n = c["trajs"].shape[:4]
    mask = c["ref/ag_role"][..., 2]
    assert pos.shape == (n_sc, A, k, n, 2) and scores.shape == (n_sc, A, k) and oid.dtype == torch.int64 and count.dtype == torch.int32
    # counts, ids, scores: exact
    assert np.array_equal(count.cpu().numpy(), golden["womd_n"]) and count.tolist() == mask.sum(-1).tolist()
    assert count.tolist()[1] == 0 and count.tolist()[2] == A, "one scene with no predicted agent, one with all"
    assert np.array_equal(oid.cpu().numpy(), golden["womd_id"])
    assert np.array_equal(scores.cpu().numpy().view(np.int32), golden["womd_scores"].view(np.int32))
    # the transform is tbx_pose_to_global's, bit for bit: the same input through it, then torch's boolean-mask compaction
    t = dev["trajs"]
    glob, _ = hip.pose_to_global(t, 3, t[..., 2], 3, dev["scenario_center"], dev["scenario_yaw"], A * k, n, n)
    glob = glob.view(n_sc, A, k, n, 2)
    for s in range(n_sc):
        m = int(count[s])
        assert torch.equal(pos[s, :m].view(torch.int32), glob[s][mask[s].to(DEV)].view(torch.int32)), f"scene {s}"
        assert not bool(pos[s, m:].any()) and not bool(scores[s, m:].any()) and bool((oid[s, m:] == -1).all())
    # against the reference's float32 torch expression
    tol = 4 * EPS * (float(c["scenario_center"].abs().max()) + float(c["trajs"][..., :2].abs().max()))
    worst = float(np.abs(pos.cpu().numpy().astype(np.float64) - golden["womd_pos"].astype(np.float64)).max())
    print(f"womd pos: largest difference {worst:.3e} m (tolerance {tol:.3e})")
    assert worst <= tol


def test_womd_predictions_write_every_element_and_capture(hip, womd):
    _, _, args, fresh = womd
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    for _ in range(2):
        out = tuple(torch.full_like(t, float("nan")) if t.is_floating_point() else torch.full_like(t, -7) for t in fresh)
        assert hip.womd_predictions(*args, out=out) is out
        for got, want in zip(out, fresh):
            assert torch.equal(bits(got), bits(want))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = hip.womd_predictions(*args)
    for t in cap:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip(cap, fresh):
        assert torch.equal(bits(got), bits(want))
    del g


def test_sub_womd_records_are_the_fixtures(tb, golden, womd):
    """SubWOMD.update -> compute -> aggregate_on_cpu -> records(): per scene the predicted agents' arrays, trimmed; the same batch a
    second time adds nothing."""
    SUB = import_module("trafficbots_amd.utils.submission")
    c, dev, _, _ = womd
    sub = SUB.SubWOMD(is_active=True)
    for _ in range(2):
        sub.update(dev, dev["trajs"], dev["scores"])
        sub.aggregate_on_cpu(sub.compute())
        sub.reset()
    recs = sub.records()
    assert [r["scenario_id"] for r in recs] == c["scenario_id"]
    for s, r in enumerate(recs):
        m = int(golden["womd_n"][s])
        assert np.array_equal(r["object_id"], golden["womd_id"][s, :m]) and np.array_equal(r["scores"], golden["womd_scores"][s, :m])
        assert r["trajs"].shape == (m,) + golden["womd_pos"].shape[2:]
