"""GPU tests of the post-processing of the joint futures: `WOMDPostProcessing.forward` (tbx_womd_modes) against the reference's
outputs in tests/golden/womd_post.npz, its mode-order rule, its in-place read of the engine's rollout log and its capture into a
graph, the reference's three `validation_step` statements after `joint_future_pred` (waymo_motion.py:602-650), and
`WOSACPostProcessing.forward` (tbx_pose_to_global) against tests/golden/wosac_forward.npz.

Tolerances: the kept futures are compared as sets on every agent whose decision margins (recorded by the fixture's
generator in float64) are at least 1e-4 m and 1e-5 relative - at most 5 % of a case's agents may fall below -, trajectories are a
gather and compared bit for bit, scores within 8 x the largest float32 - float64 difference of the reference itself on that case."""
import json
import math
from importlib import import_module

import numpy as np
import pytest
import torch

from test_hip_rollout import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23
BASE = dict(k_pred=6, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0], mtr_nms_thresh=[], aggr_thresh=[], n_iter_em=3, use_ade=True,
            step_gt=90, step_current=10)
CASES = ("default", "submission", "fde", "mtr32", "mtr48", "per_type_temp", "replay_k1", "k6")


def _pp(tb, **over):
    P = import_module("trafficbots_amd.data_modules.womd_post_processing")
    return P.WOMDPostProcessing(**{**BASE, **over})


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "womd_post.npz")


@pytest.mark.parametrize("name", CASES)
def test_modes_vs_reference(tb, golden, name):
    """Every case of the fixture: default configuration (top-k + mpa_nms, ADE) at 4 x 32 x 64 x 80 and at the submission shape
    2 x 128 x 128 x 80, FDE, mtr_nms at K = 32 and K = 48, per-type mpa_nms with a temperature, K = 1 without scores, K = 6."""
    spec = json.loads(str(golden["cases"]))[name]
    c = tb.synthetic.make_womd_case(**spec["case"])
    pp = _pp(tb, **spec["cfg"])
    dev = torch.device(DEV)
    out = pp(c["ag_type"].to(dev), c["trajs"].to(dev), c["log_prob"].to(dev) if spec["with_scores"] else None)
    idx, scores, trajs = pp.last_idx.cpu().long(), out["scores"].cpu(), out["trajs"].cpu()
    n_sc, K, A = c["log_prob"].shape
    k = min(K, 6)
    assert trajs.shape == (n_sc, A, k, 16, 3) and scores.shape == (n_sc, A, k) and trajs.dtype == scores.dtype == torch.float32
    # a gather: bit for bit, every agent
    src = c["trajs"].transpose(1, 2)[:, :, :, 4:80:5]  # [n_sc, A, K, 16, 3]
    assert torch.equal(trajs, src.gather(2, idx[..., None, None].expand(-1, -1, -1, 16, 3)))
    assert all(len(set(r.tolist())) == k for r in idx.flatten(0, 1)), "a future kept twice"
    # kept sets, on the agents whose decisions are not within rounding of a threshold / a tie
    ref_idx, ref_scores = torch.from_numpy(golden[f"{name}_idx"].astype(np.int64)), torch.from_numpy(golden[f"{name}_scores"])
    safe = torch.from_numpy((golden[f"{name}_margin_d"] >= 1e-4) & (golden[f"{name}_margin_s"] >= 1e-5))
    left_out = 1.0 - float(safe.float().mean())
    ours_sorted, ours_order = idx.sort(-1)
    ref_sorted, ref_order = ref_idx.sort(-1)
    same = (ours_sorted == ref_sorted).all(-1)
    tol = 8.0 * float(golden[f"{name}_bound"])
    diff = (scores.gather(-1, ours_order) - ref_scores.gather(-1, ref_order)).abs()
    worst = float(diff[same & safe].max())
    print(f"{name}: left out {left_out:.4f}, kept sets equal on {int((same & safe).sum())}/{int(safe.sum())} safe agents, "
          f"largest score difference {worst:.3e} (tolerance {tol:.3e}), scores at the 1e-3 floor {float((scores < 5e-3).float().mean()):.3f}")
    assert left_out <= 0.05
    assert bool(same[safe].all())
    assert worst <= tol
    torch.testing.assert_close(scores.sum(-1), torch.ones(n_sc, A), rtol=0, atol=4 * EPS)


def test_topk_order_is_descending_score_with_ties_to_the_lower_future(tb):
    """Exact ties made with equal log-probabilities: the kept modes come out in descending score, equal scores in future order."""
    dev = torch.device(DEV)
    c = tb.synthetic.make_womd_case(2, 32, 16, 80, seed=11)
    g = torch.Generator().manual_seed(0)
    logp = torch.randint(0, 4, (2, 32, 16), generator=g).float() * -0.5  # four distinct values over 32 futures: ties everywhere
    pp = _pp(tb, mpa_nms_thresh=[])
    out = pp(c["ag_type"].to(dev), c["trajs"].to(dev), logp.to(dev))
    want = torch.sort(-logp.transpose(1, 2), dim=-1, stable=True)[1][..., :6]
    assert torch.equal(pp.last_idx.cpu().long(), want)
    s = out["scores"].cpu()
    assert bool((s[..., :-1] >= s[..., 1:]).all())
    kept_lp = logp.transpose(1, 2).gather(-1, want)
    assert torch.equal(s[..., :-1] == s[..., 1:], kept_lp[..., :-1] == kept_lp[..., 1:]), "equal log-probabilities <-> equal scores"


def test_identical_futures_suppress_exactly_one_of_each_other(tb):
    """mpa_nms on K = 6 futures 100 m apart, futures 1 and 4 identical: the one with the lower score drops to 1e-3 (then renormalised),
    the other keeps its share; with EQUAL scores neither is suppressed (`scores > scores[k]` is strict)."""
    dev = torch.device(DEV)
    t = torch.arange(80, dtype=torch.float32)
    trajs = torch.zeros(1, 6, 2, 80, 3)
    trajs[0, :, :, :, 0] = t.view(1, 1, 80) * 0.5
    trajs[0, :, :, :, 1] = (torch.arange(6, dtype=torch.float32) * 100.0).view(6, 1, 1)
    trajs[0, 4] = trajs[0, 1]
    ty = torch.tensor([[[True, False, False], [False, False, False]]])  # agent 1 has no type: threshold 0, nothing is within it
    logp = torch.tensor([0.3, 0.1, -0.2, 0.0, 0.6, -0.4]).view(1, 6, 1).expand(1, 6, 2).contiguous()
    pp = _pp(tb)
    soft = logp[0, :, 0].double().softmax(-1)
    s = pp(ty.to(dev), trajs.to(dev), logp.to(dev))["scores"].cpu().double()
    want = soft.clone()
    want[1] = float(np.float32(1e-3))  # future 1 (0.1) is the lower of the identical pair
    want = want / want.sum()
    torch.testing.assert_close(s[0, 0], want, rtol=0, atol=4 * EPS)
    torch.testing.assert_close(s[0, 1], soft, rtol=0, atol=4 * EPS)
    assert torch.equal(pp.last_idx.cpu(), torch.arange(6, dtype=torch.int32).expand(1, 2, 6))
    logp[0, 4] = logp[0, 1]
    s = pp(ty.to(dev), trajs.to(dev), logp.to(dev))["scores"].cpu().double()
    torch.testing.assert_close(s[0, 0], logp[0, :, 0].double().softmax(-1), rtol=0, atol=4 * EPS)


@pytest.fixture(scope="module")
def validation(tb):
    """The reference's validation_step up to joint_future_pred at C1 sizes, as test_validation_step_in_the_references_calling_order
    replays it: -> (wm, batch, buffer_reactive_replay, buffer_joint_future_pred)."""
    dev = torch.device(DEV)
    wm, _, _, batch = _setup(tb, dev, (8, 64, 8), 4)
    model = wm.model
    mp_tokens = model.mp_encoder(batch["sc/mp_valid"], batch["sc/mp_attr"], batch["sc/mp_pose"], batch["ref/mp_type"])
    tl_tokens = model.tl_encoder.pre_compute(tl_valid=batch["gt/tl_valid"], tl_attr=batch["sc/tl_attr"], tl_pose=batch["sc/tl_pose"], **mp_tokens)
    latent_post = model.latent_encoder(ag_valid=batch["gt/ag_valid"], ag_attr=batch["sc/ag_attr"], ag_motion=batch["gt/ag_motion"],
                                       ag_pose=batch["gt/ag_pose"], ag_type=batch["ref/ag_type"], tl_state=batch["gt/tl_state"],
                                       mp_tokens=mp_tokens, tl_tokens=tl_tokens, posterior=True)
    latent_prior = model.latent_encoder(ag_valid=batch["sc/ag_valid"], ag_attr=batch["sc/ag_attr"], ag_motion=batch["sc/ag_motion"],
                                        ag_pose=batch["sc/ag_pose"], ag_type=batch["ref/ag_type"], tl_state=batch["sc/tl_state"],
                                        mp_tokens=mp_tokens, tl_tokens=tl_tokens, posterior=False)
    navi_pred = model.navi_predictor(ag_valid=batch["sc/ag_valid"], ag_attr=batch["sc/ag_attr"], ag_motion=batch["sc/ag_motion"],
                                     ag_pose=batch["sc/ag_pose"], ag_type=batch["ref/ag_type"], **mp_tokens)
    buffer_reactive_replay = wm.reactive_replay(batch=batch, mp_tokens=mp_tokens, tl_tokens=tl_tokens,
                                                ag_latent=latent_post.sample(deterministic=True), ag_latent_valid=latent_post.valid,
                                                ag_navi=batch["gt/ag_navi"], ag_navi_valid=batch["gt/ag_valid"].any(-1),
                                                teacher_forcing=wm.teacher_forcing_reactive_replay, deterministic_action=True)
    # (the engine's log is reused by the next rollout: keep what the first one wrote)
    rr_pose = buffer_reactive_replay.pred_pose.clone()
    torch.manual_seed(5)
    buffer_joint_future_pred = wm.joint_future_pred(batch=batch, mp_tokens=mp_tokens, tl_tokens=tl_tokens, ag_latent_dist=latent_prior,
                                                    ag_navi_dist=navi_pred, teacher_forcing=wm.teacher_forcing_joint_future_pred,
                                                    n_joint_future=wm.hparams.n_joint_future_wosac)
    buffer_reactive_replay.pred_pose = rr_pose
    batch.update({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in tb.synthetic.make_wosac_keys(1, 8, seed=0).items()})
    yield wm, batch, buffer_reactive_replay, buffer_joint_future_pred
    del wm


def test_forward_reads_the_engines_log_in_place_and_captures(tb, validation):
    """`buffer.pred_pose[:, :, :, start:]` / `buffer.log_prob` of a real joint_future_pred go to the kernel as they lie in memory (a time
    slice of [n_sc*K, A, T_log, 3], no transposed copy); the result equals that on a dense clone. One linear graph capture of `forward`
    and one replay reproduce the eager call: nothing in it waits for the device."""
    wm, batch, _, buf = validation
    pp = wm.womd_post_processing
    start = buf.step_future_start
    view = buf.pred_pose[:, :, :, start:]
    assert not view.is_contiguous() and view.shape == (1, 32, 8, 80, 3)
    seen = []
    hip = import_module("trafficbots_amd.hip")
    real = hip.womd_modes
    hip.womd_modes = lambda pose, *a, **k: (seen.append(pose.data_ptr()), real(pose, *a, **k))[1]
    try:
        eager = pp(batch["ref/ag_type"], view, buf.log_prob)
    finally:
        hip.womd_modes = real
    assert seen == [view.data_ptr()], "the kernel was handed a copy of the log"
    dense = pp(batch["ref/ag_type"], view.clone(memory_format=torch.contiguous_format), buf.log_prob.clone())
    assert torch.equal(eager["trajs"], dense["trajs"]) and torch.equal(eager["scores"], dense["scores"])
    assert torch.equal(eager["trajs"], view.transpose(1, 2).gather(2, pp.last_idx.long()[..., None, None].expand(-1, -1, -1, 80, 3))[:, :, :, 4:80:5])
    torch.testing.assert_close(eager["scores"].sum(-1), torch.ones(1, 8, device=DEV), rtol=0, atol=4 * EPS)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = pp(batch["ref/ag_type"], view, buf.log_prob)
    cap["trajs"].zero_()
    cap["scores"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap["trajs"], eager["trajs"]) and torch.equal(cap["scores"], eager["scores"])
    del g


def test_validation_step_continues_past_joint_future_pred(tb, validation):
    """The reference's next three statements (waymo_motion.py:610-613, :629-633, :649) on the buffers of the calling-order setup at C1
    sizes: dicts with the reference's keys, shapes and dtypes."""
    wm, batch, buffer_reactive_replay, buffer_joint_future_pred = validation
    womd_reactive_replay = wm.womd_post_processing(
        ag_type=batch["ref/ag_type"],
        trajs=buffer_reactive_replay.pred_pose[:, :, :, buffer_reactive_replay.step_future_start:],
    )
    womd_joint_future_pred = wm.womd_post_processing(
        ag_type=batch["ref/ag_type"],
        trajs=buffer_joint_future_pred.pred_pose[:, :, :, buffer_joint_future_pred.step_future_start:],
        scores=buffer_joint_future_pred.log_prob,
    )
    wosac_data = wm.wosac_post_processing(batch, buffer_joint_future_pred)
    A, K = 8, 32
    for d, k in ((womd_reactive_replay, 1), (womd_joint_future_pred, 6)):
        assert set(d) == {"trajs", "scores"}
        assert d["trajs"].shape == (1, A, k, 16, 3) and d["scores"].shape == (1, A, k)
        assert d["trajs"].dtype == d["scores"].dtype == torch.float32 and d["trajs"].is_cuda
        torch.testing.assert_close(d["scores"].sum(-1), torch.ones(1, A, device=DEV), rtol=0, atol=4 * EPS)
    assert torch.equal(womd_reactive_replay["trajs"][:, :, 0], buffer_reactive_replay.pred_pose[:, 0, :, 10:][:, :, 4:80:5])
    assert bool((womd_reactive_replay["scores"] == 1).all())
    want = {"scenario_id": ((1, 16), torch.int32), "valid_sim": ((1, A, 11), torch.bool), "pos_sim": ((1, K, A, 80, 2), torch.float32),
            "z_sim": ((1, A, 11, 1), torch.float32), "yaw_sim": ((1, K, A, 80, 1), torch.float32), "valid_no_sim": ((1, 256, 11), torch.bool),
            "object_id_sim": ((1, A), torch.int64), "pos_no_sim": ((1, 256, 11, 2), torch.float32), "z_no_sim": ((1, 256, 11, 1), torch.float32),
            "yaw_no_sim": ((1, 256, 11, 1), torch.float32), "object_id_no_sim": ((1, 256), torch.int64)}
    assert list(wosac_data) == list(want), "the reference's keys, in its order"
    for key, (shape, dtype) in want.items():
        assert tuple(wosac_data[key].shape) == shape and wosac_data[key].dtype == dtype and wosac_data[key].is_cuda, key
    assert bool(torch.isfinite(wosac_data["pos_sim"]).all())
    assert float(wosac_data["yaw_sim"].min()) >= -math.pi - 4 * EPS * math.pi and float(wosac_data["yaw_sim"].max()) <= math.pi


def _wosac_case(tb, n_k):
    """As `wosac_case` of tests/golden/make_golden_post.py."""
    n_sc, n_ag, n_step = 2, 12, 30
    c = tb.synthetic.make_filter_case(n_sc=n_sc, n_k=n_k, n_ag=n_ag, n_step=n_step, seed=3)
    hist = tb.synthetic.to_history_batch(tb.synthetic.make_scene(n_sc, n_ag, 8, 2, seed=11))
    batch = {**{k: v for k, v in hist.items() if k.startswith("history/agent/")}, **tb.synthetic.make_wosac_keys(n_sc, n_ag, seed=0),
             "ref/ag_role": c["ag_role"]}
    return batch, c


def _wosac_forward(tb, n_k, w_road_edge=0.0):
    PP = import_module("trafficbots_amd.data_modules.wosac_post_processing")
    BUF = import_module("trafficbots_amd.utils.buffer")
    dev = torch.device(DEV)
    batch, c = _wosac_case(tb, n_k)
    post = PP.WOSACPostProcessing(step_gt=90, step_current=10, const_vel_z_sim=True, const_vel_no_sim=True, w_road_edge=w_road_edge,
                                  use_wosac_col=True)
    buf = BUF.RolloutBuffer(c["pred_pose"].shape[3], 10)
    buf.pred_pose = c["pred_pose"].to(dev)
    buf.violation = {k: c[k].to(dev) for k in ("collided", "collided_wosac", "run_road_edge")}
    out = post({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}, buf)
    return batch, c, post, {k: v.cpu() for k, v in out.items()}


def _on_circle(a, b):
    d = (a.double() - b.double()).abs()
    return torch.minimum(d, 2 * math.pi - d)


def test_wosac_forward_vs_reference(tb, golden_dir):
    """Pass-through keys and scenario_id exact. Positions within 4 eps (|center|_inf + |pos|_inf) - a rounding each for the two products,
    their sum and the translation; with scenario centres up to 10 km that is ~5e-3 m, the resolution of float32 global coordinates
    (the reference returns float32 too). Yaw within 4 eps 2 pi, compared on the circle: a value within that bound of the -pi / pi seam may
    land on either side."""
    ref = np.load(golden_dir / "wosac_forward.npz")
    batch, c, _, out = _wosac_forward(tb, 32)
    assert list(out) == list(ref.files)
    for k in ("scenario_id", "valid_sim", "z_sim", "valid_no_sim", "object_id_sim", "z_no_sim", "object_id_no_sim"):
        assert out[k].dtype == torch.from_numpy(ref[k]).dtype and torch.equal(out[k], torch.from_numpy(ref[k])), k
    assert "".join(chr(int(v)) for v in out["scenario_id"][0] if v > 0) == batch["scenario_id"][0]
    cmax = float(batch["scenario_center"].abs().max())
    for key, pmax in (("pos_sim", float(c["pred_pose"][..., :2].abs().max())), ("pos_no_sim", float(batch["history/agent_no_sim/pos"][..., :2].abs().max()))):
        tol = 4 * EPS * (cmax + pmax)
        worst = float((out[key].double() - torch.from_numpy(ref[key]).double()).abs().max())
        print(f"{key}: largest difference {worst:.3e} m (tolerance {tol:.3e})")
        assert out[key].shape == ref[key].shape and worst <= tol
    for key in ("yaw_sim", "yaw_no_sim"):
        tol = 4 * EPS * 2 * math.pi
        worst = float(_on_circle(out[key], torch.from_numpy(ref[key])).max())
        print(f"{key}: largest difference on the circle {worst:.3e} rad (tolerance {tol:.3e})")
        assert out[key].shape == ref[key].shape and worst <= tol
        assert float(out[key].min()) >= -math.pi - tol and float(out[key].max()) <= math.pi + tol


def test_wosac_forward_on_filtered_futures(tb):
    """K = 48 > 32: the records are those of the futures `_filter_futures` kept (dense gather instead of a slice of the log), same
    transform - here against its float64 expression."""
    batch, c, post, out = _wosac_forward(tb, 48, w_road_edge=0.5)
    idx = post.last_idx.cpu().long()
    assert out["pos_sim"].shape == (2, 32, 12, 20, 2) and out["yaw_sim"].shape == (2, 32, 12, 20, 1)
    kept = torch.stack([c["pred_pose"][s, idx[s]] for s in range(2)])[:, :, :, 10:].double()
    th, ctr = batch["scenario_yaw"].double().view(2, 1, 1, 1), batch["scenario_center"].double().view(2, 1, 1, 1, 2)
    x, y = kept[..., 0], kept[..., 1]
    want = torch.stack([x * th.cos() - y * th.sin(), x * th.sin() + y * th.cos()], -1) + ctr
    tol = 4 * EPS * (float(ctr.abs().max()) + float(kept[..., :2].abs().max()))
    assert float((out["pos_sim"].double() - want).abs().max()) <= tol
    # (make_filter_case draws yaw from 30 * randn - tens of radians, unlike a rollout's: the float32 sums yaw + scenario_yaw + pi round
    #  at THAT magnitude before the wrap, so the bound is 4 eps (|yaw|_inf + 2 pi) here, not the 4 eps 2 pi of wrapped inputs)
    wrapped = torch.remainder(kept[..., 2:3] + th.unsqueeze(-1) + math.pi, 2 * math.pi) - math.pi
    assert float(_on_circle(out["yaw_sim"], wrapped).max()) <= 4 * EPS * (float(kept[..., 2].abs().max()) + 2 * math.pi)
