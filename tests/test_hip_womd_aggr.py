"""GPU tests of the trajectory aggregation of the WOMD post-processing: `WOMDPostProcessing.forward` with `aggr_thresh` set
(tbx_womd_aggr) against the reference's outputs in tests/golden/womd_aggr.npz, its first-index rules against the float64 restatement
(tests/womd_aggr_ref.py), its in-place read of a time slice of a longer log, repeatability and graph capture, its routing (K <= k_pred,
aggr_thresh over mtr_nms_thresh) and `test_step` with the switch turned on.

Tolerances: on every agent whose decision margins (recorded by the fixture's generator in float64) are at least 1e-4 m, 1e-5 relative
and one member - at most 5 % of a case's agents may fall below -, trajectories and scores within 8 x the largest float32 - float64
difference of the reference itself on that case (the factor of tests/test_hip_womd_post.py over the same kind of bound), the seeds exact."""
import json
from importlib import import_module

import numpy as np
import pytest
import torch

import womd_aggr_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23
CASES = ("ade32", "fde48", "k7", "k128", "iter0", "temp_type", "t91", "repair_ade", "repair_fde")
AGGR = [2.5, 1.0, 1.5]
BASE = dict(k_pred=6, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0], mtr_nms_thresh=[], aggr_thresh=AGGR, n_iter_em=3, use_ade=True,
            step_gt=90, step_current=10)


def _pp(**over):
    P = import_module("trafficbots_amd.data_modules.womd_post_processing")
    return P.WOMDPostProcessing(**{**BASE, **over})


def _run(pp, c, scores=True, trajs=None):
    dev = torch.device(DEV)
    out = pp(c["ag_type"].to(dev), c["trajs"].to(dev) if trajs is None else trajs, c["log_prob"].to(dev) if scores else None)
    return out["trajs"], out["scores"], pp.last_idx


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                                          y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "womd_aggr.npz")


@pytest.fixture(scope="module")
def ade32(tb):
    return tb.synthetic.make_womd_case(n_sc=2, n_k=32, n_ag=24, n_step=80, seed=11)


@pytest.mark.parametrize("name", CASES)
def test_aggr_vs_reference(tb, golden, name):
    """Every case of the fixture: ADE at K = 32, FDE at K = 48 (a partial wave), K = k_pred + 1, K = 128, n_iter_em = 0, per-type mpa_nms
    with a temperature, 91 steps at K = 128 (the LDS maximum) and the constructed case whose second round empties a cluster, ADE and FDE."""
    spec = json.loads(str(golden["cases"]))[name]
    c = getattr(tb.synthetic, spec["helper"])(**spec["case"])
    n_sc, K, A, T = c["trajs"].shape[:4]
    pp = _pp(**spec["cfg"], step_gt=10 + T)
    trajs, scores, idx = (t.cpu() for t in _run(pp, c))
    n_out = len(range(4, T, 5))
    assert trajs.shape == (n_sc, A, 6, n_out, 3) and scores.shape == (n_sc, A, 6) and idx.shape == (n_sc, A, 6)
    assert trajs.dtype == scores.dtype == torch.float32 and idx.dtype == torch.int32
    safe = torch.from_numpy(R.safe_agents(golden[f"{name}_margin_d"], golden[f"{name}_margin_s"], golden[f"{name}_margin_c"]))
    left_out = 1.0 - float(safe.float().mean())
    tol_t, tol_s = 8.0 * float(golden[f"{name}_bound_trajs"]), 8.0 * float(golden[f"{name}_bound_scores"])
    dt = float((trajs.double() - torch.from_numpy(golden[f"{name}_trajs"]).double()).abs()[safe].max())
    ds = float((scores.double() - torch.from_numpy(golden[f"{name}_scores"]).double()).abs()[safe].max())
    seeds_equal = (idx.long() == torch.from_numpy(golden[f"{name}_seeds"].astype(np.int64))).all(-1)
    print(f"{name}: left out {left_out:.4f}, seeds equal on {int((seeds_equal & safe).sum())}/{int(safe.sum())} safe agents, largest "
          f"difference {dt:.3e} m (tolerance {tol_t:.3e}), scores {ds:.3e} (tolerance {tol_s:.3e})")
    assert left_out <= 0.05
    assert bool(seeds_equal[safe].all())
    assert dt <= tol_t
    assert ds <= tol_s
    assert all(len(set(r.tolist())) == 6 for r in idx.flatten(0, 1)), "a future picked twice"
    torch.testing.assert_close(scores.sum(-1), torch.ones(n_sc, A), rtol=0, atol=4 * EPS)
    if spec["cfg"]["n_iter_em"] == 0:  # the picks, bit for bit, on every agent
        src = c["trajs"].transpose(1, 2)[:, :, :, 4:T:5]
        assert torch.equal(trajs, src.gather(2, idx.long()[..., None, None].expand(-1, -1, -1, n_out, 3)))


def test_time_slice_of_a_longer_log_is_read_in_place(tb, golden):
    """The t91 case as the view log[..., 11:, :] of a [n_sc, K, A, 102, 3] log (t_start > 0, ld_t > n_step): handed to the kernel as it
    lies in memory, and equal to the call on a contiguous copy bit for bit."""
    spec = json.loads(str(golden["cases"]))["t91"]
    c = tb.synthetic.make_womd_case(**spec["case"])
    dev = torch.device(DEV)
    log = torch.randn(1, 128, 4, 102, 3, generator=torch.Generator().manual_seed(0)).to(dev) * 50
    log[:, :, :, 11:] = c["trajs"].to(dev)
    view = log[:, :, :, 11:]
    assert not view.is_contiguous()
    pp = _pp(**spec["cfg"], step_gt=101)
    hip = import_module("trafficbots_amd.hip")
    seen, real = [], hip.womd_aggr
    hip.womd_aggr = lambda pose, *a, **k: (seen.append((pose.data_ptr(), a[4], a[5])), real(pose, *a, **k))[1]
    try:
        got = _run(pp, c, trajs=view)
    finally:
        hip.womd_aggr = real
    assert seen == [(view.data_ptr(), 0, 91)], "the kernel was handed a copy of the log"
    assert hip.log_row_steps(view) == 102
    want = _run(pp, c, trajs=view.contiguous())
    assert _same(got, want)


def test_without_scores_every_pick_is_the_first_index(tb, ade32):
    """scores=None: all softmax scores equal, so every pick and every suppression tie falls to the lower future index - compared with the
    float64 restatement (the fixture has no such case). mpa_nms off: centre scores that are means of equal values differ by roundings
    only, and their order would decide it. Agents whose distance / count margins are safe; the score margin is 0 by construction.
    Trajectories: a float32 sum of n <= K members in sequence and one division err by at most n u max|x|, u = 2^-24 (the inputs are
    float32 on both sides); scores are computed in float64 and rounded once: u."""
    cfg = dict(k_pred=6, aggr_thresh=AGGR, n_iter_em=3, use_ade=True, mpa_nms_thresh=[], score_temperature=-1)
    want = R.aggr_case(ade32["trajs"].double().numpy(), None, ade32["ag_type"].numpy(), cfg, 80)
    trajs, scores, idx = (t.cpu() for t in _run(_pp(mpa_nms_thresh=[]), ade32, scores=False))
    safe = torch.from_numpy((want["margin_d"] >= R.MARGIN_D) & (want["margin_c"] >= R.MARGIN_C))
    assert float(safe.float().mean()) >= 0.95
    assert torch.equal(idx.long()[safe], torch.from_numpy(want["seeds"]).long()[safe])
    untyped = ~ade32["ag_type"].any(-1)
    assert bool(untyped.any()) and bool((idx[untyped] == torch.arange(6, dtype=torch.int32)).all()), "threshold 0: nothing suppressed"
    tol = 32 * 2.0 ** -24 * float(ade32["trajs"].abs().max())
    dt = float((trajs.double() - torch.from_numpy(want["trajs"])).abs()[safe].max())
    ds = float((scores.double() - torch.from_numpy(want["scores"])).abs()[safe].max())
    print(f"scores=None: {int(safe.sum())}/{safe.numel()} agents, largest difference {dt:.3e} m (tolerance {tol:.3e}), scores {ds:.3e}")
    assert dt <= tol and ds <= 2.0 ** -24


def test_two_calls_and_two_graph_replays_leave_the_same_bytes(tb, ade32):
    pp = _pp()
    dev = torch.device(DEV)
    ty, tr, lp = ade32["ag_type"].to(dev), ade32["trajs"].to(dev), ade32["log_prob"].to(dev)
    first = _run(pp, ade32)
    assert _same(first, _run(pp, ade32))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = pp(ty, tr, lp)
        cap_idx = pp.last_idx
    for _ in range(2):
        cap["trajs"].fill_(float("nan"))
        cap["scores"].fill_(float("nan"))
        cap_idx.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert _same((cap["trajs"], cap["scores"], cap_idx), first), "every output element is written by every call"
    del g


def test_routing_of_the_three_reductions(tb, ade32):
    """K <= k_pred with aggr_thresh set: no reduction, the module without it bit for bit (K = 6 and K = 4). aggr_thresh together with
    mtr_nms_thresh: aggr_thresh wins (womd_post_processing.py:56-61), and differs from mtr_nms alone."""
    for K in (6, 4):
        c = {"trajs": ade32["trajs"][:, :K].contiguous(), "log_prob": ade32["log_prob"][:, :K].contiguous(), "ag_type": ade32["ag_type"]}
        assert _same(_run(_pp(), c), _run(_pp(aggr_thresh=[]), c))
    both, alone, mtr = _run(_pp(mtr_nms_thresh=AGGR), ade32), _run(_pp(), ade32), _run(_pp(aggr_thresh=[], mtr_nms_thresh=AGGR), ade32)
    assert _same(both, alone)
    assert not torch.equal(alone[0], mtr[0]), "cluster means, not picked futures"


def test_test_step_with_the_switch_on(tb):
    """At the scene of tests/test_hip_test_step.py with 8 joint futures (> k_pred) and womd_post_processing.aggr_thresh set: test_step
    leaves on `last_womd_joint_future_pred` what a direct call of a module of the same configuration returns on the same buffer."""
    dev = torch.device(DEV)
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg(n_joint_future_wosac=8)
    scfg["womd_post_processing"] = {**scfg["womd_post_processing"], "aggr_thresh": AGGR}
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    wm = wm.to(dev).eval()
    assert wm.womd_post_processing.aggr_thresh == AGGR and wm.womd_post_processing.n_iter_em == 3
    raw = tb.synthetic.make_scene(1, 8, 64, 8, seed=31)
    batch = {**tb.synthetic.to_history_batch(raw), **tb.synthetic.make_wosac_keys(1, 8, seed=2, n_ag_no_sim=20)}
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    calls = []
    hook = wm.womd_post_processing.register_forward_pre_hook(lambda mod, args, kwargs: calls.append(kwargs), with_kwargs=True)
    torch.manual_seed(7)
    wm.test_step(batch, 0)
    hook.remove()
    assert len(calls) == 1 and calls[0]["trajs"].shape == (1, 8, 8, 80, 3) and not calls[0]["trajs"].is_contiguous()
    got = wm.last_womd_joint_future_pred
    assert got["trajs"].shape == (1, 8, 6, 16, 3) and got["scores"].shape == (1, 8, 6)
    direct = _pp()
    want = direct(**calls[0])
    assert _same((got["trajs"], got["scores"], wm.womd_post_processing.last_idx), (want["trajs"], want["scores"], direct.last_idx))
    picked = _pp(aggr_thresh=[])(**calls[0])
    assert not torch.equal(got["trajs"], picked["trajs"]), "8 futures in 6 clusters: some mode is a mean of several"
    torch.testing.assert_close(got["scores"].sum(-1), torch.ones(1, 8, device=DEV), rtol=0, atol=4 * EPS)
    del wm
