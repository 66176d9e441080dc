#!/usr/bin/env python
"""Generate tests/golden/womd_post.npz and tests/golden/wosac_forward.npz by running the REFERENCE's WOMDPostProcessing.forward and
WOSACPostProcessing.forward (the checkout make_golden.py imports) on seeded inputs (`synthetic.make_womd_case`, `make_filter_case`,
`make_scene`, `make_wosac_keys` - ours, shipped). Container-only tooling, like make_golden.py whose shims it uses; the fixtures
hold the reference's outputs only (plus, as a JSON string, the arguments each case was made with).

Per WOMD case: the future each returned mode was taken from (the returned trajectories matched back to their future, as
`gen_filter` does), the float32 scores, `bound` = the largest difference between the reference run in float32 and in float64 (what
a float32 implementation with another summation order may be expected to differ by, before the test's factor 8), and per agent the
DECISION MARGINS in float64: `margin_d` = the smallest |distance - threshold| over the distance comparisons the configuration
consults (the pairs of kept modes for mpa_nms, the rows of the picks for mtr_nms), `margin_s` = the smallest relative gap between two
scores whose order decides something (k-th vs (k+1)-th score, the pairs of kept modes, every comparison against a suppressed 1e-3,
first vs second maximum of every mtr_nms pick). The margins come from `trace_agent` below, a float64 restatement of the reference's
semantics that must reproduce the reference's float64 run exactly (asserted). Agents below 1e-4 m / 1e-5 relative are left out
of the index comparison by the test; at most 5 % of a case's agents may be (asserted here: pick another seed, not another cap).

    python tests/golden/make_golden_post.py
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import install_shims, npz, tb  # noqa: E402

STEP_GT, STEP_CURRENT = 90, 10
MARGIN_D, MARGIN_S, MAX_LEFT_OUT = 1e-4, 1e-5, 0.05
BASE = dict(k_pred=6, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0], mtr_nms_thresh=[], aggr_thresh=[], n_iter_em=3, use_ade=True)
# name -> (make_womd_case arguments, configuration overrides, scores given?)
WOMD_CASES = {
    "default": (dict(n_sc=4, n_k=32, n_ag=64, n_step=80, seed=1), {}, True),
    "submission": (dict(n_sc=2, n_k=128, n_ag=128, n_step=80, seed=2), {}, True),
    "fde": (dict(n_sc=4, n_k=32, n_ag=64, n_step=80, seed=3), dict(use_ade=False), True),
    "mtr32": (dict(n_sc=4, n_k=32, n_ag=64, n_step=80, seed=4), dict(mtr_nms_thresh=[2.5, 1.0, 1.5], mpa_nms_thresh=[]), True),
    "mtr48": (dict(n_sc=3, n_k=48, n_ag=20, n_step=80, seed=5), dict(mtr_nms_thresh=[2.5, 1.0, 1.5], mpa_nms_thresh=[]), True),
    "per_type_temp": (dict(n_sc=4, n_k=32, n_ag=64, n_step=80, seed=6), dict(mpa_nms_thresh=[2.0, 1.0, 1.5], score_temperature=0.5), True),
    "replay_k1": (dict(n_sc=4, n_k=1, n_ag=64, n_step=80, seed=7), {}, False),
    "k6": (dict(n_sc=4, n_k=6, n_ag=64, n_step=80, seed=8), {}, True),
}


def rel_gap(a: float, b: float) -> float:
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def trace_agent(xy, logp, ty, cfg):
    """float64 restatement of womd_post_processing.py:37-182 for one agent. xy [K, T, 2], logp [K], ty [3] bool
    -> (kept future indices, scores, margin_d, margin_s)."""
    K, k_pred = xy.shape[0], cfg["k_pred"]
    md, ms = [np.inf], [np.inf]

    def thresh(t3):  # float32 sum as the reference forms it
        return float(sum((np.float32(bool(ty[i])) * np.float32(t3[i]) for i in range(3)), np.float32(0)))

    def dist(i, j):
        d = np.linalg.norm(xy[i] - xy[j], axis=-1)
        return float(d.mean() if cfg["use_ade"] else d[-1])

    def within(i, j, thr):
        d = dist(i, j)
        if i != j:  # (the distance of a future to itself is 0 in every precision)
            md.append(abs(d - thr))
        return d < thr

    s = np.exp(logp - logp.max())
    s = s / s.sum()
    idx = list(range(K))
    if K > k_pred:
        if len(cfg["mtr_nms_thresh"]) > 0:
            thr, work, idx = thresh(cfg["mtr_nms_thresh"]), s.copy(), []
            for _ in range(k_pred):
                order = np.argsort(-work, kind="stable")
                ms.append(rel_gap(work[order[0]], work[order[1]]))
                p = int(order[0])
                for j in range(K):
                    work[j] *= float(np.float32(0.01)) if within(p, j, thr) else 1.0
                work[p] = -1.0
                idx.append(p)
        else:
            order = np.argsort(-s, kind="stable")
            ms.append(rel_gap(s[order[k_pred - 1]], s[order[k_pred]]))
            idx = [int(i) for i in order[:k_pred]]
        s = s[idx] / s[idx].sum()
    k = len(idx)
    if len(cfg["mpa_nms_thresh"]) > 0:
        thr = thresh(cfg["mpa_nms_thresh"])
        w = np.array([[within(idx[a], idx[b], thr) for b in range(k)] for a in range(k)])
        for a in range(k):
            for b in range(a):
                ms.append(rel_gap(s[a], s[b]))
        for m in np.argsort(-s, kind="stable"):
            for j in range(k):
                if j != m and w[m, j]:
                    ms.append(rel_gap(s[j], s[m]))
            if any(w[m, j] and s[j] > s[m] for j in range(k)):
                s[m] = 1e-3
        s = s / s.sum()
    if cfg["score_temperature"] > 0:
        z = np.log(s) / cfg["score_temperature"]
        s = np.exp(z - z.max())
        s = s / s.sum()
    return idx, s, min(md), min(ms)


def match_futures(trajs, out_trajs):
    """trajs [n_sc, K, A, T, 3], out_trajs [n_sc, A, k, n, 3] -> [n_sc, A, k] the future each returned mode equals."""
    cand = trajs.transpose(1, 2)[:, :, :, 4:STEP_GT - STEP_CURRENT:5]  # [n_sc, A, K, n, 3]
    eq = (cand.unsqueeze(2) == out_trajs.unsqueeze(3)).flatten(4).all(-1)  # [n_sc, A, k, K]
    assert (eq.sum(-1) == 1).all(), "a returned mode matches no / several futures"
    return eq.float().argmax(-1)


def gen_womd():
    from data_modules.womd_post_processing import WOMDPostProcessing

    out = {}
    for name, (case_kw, over, with_scores) in WOMD_CASES.items():
        cfg = {**BASE, **over}
        c = tb.synthetic.make_womd_case(**case_kw)
        pp = WOMDPostProcessing(step_gt=STEP_GT, step_current=STEP_CURRENT, **cfg)
        sc = c["log_prob"] if with_scores else None
        r32 = pp(c["ag_type"], c["trajs"].clone(), None if sc is None else sc.clone())
        r64 = pp(c["ag_type"], c["trajs"].double(), None if sc is None else sc.double())
        i32, i64 = match_futures(c["trajs"], r32["trajs"]), match_futures(c["trajs"].double(), r64["trajs"])
        n_sc, A, k = i32.shape
        md, ms = np.zeros((n_sc, A)), np.zeros((n_sc, A))
        xy = c["trajs"][..., :2].double().numpy()
        lp = (c["log_prob"] if with_scores else torch.zeros_like(c["log_prob"])).double().numpy()
        for s in range(n_sc):
            for a in range(A):
                idx, scr, md[s, a], ms[s, a] = trace_agent(xy[s, :, a], lp[s, :, a], c["ag_type"][s, a].numpy(), cfg)
                # the restatement IS the reference in float64: same futures (as a set: topk(sorted=False) fixes no order), same scores
                ref = {int(i): float(v) for i, v in zip(i64[s, a], r64["scores"][s, a])}
                assert sorted(idx) == sorted(ref), (name, s, a, idx, sorted(ref))
                assert max(abs(ref[i] - v) for i, v in zip(idx, scr)) < 1e-12, (name, s, a)
        safe = (md >= MARGIN_D) & (ms >= MARGIN_S)
        left_out = 1.0 - safe.mean()
        assert left_out <= MAX_LEFT_OUT, f"{name}: {left_out:.3f} of the agents below the decision margins - pick another seed"
        # float32 vs float64 reference: same kept sets on the safe agents, and the largest score difference after matching by future
        same = (i32.sort(-1)[0] == i64.sort(-1)[0]).all(-1).numpy()
        assert same[safe].all(), f"{name}: the reference's float32 and float64 runs keep different futures on an agent with safe margins"
        o32, o64 = i32.argsort(-1), i64.argsort(-1)
        diff = (r32["scores"].gather(-1, o32).double() - r64["scores"].gather(-1, o64)).abs().numpy()
        bound = float(diff[same].max())
        floor = float((r32["scores"] < 5e-3).float().mean())
        print(f"{name}: kept {tuple(r32['trajs'].shape)}, left out {left_out:.4f}, f32-f64 bound {bound:.3e}, scores < 5e-3: {floor:.3f}")
        out.update({f"{name}_idx": i32.numpy().astype(np.int16), f"{name}_scores": r32["scores"], f"{name}_margin_d": md,
                    f"{name}_margin_s": ms, f"{name}_bound": np.float64(bound)})
    # the cases travel with their results: the test rebuilds the inputs from these arguments
    out["cases"] = json.dumps({n: dict(case=c, cfg={**BASE, **o}, with_scores=w) for n, (c, o, w) in WOMD_CASES.items()})
    npz("womd_post.npz", **out)


def wosac_case(n_k):
    """Inputs of WOSACPostProcessing.forward: a rollout log of `make_filter_case`, the history keys of a small `make_scene`, the
    scenario keys of `make_wosac_keys`. -> (batch, RolloutBuffer fields as a dict)."""
    n_sc, n_ag, n_step = 2, 12, 30
    c = tb.synthetic.make_filter_case(n_sc=n_sc, n_k=n_k, n_ag=n_ag, n_step=n_step, seed=3)
    hist = tb.synthetic.to_history_batch(tb.synthetic.make_scene(n_sc, n_ag, 8, 2, seed=11))
    batch = {**{k: v for k, v in hist.items() if k.startswith("history/agent/")}, **tb.synthetic.make_wosac_keys(n_sc, n_ag, seed=0),
             "ref/ag_role": c["ag_role"]}
    return batch, c


def gen_wosac():
    from data_modules.wosac_post_processing import WOSACPostProcessing
    from utils.buffer import RolloutBuffer

    batch, c = wosac_case(32)
    pp = WOSACPostProcessing(step_gt=STEP_GT, step_current=STEP_CURRENT, const_vel_z_sim=True, const_vel_no_sim=True, w_road_edge=0.0,
                             use_wosac_col=True)
    buf = RolloutBuffer(c["pred_pose"].shape[3], STEP_CURRENT)
    buf.pred_pose = c["pred_pose"]
    buf.violation = {k: c[k] for k in ("collided", "collided_wosac", "run_road_edge")}
    out = pp(batch, buf)
    print({k: (tuple(v.shape), str(v.dtype)) for k, v in out.items()})
    npz("wosac_forward.npz", **out)


if __name__ == "__main__":
    install_shims()
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["womd", "wosac"]
    if "wosac" in which:
        gen_wosac()
    if "womd" in which:
        gen_womd()
