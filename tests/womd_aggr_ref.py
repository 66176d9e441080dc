"""A float64 restatement, per (scene, agent), of `WOMDPostProcessing.forward` with `aggr_thresh` set (the reference's
data_modules/womd_post_processing.py:37-72 and traj_aggr :178-278) on numpy arrays. No package code, CPU only: what
tests/golden/make_golden_aggr.py proves equal to the reference's float64 run (and takes the decision margins from), what
tests/test_womd_aggr_host.py reproduces the fixture with, and what tests/test_hip_womd_aggr.py compares the kernel against where the
fixture has no case.

Rules the reference leaves to torch, stated here: every maximum / minimum is the FIRST one (`torch.max` / `torch.min` / `argmax`
return the first index of equal values on the CPU), empty clusters are repaired in ascending cluster index (`torch.where` lists them
so), the donor gives its first count // 2 members in ascending future index.

Decision margins (float64; np.inf where nothing was decided):
  d   the smallest of |distance - threshold| over the rows of the seeds and the pairs of final centres mpa_nms consults, and of the gap
      between the nearest and the second-nearest centre of every future in every E-step;
  s   the smallest relative gap between first and second maximum of every pick, and between the scores mpa_nms orders / compares;
  c   the smallest gap between the largest and the second-largest cluster's member count at a repair.
"""
import numpy as np

SAMPLE_FIRST, SAMPLE_STRIDE = 4, 5
MARGIN_D, MARGIN_S, MARGIN_C = 1e-4, 1e-5, 1  # the project's decision margins (tests/golden/make_golden_post.py)


def rel_gap(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def type_thresh(ty, t3):
    """The float32 sum ((0 + ty0 a0) + ty1 a1) + ty2 a2 as a Python float."""
    acc = np.float32(0)
    for i in range(3):
        acc = np.float32(acc + np.float32(bool(ty[i])) * np.float32(t3[i]))
    return float(acc)


def traj_dist(a, b, use_ade):
    """a, b [..., T, 2] (broadcast) -> the mean over the steps of the xy distance, or the last step's."""
    d = np.linalg.norm(a - b, axis=-1)
    return d.mean(-1) if use_ade else d[..., -1]


def aggr_agent(tr, logp, ty, cfg, n_sample_end):
    """tr [K, T, 3] float64 (x, y, yaw), logp [K] or None, ty [3] bool, cfg: k_pred, aggr_thresh, n_iter_em, use_ade, mpa_nms_thresh,
    score_temperature; K > k_pred. -> dict: trajs [k, n_out, 3] the centres at the sampled steps, scores [k], seeds [k], centres
    [k, T, 3], assign [K] of the last round (or None), n_repair, margin_d, margin_s, margin_c."""
    tr = np.asarray(tr, dtype=np.float64)
    K, k, use_ade = tr.shape[0], cfg["k_pred"], cfg["use_ade"]
    assert K > k
    xy = tr[..., :2]
    md, ms, mc = [np.inf], [np.inf], [np.inf]
    lp = np.zeros(K) if logp is None else np.asarray(logp, dtype=np.float64)
    s = np.exp(lp - lp.max())
    s = s / s.sum()

    # seeds (:220-232)
    thr, work, seeds = type_thresh(ty, cfg["aggr_thresh"]), s.copy(), []
    for _ in range(k):
        order = np.argsort(-work, kind="stable")
        p = int(order[0])
        ms.append(rel_gap(work[order[0]], work[order[1]]))
        d = traj_dist(xy[p][None], xy, use_ade)
        md.append(np.abs(np.delete(d, p) - thr).min())  # (the distance of a future to itself is 0 in every precision)
        work = work * np.where(d < thr, float(np.float32(0.1)), 1.0)
        work[p] -= 1.0
        seeds.append(p)
    centres, cs = tr[seeds].copy(), s[seeds].copy()

    # EM (:242-275)
    assign, n_repair = None, 0
    for _ in range(cfg["n_iter_em"]):
        dm = traj_dist(xy[:, None], centres[None, :, :, :2], use_ade)  # [K, k]
        assign = dm.argmin(-1)
        two = np.sort(dm, axis=-1)[:, :2]
        md.append((two[:, 1] - two[:, 0]).min())
        n = np.bincount(assign, minlength=k)
        for c in np.flatnonzero(n == 0):
            top = np.sort(n)[::-1]
            mc.append(top[0] - top[1])
            big = int(n.argmax())
            assign[np.flatnonzero(assign == big)[: n[big] // 2]] = c
            n = np.bincount(assign, minlength=k)
            n_repair += 1
        for c in range(k):
            centres[c] = tr[assign == c].mean(0)
            cs[c] = s[assign == c].mean()
    sc = cs / cs.sum()

    # mpa_nms on the centres (:74-105)
    if len(cfg["mpa_nms_thresh"]) > 0:
        thr = type_thresh(ty, cfg["mpa_nms_thresh"])
        d = traj_dist(centres[:, None, :, :2], centres[None, :, :, :2], use_ade)
        md.append(np.abs(d - thr)[~np.eye(k, dtype=bool)].min())
        w = d < thr
        ms.extend(rel_gap(sc[a], sc[b]) for a in range(k) for b in range(a))
        for m in np.argsort(-sc, kind="stable"):
            ms.extend(rel_gap(sc[j], sc[m]) for j in range(k) if j != m and w[m, j])
            if any(w[m, j] and sc[j] > sc[m] for j in range(k)):
                sc[m] = 1e-3
        sc = sc / sc.sum()
    if cfg["score_temperature"] > 0:  # :69-70
        z = np.log(sc) / cfg["score_temperature"]
        sc = np.exp(z - z.max())
        sc = sc / sc.sum()
    return dict(trajs=centres[:, SAMPLE_FIRST:n_sample_end:SAMPLE_STRIDE], scores=sc, seeds=np.asarray(seeds), centres=centres, assign=assign,
                n_repair=n_repair, margin_d=float(min(md)), margin_s=float(min(ms)), margin_c=float(min(mc)))


def aggr_case(trajs, log_prob, ag_type, cfg, n_sample_end):
    """trajs [n_sc, K, A, T, 3], log_prob [n_sc, K, A] or None, ag_type [n_sc, A, 3] (numpy) -> dict of arrays stacked over [n_sc, A]:
    trajs, scores, seeds, n_repair, margin_d, margin_s, margin_c."""
    n_sc, K, A = trajs.shape[:3]
    keys = ("trajs", "scores", "seeds", "n_repair", "margin_d", "margin_s", "margin_c")
    rows = [[aggr_agent(trajs[s, :, a], None if log_prob is None else log_prob[s, :, a], ag_type[s, a], cfg, n_sample_end) for a in range(A)]
            for s in range(n_sc)]
    return {key: np.stack([np.stack([np.asarray(r[key]) for r in row]) for row in rows]) for key in keys}


def safe_agents(margin_d, margin_s, margin_c):
    return (margin_d >= MARGIN_D) & (margin_s >= MARGIN_S) & (margin_c >= MARGIN_C)
