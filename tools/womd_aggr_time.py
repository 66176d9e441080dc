"""Time of `WOMDPostProcessing.forward` with `aggr_thresh` set (greedy seeds + n_iter_em rounds of k-means over whole trajectories + mpa_nms)
at 4 x 32 x 64 x 80 and 2 x 128 x 128 x 80 (scenes x futures x agents x steps):
  new    tbx_womd_aggr, one launch, one workgroup per (scene, agent)
  torch  the same result from torch ops on the device, vectorised over scenes and agents, float32: dense [n_sc, A, K, K] and
         [n_sc, A, K, k] distance tensors as the reference forms them, the empty-cluster repair and the mpa_nms loop as k masked steps
         each - no host read anywhere (the reference itself branches on the host per empty cluster and per mode)
  mtr    tbx_womd_modes with mtr_nms at the same shape: the in-project yardstick (seeds of the same kind, no k-means)
  new_iter0, new_iter1  the new call with n_iter_em = 0 and 1 instead of 3: staging + seeds + outputs, and the cost of a round
Device events around back-to-back iterations after warm-up, the paths alternating, several rounds; medians.
    python tools/womd_aggr_time.py [--iters 20] [--rounds 5]"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import torch
from importlib import import_module
from __graft_entry__ import load_package

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

tb = load_package()
P = import_module("trafficbots_amd.data_modules.womd_post_processing")
dev = torch.device("cuda:0")
CFG = dict(k_pred=6, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0], n_iter_em=3, use_ade=True, step_gt=90, step_current=10)
AGGR = [2.5, 1.0, 1.5]


def type_thresh(ag_type, t3):
    thr = 0
    for i in range(3):
        thr = thr + ag_type[:, :, i] * t3[i]
    return thr[:, :, None, None]  # [n_sc, A, 1, 1] float32


def ade(a, b):
    """a [n_sc, A, I, 1, T, 2], b [n_sc, A, 1, J, T, 2] -> [n_sc, A, I, J]"""
    return torch.linalg.vector_norm(a - b, dim=-1).mean(-1)


def by_torch(ag_type, trajs, log_prob):
    trajs = trajs.transpose(1, 2)  # [n_sc, A, K, T, 3]
    n_sc, A, K = trajs.shape[:3]
    k = CFG["k_pred"]
    s = log_prob.transpose(1, 2).softmax(-1)
    xy = trajs[..., :2]
    within = ade(xy.unsqueeze(3), xy.unsqueeze(2)) < type_thresh(ag_type, AGGR)
    work, seeds = s.clone(), []
    for _ in range(k):
        p = work.argmax(-1, keepdim=True)  # [n_sc, A, 1]
        near = within.gather(2, p[..., None].expand(-1, -1, -1, K)).squeeze(2)
        work = work * torch.where(near, 0.1, 1.0)
        work.scatter_add_(-1, p, -torch.ones_like(p, dtype=work.dtype))
        seeds.append(p)
    seeds = torch.cat(seeds, -1)  # [n_sc, A, k]
    centres = trajs.gather(2, seeds[..., None, None].expand(-1, -1, -1, *trajs.shape[3:]))
    cs = s.gather(-1, seeds)
    ar = torch.arange(k, device=trajs.device)
    for _ in range(CFG["n_iter_em"]):
        assign = ade(xy.unsqueeze(3), centres[..., :2].unsqueeze(2)).argmin(-1)  # [n_sc, A, K]
        onehot = assign[..., None] == ar  # [n_sc, A, K, k]
        empty0 = onehot.sum(2) == 0
        for c in range(k):  # the repair, masked: cluster c takes the first count // 2 members of the largest one where it was empty
            n = onehot.sum(2)
            cnt, big = n.max(-1, keepdim=True)
            of_big = onehot.gather(3, big[:, :, None].expand(-1, -1, K, -1)).squeeze(3)
            move = of_big & (of_big.cumsum(-1) <= cnt // 2) & empty0[..., c, None]
            assign = torch.where(move, c, assign)
            onehot = assign[..., None] == ar
        w = onehot.to(trajs.dtype)
        n = w.sum(2)
        centres = torch.einsum("sajc,sajtd->sactd", w, trajs) / n[..., None, None]
        cs = torch.einsum("sajc,saj->sac", w, s) / n
    v = cs / cs.sum(-1, keepdim=True)
    cxy = centres[..., :2]
    wd = ade(cxy.unsqueeze(3), cxy.unsqueeze(2)) < type_thresh(ag_type, CFG["mpa_nms_thresh"])
    for m in v.argsort(dim=-1, descending=True, stable=True).unbind(-1):  # mpa_nms, masked: one visit per rank
        m = m[..., None]
        vm = v.gather(-1, m)
        hit = (wd.gather(2, m[..., None].expand(-1, -1, -1, k)).squeeze(2) & (v > vm)).any(-1, keepdim=True)
        v = v.scatter(-1, m, torch.where(hit, torch.full_like(vm, 1e-3), vm))
    v = v / v.sum(-1, keepdim=True)
    return {"trajs": centres[:, :, :, 4:80:5], "scores": v, "seeds": seeds}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.iters  # us per iteration


result = []
for n_sc, K, A in ((4, 32, 64), (2, 128, 128)):
    c = {k: v.to(dev) for k, v in tb.synthetic.make_womd_case(n_sc=n_sc, n_k=K, n_ag=A, n_step=80, seed=1).items()}
    pp_aggr = P.WOMDPostProcessing(aggr_thresh=AGGR, mtr_nms_thresh=[], **CFG)
    pp_mtr = P.WOMDPostProcessing(aggr_thresh=[], mtr_nms_thresh=AGGR, **CFG)
    pp_iter = [P.WOMDPostProcessing(aggr_thresh=AGGR, mtr_nms_thresh=[], **{**CFG, "n_iter_em": n}) for n in (0, 1)]
    paths = {"new": lambda: pp_aggr(c["ag_type"], c["trajs"], c["log_prob"]), "torch": lambda: by_torch(c["ag_type"], c["trajs"], c["log_prob"]),
             "mtr": lambda: pp_mtr(c["ag_type"], c["trajs"], c["log_prob"]),
             # the new call with 0 and 1 rounds instead of 3: what staging + seeds + outputs cost, and what a round costs
             "new_iter0": lambda: pp_iter[0](c["ag_type"], c["trajs"], c["log_prob"]), "new_iter1": lambda: pp_iter[1](c["ag_type"], c["trajs"], c["log_prob"])}
    r, ref = paths["new"](), paths["torch"]()
    same = (pp_aggr.last_idx.long() == ref["seeds"]).all(-1)  # (float32 against float32: an agent near a threshold may differ)
    agree = dict(agents=int(same.numel()), seeds_equal=int(same.sum()),
                 max_abs_trajs=float((r["trajs"] - ref["trajs"])[same].abs().max()), max_abs_scores=float((r["scores"] - ref["scores"])[same].abs().max()))
    for fn in paths.values():
        for _ in range(5):
            fn()
    rows = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            rows[k].append(timed(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    result.append(dict(n_sc=n_sc, K=K, A=A, T=80, iters=args.iters, us_per_iteration=rows, median_us=med, agreement=agree,
                       torch_peak_bytes=torch.cuda.max_memory_allocated()))
    print(json.dumps(result[-1]), flush=True)
