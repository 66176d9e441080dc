#!/usr/bin/env python
"""Generate tests/golden/womd_aggr.npz by running the REFERENCE's WOMDPostProcessing.forward with `aggr_thresh` set (the checkout
make_golden.py imports) on seeded inputs (`synthetic.make_womd_case`, `make_womd_repair_case` - ours, shipped). Container-only tooling,
like make_golden_post.py; it uses make_golden.py's shims and is the only file of the aggregation work that imports the reference. The
fixture holds the reference's outputs only (plus, as a JSON string, the arguments each case was made with).

The reference's `forward` hands the LIST `aggr_thresh` to `traj_aggr`, which compares a tensor with it: TypeError. Its `forward` stays
untouched here: the module is built with the 3-list, then `pp.aggr_thresh` is set to the tensor [n_sc, n_ag, 1, 1] `mtr_nms` would form
of it (float32 sum of type_i * thresh_i); `len()` of that tensor is positive, the branch is taken and `mpa_nms`, temperature and
sampling run behind the aggregation as written.

Per case: the reference's float32 `trajs` and `scores`, the seeds, `bound_trajs` / `bound_scores` = the largest difference between the
reference run in float32 and in float64 on the agents with safe margins, and per agent the DECISION MARGINS in float64 from the
restatement tests/womd_aggr_ref.py, which must reproduce the reference's float64 run (asserted). Safe: margin_d >= 1e-4 m, margin_s >=
1e-5, margin_c >= 1; at most 5 % of a case's agents may be unsafe (asserted: pick another seed, not another cap).

    python tests/golden/make_golden_aggr.py
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from make_golden import install_shims, npz, tb  # noqa: E402
from womd_aggr_ref import aggr_case, safe_agents  # noqa: E402

STEP_CURRENT, MAX_LEFT_OUT = 10, 0.05
BASE = dict(k_pred=6, score_temperature=-1, mpa_nms_thresh=[2.0, 2.0, 2.0], mtr_nms_thresh=[], aggr_thresh=[2.5, 1.0, 1.5], n_iter_em=3,
            use_ade=True)
REPAIR = dict(aggr_thresh=[1.0, 0.5, 0.8], mpa_nms_thresh=[])
# name -> (helper, its arguments, configuration overrides)
AGGR_CASES = {
    "ade32": ("make_womd_case", dict(n_sc=2, n_k=32, n_ag=24, n_step=80, seed=11), {}),
    "fde48": ("make_womd_case", dict(n_sc=2, n_k=48, n_ag=12, n_step=80, seed=12), dict(use_ade=False)),
    "k7": ("make_womd_case", dict(n_sc=1, n_k=7, n_ag=16, n_step=80, seed=13), {}),
    "k128": ("make_womd_case", dict(n_sc=1, n_k=128, n_ag=8, n_step=80, seed=15, n_bundle=2), dict(n_iter_em=2)),
    "iter0": ("make_womd_case", dict(n_sc=1, n_k=32, n_ag=16, n_step=80, seed=16), dict(n_iter_em=0)),
    "temp_type": ("make_womd_case", dict(n_sc=1, n_k=32, n_ag=16, n_step=80, seed=17), dict(mpa_nms_thresh=[2.0, 1.0, 1.5], score_temperature=0.5)),
    "t91": ("make_womd_case", dict(n_sc=1, n_k=128, n_ag=4, n_step=91, seed=18), {}),
    "repair_ade": ("make_womd_repair_case", dict(n_ag=16, n_step=80, seed=0), REPAIR),
    "repair_fde": ("make_womd_repair_case", dict(n_ag=16, n_step=80, seed=0), dict(use_ade=False, **REPAIR)),
}


def run_reference(WOMDPostProcessing, c, cfg, dtype):
    n_step = c["trajs"].shape[3]
    pp = WOMDPostProcessing(step_gt=STEP_CURRENT + n_step, step_current=STEP_CURRENT, **cfg)
    thresh = 0
    for i in range(3):
        thresh = thresh + c["ag_type"][:, :, i] * cfg["aggr_thresh"][i]
    assert thresh.dtype == torch.float32
    pp.aggr_thresh = thresh[:, :, None, None]
    return pp(c["ag_type"], c["trajs"].to(dtype), c["log_prob"].to(dtype))


def gen_aggr():
    from data_modules.womd_post_processing import WOMDPostProcessing

    out = {}
    for name, (helper, case_kw, over) in AGGR_CASES.items():
        cfg = {**BASE, **over}
        c = getattr(tb.synthetic, helper)(**case_kw)
        n_step = c["trajs"].shape[3]
        r32, r64 = run_reference(WOMDPostProcessing, c, cfg, torch.float32), run_reference(WOMDPostProcessing, c, cfg, torch.float64)
        assert r32["trajs"].dtype == torch.float32 and r64["trajs"].dtype == torch.float64
        ours = aggr_case(c["trajs"].double().numpy(), c["log_prob"].double().numpy(), c["ag_type"].numpy(), cfg, n_step)
        # the restatement IS the reference in float64
        dt = np.abs(ours["trajs"] - r64["trajs"].numpy()).max()
        ds = np.abs(ours["scores"] - r64["scores"].numpy()).max()
        assert dt < 1e-9 and ds < 1e-12, (name, dt, ds)
        safe = safe_agents(ours["margin_d"], ours["margin_s"], ours["margin_c"])
        left_out = 1.0 - safe.mean()
        assert left_out <= MAX_LEFT_OUT, f"{name}: {left_out:.3f} of the agents below the decision margins - pick another seed"
        bt = float((r32["trajs"].double() - r64["trajs"]).abs().numpy()[safe].max())
        bs = float((r32["scores"].double() - r64["scores"]).abs().numpy()[safe].max())
        if helper == "make_womd_repair_case":
            assert (ours["n_repair"] >= 1).all(), f"{name}: an agent whose clusters all kept members"
        print(f"{name}: {tuple(r32['trajs'].shape)}, left out {left_out:.4f}, restatement - float64 reference {dt:.1e} / {ds:.1e}, "
              f"float32 - float64 bounds {bt:.3e} m / {bs:.3e}, repairs {int(ours['n_repair'].sum())}")
        out.update({f"{name}_trajs": r32["trajs"], f"{name}_scores": r32["scores"], f"{name}_seeds": ours["seeds"].astype(np.int16),
                    f"{name}_bound_trajs": np.float64(bt), f"{name}_bound_scores": np.float64(bs), f"{name}_margin_d": ours["margin_d"],
                    f"{name}_margin_s": ours["margin_s"], f"{name}_margin_c": ours["margin_c"]})
    # the cases travel with their results: the tests rebuild the inputs from these arguments
    out["cases"] = json.dumps({n: dict(helper=h, case=c, cfg={**BASE, **o}) for n, (h, c, o) in AGGR_CASES.items()})
    npz("womd_aggr.npz", **out)


if __name__ == "__main__":
    install_shims()
    torch.set_num_threads(8)
    gen_aggr()
