#!/usr/bin/env python
"""Generate tests/golden/val_metrics.npz by running the REFERENCE's ErrorMetrics and TrafficRuleMetrics (models/metrics/logging.py of the
checkout make_golden.py imports) on synthetic rollout buffers. Container-only tooling, like make_golden.py whose shims it uses
(`torchmetrics.Metric.add_state` among them); the fixture holds the inputs (the seven violation flags of a step as bit i = FLAGS[i] of one byte), the reference's raw states and its `compute()` outputs.

The float inputs are float32 values; the reference is run on their float64 casts with float64 states (torch's default dtype is set to
float64 before the metrics are built, so `tensor(0.0)` is a float64 state), which makes its sums the exact ones rounded once per
operation in float64 - the comparison side of tests/test_hip_val_metrics.py at rtol 1e-5.

Cases (name -> n scenes, K joint futures, A agents, T buffer steps): the smallest shapes at which tbx_rollout_metrics can go wrong.
  k3       2, 3, 5, 7    rule half only (the error half is defined for K = 1): A is no multiple of the 4 waves of a workgroup, K
                         broadcasts over ag_type; two updates
  k3_noveh 2, 3, 5, 7    no agent is a vehicle: counter_veh = 0, the three per-vehicle rates are 0/0 = nan; goal_reached all false on valid steps
  k1       2, 1, 5, 7    both halves, two updates
  long     1, 1, 3, 130  more than two 64-lane strides along time, two updates
  slice    2, 1, 5, 7    buffer = steps 1..7 of an 11-step log (the arrays hold the whole log), step_start = 1, 10 ground-truth steps
Contents of every update: agent 0 never valid - with every flag set at every step; the last row without any valid agent (where
there is more than one row); agent 1 valid in the prediction but never in the ground truth; flags drawn independently of validity,
so some sit on invalid steps; heading differences 1e-3 inside and outside of +-pi and +-2 pi on the first valid steps.

    python tests/golden/make_golden_val.py
"""
import json
import math
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import install_shims, npz  # noqa: E402

FLAGS = ("outside_map", "collided", "run_road_edge", "run_red_light", "passive", "goal_reached", "dest_reached")
ERR_STATES = ("err_counter", "err_pos_meter", "err_rot_deg", "err_spd_m_per_s")
RULE_STATES = ("counter_agent", "counter_veh") + FLAGS  # the order of tbx_rollout_metrics' acc[4:13]
# name -> n, K, A, T (buffer steps), n_updates, log steps (None: dense), first log step of the buffer, vehicles?, seed
CASES = {
    "k3": dict(n=2, K=3, A=5, T=7, n_updates=2, log_T=7, t0=0, veh=True, seed=1),
    "k3_noveh": dict(n=2, K=3, A=5, T=7, n_updates=1, log_T=7, t0=0, veh=False, seed=2),
    "k1": dict(n=2, K=1, A=5, T=7, n_updates=2, log_T=7, t0=0, veh=True, seed=3),
    "long": dict(n=1, K=1, A=3, T=130, n_updates=2, log_T=130, t0=0, veh=True, seed=4),
    "slice": dict(n=2, K=1, A=5, T=7, n_updates=2, log_T=11, t0=1, veh=True, seed=5),
}
SEAMS = [s * (m * math.pi + e) for m in (1, 2) for s in (1, -1) for e in (-1e-3, 1e-3)]


def make_update(c, g):
    """One update's inputs: the whole log [n, K, A, log_T, ..] and the ground truth [n, A, Tg, ..], float32 / bool."""
    n, K, A, L = c["n"], c["K"], c["A"], c["log_T"]
    step_start = 1
    Tg = c["T"] + step_start + 2  # the ground truth is longer than the buffer on both sides
    r = lambda *s: torch.rand(*s, generator=g)
    rn = lambda *s: (torch.randn(*s, generator=g) * 256).round() / 256  # (a 1/256 grid: exact in float32, and the file stays small)
    gt_valid = r(n, A, Tg) > 0.3
    gt_pose = torch.cat([rn(n, A, Tg, 2) * 20, ((r(n, A, Tg, 1) * 2 - 1) * math.pi * 256).round() / 256], -1).float()
    gt_motion = (rn(n, A, Tg, 3) * 5).float()
    pv = r(n, K, A, L) > 0.3
    pv[:, :, 0] = False
    if n * K > 1:
        pv[-1, -1] = False
    gt_valid[:, 1] = False
    # the log's step j is ground-truth step j - t0 + step_start
    sl = slice(step_start - c["t0"], step_start - c["t0"] + L)
    base_pose = torch.zeros(n, A, L, 3)
    base_motion = torch.zeros(n, A, L, 3)
    lo, hi = max(sl.start, 0), min(sl.stop, Tg)
    base_pose[:, :, lo - sl.start:hi - sl.start] = gt_pose[:, :, lo:hi]
    base_motion[:, :, lo - sl.start:hi - sl.start] = gt_motion[:, :, lo:hi]
    d = torch.cat([rn(n, K, A, L, 2) * 2, rn(n, K, A, L, 1) * 0.5], -1)
    seam = torch.tensor(SEAMS)
    k = 0  # the seams go to steps that count: valid in both, in scene 0 (never the row without valid agents)
    for a in range(2, A):
        for t in range(c["t0"], c["t0"] + c["T"]):
            if k < len(SEAMS):
                pv[0, 0, a, t] = gt_valid[0, a, t - c["t0"] + step_start] = True
                d[0, 0, a, t, 2] = seam[k]
                k += 1
    assert k == len(SEAMS), "not every seam value was placed"
    pred_pose = (base_pose[:, None] + d).float()
    pred_motion = (base_motion[:, None] + rn(n, K, A, L, 3)).float()
    flags = {f: r(n, K, A, L) > 0.8 for f in FLAGS}
    if not c["veh"]:  # (the per-vehicle checks flag nobody: 0 / 0)
        for f in ("run_road_edge", "run_red_light", "passive", "goal_reached"):
            flags[f][:] = False
    for f in FLAGS:
        flags[f][:, :, 0] = True
    ag_type = torch.nn.functional.one_hot((torch.arange(A) + 2) % 3 if c["veh"] else 1 + torch.arange(A) % 2, 3).bool()[None].repeat(n, 1, 1)
    return dict(pred_valid=pv, pred_pose=pred_pose, pred_motion=pred_motion, gt_valid=gt_valid, gt_pose=gt_pose, gt_motion=gt_motion,
                ag_type=ag_type), flags, step_start


def main():
    install_shims()
    torch.set_default_dtype(torch.float64)
    from models.metrics.logging import ErrorMetrics, TrafficRuleMetrics  # the reference's

    out = {}
    for name, c in CASES.items():
        g = torch.Generator().manual_seed(c["seed"])
        err, rule = ErrorMetrics("p"), TrafficRuleMetrics("p")
        for u in range(c["n_updates"]):
            x, flags, step_start = make_update(c, g)
            t = slice(c["t0"], c["t0"] + c["T"])
            buf = SimpleNamespace(step_start=step_start, step_end=step_start + c["T"] - 1, pred_valid=x["pred_valid"][..., t],
                                  pred_pose=x["pred_pose"][..., t, :].double(), pred_motion=x["pred_motion"][..., t, :].double(),
                                  violation={f: flags[f][..., t] for f in FLAGS})
            if c["K"] == 1:
                err.update(buf, x["gt_valid"], x["gt_pose"].double(), x["gt_motion"].double())
            rule.update(buf, x["ag_type"])
            for k, v in x.items():
                out[f"{name}_u{u}_{k}"] = v
            # the seven flags as bit i = FLAGS[i] of one byte
            out[f"{name}_u{u}_flag_bits"] = sum(flags[f].to(torch.uint8) << i for i, f in enumerate(FLAGS))
        c["step_start"] = step_start
        if c["K"] == 1:
            assert float(err.err_counter) > 0
            out[f"{name}_err_state"] = torch.stack([getattr(err, s) for s in ERR_STATES]).double()
            ce = err.compute()
            out[f"{name}_err_compute"] = torch.stack(list(ce.values())).double()
            c["err_keys"] = list(ce)
        out[f"{name}_rule_state"] = torch.stack([getattr(rule, s) for s in RULE_STATES]).double()
        cr = rule.compute()
        out[f"{name}_rule_compute"] = torch.stack(list(cr.values())).double()
        c["rule_keys"] = list(cr)
        print(name, "rule state", out[f"{name}_rule_state"].tolist(), "err state", out.get(f"{name}_err_state", torch.zeros(0)).tolist())
        assert float(rule.counter_agent) > 0 and (float(rule.counter_veh) > 0) == c["veh"]
    out["cases"] = json.dumps(CASES)
    npz("val_metrics.npz", **out)
    size = (Path(__file__).resolve().parent / "val_metrics.npz").stat().st_size
    print(f"val_metrics.npz: {size / 1e3:.1f} kB")
    assert size < 100_000


if __name__ == "__main__":
    main()
