"""Launch time of tbx_rollout_metrics (ErrorMetrics + TrafficRuleMetrics updates of one reactive-replay-shaped log: two calls, four
launches) against the float32 torch restatement of the same two `update`s on the same device, warm, device events over N calls, at the
WOSAC shape 32 x 128 x 90 and at 1 x 64 x 90. Prints one JSON line per shape.   python tools/val_metrics_time.py [--calls 200]"""
import argparse
import json
import math
import sys
from types import SimpleNamespace

sys.path.insert(0, ".")
import torch
from importlib import import_module
from __graft_entry__ import load_package

FLAGS = ("outside_map", "collided", "run_road_edge", "run_red_light", "passive", "goal_reached", "dest_reached")


def torch_update(state, buf, gt_valid, gt_pose, gt_motion, ag_type):
    """logging.py:36-49 and :87-107 in the reference's dtype (float32 states)."""
    sl = slice(buf.step_start, buf.step_end + 1)
    gv, gp, gm = gt_valid[:, :, sl], gt_pose[:, :, sl], gt_motion[:, :, sl]
    ev = buf.pred_valid.squeeze(1) & gv
    inv = ~ev.unsqueeze(-1)
    ep = (buf.pred_pose.squeeze(1) - gp).masked_fill(inv, 0.0)
    em = (buf.pred_motion.squeeze(1) - gm).masked_fill(inv, 0.0)
    state[0] += ev.sum()
    state[1] += torch.norm(ep[..., :2], dim=-1).sum()
    state[2] += torch.abs(torch.rad2deg((ep[..., 2] + math.pi) % (2 * math.pi) - math.pi)).sum()
    state[3] += torch.abs(em[..., 0]).sum()
    valid, invalid = buf.pred_valid, ~buf.pred_valid
    anyv = valid.any(-1)
    state[4] += anyv.sum()
    state[5] += (anyv & ag_type[:, None, :, 0]).sum()
    for i, k in enumerate(FLAGS):
        state[6 + i] += buf.violation[k].masked_fill(invalid, 0).any(-1).sum()


def timed(fn, calls):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    load_package()
    L = import_module("trafficbots_amd.models.metrics.logging")
    hip = import_module("trafficbots_amd.hip")
    dev = torch.device("cuda:0")
    for n, A, T in ((32, 128, 90), (1, 64, 90)):
        g = torch.Generator().manual_seed(0)
        r = lambda *s: torch.rand(*s, generator=g).to(dev)
        buf = SimpleNamespace(step_start=1, step_end=T, pred_valid=r(n, 1, A, T) > 0.3, pred_pose=r(n, 1, A, T, 3), pred_motion=r(n, 1, A, T, 3),
                              violation={k: r(n, 1, A, T) > 0.9 for k in FLAGS})
        gt = r(n, A, T + 1) > 0.3, r(n, A, T + 1, 3), r(n, A, T + 1, 3)
        ag_type = torch.nn.functional.one_hot(torch.randint(0, 3, (n, A), generator=g), 3).bool().to(dev)
        err, rule = L.ErrorMetrics("p"), L.TrafficRuleMetrics("p")
        state32 = torch.zeros(16, device=dev)

        def modules():
            err.update(buf, *gt)
            rule.update(buf, ag_type)

        # the kernel alone, both halves in ONE call (the flag byte packed beforehand)
        four = torch.stack([buf.violation[k].flatten(0, 1) for k in ("collided", "run_road_edge", "run_red_light", "passive")]).view(torch.uint8)
        flags = (four[0] | (four[1] << 2) | (four[2] << 3) | (four[3] << 4)).contiguous()
        acc = torch.zeros(16, dtype=torch.float64, device=dev)
        part = torch.zeros(256 * 16, dtype=torch.float64, device=dev)
        u8 = lambda t: t.flatten(0, 1).view(torch.uint8)

        def kernel():
            hip.rollout_metrics(acc, part, u8(buf.pred_valid), 1, T, 0, T, pred_pose=buf.pred_pose.flatten(0, 1), pred_motion=buf.pred_motion.flatten(0, 1),
                                gt_valid=gt[0].view(torch.uint8), gt_pose=gt[1], gt_motion=gt[2], gt_t0=1, flags=flags, ld_flags=T,
                                outside_map=u8(buf.violation["outside_map"]), dest_reached=u8(buf.violation["dest_reached"]),
                                goal_reached=u8(buf.violation["goal_reached"]), ag_type=ag_type.view(torch.uint8))

        res = {"shape": [n, A, T], "calls": args.calls,
               "kernel_one_call_us": round(timed(kernel, args.calls), 2),
               "modules_two_updates_us": round(timed(modules, args.calls), 2),
               "torch_float32_two_updates_us": round(timed(lambda: torch_update(state32, buf, *gt, ag_type), args.calls), 2)}
        # same numbers? (float32 states against float64 ones)
        err.reset(), rule.reset(), state32.zero_()
        modules()
        torch_update(state32, buf, *gt, ag_type)
        res["max_rel_diff_vs_float32_torch"] = float(((err.state + rule.state)[:13].float() - state32[:13]).abs().div(state32[:13].abs().clamp_min(1)).max())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
