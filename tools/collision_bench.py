"""What the collision term of the differentiable reward (w_collision > 0) costs on the device.

  python tools/collision_bench.py kernels   tbx_collision_reward_fwd + _bwd over a whole log, against the torch expression of the same term
                                            (tests/collision_ref.py in float32, forward + autograd backward, one step at a time as the
                                            reference's rollout evaluates it - fused by nothing)
  python tools/collision_bench.py step      the captured training step (GraphedTrainStep, bench.py's training shape) with w_collision = 1
                                            against the same step with w_collision = 0, and the calls of the term's entry points per step

HIP events around `reps` back-to-back repetitions after `warmup` untimed ones; medians over `rounds` such measurements. One JSON line per
measurement."""
import json
import statistics
import sys
from importlib import import_module
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402


def timed(fn, warmup=3, reps=5, rounds=7):
    """Median ms per call of fn over `rounds` event-timed runs of `reps` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def kernels(tb):
    import collision_ref as CR

    hip = import_module("trafficbots_amd.hip")
    dev = torch.device("cuda:0")
    for n, T, A, spread in ((8, 90, 64, 60.0), (32, 90, 128, 120.0)):
        case = tb.synthetic.make_collision_case(n * T, A, seed=5, spread=spread)
        valid = case["pred_valid"].view(n, T, A).to(torch.uint8).to(dev)
        pose = case["pred_pose"].view(n, T, A, 3).to(dev).contiguous()
        size = case["ag_size"][:n].to(dev).contiguous()
        g = torch.rand(n, T, A, device=dev) + 0.5
        for mode in (True, False):
            def pair():
                c, arg = hip.collision_reward_fwd(pose, valid, size, mode)
                return c, hip.collision_reward_bwd(pose, valid, size, mode, g, arg)

            def torch_steps():
                out = []
                for t in range(T):  # the reference evaluates the term inside every step of its rollout
                    p = pose[:, t].detach().requires_grad_(True)
                    c = CR.term(valid[:, t].bool(), p, size, mode, dtype=torch.float32)
                    (c * g[:, t]).sum().backward()
                    out.append(p.grad)
                return out

            c, d = pair()
            ref = torch.stack(torch_steps(), 1)
            k_ms, t_ms = timed(pair), timed(torch_steps, warmup=1, reps=1, rounds=5)
            print(json.dumps({"what": "collision kernel pair vs torch expression", "n": n, "T": T, "A": A, "reduce_with_max": mode,
                              "pair_ms": round(k_ms[0], 4), "pair_ms_min_max": [round(k_ms[1], 4), round(k_ms[2], 4)],
                              "torch_ms": round(t_ms[0], 3), "torch_ms_min_max": [round(t_ms[1], 3), round(t_ms[2], 3)],
                              "speedup": round(t_ms[0] / k_ms[0], 1), "rows_nonzero": round(float((c > 0).float().mean()), 3),
                              "grad_max_abs_diff": float((d - ref).abs().max())}), flush=True)


def step(tb, scenes=16, agents=64, polylines=1024, lights=128):
    hip = import_module("trafficbots_amd.hip")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    dev = torch.device("cuda:0")
    torch.backends.cuda.preferred_blas_library("cublas")
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(scenes, agents, polylines, lights, seed=0).items()}
    names = ("collision_reward_fwd", "collision_reward_bwd", "train_chain_bwd_pose", "train_chain_bwd")
    res = {}
    for w in (0.0, 1.0):
        torch.manual_seed(0)
        scfg = tb.config.default_sim_cfg()
        scfg["differentiable_reward"]["w_collision"] = w
        wm = W.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
        wm.train_precision = "bf16"
        (opt,), _ = wm.configure_optimizers()
        calls = {k: 0 for k in names}
        orig = {k: getattr(hip, k) for k in names}
        for k in names:
            setattr(hip, k, (lambda k: lambda *a, **kw: (calls.__setitem__(k, calls[k] + 1), orig[k](*a, **kw))[1])(k))
        try:
            torch.manual_seed(1234)
            gstep = DP.GraphedTrainStep(wm, opt, batch)  # (capture: 2 eager warm-up passes + the captured one)
        finally:
            for k in names:
                setattr(hip, k, orig[k])
        ms = timed(lambda: gstep(batch), warmup=3, reps=3, rounds=5)
        m = gstep(batch)
        res[w] = ms[0]
        print(json.dumps({"what": "captured training step", "w_collision": w, "scenes": scenes, "agents": agents, "ms_per_step": round(ms[0], 2),
                          "ms_min_max": [round(ms[1], 2), round(ms[2], 2)], "calls_per_pass": {k: v / 3 for k, v in calls.items()},
                          "loss": float(m["loss"].detach()), "dr_rule_apx": float(m.get("dr_rule_apx", 0.0))}), flush=True)
        del gstep, wm, opt
    print(json.dumps({"what": "the term's share of the captured step", "added_ms": round(res[1.0] - res[0.0], 2),
                      "added_percent": round(100 * (res[1.0] - res[0.0]) / res[0.0], 2)}), flush=True)


if __name__ == "__main__":
    tb = load_package()
    which = sys.argv[1:] or ["kernels", "step"]
    if "kernels" in which:
        kernels(tb)
    if "step" in which:
        step(tb)
