"""What another criterion / angular type of the differentiable reward's imitation terms costs on the device.

  python tools/il_loss_time.py      (a) tbx_il_reward_fwd and tbx_il_reward_bwd + tbx_train_chain_bwd_state's extra inputs at the training
                                    shape, 16 scenes x 90 steps x 64 agents in the chain's [n, T, A] layout: HIP events around back-to-back
                                    launches; (b) bench.py --mode train's step (16 scenes of 64 agents / 1024 polylines / 128 lights, the
                                    default model, bf16 class, forward + backward as one hipGraph replay, clip, AdamW) with the default
                                    configuration and with MSE position / L1 speed / cast + SmoothL1 heading - two extra launches per
                                    step - in the same process, in alternating rounds.

One JSON line."""
import json
import statistics
import sys
import time
from importlib import import_module
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

NON_DEFAULT = dict(l_pos=dict(weight=0.1, criterion="MSELoss"), l_rot=dict(weight=10.0, criterion="SmoothL1Loss", angular_type="cast"),
                   l_spd=dict(weight=0.1, criterion="L1Loss"))


def timed(fn, warmup=5, reps=20, rounds=9):
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
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


def kernels(hip, dev, n=16, T=90, A=64, Tg=91):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    pv, gv = (r(n, T, A) < 0.85).to(torch.uint8), (r(n, A, Tg) < 0.9).to(torch.uint8)
    pp, pm, gp, gm = r(n, T, A, 3) * 50, r(n, T, A, 3) * 10, r(n, A, Tg, 3) * 50, r(n, A, Tg, 3) * 10
    up = r(n, T, A)
    codes, w = (hip.IL_MSE, hip.IL_SMOOTH_L1, hip.IL_L1, hip.IL_ANG_CAST), (0.1, 10.0, 0.1)
    out = torch.empty(n, T, A, device=dev)
    fwd = lambda: hip.il_reward_fwd(pv, pp, pm, gv, gp, gm, codes, w, gt_offset=1, out_sum=out)
    bwd = lambda: hip.il_reward_bwd(pv, pp, pm, gv, gp, gm, codes, w, gt_offset=1, g=up)
    return {"shape": [n, T, A], "fwd_ms": timed(fwd), "bwd_ms": timed(bwd)}


def train_steps(tb, dev, scenes=16, steps=5, rounds=3):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    torch.backends.cuda.preferred_blas_library("cublas")  # (as tools/benchlib/training.py)
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(scenes, 64, 1024, 128, seed=0).items()}
    run = {}
    for name, over in (("default", None), ("mse_l1_cast", NON_DEFAULT)):
        torch.manual_seed(0)
        scfg = tb.config.default_sim_cfg()
        if over is not None:
            scfg["differentiable_reward"].update(over)
        wm = W.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
        wm.train_precision = "bf16"
        (opt,), _ = wm.configure_optimizers()
        gstep = DP.GraphedTrainStep(wm, opt, batch)
        for _ in range(3):
            m = gstep(batch)
        run[name] = (gstep, [], float(m["loss"].detach()))
    for _ in range(rounds):
        for name, (gstep, ms, _) in run.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                gstep(batch)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / steps * 1e3)
    return {name: {"ms_per_step": [round(x, 3) for x in ms], "median": round(statistics.median(ms), 3), "loss_after_warmup": loss}
            for name, (_, ms, loss) in run.items()}


def main():
    tb = load_package()
    hip = import_module("trafficbots_amd.hip")
    dev = torch.device("cuda:0")
    print(json.dumps({"what": "imitation terms with configured criteria: kernel pair and training step", "kernels": kernels(hip, dev),
                      "train_step_16_scenes_bf16": train_steps(tb, dev)}), flush=True)


if __name__ == "__main__":
    main()
