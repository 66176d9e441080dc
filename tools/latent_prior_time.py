"""What a learned latent prior costs on the device.

  python tools/latent_prior_time.py [--cases default,prior_gaus,cat_cat] [--classes bf16,fp32] [--steps 5] [--rounds 3]

(a) bench.py --mode train's step (16 scenes of 64 agents / 1024 polylines / 128 lights, 90 steps, forward + backward as one hipGraph
    replay, clip, AdamW) in both precision classes for the default configuration (std_gaus prior: no prior pass), for `prior_gaus` (a
    diag_gaus prior with fixed log_std: a second differentiated encoder pass over the history) and for `cat_cat` (both sides categorical
    with per-type branches) - in one process, in alternating rounds; the added milliseconds per step are against the default's median
    of the same process. `--cases default` runs on any earlier checkout as well (the A/B of the default configuration).
(b) the eval-mode prior of one scene at K = 32 joint futures: latent_encoder(posterior=False), repeat_interleave_(32), sample - HIP
    events around back-to-back calls.

One JSON line."""
import argparse
import copy
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

_D = dict(n_cat=8, log_std=0.0, mlp_use_layernorm=False, n_layer=3, branch_type=False)
CASES = {"default": None,
         "prior_gaus": dict(latent_prior=dict(_D, dist_type="diag_gaus")),
         "cat_cat": dict(latent_post=dict(_D, dist_type="cat", branch_type=True), latent_prior=dict(_D, dist_type="cat", branch_type=True))}


def model_cfg(tb, case):
    mcfg = tb.config.default_model_cfg()
    for k, v in copy.deepcopy(CASES[case] or {}).items():
        mcfg["latent_encoder"][k] = tb.config.to_attr(v)
    return mcfg


def train_steps(tb, dev, cases, precision, scenes=16, steps=5, rounds=3):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    torch.backends.cuda.preferred_blas_library("cublas")  # (as tools/benchlib/training.py)
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(scenes, 64, 1024, 128, seed=0).items()}
    run = {}
    for name in cases:
        torch.manual_seed(0)
        wm = W.WaymoMotion(model=model_cfg(tb, name), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg()).to(dev).train()
        wm.train_precision = precision
        (opt,), _ = wm.configure_optimizers()
        gstep = DP.GraphedTrainStep(wm, opt, batch)
        for _ in range(3):
            m = gstep(batch)
        run[name] = (gstep, [], float(m["loss"].detach()), len(gstep.live))
        print(f"[{precision}] {name}: captured, {len(gstep.live)} live parameters", file=sys.stderr, flush=True)
    for _ in range(rounds):
        for name, (gstep, ms, _, _) in run.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                gstep(batch)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / steps * 1e3)
    out = {name: {"ms_per_step": [round(x, 3) for x in ms], "median": round(statistics.median(ms), 3), "loss_after_warmup": loss, "live_parameters": live}
           for name, (_, ms, loss, live) in run.items()}
    if "default" in out:
        for name in out:
            if name != "default":
                out[name]["added_ms"] = round(out[name]["median"] - out["default"]["median"], 3)
    return out


@torch.no_grad()
def eval_prior(tb, dev, cases, K=32, reps=10, rounds=5):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    raw = tb.synthetic.make_scene(1, 64, 1024, 128, seed=0)
    out = {}
    for name in cases:
        torch.manual_seed(0)
        wm = W.WaymoMotion(model=model_cfg(tb, name), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg()).to(dev).eval()
        bd = wm.pre_processing({k: v.to(dev) for k, v in {**raw, **tb.synthetic.to_history_batch(raw)}.items()})
        mp, tl = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")

        def fn():
            d = wm.model.latent_encoder(ag_valid=bd["sc/ag_valid"], ag_attr=bd["sc/ag_attr"], ag_motion=bd["sc/ag_motion"], ag_pose=bd["sc/ag_pose"],
                                        ag_type=bd["ref/ag_type"], tl_state=bd["sc/tl_state"], mp_tokens=mp, tl_tokens=tl, posterior=False)
            d.repeat_interleave_(K, 0)
            return d.log_prob(d.sample(False))

        for _ in range(3):
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
        out[name] = [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="default,prior_gaus,cat_cat")
    ap.add_argument("--classes", default="bf16,fp32")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-eval", action="store_true")
    a = ap.parse_args()
    cases = a.cases.split(",")
    tb = load_package()
    dev = torch.device("cuda:0")
    res = {"what": "learned latent prior: graph-replayed training step (16 scenes, 90 steps) and the eval-mode prior of one scene at K = 32"}
    for cls in a.classes.split(","):
        res[f"train_step_16_scenes_{cls}"] = train_steps(tb, dev, cases, cls, steps=a.steps, rounds=a.rounds)
        torch.cuda.empty_cache()
    if not a.no_eval:
        res["eval_prior_ms_per_scene_K32_median_min_max"] = eval_prior(tb, dev, cases)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
