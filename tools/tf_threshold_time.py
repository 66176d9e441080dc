"""What error-threshold teacher forcing (TeacherForcing's threshold_xy / _yaw / _spd) costs in the closed loop: one extra launch
(tbx_tf_threshold) at the head of every step.

  python tools/tf_threshold_time.py      reactive_replay's engine at the c1 sizes (8 agents / 64 polylines / 8 lights) and at configs[1]'s
                                         scene (64 / 1024 / 128), default schedule (the one-queue step: five paired launches), captured
                                         graphs; per size one engine with threshold_xy on and one with every threshold off - the off engine
                                         is launch for launch the engine without the feature

Same process, both engines alive, alternating: per round restore() (untimed), then HIP events around run(T) - T = 90 graph-replayed steps.
Medians over `rounds` rounds, in microseconds per step. One JSON line per size."""
import json
import statistics
import sys
from importlib import import_module
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

DEV, T = "cuda:0", 90


def engine(tb, sizes, knn, thr):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg()
    if thr is not None:
        scfg["teacher_forcing_reactive_replay"] = dict(scfg["teacher_forcing_reactive_replay"], threshold_xy=thr)
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=knn), data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    with torch.no_grad():  # damped action head: a free-running loop that stays on the map
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    wm = wm.to(DEV).eval()
    batch = tb.synthetic.make_scene(1, *sizes, seed=0)
    bd = wm.pre_processing({k: v.to(DEV) for k, v in {**batch, **tb.synthetic.to_history_batch(batch)}.items()})
    mp, tl = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")
    z = torch.randn(1, sizes[0], 16, generator=torch.Generator().manual_seed(6)).to(DEV)
    v = bd["gt/ag_valid"].any(-1)
    buf = wm.reactive_replay(bd, mp, tl, z, v, bd["gt/ag_navi"], v, wm.teacher_forcing_reactive_replay, True, step_end=T)  # captures
    return wm, wm._engine, buf


def one_round(eng):
    eng.restore()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    eng.run(T)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / T


def main(rounds=21, thr=3.38):
    tb = load_package()
    for name, sizes, knn in (("c1", (8, 64, 8), 4), ("configs[1]", (64, 1024, 128), 32)):
        keep_off, off, buf_off = engine(tb, sizes, knn, None)
        keep_on, on, buf_on = engine(tb, sizes, knn, thr)
        assert off._tf_args is None and on._tf_args is not None and off.one_queue and on.one_queue
        resets = int((on.S["tf_mask"] & ~on.init_state["tf_mask"]).sum())
        for e in (off, on, off, on):  # warm-up rounds, untimed
            one_round(e)
        us = {"off": [], "on": []}
        for _ in range(rounds):
            us["off"].append(one_round(off))
            us["on"].append(one_round(on))
        m_off, m_on = statistics.median(us["off"]), statistics.median(us["on"])
        print(json.dumps({"what": "closed-loop step, one-queue schedule, graph replay, us per step", "size": name, "steps": T, "rounds": rounds,
                          "threshold_xy": thr, "resets_in_the_rollout": resets,
                          "off_us": round(m_off, 2), "off_min_max": [round(min(us["off"]), 2), round(max(us["off"]), 2)],
                          "on_us": round(m_on, 2), "on_min_max": [round(min(us["on"]), 2), round(max(us["on"]), 2)],
                          "extra_us_per_step": round(m_on - m_off, 2), "off_launch_spacing_us": round(m_off / 5, 2)}), flush=True)


if __name__ == "__main__":
    main()
