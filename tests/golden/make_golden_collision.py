#!/usr/bin/env python
"""Generate tests/golden/collision_reward.npz and tests/golden/train_c1_collision.npz by running the REFERENCE (the checkout
make_golden.py imports, through its shims) with the collision term of the differentiable reward on. Container-only tooling, like
make_golden.py; the fixtures hold data only.

collision_reward.npz - `DifferentiableReward._get_r_traffic_rule_approx` and `get` (w_collision = 0.7, use_il_loss on and off) on the
one-step inputs of synthetic.make_collision_case, in float32 and in float64 (torch's default dtype set to float64 for that run: the
reference allocates its distance tensor with the default). Per case, for both reductions: the float64 term, the float64 gradient with
respect to the pose under tests/collision_ref.py's upstream_weight, the decision margins of tests/collision_ref.py::margins; once:
bound_c / bound_g, the largest float32 - float64 difference of the reference itself over all cases. At most 5 % of a case's agents may
fall below the margin floors (asserted; pick another seed, never another cap).

train_c1_collision.npz - the reference's training_step at the c1 sizes, neutralised as make_golden.py::gen_train does, with
differentiable_reward.w_collision = 1.0, one run per reduction, on synthetic.crowd_scene(make_scene(seed=0)) - a scene that collides
(asserted: dr_rule_apx non-zero, and the action head's gradient norm away from the w_collision = 0 run's by more than ten times the
test's gradient-norm tolerance).

    python tests/golden/make_golden_collision.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import collision_ref as CR  # noqa: E402
from make_golden import AttrDict, build_wm, install_shims, npz, ref_model_cfg, tb, to_attr  # noqa: E402

# (n_sc, A, spread, seed)
CASES = [(3, 5, 8.0, 1), (2, 64, 60.0, 1), (2, 65, 40.0, 1), (4, 33, 25.0, 1), (2, 128, 120.0, 1), (1, 1, 1.0, 1)]
W_COLLISION = 0.7
IL = dict(l_pos=dict(weight=1e-1, criterion="SmoothL1Loss"), l_rot=dict(weight=1e1, criterion="SmoothL1Loss", angular_type="cosine"),
          l_spd=dict(weight=1e-1, criterion="SmoothL1Loss"))
GNORM_TOL = 1e-2  # tests/test_hip_training.py TRAIN_TOL["fp32"]["gnorm"]
CROWD = dict(pull=0.06, size_scale=1.0)


def case_name(n_sc, A, spread):
    return f"s{n_sc}_a{A}_w{int(spread)}"


def gen_reward():
    from utils.rewards import DifferentiableReward

    out, bound_c, bound_g = {}, 0.0, 0.0
    for n_sc, A, spread, seed in CASES:
        c = tb.synthetic.make_collision_case(n_sc, A, seed, spread)
        name = case_name(n_sc, A, spread)
        assert bool(c["pred_valid"].any(-1).all()), f"{name}: a scene without a valid agent (the reference gives NaN): pick another seed"
        for k, v in c.items():
            out[f"{name}/{k}"] = v
        w = CR.upstream_weight(n_sc, A)
        for mode in (True, False):
            tag = f"{name}/{'max' if mode else 'sum'}"
            res = {}
            for dt in (torch.float32, torch.float64):
                torch.set_default_dtype(dt)
                try:
                    pose = c["pred_pose"].to(dt).clone().requires_grad_(True)
                    term = DifferentiableReward._get_r_traffic_rule_approx(c["pred_valid"], pose, c["ag_size"].to(dt), mode)
                    (term * w.to(dt)).sum().backward()
                    res[dt] = (term.detach().double(), pose.grad.double())
                    if dt == torch.float64:
                        for il in (True, False):
                            dr = DifferentiableReward(**to_attr(IL), w_collision=W_COLLISION, use_il_loss=il, reduce_collsion_with_max=mode, is_enabled=True)
                            f = lambda k: c[k].to(dt)
                            got = dr.get(c["pred_valid"], f("pred_pose"), f("pred_motion"), c["gt_valid"], f("gt_pose"), f("gt_motion"), f("ag_size"))
                            for k, v in got.items():
                                out[f"{tag}/get_il{int(il)}/{k}"] = v
                finally:
                    torch.set_default_dtype(torch.float32)
            assert torch.isfinite(res[torch.float64][0]).all() and torch.isfinite(res[torch.float64][1]).all()
            bound_c = max(bound_c, float((res[torch.float32][0] - res[torch.float64][0]).abs().max()))
            bound_g = max(bound_g, float((res[torch.float32][1] - res[torch.float64][1]).abs().max()))
            out[f"{tag}/term"], out[f"{tag}/grad"] = res[torch.float64]
            m = CR.margins(c["pred_valid"], c["pred_pose"], c["ag_size"], mode)
            for k, v in m.items():
                out[f"{tag}/margin_{k}"] = v
            left_out = int((~CR.inside_margins(m)).sum())
            nz = float((res[torch.float64][0] > 0).double().mean())
            fin = lambda t: float(t[torch.isfinite(t)].min()) if torch.isfinite(t).any() else float("inf")
            print(f"{tag}: {100 * nz:.0f} % rows non-zero, {left_out} of {n_sc * A} agents outside the margins; smallest margins "
                  f"{fin(m['max_rel']):.3g} rel, {fin(m['min_gap']):.3g} m, {fin(m['clamp']):.3g}")
            assert left_out <= 0.05 * n_sc * A, f"{tag}: {left_out} agents below the margin floors: pick another seed"
    out["bound_c"], out["bound_g"], out["w_collision"] = np.float64(bound_c), np.float64(bound_g), np.float64(W_COLLISION)
    print(f"reference float32 - float64: term {bound_c:.3g}, gradient {bound_g:.3g}")
    npz("collision_reward.npz", **out)


def _train_run(w_collision, reduce_max):
    torch.manual_seed(0)
    mcfg0 = ref_model_cfg(n_tgt_knn=4)
    mcfg0["tf_cfg"]["dropout_p"] = 0.0
    mcfg0["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    mcfg0["add_navi_latent"]["mlp_dropout_p"] = 0.0
    wm_t = build_wm(mcfg0, p_training_rollout_prior=0.0, differentiable_reward=dict(IL, w_collision=w_collision, reduce_collsion_with_max=reduce_max,
                                                                                    use_il_loss=True))
    wm_t.teacher_forcing_training.prob_forcing_agent = 0.0
    wm_t.pre_processing[0].dropout_p_history = -1.0
    tb.utils.det_fill(wm_t.model, 0)
    wm_t.train()
    with torch.no_grad():
        for k, p in wm_t.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    batch = tb.synthetic.crowd_scene(tb.synthetic.make_scene(1, 8, 64, 8, seed=0), **CROWD)
    torch.manual_seed(7)
    loss = wm_t.training_step({k: v.clone() for k, v in batch.items()}, 0)
    loss.backward()
    out = {"dtrain_loss": loss.detach()}
    for k, v in wm_t.logged.items():
        out["dtrain_" + k.split("/")[1]] = v.detach()
    gn = {}
    for k, p in wm_t.model.named_parameters():
        if p.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(p.grad.double().pow(2).sum())
    for k, v in gn.items():
        out["dgradnorm_" + k] = np.float64(v) ** 0.5
    for k in ("ag_encoder.tf_ag2agmptl.layers.3.attn.linear_rpe.weight", "mp_encoder.tf_mp2mp.layers.0.attn.in_proj_weight",
              "tl_encoder.tf_tl2tlmp.layers.1.attn_src.out_proj_weight", "latent_encoder.ag_encoder_post.input_encoder.mlp.fc_layers.0.weight",
              "navi_predictor.mlp.fc_layers.0.weight", "action_head.mlp_mean.0.fc_layers.0.weight"):
        out["dgrad_" + k] = dict(wm_t.model.named_parameters())[k].grad[:8, :16]
    return out


def gen_train():
    base = _train_run(0.0, True)
    out = {"crowd_pull": np.float64(CROWD["pull"]), "crowd_size_scale": np.float64(CROWD["size_scale"]), "w_collision": np.float64(1.0)}
    for mode in (True, False):
        r = _train_run(1.0, mode)
        tag = "max" if mode else "sum"
        apx, g1, g0 = float(r["dtrain_dr_rule_apx"]), float(r["dgradnorm_action_head"]), float(base["dgradnorm_action_head"])
        print(f"train_c1_collision {tag}: dr_rule_apx {apx:.6g}, loss {float(r['dtrain_loss']):.6g} (w_collision = 0: {float(base['dtrain_loss']):.6g}), "
              f"action_head gradient norm {g1:.6g} (w_collision = 0: {g0:.6g})")
        assert apx != 0.0, "the scene does not collide"
        assert abs(g1 - g0) > 10 * GNORM_TOL * max(g0, 1e-6), "the collision term does not move the action head's gradient enough"
        for k, v in r.items():
            out[f"{tag}/{k}"] = v
    npz("train_c1_collision.npz", **out)


if __name__ == "__main__":
    install_shims()
    which = sys.argv[1:] or ["reward", "train"]
    if "reward" in which:
        gen_reward()
    if "train" in which:
        gen_train()
