#!/usr/bin/env python
"""Generate tests/golden/il_loss.npz and tests/golden/train_c1_il.npz by running the REFERENCE (the checkout make_golden.py imports,
through its shims) with the imitation terms of the differentiable reward at other criteria / angular types than the default.
Container-only tooling, like make_golden.py; the fixtures hold data only.

il_loss.npz - `DifferentiableReward.get` and `AngularError.compute` on the one-step inputs of tests/il_loss_ref.py::make_case
(GOLDEN_CASE; stored, so the tests read them back), in float32 and in float64, for every configuration of il_loss_ref.CONFIGS: the four
criteria on position and speed with the cosine heading, {null, cast, vector} x {SmoothL1Loss, MSELoss, L1Loss} on the heading, and one
mixed configuration. Per configuration: the float64 terms r4 = (r_pos, r_rot, r_spd, sum), the mask, the float64 gradients with respect
to pred_pose / the predicted speed under il_loss_ref.upstream_weight, the float64 AngularError, and bound_r / bound_g: the reference's
own largest float32 - float64 difference in value / gradient relative to the case's largest magnitude (gradients at the elements
il_loss_ref.excluded leaves out are skipped; at most 5 % of the elements may be left out - asserted: pick another seed, never another cap).

train_c1_il.npz - the reference's training_step at the c1 sizes, neutralised as make_golden.py::gen_train does, for the two
configurations of il_loss_ref.TRAIN_CONFIGS: loss, logged terms, per-module gradient norms, the spot gradients of train_c1_collision.npz.
Asserted: the action head's gradient norm is away from the default criteria's by more than ten times the test's gradient-norm tolerance.

    python tests/golden/make_golden_il_loss.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import il_loss_ref as IL  # noqa: E402
from make_golden import build_wm, install_shims, npz, ref_model_cfg, tb, to_attr  # noqa: E402

GNORM_TOL = 1e-2  # tests/test_hip_training.py TRAIN_TOL["fp32"]["gnorm"]


def gen_reward():
    from models.metrics.loss import AngularError
    from utils.rewards import DifferentiableReward

    case = IL.make_case(**IL.GOLDEN_CASE)
    assert case["pred_pose"].shape[1] == 1
    one = lambda x: x[:, 0]  # [rows, 1, A, ..] -> [n_sc, n_ag, ..]
    gt1 = lambda x: x[:, :, 0]
    out = {k: v for k, v in case.items() if torch.is_tensor(v)}
    w = one(IL.upstream_weight(*case["pred_valid"].shape))
    # what the inputs must contain
    d = gt1(case["gt_pose"]) - one(case["pred_pose"])
    live = (one(case["pred_valid"]) & gt1(case["gt_valid"]))
    assert bool(((d[..., 0].abs() < 1) & live).any()) and bool(((d[..., 0].abs() > 1) & (d[..., 0].abs() < 2) & live).any()), "|d| does not straddle 1"
    assert bool(((d == 0) & live.unsqueeze(-1)).any(0).any(0).all()), "no planted zero in one of x, y, yaw"
    assert float(d[..., :2].abs().max()) > 90, "no position error near 100 m"
    assert float(d[..., 2].min()) < -1.8 * np.pi and float(d[..., 2].max()) > 1.8 * np.pi, "yaw differences do not span [-2 pi, 2 pi]"
    assert not bool(one(case["pred_valid"]).all()) and not bool(gt1(case["gt_valid"]).all())
    for name, cfg in IL.CONFIGS.items():
        ex = one(IL.excluded(case, cfg))
        frac = float(ex.double().mean())
        assert frac <= IL.MAX_EXCLUDED, f"{name}: {100 * frac:.2f} % of the elements excluded: pick another seed"
        res = {}
        for dt in (torch.float32, torch.float64):
            dr = DifferentiableReward(**to_attr(IL.reward_cfg(cfg)), w_collision=0.0, use_il_loss=True, reduce_collsion_with_max=True, is_enabled=True)
            pp = one(case["pred_pose"]).to(dt).clone().requires_grad_(True)
            pm = one(case["pred_motion"]).to(dt).clone().requires_grad_(True)
            got = dr.get(one(case["pred_valid"]), pp, pm, gt1(case["gt_valid"]), gt1(case["gt_pose"]).to(dt), gt1(case["gt_motion"]).to(dt), None)
            (got["diffbar_reward"] * w.to(dt)).sum().backward()
            assert not bool(pm.grad[..., 1:].any())
            r4 = torch.stack([got["r_imitation_pos"], got["r_imitation_rot"], got["r_imitation_spd"], got["diffbar_reward"]], -1).detach().double()
            ang = AngularError(cfg[1], cfg[3]).compute(gt1(case["gt_pose"])[..., 2].to(dt), one(case["pred_pose"])[..., 2].to(dt)).double()
            res[dt] = (r4, pp.grad.double(), pm.grad[..., 0].double(), ang, got["diffbar_reward_valid"])
        r64, gp64, gs64, ang64, valid = res[torch.float64]
        r32, gp32, gs32, _, _ = res[torch.float32]
        assert torch.isfinite(r64).all() and torch.isfinite(gp64).all() and torch.isfinite(gs64).all()
        keep = ~ex
        bound_r = float((r32 - r64).abs().max()) / float(r64.abs().max())
        g_scale = max(float(gp64[keep].abs().max()), float(gs64[keep].abs().max()))
        bound_g = max(float((gp32 - gp64)[keep].abs().max()), float((gs32 - gs64)[keep].abs().max())) / g_scale
        print(f"{name}: {100 * frac:.2f} % excluded; reference float32 - float64 relative to the largest magnitude: value {bound_r:.3g} "
              f"(max |r| {float(r64.abs().max()):.4g}), gradient {bound_g:.3g} (max |g| {g_scale:.4g})")
        out[f"{name}/r4"], out[f"{name}/d_pose"], out[f"{name}/d_spd"], out[f"{name}/ang"], out[f"{name}/valid"] = r64, gp64, gs64, ang64, valid
        out[f"{name}/bound_r"], out[f"{name}/bound_g"] = np.float64(bound_r), np.float64(bound_g)
    out["weights"] = np.asarray(IL.WEIGHTS, dtype=np.float64)
    npz("il_loss.npz", **out)


def _train_run(cfg):
    torch.manual_seed(0)
    mcfg0 = ref_model_cfg(n_tgt_knn=4)
    mcfg0["tf_cfg"]["dropout_p"] = 0.0
    mcfg0["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    mcfg0["add_navi_latent"]["mlp_dropout_p"] = 0.0
    wm_t = build_wm(mcfg0, p_training_rollout_prior=0.0, differentiable_reward=dict(IL.reward_cfg(cfg), w_collision=0.0, reduce_collsion_with_max=True,
                                                                                    use_il_loss=True))
    wm_t.teacher_forcing_training.prob_forcing_agent = 0.0
    wm_t.pre_processing[0].dropout_p_history = -1.0
    tb.utils.det_fill(wm_t.model, 0)
    wm_t.train()
    with torch.no_grad():
        for k, p in wm_t.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
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
    base = _train_run(("SmoothL1Loss", "SmoothL1Loss", "SmoothL1Loss", "cosine"))
    out = {}
    for tag, cfg in IL.TRAIN_CONFIGS.items():
        r = _train_run(cfg)
        g1, g0 = float(r["dgradnorm_action_head"]), float(base["dgradnorm_action_head"])
        print(f"train_c1_il {tag}: loss {float(r['dtrain_loss']):.6g} (default criteria: {float(base['dtrain_loss']):.6g}), diffbar_reward "
              f"{float(r['dtrain_diffbar_reward']):.6g} ({float(base['dtrain_diffbar_reward']):.6g}), action_head gradient norm {g1:.6g} ({g0:.6g})")
        assert abs(g1 - g0) > 10 * GNORM_TOL * max(g0, 1e-6), "the configuration does not move the action head's gradient enough"
        for k, v in r.items():
            out[f"{tag}/{k}"] = v
    npz("train_c1_il.npz", **out)


if __name__ == "__main__":
    install_shims()
    which = sys.argv[1:] or ["reward", "train"]
    if "reward" in which:
        gen_reward()
    if "train" in which:
        gen_train()
