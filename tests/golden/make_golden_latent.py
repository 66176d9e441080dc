#!/usr/bin/env python
"""Generate tests/golden/latent_c1.npz, tests/golden/train_c1_latent.npz and tests/golden/latent_state_dict_keys.txt by running the
REFERENCE (the checkout make_golden.py imports, through its shims) with the `latent_encoder` section at the configurations of
tests/latent_ref.py::TAGS: a learned (conditional) prior, per-type branches with learned log_std, LayerNorm and shared encoders, and
the categorical family. Container-only tooling, like make_golden.py; the fixtures hold data only.

Weights: latent_ref.det_fill - utils.det_fill(model, 0), then the same name-keyed fill for the `mlp_log_std` heads, which det_fill skips
(every name that contains "log_std") and which would otherwise keep the constructor's random draw.

Scene: make_scene at the c1 sizes with two planted agents (latent_ref.plant, validity bits only; the edited agent/valid is stored):
one seen in the history only at steps the down-sampling skips, one seen in the future only. Both have an invalid learned prior and a
valid posterior.

latent_c1.npz - per tag, eval mode, inputs as validation_step passes them (posterior from gt/*, prior from sc/*): the two
distributions' parameters (mean and per-agent log_std, or logits) and `valid`, the deterministic sample of each and its log_prob, and
the balanced KL [n, A] of (posterior, prior) and of (posterior, posterior) for every (kl_balance_scale, kl_free_nats) of
latent_ref.KL_GRID in float32 and on the parameters cast to float64, with kl_bound = the reference's own largest float32 - float64
difference.

train_c1_latent.npz - the reference's training_step (neutralised as make_golden.py::gen_train does, damped action head) under
torch.manual_seed(7) for latent_ref.TRAIN_RUNS: loss, logged terms, per-module gradient norms, the six spot gradients of
train_c1_il.npz and two more in the prior encoder and the prior head. The categorical runs replace the ONE sampling call of the step by
latent_ref.gumbel_sample on a stored uniform tensor u drawn from torch.Generator().manual_seed(11) (our convention, written here; the
Gaussian runs draw rand(1), then the normal noise, from the CPU stream as the other fixtures rely on).
Asserted per run (a failure is fixed by another seed, never by another cap): at least a quarter of the KL-valid agents have a KL above
kl_free_nats (else the run is recorded with kl_free_nats = 0.0, stored as `kl_free_nats`); the prior encoders' gradient norm is > 0 and
none of their parameters is left without a gradient; vae_kl is away from model_c1.npz's by more than ten times the test's loss tolerance.

    python tests/golden/make_golden_latent.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import latent_ref as LR  # noqa: E402
from make_golden import build_wm, install_shims, npz, ref_model_cfg, tb  # noqa: E402

LOSS_TOL = 1e-3  # tests/test_hip_training.py TRAIN_TOL["fp32"]["loss"]
SPOTS = ("ag_encoder.tf_ag2agmptl.layers.3.attn.linear_rpe.weight", "mp_encoder.tf_mp2mp.layers.0.attn.in_proj_weight",
         "tl_encoder.tf_tl2tlmp.layers.1.attn_src.out_proj_weight", "latent_encoder.ag_encoder_post.input_encoder.mlp.fc_layers.0.weight",
         "navi_predictor.mlp.fc_layers.0.weight", "action_head.mlp_mean.0.fc_layers.0.weight")


def _mcfg(tag):
    assert ref_model_cfg(n_tgt_knn=4).keys() == LR.model_cfg(tb, tag).keys()
    return LR.model_cfg(tb, tag)


def _params(d):
    if hasattr(d, "logits"):
        return {"logits": d.logits}
    return {"mean": d.mean, "log_std": d.stddev.expand_as(d.mean).log()}


def _f64(d):
    from torch.distributions import Independent, Normal, OneHotCategoricalStraightThrough

    if hasattr(d, "logits"):
        return Independent(OneHotCategoricalStraightThrough(logits=d.logits.double()), 1)
    return Independent(Normal(d.mean.double(), d.stddev.expand_as(d.mean).double()), 1)


@torch.no_grad()
def gen_eval():
    from models.metrics.loss import BalancedKL

    batch = LR.c1_batch(tb)
    out, keys = {"agent/valid": batch["agent/valid"]}, []
    for tag in LR.TAGS:
        torch.manual_seed(0)
        wm = build_wm(_mcfg(tag))
        LR.det_fill(tb, wm.model)
        wm.eval()
        sd = wm.model.state_dict()
        keys += [f"{tag} {k} {tuple(v.shape)}" for k, v in sorted(sd.items()) if k.startswith("latent_encoder.latent_dist_")]
        b = wm.pre_processing({k: v.clone() for k, v in {**batch, **tb.synthetic.to_history_batch(batch)}.items()})
        mp_tokens = wm.model.mp_encoder(b["sc/mp_valid"], b["sc/mp_attr"], b["sc/mp_pose"], b["ref/mp_type"])
        tl_tokens = wm.model.tl_encoder.pre_compute(tl_valid=b["gt/tl_valid"], tl_attr=b["sc/tl_attr"], tl_pose=b["sc/tl_pose"], **mp_tokens)
        kw = dict(ag_attr=b["sc/ag_attr"], ag_type=b["ref/ag_type"], mp_tokens=mp_tokens, tl_tokens=tl_tokens)
        post = wm.model.latent_encoder(ag_valid=b["gt/ag_valid"], ag_motion=b["gt/ag_motion"], ag_pose=b["gt/ag_pose"], tl_state=b["gt/tl_state"],
                                       posterior=True, **kw)
        prior = wm.model.latent_encoder(ag_valid=b["sc/ag_valid"], ag_motion=b["sc/ag_motion"], ag_pose=b["sc/ag_pose"], tl_state=b["sc/tl_state"],
                                        posterior=False, **kw)
        learned = not wm.model.latent_encoder.latent_dist_prior.skip_forward
        for side, d in (("post", post), ("prior", prior)):
            for k, v in _params(d).items():
                out[f"{tag}/{side}_{k}"] = v
            out[f"{tag}/{side}_valid"] = d.valid
            s = d.sample(deterministic=True)
            out[f"{tag}/{side}_det_sample"], out[f"{tag}/{side}_det_log_prob"] = s, d.log_prob(s)
        # the planted agents: a valid posterior; under a learned prior an invalid prior (a fixed prior takes the full-rate any())
        for a in (LR.AG_BETWEEN, LR.AG_FUTURE):
            assert bool(post.valid[0, a])
        assert bool(prior.valid[0, LR.AG_BETWEEN]) == (not learned) and not bool(prior.valid[0, LR.AG_FUTURE]), tag
        bound = 0.0
        for alpha, fn in LR.KL_GRID:
            for name, q32, q64 in (("kl", prior.distribution, _f64(prior)), ("kl_same", post.distribution, _f64(post))):
                k32 = BalancedKL(alpha, fn).compute(post.distribution, q32)
                k64 = BalancedKL(alpha, fn).compute(_f64(post), q64)
                assert k32.shape == post.valid.shape and torch.isfinite(k64).all()
                out[f"{tag}/{name}32_a{alpha}_f{fn}"], out[f"{tag}/{name}64_a{alpha}_f{fn}"] = k32, k64
                bound = max(bound, float((k32.double() - k64).abs().max()))
        out[f"{tag}/kl_bound"] = np.float64(bound)
        print(f"latent_c1 {tag}: prior valid {prior.valid[0].int().tolist()}, posterior valid {post.valid[0].int().tolist()}; KL(post || prior) "
              f"{[round(float(x), 3) for x in out[f'{tag}/kl64_a0.0_f0.0'][0]]}; reference float32 - float64: {bound:.3g}")
    (HERE / "latent_state_dict_keys.txt").write_text("\n".join(keys) + "\n")
    npz("latent_c1.npz", **out)


def _train_run(tag, p_prior, free_nats):
    import models.modules.distributions as RD
    from torch.distributions import kl_divergence

    torch.manual_seed(0)
    tm = dict(tb.config.default_sim_cfg()["training_metrics"], kl_free_nats=free_nats)
    wm_t = build_wm(_mcfg(tag), p_training_rollout_prior=float(p_prior), training_metrics=tm)
    wm_t.teacher_forcing_training.prob_forcing_agent = 0.0
    wm_t.pre_processing[0].dropout_p_history = -1.0
    LR.det_fill(tb, wm_t.model)
    wm_t.train()
    with torch.no_grad():
        for k, p in wm_t.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    batch = LR.c1_batch(tb)
    seen, out = {}, {}
    metrics = wm_t.train_metrics_training
    update0 = metrics.update

    def update(buffer, ag_role, navi_pred, navi_gt, latent_post, latent_prior):
        lv = buffer.pred_valid.squeeze(1).clone()
        lv[:, :, : metrics.step_training_start] = False
        seen.update(post=latent_post, prior=latent_prior, kl_valid=latent_post.valid & lv.any(-1))
        return update0(buffer=buffer, ag_role=ag_role, navi_pred=navi_pred, navi_gt=navi_gt, latent_post=latent_post, latent_prior=latent_prior)

    metrics.update = update
    sample0 = RD.MultiCategorical.sample
    if tag in LR.CATEGORICAL:
        calls = []

        def sample(self, deterministic):
            assert deterministic is False and not calls  # the one sampling call of a training step
            u = torch.rand(self.logits.shape, generator=torch.Generator().manual_seed(11)).clamp_(min=torch.finfo(torch.float32).tiny)
            calls.append(u)
            return LR.gumbel_sample(self.logits, u)

        RD.MultiCategorical.sample = sample
    try:
        torch.manual_seed(7)
        loss = wm_t.training_step({k: v.clone() for k, v in batch.items()}, 0)
    finally:
        RD.MultiCategorical.sample = sample0
    loss.backward()
    if tag in LR.CATEGORICAL:
        out["u"] = calls[0]
    out["agent/valid"], out["kl_free_nats"], out["dtrain_loss"] = batch["agent/valid"], np.float64(free_nats), loss.detach()
    for k, v in wm_t.logged.items():
        out["dtrain_" + k.split("/")[1]] = v.detach()
    named = dict(wm_t.model.named_parameters())
    gn = {}
    for k, p in named.items():
        if p.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(p.grad.double().pow(2).sum())
    for k, v in gn.items():
        out["dgradnorm_" + k] = np.float64(v) ** 0.5
    for k in SPOTS + (LR.SPOT_PRIOR_ENC, LR.prior_head_spot(tag)):
        out["dgrad_" + k] = wm_t.model.get_parameter(k).grad[:8, :16]  # (by path: shared encoders are listed once, under _post)
    # ---- what the run must contain
    with torch.no_grad():
        kl = kl_divergence(seen["post"].distribution, seen["prior"].distribution)
    kv = seen["kl_valid"]
    frac = float((kl[kv] > free_nats).double().mean())
    prior_names = [k for k in named if "_encoder_prior." in k or ".latent_dist_prior." in k]
    g_prior = sum(float(named[k].grad.double().pow(2).sum()) for k in prior_names if named[k].grad is not None) ** 0.5
    dead = [k for k in prior_names if named[k].grad is None and named[k].requires_grad]
    base = float(np.load(HERE / "model_c1.npz")["dtrain_vae_kl"])
    vae = float(out["dtrain_vae_kl"])
    print(f"train_c1_latent {tag} p={p_prior} free_nats={free_nats}: loss {float(loss):.6g}, vae_kl {vae:.6g} (default configuration {base:.6g}), "
          f"{int(kv.sum())} KL-valid agents, {100 * frac:.0f} % above the free nats, prior-side gradient norm {g_prior:.4g}, {len(prior_names)} prior-side parameters")
    out["_frac"] = frac
    assert g_prior > 0 and not dead, dead[:4]
    assert abs(vae - base) > 10 * LOSS_TOL * abs(base), "vae_kl is not away from the default configuration's"
    return out


def gen_train():
    res = {}
    for tag, p in LR.TRAIN_RUNS:
        r = _train_run(tag, p, 1.0)
        if r["_frac"] < 0.25:
            r = _train_run(tag, p, 0.0)
            assert r["_frac"] >= 0.25, "fewer than a quarter of the KL-valid agents have a positive KL: pick another seed"
        del r["_frac"]
        for k, v in r.items():
            res[f"{tag}_p{p}/{k}"] = v
    npz("train_c1_latent.npz", **res)


if __name__ == "__main__":
    install_shims()
    which = sys.argv[1:] or ["eval", "train"]
    if "eval" in which:
        gen_eval()
    if "train" in which:
        gen_train()
