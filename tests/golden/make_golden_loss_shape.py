#!/usr/bin/env python
"""Generate tests/golden/loss_shape.npz and tests/golden/train_c1_shaped.npz by running the REFERENCE (the checkout make_golden.py
imports, through its shims) with the loss-shaping switches of `training_metrics` on (temporal_discount, p_loss_for_irrelevant,
w_relevant_agent). Container-only tooling, like make_golden.py; the fixtures hold data only.

loss_shape.npz - the reference's `TrainingMetrics.update` + `compute` on synthetic buffers made from seeded tensors, per case (rows, A, T)
crossed with the switches (the `settings` table, tests/loss_shape_ref.py::SETTING_FIELDS). Per setting: compute()'s dict (`out`, NaN where a
key is left out), the metric's raw states (`sums`), the Bernoulli draw of p_loss_for_irrelevant (`pick`, recorded by wrapping
torch.bernoulli during update: exactly one call when 0 < p < 1, asserted). Per case: the inputs, the reference's per-agent KL / navigation
errors and its float32 discount chain `m` (the `mask_temp` it builds, recorded by wrapping torch.ones_like). w_relevant_agent = 2 is
generated on the A == 1 cases only: the reference's `w_mask_rel.unsqueeze(1)` does not broadcast otherwise. Asserted per case with A >= 5: an
irrelevant agent is picked and one is not; a teacher-forcing reset occurs after the start step; the shaped diffbar_reward is more than 1e-3
(relative) away from the unshaped one. Pick another seed if an assertion fails; never loosen one.

train_c1_shaped.npz - the reference's training_step at the c1 sizes, neutralised as make_golden_collision.py::_train_run does, with
teacher_forcing_training.gt_sdc = True (forced steps inside the free horizon without a random draw), temporal_discount = 0.9,
p_loss_for_irrelevant = 0.5 (the draw recorded), w_relevant_agent = 0. Asserted: the loss and the action head's gradient norm are more than
ten times the test's tolerances away from the unshaped run's.

    python tests/golden/make_golden_loss_shape.py
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import loss_shape_ref as LR  # noqa: E402
from make_golden import build_wm, install_shims, npz, ref_model_cfg, tb  # noqa: E402

# (rows, A, T, seed)
CASES = [(3, 5, 12, 4), (2, 64, 91, 1), (2, 65, 30, 1), (1, 1, 1, 1), (4, 33, 90, 1), (2, 1, 40, 1)]
W_RELEVANT = 2.0
LOSS_TOL, GNORM_TOL = 1e-3, 1e-2  # tests/test_hip_training.py TRAIN_TOL["fp32"]
N_TL, N_MP, LATENT = 3, 20, 16
METRIC_KW = dict(prefix="training", train_navi=True, train_latent=True, w_vae_kl=1.0, kl_balance_scale=0.2, kl_free_nats=1.0, kl_for_unseen_agent=True,
                 w_diffbar_reward=1.0, w_navi=1.0, w_tl_state=1.0)


def case_name(rows, A, T):
    return f"r{rows}_a{A}_t{T}"


def make_case(rows, A, T, seed):
    """Seeded inputs of TrainingMetrics.update with axes [rows, A, T]: teacher forcing over the warm start plus random resets (p = 0.1 per
    step) after it, agent 0 forced throughout and agent 1 never (A >= 2); the last agent never valid (A >= 5); rewards scaled per agent, the
    relevant agents' doubled."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    pred_valid = r(rows, A, T) < 0.85
    tf = (torch.arange(T) < 10).expand(rows, A, T) | (r(rows, A, T) < 0.1)
    if A >= 2:
        tf[:, 0], tf[:, 1] = True, False
    if A >= 5:
        pred_valid[:, A - 1] = False
    reward_valid = pred_valid & (r(rows, A, T) < 0.9)
    ag_role = r(rows, A, 3) < 0.2
    reward = -(0.2 + 1.8 * r(rows, A, 1)) * (1.0 + ag_role.any(-1, keepdim=True).float()) * r(rows, A, T)
    return dict(pred_valid=pred_valid, tf=tf, reward_valid=reward_valid, reward=reward, ag_role=ag_role,
                post_mean=torch.randn(rows, A, LATENT, generator=g), post_log_std=torch.randn(rows, A, LATENT, generator=g) * 0.3,
                post_valid=r(rows, A) < 0.9, prior_valid=r(rows, A) < 0.8, navi_logits=torch.randn(rows, A, N_MP, generator=g),
                navi_valid=r(rows, A) < 0.9, navi_gt=torch.randint(0, N_MP, (rows, A), generator=g), tl_nll=r(rows, N_TL, T),
                tl_nll_invalid=r(rows, N_TL, T) < 0.3)


def settings_of(A, T):
    out = []
    for w in ((0.0, W_RELEVANT) if A == 1 else (0.0,)):
        for d in (-1.0, 0.9):
            for p in (1.0, 0.5, 0.0):
                for tfl in (True, False):
                    for start in (0, 10, T + 1):
                        out.append((d, p, float(tfl), float(start), w))
    return out


class _Recorder:
    """torch.bernoulli / torch.ones_like wrapped for the duration of one update: the draws and the tensors made."""

    def __enter__(self):
        self.draws, self.ones = [], []
        self._b, self._o = torch.bernoulli, torch.ones_like

        def bern(*a, **k):
            out = self._b(*a, **k)
            self.draws.append(out)
            return out

        def ones(*a, **k):
            out = self._o(*a, **k)
            self.ones.append(out)
            return out

        torch.bernoulli, torch.ones_like = bern, ones
        return self

    def __exit__(self, *exc):
        torch.bernoulli, torch.ones_like = self._b, self._o


def gen_case(rows, A, T, seed):
    from models.metrics.training import TrainingMetrics
    from models.modules.distributions import DestCategorical, DiagGaussian

    out = {}
    if True:
        name, c = case_name(rows, A, T), make_case(rows, A, T, seed)
        for k, v in c.items():
            out[f"{name}/{k}"] = v
        j = lambda x: x.clone().unsqueeze(1)  # the joint-future axis update() squeezes; a copy: update() masks pred_valid IN PLACE (:102)
        bufs = lambda: SimpleNamespace(pred_valid=j(c["pred_valid"]), mask_teacher_forcing=j(c["tf"]), tl_state_nll=j(c["tl_nll"]),
                              tl_state_nll_invalid=j(c["tl_nll_invalid"]),
                              diffbar_reward={"diffbar_reward_valid": j(c["reward_valid"]), "diffbar_reward": j(c["reward"])})
        dists = lambda: (DestCategorical(logits=c["navi_logits"].clone(), valid=c["navi_valid"].clone()),
                         DiagGaussian(c["post_mean"].clone(), c["post_log_std"].clone(), valid=c["post_valid"].clone()),
                         DiagGaussian(torch.zeros(rows, A, LATENT), torch.zeros(LATENT), valid=c["prior_valid"].clone()))
        navi, post, prior = dists()
        probe = TrainingMetrics(**METRIC_KW, w_relevant_agent=0, p_loss_for_irrelevant=1.0, step_training_start=0)
        out[f"{name}/kl_err"] = probe.l_vae_kl.compute(post.distribution, prior.distribution)
        out[f"{name}/navi_nll"] = -navi.log_prob(c["navi_gt"])
        settings = settings_of(A, T)
        res, sums, picks, m_ref = np.full((len(settings), len(LR.OUT_KEYS)), np.nan), np.zeros((len(settings), len(LR.SUM_KEYS))), [], None
        relevant = c["ag_role"].any(-1)
        for i, (d, p, tfl, start, w) in enumerate(settings):
            tm = TrainingMetrics(**METRIC_KW, w_relevant_agent=w, p_loss_for_irrelevant=p, step_training_start=int(start), temporal_discount=d,
                                 loss_for_teacher_forcing=bool(tfl))
            navi, post, prior = dists()
            torch.manual_seed(1000 * seed + i)  # (the draw of p_loss_for_irrelevant comes from the global generator)
            with _Recorder() as rec:
                tm.update(bufs(), c["ag_role"].clone(), navi, c["navi_gt"], post, prior)
            assert len(rec.draws) == (1 if 0.0 < p < 1.0 else 0), (name, p, len(rec.draws))
            pick = rec.draws[0].bool().reshape(rows, A) if rec.draws else torch.zeros(rows, A, dtype=torch.bool)
            picks.append(pick)
            if d > 0:
                m = [t for t in rec.ones if t.is_floating_point() and tuple(t.shape) == (rows, A, T)][-1]
                assert m_ref is None or torch.equal(m, m_ref)
                m_ref = m
            got = tm.compute()
            for q, k in enumerate(LR.OUT_KEYS):
                if f"training/{k}" in got:
                    res[i, q] = float(got[f"training/{k}"])
            sums[i] = [float(getattr(tm, k)) for k in LR.SUM_KEYS]
            if A >= 5:
                if 0.0 < p < 1.0:
                    assert bool((pick & ~relevant).any()) and bool((~pick & ~relevant).any()), f"{name}: the draw does not split the irrelevant agents"
                if start <= 10:
                    # (among the agents that are neither forced throughout, nor never, nor never valid; past the warm start too)
                    assert bool((c["tf"] & c["pred_valid"])[:, 2:-1, max(int(start), 10) + 1:].any()), f"{name}: no reset after the start step"
        out[f"{name}/settings"], out[f"{name}/out"], out[f"{name}/sums"] = np.asarray(settings), res, sums
        out[f"{name}/pick"], out[f"{name}/m"] = torch.stack(picks), m_ref
        if A >= 5:  # every shaped setting against the unshaped one of the same start step / forcing switch
            col = LR.OUT_KEYS.index("diffbar_reward")
            base = {(s[2], s[3]): res[i, col] for i, s in enumerate(settings) if s[0] < 0 and s[1] == 1.0}
            for i, s in enumerate(settings):
                if (s[0] > 0 or s[1] < 1.0) and s[3] <= 10:
                    rel = abs(res[i, col] - base[(s[2], s[3])]) / abs(base[(s[2], s[3])])
                    assert rel > 1e-3, f"{name} {s}: the shaping moves diffbar_reward by {rel:.3g} only: pick another seed"
        print(f"{name}: {len(settings)} settings")
    return out


def gen_loss_shape():
    out = {}
    for rows, A, T, seed in CASES:
        out.update(gen_case(rows, A, T, seed))
    npz("loss_shape.npz", **out)


def _train_run(shaped):
    torch.manual_seed(0)
    mcfg0 = ref_model_cfg(n_tgt_knn=4)
    mcfg0["tf_cfg"]["dropout_p"] = 0.0
    mcfg0["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    mcfg0["add_navi_latent"]["mlp_dropout_p"] = 0.0
    d = tb.config.default_sim_cfg()
    tfc, tmc = dict(d["teacher_forcing_training"], gt_sdc=True), dict(d["training_metrics"])
    if shaped:
        tmc.update(temporal_discount=0.9, p_loss_for_irrelevant=0.5, w_relevant_agent=0)
    wm_t = build_wm(mcfg0, p_training_rollout_prior=0.0, teacher_forcing_training=tfc, training_metrics=tmc)
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
    with _Recorder() as rec:
        loss = wm_t.training_step({k: v.clone() for k, v in batch.items()}, 0)
    loss.backward()
    out = {"dtrain_loss": loss.detach()}
    if shaped:
        assert len(rec.draws) == 1, len(rec.draws)
        out["pick"] = rec.draws[0].bool().reshape(1, 8)
    for k, v in wm_t.logged.items():
        out["dtrain_" + k.split("/")[1]] = v.detach() if torch.is_tensor(v) else np.float64(v)
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
    base, r = _train_run(False), _train_run(True)
    l1, l0 = float(r["dtrain_loss"]), float(base["dtrain_loss"])
    g1, g0 = float(r["dgradnorm_action_head"]), float(base["dgradnorm_action_head"])
    role = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)["agent/role"].any(-1)
    print(f"train_c1_shaped: loss {l1:.6g} (unshaped {l0:.6g}), action_head gradient norm {g1:.6g} (unshaped {g0:.6g}); pick {r['pick'].int().tolist()}, "
          f"relevant {role.int().tolist()}")
    assert abs(l1 - l0) > 10 * LOSS_TOL * max(abs(l0), 1e-1), "the shaping does not move the loss enough"
    assert abs(g1 - g0) > 10 * GNORM_TOL * max(g0, 1e-6), "the shaping does not move the action head's gradient enough"
    out = {"temporal_discount": np.float64(0.9), "p_loss_for_irrelevant": np.float64(0.5)}
    out.update(r)
    out.update({"unshaped/" + k: v for k, v in base.items() if k.startswith(("dtrain_", "dgradnorm_"))})
    npz("train_c1_shaped.npz", **out)


if __name__ == "__main__":
    install_shims()
    which = sys.argv[1:] or ["loss", "train"]
    if "loss" in which:
        gen_loss_shape()
    if "train" in which:
        gen_train()
