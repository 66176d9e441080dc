#!/usr/bin/env python
"""Generate tests/golden/tf_threshold.npz, rollout_c1_tfthr.npz and train_c1_tfthr.npz by running the REFERENCE (the checkout
make_golden.py imports, through its shims) with the error thresholds of `TeacherForcing` on (threshold_xy, threshold_yaw, threshold_spd).
Container-only tooling, like make_golden.py; the fixtures hold data only.

tf_threshold.npz - the reference's `TeacherForcing.init` + `get` on seeded tensors, per case (rows, A, Tg, step) of
tests/tf_threshold_ref.py::CASES crossed with its SETTINGS (each threshold alone, all three together). Per case: the inputs, the table after
init (`tf_init`, scheduled sampling at 0.2 so that column `step` already holds bits), the override's pose / motion; per setting the
override's valid and the table AFTER the call (the reference ORs the resets into it in place). Agents 0-4 of a case with A >= 5 are built:
  0  the exactly representable edges: an xy offset of (3, 4) on integer ground truth and a speed offset of 1.5 - reset by 4.99 / 1.25, not
     by 5.0 / 1.5 (strict comparisons), and by nothing in the all-three setting;
  1  invalid in the state, 2 invalid in gt[s-1], both with large errors: no reset;
  3  valid at s-1, invalid at s, with an xy error of 8 (row 0) / a speed error of 3 (row 1): reset although gt[s] is invalid;
  4  a yaw error of -6 rad (row 0: 16.2 degrees after cast_rad, no reset at 20), of +3.3 rad (row 1: 170.9 degrees on the other side of pi:
     reset), of 6.5 rad (further rows).
The other agents draw random errors. Asserted: no random error lies within 1e-4 (relative) of its threshold; every case with A >= 5 has a
reset from each of the three terms alone and an agent none of them resets. Pick another seed if an assertion fails; never loosen one.

rollout_c1_tfthr.npz - the reference's `reactive_replay` at the c1 sizes of model_c1.npz (1 scene, 8 agents; ROLL_STEPS steps) with
thresholds in teacher_forcing_reactive_replay and the damped action head (x 0.02); the flag log, pred_valid, poses, the table after the
rollout, the latent and the thresholds used.
train_c1_tfthr.npz - the reference's training_step, neutralised as make_golden_loss_shape.py::_train_run does (TRAIN_STEPS steps), with
thresholds in teacher_forcing_training: loss, logged terms, gradient norms, gradient slices, the table after the step (column s is step
s's logged flag), and the loss / norms / table of the same step without thresholds (`off/`).
Asserted for both: a reset after the warm start on at least two agents; not every free step is a reset; at every (agent, step) the
schedule leaves free, the error the decision rests on is farther from its threshold than ten times the pose / speed tolerance of the
existing closed-loop test of the family (_GetRecorder.check; the smallest margin is printed); for training, the loss and the action
head's gradient norm move by more than ten times TRAIN_TOL. The thresholds are the first of CANDIDATES that pass.

    python tests/golden/make_golden_tf_threshold.py [kernel] [rollout] [train]
"""
import math
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import tf_threshold_ref as TR  # noqa: E402
from make_golden import build_wm, install_shims, npz, ref_model_cfg, tb  # noqa: E402

N_TL = 2
TF_KW = dict(step_spawn_agent=10, step_warm_start=2, prob_scheduled_sampling=0.2)
XY_THR, YAW_THR, SPD_THR = (5.0, 4.99), (20.0,), (1.5, 1.25)  # every value a setting uses, per term


def make_case(rows, A, Tg, step, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    gt_valid = r(rows, A, Tg) < 0.85
    gt_pose = torch.cat([(r(rows, A, Tg, 2) - 0.5) * 100.0, (r(rows, A, Tg, 1) - 0.5) * 2 * math.pi], -1)
    gt_motion = torch.cat([r(rows, A, Tg, 1) * 15.0, r(rows, A, Tg, 2) - 0.5], -1)
    tl_state = torch.nn.functional.one_hot(torch.randint(0, 5, (rows, N_TL, Tg), generator=g), 5).bool()
    b = min(step - 1, Tg - 1)  # the column the errors are measured against (step > Tg: none is; the last one stands in)
    pred_valid = r(rows, A) < 0.9
    if A == 1:  # the state IS the ground truth
        return dict(gt_valid=gt_valid | True, gt_pose=gt_pose, gt_motion=gt_motion, tl_state=tl_state, pred_valid=pred_valid | True,
                    pred_pose=gt_pose[:, :, b].clone(), pred_motion=gt_motion[:, :, b].clone()), None
    # random errors: a distance in [0, 10] m in a random direction, a yaw error in [-2 pi, 2 pi], a speed error in [-3, 3]
    dist, ang = r(rows, A) * 10.0, r(rows, A) * 2 * math.pi
    err = torch.stack([dist * torch.cos(ang), dist * torch.sin(ang), (r(rows, A) - 0.5) * 4 * math.pi], -1)
    err_spd = (r(rows, A) - 0.5) * 6.0
    built = torch.zeros(rows, A, dtype=torch.bool)
    built[:, :5] = True
    gt_valid[:, :5, b] = True
    pred_valid[:, :5] = True
    s = min(step, Tg - 1)
    # 0: the exact edges
    gt_pose[:, 0, b] = torch.tensor([10.0, -20.0, 0.5])
    gt_motion[:, 0, b, 0] = 4.0
    err[:, 0], err_spd[:, 0] = torch.tensor([3.0, 4.0, 0.0]), 1.5
    # 1: invalid state, 2: invalid gt[s-1]; large errors
    pred_valid[:, 1], gt_valid[:, 2, b] = False, False
    err[:, 1:3], err_spd[:, 1:3] = torch.tensor([30.0, 0.0, 1.0]), 5.0
    # 3: the track ends at s-1
    if s != b:
        gt_valid[:, 3, s] = False
    err[:, 3], err_spd[:, 3] = 0.0, 0.0
    err[0::2, 3, 0], err_spd[1::2, 3] = 8.0, 3.0
    # 4: yaw errors on both sides of pi
    err[:, 4], err_spd[:, 4] = 0.0, 0.0
    gt_pose[:, 4, b, 2] = 3.0
    err[:, 4, 2] = 6.5
    err[0, 4, 2], err[1, 4, 2] = -6.0, 3.3
    pred_pose = gt_pose[:, :, b] + err
    pred_motion = gt_motion[:, :, b].clone()
    pred_motion[..., 0] += err_spd
    return dict(gt_valid=gt_valid, gt_pose=gt_pose, gt_motion=gt_motion, tl_state=tl_state, pred_valid=pred_valid, pred_pose=pred_pose,
                pred_motion=pred_motion), built


def margins(c, built, b):
    """The random agents' errors in float64 against every threshold value in use: the smallest relative distance."""
    ok = (c["pred_valid"] & c["gt_valid"][:, :, b] & ~built)
    e = (c["pred_pose"].double() - c["gt_pose"][:, :, b].double())
    d_xy = e[..., :2].norm(dim=-1)
    d_yaw = torch.rad2deg(torch.remainder(e[..., 2] + math.pi, 2 * math.pi) - math.pi).abs()
    d_spd = (c["pred_motion"][..., 0].double() - c["gt_motion"][:, :, b, 0].double()).abs()
    m = math.inf
    for d, thrs in ((d_xy, XY_THR), (d_yaw, YAW_THR), (d_spd, SPD_THR)):
        for t in thrs:
            if ok.any():
                m = min(m, float(((d[ok] - t).abs() / t).min()))
    return m


@torch.no_grad()
def gen_kernel():
    from utils.teacher_forcing import TeacherForcing

    out = {"settings": np.asarray(TR.SETTINGS)}
    for ci, (rows, A, Tg, step) in enumerate(TR.CASES):
        name = TR.case_name(rows, A, Tg, step)
        c, built = make_case(rows, A, Tg, step, seed=10 + ci)
        b = min(step - 1, Tg - 1)
        if built is not None:
            m = margins(c, built, b)
            assert m > 1e-4, f"{name}: a random error lies within {m:.3g} (relative) of a threshold: pick another seed"
        ov_valid, tf_after, tf_init, ov_pm = [], [], None, None
        for thr in TR.SETTINGS:
            tf = TeacherForcing(**TF_KW, threshold_xy=thr[0], threshold_yaw=thr[1], threshold_spd=thr[2])
            torch.manual_seed(100 + ci)  # (scheduled sampling draws from the global generator: the same table for every setting)
            tf.init(c["gt_valid"].clone(), c["gt_pose"].clone(), c["gt_motion"].clone(), c["tl_state"].clone(), 0)
            t0 = tf.ag_teacher_forcing.clone()
            assert tf_init is None or torch.equal(t0, tf_init)
            tf_init = t0
            ov, _ = tf.get(step, c["pred_valid"].clone(), c["pred_pose"].clone(), c["pred_motion"].clone())
            ov_valid.append(ov["valid"].clone())
            tf_after.append(tf.ag_teacher_forcing.clone())
            pm = (ov["pose"].clone(), ov["motion"].clone())
            assert ov_pm is None or (torch.equal(pm[0], ov_pm[0]) and torch.equal(pm[1], ov_pm[1]))
            ov_pm = pm
        ov_valid, tf_after = torch.stack(ov_valid), torch.stack(tf_after)
        if 0 < step < Tg:
            new = tf_after[:, :, :, step] & ~tf_init[:, :, step]  # [n_set, rows, A]
            assert torch.equal(ov_valid, tf_after[:, :, :, step])  # the override's mask IS the table's column
            if A >= 5:
                alone = {"xy": new[0], "yaw": new[2], "spd": new[3]}
                for k, v in alone.items():
                    assert bool(v.any()), f"{name}: no reset from the {k} term"
                free = c["pred_valid"] & c["gt_valid"][:, :, step - 1] & ~tf_init[:, :, step]
                assert bool((free & ~new.any(0)).any()), f"{name}: every free agent is reset by some setting"
                # the edges: agent 0 is reset by 4.99 / 1.25 and not by 5.0 / 1.5 (where the schedule leaves it free)
                f0 = ~tf_init[:, 0, step]
                assert torch.equal(new[1][:, 0], f0) and torch.equal(new[4][:, 0], f0) and not new[0][:, 0].any() and not new[3][:, 0].any()
                assert not new[5][:, 0].any()
                assert not new[:, :, 1].any() and not new[:, :, 2].any()  # invalid in the state / in gt[s-1]
                assert not c["gt_valid"][:, 3, step].any() and bool(new[5][:, 3].all())  # reset onto invalid ground truth
        else:
            assert not ov_valid.any() and torch.equal(tf_after, tf_init.expand_as(tf_after))
        for k, v in c.items():
            out[f"{name}/{k}"] = v
        out[f"{name}/tf_init"], out[f"{name}/ov_valid"], out[f"{name}/tf_after"] = tf_init, ov_valid, tf_after
        out[f"{name}/ov_pose"], out[f"{name}/ov_motion"] = ov_pm
        print(f"{name}: {int((tf_after & ~tf_init).sum())} new bits over {len(TR.SETTINGS)} settings")
    npz("tf_threshold.npz", **out)

# ---------------------------------------------------------------------------------------------- the two closed-loop fixtures
# Ten times the tolerances of the existing closed-loop tests of the c1 family: tests/test_hip_rollout.py compares poses with the reference
# at atol 5e-3 (metres and radians) and speeds with the oracle at atol <= 1e-2. tests/test_hip_training.py's TRAIN_TOL bounds the loss and
# the gradient norms (relative 1e-3 / 2e-2 at most), not states: the training fixture asks for the same absolute margins and, on top, for
# 10 x 1e-3 of the threshold itself.
POSE_TOL, SPD_TOL = 5e-3, 1e-2
MARGIN = (10 * POSE_TOL, math.degrees(10 * POSE_TOL), 10 * SPD_TOL)  # xy [m], yaw [deg], spd [m/s]
LOSS_TOL, GNORM_TOL = 1e-3, 2e-2  # TRAIN_TOL: the larger of the two precision classes, per quantity
ROLL_STEPS = 40
# candidates (threshold_xy, threshold_yaw, threshold_spd), tried in order: the first that passes every assertion is used. In these scenes
# the damped policy lets the yaw error grow by ~1.5 degrees and the speed error by ~0.05 m/s per step: either would sit inside its band
# (+- 2.9 degrees, +- 0.1 m/s) for several steps around ANY threshold it reaches, so no choice of theirs can decide with the margin asked
# for. The position error grows by 0.3 - 0.7 m per step near 3 m and can step over its band (+- 0.05 m). The yaw and speed thresholds
# are therefore ON but above what a free agent reaches before the position threshold puts it back (tf_threshold.npz is where each term
# decides alone); the position threshold is searched on a grid.
CANDIDATES = [(3.38, 60.0, 3.0), (4.64, 60.0, 3.0)] + [(round(1.0 + 0.07 * i, 2), 60.0, 3.0) for i in range(60)]  # (the two found first)


class _GetRecorder:
    """Wraps a reference TeacherForcing's `get`: per call inside (0, Tg) the three errors in float64 ([n, A, 3]: metres, degrees, m/s; 0 where
    the pair is invalid, as the reference masks them) and the column before the call."""

    def __init__(self, tf):
        self.tf, self.rec, self._get = tf, [], tf.get
        tf.get = self

    def __call__(self, step, pv, pp, pm):
        tf = self.tf
        if 0 < step < tf.ag_teacher_forcing.shape[-1]:
            ok = pv & tf.ag_valid[:, :, step - 1]
            e = pp.double() - tf.ag_pose[:, :, step - 1].double()
            d = torch.stack([e[..., :2].norm(dim=-1), torch.rad2deg(torch.remainder(e[..., 2] + math.pi, 2 * math.pi) - math.pi).abs(),
                             (pm[..., 0].double() - tf.ag_motion[:, :, step - 1, 0].double()).abs()], -1)
            self.rec.append((step, d * ok.unsqueeze(-1), tf.ag_teacher_forcing[:, :, step].clone()))
        return self._get(step, pv, pp, pm)

    def check(self, thr, warm, what, rel=0.0):
        """The generator's assertions on a finished run; returns (smallest margin in units of the required one, new bits [n, A, Tg]).
        The margin of a decision, per (agent, step) the schedule leaves free: a reset stands while ONE term stays above its threshold, so its
        margin is the largest excess among the terms that are on; a non-reset stands while EVERY term stays below, so its margin is the
        smallest shortfall. Each in units of the term's required margin (MARGIN, or rel x the threshold where that is larger). A margin
        above 1 means that no term within ten tolerances of its threshold is the one the decision rests on."""
        tf = self.tf
        new = torch.zeros_like(tf.ag_teacher_forcing)
        worst = math.inf
        on = [j for j, t in enumerate(thr) if t > 0]
        for step, d, before in self.rec:
            new[:, :, step] = tf.ag_teacher_forcing[:, :, step] & ~before
            excess = torch.stack([(d[..., j] - thr[j]) / max(MARGIN[j], rel * thr[j]) for j in on], -1)  # [n, A, terms on]
            m = torch.where((excess > 0).any(-1), excess.max(-1).values, (-excess).min(-1).values)
            assert torch.equal((excess > 0).any(-1) & ~before, new[:, :, step]), f"{what}: the float64 errors decide step {step} differently"
            if (~before).any():
                worst = min(worst, float(m[~before].min()))
        late = new[:, :, warm + 1:]
        assert int(late.any(-1).sum()) >= 2, f"{what}: resets after the warm start on {int(late.any(-1).sum())} agents only"
        free = torch.stack([~b for s_, _, b in self.rec if s_ > warm], -1)  # [n, A, steps after the warm start]: not forced by the schedule
        got = torch.stack([new[:, :, s_] for s_, _, _ in self.rec if s_ > warm], -1)
        assert bool((free & ~got).any()), f"{what}: every free step is a reset"
        assert worst > 1.0, f"{what}: a decision rests on an error within {worst:.3g} x the required margin of its threshold"
        d_all, free_all = torch.stack([r[1] for r in self.rec]), torch.stack([~r[2] for r in self.rec])  # [steps, n, A, 3], [steps, n, A]
        self.by_term = [int(((d_all[..., j] > thr[j]) & free_all).sum()) if thr[j] > 0 else 0 for j in range(3)]  # resets each term alone would make
        return worst, new


def _damp(model):
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)


def _first_passing(run, what):
    errs = []
    for thr in CANDIDATES:
        try:
            return thr, run(thr)
        except AssertionError as e:
            errs.append(f"{thr}: {e}")
            print(f"  {what} {thr}: {e}")
    raise AssertionError(f"{what}: no candidate passes\n" + "\n".join(errs))


@torch.no_grad()
def _rollout_run(thr):
    torch.manual_seed(0)
    d = tb.config.default_sim_cfg()
    tfc = dict(d["teacher_forcing_reactive_replay"], threshold_xy=thr[0], threshold_yaw=thr[1], threshold_spd=thr[2])
    wm = build_wm(ref_model_cfg(n_tgt_knn=4), teacher_forcing_reactive_replay=tfc)
    tb.utils.det_fill(wm.model, 0)
    _damp(wm.model)
    wm.eval()
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    b = wm.pre_processing({k: v.clone() for k, v in {**batch, **tb.synthetic.to_history_batch(batch)}.items()})
    mp_tokens = wm.model.mp_encoder(b["sc/mp_valid"], b["sc/mp_attr"], b["sc/mp_pose"], b["ref/mp_type"])
    tl_tokens = wm.model.tl_encoder.pre_compute(tl_valid=b["gt/tl_valid"], tl_attr=b["sc/tl_attr"], tl_pose=b["sc/tl_pose"], **mp_tokens)
    post = wm.model.latent_encoder(ag_valid=b["gt/ag_valid"], ag_attr=b["sc/ag_attr"], ag_motion=b["gt/ag_motion"], ag_pose=b["gt/ag_pose"],
                                   ag_type=b["ref/ag_type"], tl_state=b["gt/tl_state"], mp_tokens=mp_tokens, tl_tokens=tl_tokens, posterior=True)
    tf = wm.teacher_forcing_reactive_replay
    rec = _GetRecorder(tf)
    wm.hparams.time_step_end = ROLL_STEPS
    buf = wm.reactive_replay(batch=b, mp_tokens=mp_tokens, tl_tokens=tl_tokens, ag_latent=post.sample(deterministic=True),
                             ag_latent_valid=post.valid, ag_navi=b["gt/ag_navi"], ag_navi_valid=b["gt/ag_valid"].any(-1), teacher_forcing=tf,
                             deterministic_action=True)
    worst, new = rec.check(thr, tfc["step_warm_start"], "rollout_c1_tfthr")
    return dict(thresholds=np.asarray(thr), n_step=np.int64(ROLL_STEPS), latent=post.sample(deterministic=True), latent_valid=post.valid,
                mask_teacher_forcing=buf.mask_teacher_forcing[:, 0], pred_valid=buf.pred_valid[:, 0], pred_pose=buf.pred_pose[:, 0],
                pred_motion=buf.pred_motion[:, 0], tf_table=tf.ag_teacher_forcing, new_bits=new, min_margin=np.float64(worst), by_term=np.asarray(rec.by_term))


def gen_rollout():
    thr, out = _first_passing(_rollout_run, "rollout_c1_tfthr")
    new = out["new_bits"]
    print(f"rollout_c1_tfthr: thresholds {thr}; {int(new.sum())} resets on {int(new.any(-1).sum())} agents over {ROLL_STEPS} steps; smallest margin "
          f"{float(out['min_margin']):.3g} x the required one {MARGIN}")
    npz("rollout_c1_tfthr.npz", **out)


TRAIN_STEPS = 60  # hparams.time_step_end of the training fixture: 10 warm-start steps + 50 free ones


def _train_run(thr, backward=True):
    """make_golden_loss_shape.py::_train_run's neutralised training_step (no dropout, posterior latent, no random forcing, damped action
    head, seeds 0 / 7) with thr in teacher_forcing_training (None: the run without thresholds) over TRAIN_STEPS steps."""
    torch.manual_seed(0)
    mcfg0 = ref_model_cfg(n_tgt_knn=4)
    mcfg0["tf_cfg"]["dropout_p"] = 0.0
    mcfg0["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    mcfg0["add_navi_latent"]["mlp_dropout_p"] = 0.0
    d = tb.config.default_sim_cfg()
    tfc = dict(d["teacher_forcing_training"])
    if thr is not None:
        tfc.update(threshold_xy=thr[0], threshold_yaw=thr[1], threshold_spd=thr[2])
    wm_t = build_wm(mcfg0, p_training_rollout_prior=0.0, teacher_forcing_training=tfc, time_step_end=TRAIN_STEPS)
    wm_t.teacher_forcing_training.prob_forcing_agent = 0.0
    wm_t.pre_processing[0].dropout_p_history = -1.0
    tb.utils.det_fill(wm_t.model, 0)
    wm_t.train()
    _damp(wm_t.model)
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    tf = wm_t.teacher_forcing_training
    rec = _GetRecorder(tf)
    torch.manual_seed(7)
    loss = wm_t.training_step({k: v.clone() for k, v in batch.items()}, 0)
    out = {"dtrain_loss": loss.detach(), "tf_table": tf.ag_teacher_forcing.clone()}
    if thr is not None:
        worst, new = rec.check(thr, tfc["step_warm_start"], "train_c1_tfthr", rel=10 * LOSS_TOL)
        out.update(new_bits=new, min_margin=np.float64(worst), by_term=np.asarray(rec.by_term))
    if not backward:
        return out
    loss.backward()
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
    base = _train_run(None)
    l0 = float(base["dtrain_loss"])

    def probe(t):  # forward only: the margins, and the loss against the run without thresholds
        l1 = float(_train_run(t, backward=False)["dtrain_loss"])
        assert abs(l1 - l0) > 10 * LOSS_TOL * max(abs(l0), 1e-1), f"the resets move the loss by {abs(l1 - l0) / abs(l0):.3g} only"

    thr, _ = _first_passing(probe, "train_c1_tfthr")
    r = _train_run(thr)
    l1 = float(r["dtrain_loss"])
    g1, g0 = float(r["dgradnorm_action_head"]), float(base["dgradnorm_action_head"])
    new = r["new_bits"]
    print(f"train_c1_tfthr: thresholds {thr}; {int(new.sum())} resets on {int(new.any(-1).sum())} agents over {TRAIN_STEPS} steps, by term {r['by_term'].tolist()}; "
          f"smallest margin {float(r['min_margin']):.3g} x the required one; loss {l1:.6g} (without thresholds {l0:.6g}), action_head gradient norm "
          f"{g1:.6g} (without {g0:.6g})")
    assert abs(l1 - l0) > 10 * LOSS_TOL * max(abs(l0), 1e-1), "the resets do not move the loss enough"
    assert abs(g1 - g0) > 10 * GNORM_TOL * max(g0, 1e-6), "the resets do not move the action head's gradient enough"
    out = {"thresholds": np.asarray(thr), "n_step": np.int64(TRAIN_STEPS)}
    out.update(r)
    out.update({"off/" + k: v for k, v in base.items() if k.startswith(("dtrain_", "dgradnorm_", "tf_table"))})
    npz("train_c1_tfthr.npz", **out)


if __name__ == "__main__":
    install_shims()
    which = sys.argv[1:] or ["kernel", "rollout", "train"]
    if "kernel" in which:
        gen_kernel()
    if "rollout" in which:
        gen_rollout()
    if "train" in which:
        gen_train()
