"""CPU tests that pin the float64 reference of the closed-loop step and the feature preparation (tests/sim_step_ref.py) and the inputs of
its GPU sweep (tests/sim_step_cases.py) before anything runs on a GPU: the reference is the oracle, the inputs tell every listed defect
from the correct step, the decision band is as thin as the GPU test assumes, and the tolerances are 4 x the float32 yardstick."""
from importlib import import_module

import pytest
import torch

import sim_step_cases as K
import sim_step_ref as R
from oracle import hptr_ops as H
from oracle import trafficbots_oracle as O
from test_oracle_model import build, eval_tokens

N_STEP = 90
# float32 round-off of a logged value after N_STEP closed-loop steps: every step adds a handful (4) of roundings of relative size 2^-24
# to a state entry, the oracle's float32 trajectory carries all of them and the float64 reference none
DRIFT = N_STEP * 4 * 2.0 ** -24


@pytest.fixture(scope="module")
def c1(tb):
    """The model_c1.npz scene (1 scene, 8 agents, 64 polylines, 8 lights): the oracle's reactive replay in eval mode, 90 steps, with the
    rows its agent / map encoders hand to their input encoders captured at every call."""
    cfg, P = build(tb, 4)
    P.pop("__trainable__")
    seen = {"ag_encoder.input_encoder": [], "mp_encoder.input_encoder": []}
    real = H.input_encoder

    def spy(P_, prefix, mode, attr, pe):
        if prefix in seen:
            seen[prefix].append((attr.clone(), pe.clone()))
        return real(P_, prefix, mode, attr, pe)

    H.input_encoder = spy
    try:
        with torch.no_grad():
            b, m, mp, tl = eval_tokens(tb, cfg, P, (8, 64, 8))
            post = m.latent_encoder(b["gt/ag_valid"], b["sc/ag_attr"], b["gt/ag_motion"], b["gt/ag_pose"], b["ref/ag_type"],
                                    b["gt/tl_state"], mp, tl, posterior=True)
            scfg = tb.config.default_sim_cfg()
            ro = O.Sim(m, scfg, training=False).rollout(b, mp, tl, post.sample(True), post.valid, b["gt/ag_navi"], b["gt/ag_valid"].any(-1),
                                                        scfg.teacher_forcing_joint_future_pred, N_STEP)
    finally:
        H.input_encoder = real
    return dict(P=P, b=b, mp=mp, ro=ro, scfg=scfg, seen=seen)


def _mask5(onehot):
    return (onehot.long() << torch.arange(5)).sum(-1).to(torch.uint8)


def _c1_state(c1, W=11):
    """tbx_sim_state_t's fields for the oracle's rollout of the scene: Dynamics.init, empty windows, TrafficRuleChecker._get_dest."""
    b, scfg = c1["b"], c1["scfg"]
    gt_valid, n_gt = b["gt/ag_valid"], b["gt/ag_valid"].shape[2]
    n, A = gt_valid.shape[:2]
    L = b["gt/tl_state"].shape[1]
    dest = O.Sim.dest_info(b["gt/ag_navi"], b["map/valid"], b["map/type"], b["map/pos"], b["map/dir"])
    u8 = lambda x: x.to(torch.uint8)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    rc, T = scfg.differentiable_reward, N_STEP
    S = dict(max_acc=[a for a, _ in O.MAX_ACTION], max_yaw_rate=[y for _, y in O.MAX_ACTION], dt=O.Sim.dt, w_pos=rc.l_pos.weight,
             w_rot=rc.l_rot.weight, w_spd=rc.l_spd.weight, step=torch.tensor([1, 0], dtype=torch.int32),
             ag_valid=u8(gt_valid[:, :, 0]), ag_disabled=z(n, A, dt=torch.uint8), ag_pose=b["gt/ag_pose"][:, :, 0].clone(),
             ag_motion=b["gt/ag_motion"][:, :, 0].clone(), navi_valid=u8(gt_valid.any(-1)), outside_map=z(n, A, dt=torch.uint8),
             dest_reached=z(n, A, dt=torch.uint8), tl_state=_mask5(b["gt/tl_state"][:, :, 0]), hist_valid=z(n, A, W, dt=torch.uint8),
             hist_pose=z(n, A, W, 3), hist_motion=z(n, A, W, 3), hist_tl=torch.full((n, L, W), 0xFF, dtype=torch.uint8),
             ag_type_idx=u8(b["ref/ag_type"].int().argmax(-1)), gt_valid=u8(gt_valid), gt_pose=b["gt/ag_pose"], gt_motion=b["gt/ag_motion"],
             tf_mask=u8(O.Sim.teacher_forcing_mask(gt_valid, **scfg.teacher_forcing_joint_future_pred)), tl_gt=_mask5(b["gt/tl_state"]),
             boundary=b["map/boundary"], dest_pos=dest["pos"].contiguous(), dest_dir=dest["dir"].contiguous(), dest_invalid=u8(dest["invalid"]),
             dest_kind=u8(dest["type"][:, :, :4].any(-1).int() + 2 * dest["type"][:, :, 4].int()), dest_thresh=dest["thresh"],
             out_valid=z(n, A, T, dt=torch.uint8), out_pose=z(n, A, T, 3), out_motion=z(n, A, T, 3), out_action=z(n, A, T, 2),
             out_tl_state=z(n, L, T, dt=torch.uint8), out_outside_map=z(n, A, T, dt=torch.uint8), out_dest_reached=z(n, A, T, dt=torch.uint8),
             out_reward=z(n, A, T, 4), out_reward_valid=z(n, A, T, dt=torch.uint8), out_tf=z(n, A, T, dt=torch.uint8), out_tl_nll=z(n, L, T))
    # the append that opens TrafficBots.forward: the state a step's model call sees is the window's last entry
    S.update({k: v.to(S[k].dtype) for k, v in R.step(S, None, None, R.APPEND)[0].items()})
    return S


def test_the_reference_is_the_oracle(c1):
    """Stepped from the oracle's initial state on the oracle's logged action means and light logits, the reference reproduces every
    logged key of its 90-step rollout: masks equal, floats within DRIFT * (1 + the key's largest magnitude) - the reward within (w_pos + w_rot + w_spd) times
    that, its terms being weighted errors of the pose. At the steps checked, the windows the reference keeps are the oracle's encoder inputs:
    agent_rows equals attr / pe of ag_encoder's input encoder, map_rows those of mp_encoder's."""
    ro, P = c1["ro"], c1["P"]
    S = _c1_state(c1)
    W = S["hist_valid"].shape[2]
    fx, fy = P["ag_encoder.pose_emb.pe_xy.freqs"], P["ag_encoder.pose_emb.pe_yaw.freqs"]
    worst = {}
    for t in range(1, N_STEP + 1):
        if t in (1, 2, 10, 11, 12, 13, 45, 90):  # the window while it fills, full, past the forced steps
            rows = R.agent_rows(S["hist_valid"], S["hist_pose"], S["hist_motion"], c1["b"]["sc/ag_attr"], None, fx, fy, 4 * fx.numel())
            attr, pe = c1["seen"]["ag_encoder.input_encoder"][t - 1]
            k = attr.shape[2]
            n, A = attr.shape[:2]
            assert k == min(t, W) and torch.equal(rows["row_invalid"].view(n, A, W)[:, :, :W - k], torch.ones(n, A, W - k, dtype=torch.bool))
            got_attr, got_pe = rows["attr"].view(n, A, W, 32)[:, :, W - k:], rows["pe"].view(n, A, W, -1)[:, :, W - k:]
            live = ~rows["tok_invalid"]
            torch.testing.assert_close(got_attr[..., :9][live], attr[..., :9].double()[live], rtol=0, atol=DRIFT * 100)
            assert torch.equal(got_attr[..., 9:9 + W], attr[..., 9:].double()) and not bool(got_attr[..., 9 + W:].any())
            err = ((got_pe - pe.double()).abs() / rows["pe__scale"].view(n, A, W, -1)[:, :, W - k:])[live]
            worst["agent pe"] = max(worst.get("agent pe", 0.0), float(err.max()))
            assert float(err.max()) <= DRIFT * 100, t  # (the argument is a rotated offset of up to ~100 m)
        S["action_mean"], S["tl_logits"] = ro["action_mean"][:, :, t - 1].reshape(-1, 2), ro["tl_logits"][:, :, t - 1]
        new, log, _, _ = R.step(S, S["action_mean"], S["tl_logits"])
        want = {"out_valid": ro["pred_valid"], "out_outside_map": ro["outside_map"], "out_dest_reached": ro["dest_reached"],
                "out_reward_valid": ro["diffbar_reward_valid"], "out_tf": ro["mask_teacher_forcing"]}
        for k, v in want.items():
            assert torch.equal(log[k] != 0, v[:, :, t - 1]), (k, t)
        assert torch.equal(log["out_tl_state"], _mask5(ro["tl_state"][:, :, t - 1])), t
        rc = c1["scfg"].differentiable_reward
        for k, got, ref, factor in (("pred_pose", log["out_pose"], ro["pred_pose"], 1), ("pred_motion", log["out_motion"], ro["pred_motion"], 1),
                                    ("action", log["out_action"], ro["action"], 1), ("tl_state_nll", log["out_tl_nll"], ro["tl_state_nll"], 1),
                                    ("diffbar_reward", log["out_reward"][..., 3], ro["diffbar_reward"], rc.l_pos.weight + rc.l_rot.weight + rc.l_spd.weight)):
            size = 1 + float(ref.abs().max())  # roundings are relative to what an entry's terms reach along the rollout, not to where it ends
            err = ((got - ref[:, :, t - 1].double()).abs() / (factor * size)).max()
            worst[k] = max(worst.get(k, 0.0), float(err))
            assert float(err) <= DRIFT, (k, t, float(err))
        S = K.commit(S, new, log)
    print("[reference vs oracle, 90 steps] worst err / (1 + max |key|): " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" (bound {DRIFT:.3g})")


def test_map_rows_are_the_oracles_encoder_inputs(c1):
    b = c1["b"]
    attr, pe = c1["seen"]["mp_encoder.input_encoder"][0]
    rows = R.map_rows(b["sc/mp_valid"], b["sc/mp_attr"], b["sc/mp_pose"])
    n, M, N = b["sc/mp_valid"].shape
    got_attr, got_pe = rows["attr"].view(n, M, N, 32), rows["pe"].view(n, M, N, 8)
    assert torch.equal(got_attr[..., :11 + N], attr.double()) and not bool(got_attr[..., 11 + N:].any()) and not bool(got_pe[..., 7].any())
    err = (got_pe[..., :7] - pe.double()).abs() / rows["pe__scale"].view(n, M, N, 8)[..., :7]
    print(f"[map_rows vs mp_encoder] worst err / scale {float(err.max()):.3g} (bound {8 * 2.0 ** -23:.3g})")
    assert float(err.max()) <= 8 * 2.0 ** -23  # one float32 evaluation (the oracle's) of a handful of operations
    assert torch.equal(rows["tok_pose"], b["sc/mp_pose"][:, :, 0].double()) and torch.equal(rows["tok_invalid"], c1["mp"]["mp_token_invalid"])
    assert torch.equal(rows["row_invalid"].view(n, M, N), ~b["sc/mp_valid"])


def _noise(tb):
    return import_module("trafficbots_amd.hip_base").action_noise


@pytest.fixture(scope="module")
def sim_walks(tb):
    """Per case, the clean float64 trajectory with the float32 evaluation of every launch beside it."""
    return {name: list(K.walk(c, _noise(tb), dtype=torch.float32)) for name, c in K.sim_cases().items()}


def test_decision_band_and_branches(sim_walks):
    """Per step case, the reference alone: the share of (agent, step) pairs with a decision margin inside the band of the GPU test stays
    within its cap, the float64 and the float32 evaluation agree on every mask outside the band, and both branches of every decision are
    taken somewhere in the sweep."""
    seen = {"outside": 0, "inside": 0, "reached": 0, "not reached": 0, "disabled": 0, "forced": 0}
    for name, launches in sim_walks.items():
        n_band = n_pair = 0
        for S, parts, ld, (new, log, scale, mg), (new32, log32, _, _) in launches:
            band = K.band_of(mg)
            if band is None:
                continue
            n_band, n_pair = n_band + int(band.sum()), n_pair + band.numel()
            for k in list(new) + list(log):
                ref, got = (new[k], new32[k]) if k in new else (log[k], log32[k])
                if not ref.dtype.is_floating_point and k in K.AG_KEYS:
                    ne = (ref != got).view(band.shape + (-1,)).any(-1)
                    assert not bool((ne & ~band).any()), (name, k)
            v0 = S["ag_valid"] != 0
            out_now = new["outside_map"] & ~(S["outside_map"] != 0)
            seen["outside"] += int(out_now.sum())
            seen["inside"] += int((v0 & ~out_now).sum())
            reach = new["dest_reached"] & ~(S["dest_reached"] != 0)
            seen["reached"] += int(reach.sum())
            seen["not reached"] += int((v0 & ~new["dest_reached"]).sum())
            seen["disabled"] += int((new["ag_disabled"] & ~(S["ag_disabled"] != 0)).sum())
            seen["forced"] += int((log["out_tf"] != 0).sum()) if "out_tf" in log else 0
        print(f"[band] {name}: {n_band} of {n_pair} agent-steps (allowed {K.band_allowed(n_pair)})")
        assert n_band <= K.band_allowed(n_pair), name
    print(f"[branches] {seen}")
    assert all(v > 0 for v in seen.values()), seen


def test_feedback_checks_are_the_oracles(sim_walks):
    """The scene above leaves the map nowhere and reaches no destination; on the sweep's own states, where both happen, the accumulated
    flags the reference returns are Sim.feedback_checks' on the reference's prediction."""
    n_out = n_reach = 0
    for name in ("base", "nodes33", "nodes70", "stepwise", "past_log"):
        for S, parts, ld, (new, log, scale, mg), _ in sim_walks[name]:
            if not parts & R.AGENTS or not log:
                continue
            kind = S["dest_kind"]
            ty = torch.zeros(kind.shape + (5,), dtype=torch.bool)
            ty[..., 0], ty[..., 4] = (kind & 1) != 0, (kind & 2) != 0
            dest = dict(pos=S["dest_pos"].double(), dir=S["dest_dir"].double(), invalid=S["dest_invalid"] != 0, thresh=S["dest_thresh"].double(), type=ty)
            out_now, reach_now = O.Sim.feedback_checks(S["ag_valid"] != 0, log["out_pose"], S["boundary"].double(), dest, S["dest_reached"] != 0)
            assert torch.equal(new["outside_map"], (S["outside_map"] != 0) | out_now) and torch.equal(new["dest_reached"], (S["dest_reached"] != 0) | reach_now), name
            n_out, n_reach = n_out + int(out_now.sum()), n_reach + int(reach_now.sum())
    assert n_out > 0 and n_reach > 0


def _yardstick(sim_walks):
    inf = {k: float("inf") for k in K.C}
    per_case, worst = {}, {}
    for name, launches in sim_walks.items():
        stats = {}
        for S, parts, ld, (new, log, scale, mg), (new32, log32, _, _) in launches:
            K.check_launch(S, K.commit(S, new32, log32), new, log, scale, K.band_of(mg), stats, name, inf)
        per_case[name] = stats
    for name, c in K.agent_prep_cases().items():
        per_case["agent_prep " + name] = stats = {}
        K.check_rows(K.agent_rows_of(c, dtype=torch.float32), K.agent_rows_of(c), K.PREP_GROUPS, stats, name, inf)
    for name, c in K.map_prep_cases().items():
        per_case["map_prep " + name] = stats = {}
        K.check_rows(R.map_rows(**c, dtype=torch.float32), R.map_rows(**c), K.MAP_GROUPS, stats, name, inf)
    c = K.reward_case()
    per_case["diffbar_reward"] = stats = {}
    a, b = R.reward(**c), R.reward(**c, dtype=torch.float32)
    K._float_check("out4", b[0], a[0], a[2], "reward", None, stats, "reward", inf)
    for stats in per_case.values():
        for k, v in stats.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return per_case, worst


def test_float32_yardstick(sim_walks):
    """The tolerances of the GPU sweep are not taken from a kernel: per output group, c (sim_step_cases.C) is at least 4 x the worst error,
    in units of 2^-23 * scale, of the reference evaluated in float32 on the CPU against its float64 evaluation on the sweep's inputs, and
    c * 2^-23 * scale stays below the cap the rollout tests state for the quantity wherever the value is of the scale's size."""
    per_case, worst = _yardstick(sim_walks)
    for name, stats in per_case.items():
        print(f"[yardstick] {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in stats.items()))
    print("[yardstick] worst: " + ", ".join(f"{k} {v:.3g} (c = {K.C[k]})" for k, v in worst.items()))
    assert set(worst) == set(K.C)
    for k, v in worst.items():
        assert v > 0 and 4 * v <= K.C[k], (k, v, K.C[k])
        assert K.C[k] * K.ULP <= K.CAP.get(k, K.CAP_REST)[0], k


def _detects_sim(defect, sim_cases, noise):
    for name, c in sim_cases.items():
        for S, parts, ld, (new, log, scale, mg), (bnew, blog, _, _) in K.walk(c, noise, defects=(defect,)):
            after = K.commit(S, bnew, blog)
            if K.check_launch(S, after, new, log, scale, K.band_of(mg), {}, name):
                return name
    return None


def test_inputs_discriminate_the_defects(tb):
    """Every defect of sim_step_ref.DEFECTS, injected into the reference (never into anything that runs on a GPU), moves at least one
    compared output of at least one case of the GPU sweep beyond that output's tolerance, or flips a mask - through the comparison the
    GPU test itself uses (check_launch / check_rows). A defect no case catches means a case is missing."""
    sim_cases, caught = K.sim_cases(), {}
    prep = {"last_step", "win64", "dest_tok_frame", "no_batch_div"}
    for d in R.DEFECTS:
        if d in prep:
            hit = [n for n, c in K.agent_prep_cases().items() if K.check_rows(K.agent_rows_of(c, defects=(d,)), K.agent_rows_of(c), K.PREP_GROUPS, {}, n)]
            caught[d] = hit[0] if hit else None
        elif d == "no_clamp":
            hit = [n for n, c in K.map_prep_cases().items() if K.check_rows(R.map_rows(**c, defects=(d,)), R.map_rows(**c), K.MAP_GROUPS, {}, n)]
            caught[d] = hit[0] if hit else None
        else:
            caught[d] = _detects_sim(d, sim_cases, _noise(tb))
    print("[defects] " + ", ".join(f"{d}: {n}" for d, n in caught.items()))
    assert all(caught.values()), [d for d, n in caught.items() if n is None]
    # and the clean reference passes its own comparison everywhere
    assert _detects_sim_clean(sim_cases, _noise(tb)) is None


def _detects_sim_clean(sim_cases, noise):
    for name, c in sim_cases.items():
        for S, parts, ld, (new, log, scale, mg), _ in K.walk(c, noise):
            if K.check_launch(S, K.commit(S, new, log), new, log, scale, K.band_of(mg), {}, name):
                return name
    return None


def test_prep_cases_reach_the_edges():
    """The feature-preparation inputs hold what their docstrings claim: windows whose floats pass index 64 with a last valid step there,
    every validity pattern, both clamps of the projection and a node on the origin."""
    ap = K.agent_prep_cases()
    for W in (22, 23):
        c = ap[f"W{W}_tok3_pe64_full_div1"]
        assert 3 * W > 64 and bool(c["hist_valid"][:, :, W - 1].any()) and bool((c["hist_valid"].sum(-1) == 0).any())
    c = ap["W11_tok515_pe64_full_div1"]
    v = c["hist_valid"].bool()
    last_valid = (v * torch.arange(11)).amax(-1)
    assert bool((v.any(-1) & (last_valid < 10)).any()) and bool((~v.any(-1)).any()) and bool(v.all(-1).any())
    for name, c in K.map_prep_cases().items():
        rows = R.map_rows(**c)
        if name != "nodes1":
            p = rows["proj"]
            assert bool((p < 0).any()) and bool((p > 1).any()) and bool(((p > 0) & (p < 1)).any())
            assert bool((rows["pe"][:, 0].view(p.shape)[:, :, 1:] == 0).any())  # a node on the origin besides the first
