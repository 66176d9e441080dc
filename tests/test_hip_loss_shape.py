"""GPU checks of the training objective's loss shaping (temporal_discount, p_loss_for_irrelevant, w_relevant_agent): tbx_loss_shape
against the float64 restatement tests/loss_shape_ref.py on every case of tests/golden/loss_shape.npz, `TrainingMetrics` against the
reference's numbers in that fixture, `training_step` + backward against the reference's recorded step (tests/golden/train_c1_shaped.npz),
the relevance weight end to end, the captured step, and the default configuration launching none of it.

Tolerances: the kernel's masks and float32 weights are exact / bit-equal, its float64 sums within 1e-6 * sum |summand| (the restatement's
own distance to the reference's float32 sums is 1.4e-7 of that, tests/test_loss_shape_ref.py); TrainingMetrics rtol 1e-5, this class's
level in tests/test_hip_utils_surface.py; the training step TRAIN_TOL of tests/test_hip_training.py; the captured step the bounds of
tests/test_hip_collision_training.py::test_graphed_train_step_with_the_term_equals_eager."""
import sys
from importlib import import_module
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import loss_shape_ref as LR  # noqa: E402
from test_hip_training import TRAIN_TOL  # noqa: E402
from test_loss_shape_ref import CASES, case_settings  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _fp32_class_by_default():
    TG = import_module("trafficbots_amd.train_graph")
    prev = TG.state.DEFAULT_PRECISION
    TG.state.DEFAULT_PRECISION = "fp32"
    yield
    TG.state.DEFAULT_PRECISION = prev


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(golden_dir / "loss_shape.npz")


def _layouts(x, T_pad=7):
    """A [rows, A, T] host array on the device three ways, each a [rows, A, T] view: the training chain's [rows, T, A] log permuted, a
    buffer's contiguous [rows, A, T], and a time slice of a wider [rows, A, 3 + T + T_pad] log."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    wide = torch.zeros(*t.shape[:2], 3 + t.shape[2] + T_pad, dtype=t.dtype, device=DEV)
    if t.dtype == torch.bool:
        wide[:] = True  # (what lies beside the slice must not be read: it would turn masks on)
    else:
        wide[:] = float("nan")
    wide[:, :, 3:3 + t.shape[2]] = t
    return {"chain": t.permute(0, 2, 1).contiguous().permute(0, 2, 1), "buffer": t, "slice": wide[:, :, 3:3 + t.shape[2]]}


@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_restatement(tb, fixture, name):
    hip = import_module("trafficbots_amd.hip")
    g = fixture
    arrs = {k: _layouts(g[f"{name}/{k}"]) for k in ("pred_valid", "tf", "reward_valid", "reward")}
    relevant_h = g[f"{name}/ag_role"].any(-1)
    relevant = torch.from_numpy(relevant_h).to(DEV)
    worst_acc, worst_w = 0.0, 0.0
    for i, s in case_settings(g, name):
        pick_h = g[f"{name}/pick"][i]
        ref = LR.shape(g[f"{name}/pred_valid"], g[f"{name}/tf"], relevant_h, pick_h, reward=g[f"{name}/reward"], reward_valid=g[f"{name}/reward_valid"],
                       **{k: s[k] for k in LR.SETTING_FIELDS})
        p = s["p_loss_for_irrelevant"]
        kw = dict(relevant=relevant, pick=torch.from_numpy(pick_h).to(DEV) if 0.0 < p < 1.0 else None, mask_irrelevant=p < 1.0,
                  w_relevant=s["w_relevant_agent"], discount=s["temporal_discount"])
        for lay in ("chain", "buffer", "slice"):
            a = {k: v[lay] for k, v in arrs.items()}
            call = lambda: hip.loss_shape(a["pred_valid"], a["tf"], s["step_training_start"], s["loss_for_teacher_forcing"], reward=a["reward"],
                                          reward_valid=a["reward_valid"], want_w=True, **kw)
            any_valid, w_agent, w, acc = call()
            tag = (name, s, lay)
            assert np.array_equal(any_valid.cpu().numpy().astype(bool), ref["any_valid"]), tag
            assert np.array_equal(w_agent.cpu().numpy().view(np.uint32), ref["w_agent"].view(np.uint32)), tag
            w_h = w.cpu().numpy()
            assert np.array_equal(w_h != 0, ref["rv"]) and np.all(w_h[~ref["rv"]] == 0), tag
            if s["w_relevant_agent"] <= 0:  # w = rv ? m : 0: the discount chain, bit for bit
                assert np.array_equal(w_h[ref["rv"]].view(np.uint32), ref["m"][ref["rv"]].view(np.uint32)), tag
            np.testing.assert_allclose(w_h, ref["w"], rtol=1e-6, atol=0, err_msg=str(tag))
            if ref["rv"].any():
                worst_w = max(worst_w, float(np.max(np.abs(w_h[ref["rv"]] / ref["w"][ref["rv"]] - 1))))
            acc_h = acc.cpu().numpy()
            assert acc_h[1] == ref["count"], tag
            assert abs(acc_h[0] - ref["total"]) <= 1e-6 * ref["abs_total"], (tag, acc_h[0], ref["total"])
            worst_acc = max(worst_acc, abs(acc_h[0] - ref["total"]) / max(ref["abs_total"], 1e-30))
            # a second call: bit-equal
            any2, wa2, w2, acc2 = call()
            assert torch.equal(any2, any_valid) and torch.equal(wa2.view(torch.int32), w_agent.view(torch.int32)), tag
            assert torch.equal(w2.view(torch.int32), w.view(torch.int32)) and torch.equal(acc2.view(torch.int64), acc.view(torch.int64)), tag
            # acc is added to: a caller's accumulator
            mine = torch.tensor([1.5, 2.0], dtype=torch.float64, device=DEV)
            hip.loss_shape(a["pred_valid"], a["tf"], s["step_training_start"], s["loss_for_teacher_forcing"], reward=a["reward"],
                           reward_valid=a["reward_valid"], acc=mine, **kw)
            assert torch.equal(mine, acc + torch.tensor([1.5, 2.0], dtype=torch.float64, device=DEV)), tag
            # the masks alone
            any3, wa3, w3, acc3 = hip.loss_shape(a["pred_valid"], a["tf"], s["step_training_start"], s["loss_for_teacher_forcing"], relevant=kw["relevant"],
                                                 pick=kw["pick"], mask_irrelevant=kw["mask_irrelevant"], w_relevant=kw["w_relevant"])
            assert w3 is None and acc3 is None and torch.equal(any3, any_valid) and torch.equal(wa3.view(torch.int32), w_agent.view(torch.int32)), tag
    print(f"[tbx_loss_shape vs restatement, {name}] acc worst |d| / sum |summand| {worst_acc:.3g} (bound 1e-6); w worst relative {worst_w:.3g} (bound 1e-6)")


@pytest.mark.parametrize("name", ["r3_a5_t12", "r2_a65_t30"])
def test_fully_invalid_log_gives_zero_and_no_nan(tb, fixture, name):
    hip = import_module("trafficbots_amd.hip")
    g = fixture
    a = {k: _layouts(g[f"{name}/{k}"])["chain"] for k in ("pred_valid", "tf", "reward_valid", "reward")}
    relevant = torch.from_numpy(g[f"{name}/ag_role"].any(-1)).to(DEV)
    for pv, rv in ((torch.zeros_like(a["pred_valid"]), a["reward_valid"]), (a["pred_valid"], torch.zeros_like(a["reward_valid"]))):
        reward = torch.full_like(a["reward"], float("nan"))  # (an invalid entry's reward is never read into a sum)
        any_valid, w_agent, w, acc = hip.loss_shape(pv, a["tf"], 0, True, reward=reward, reward_valid=rv, relevant=relevant, w_relevant=2.0, discount=0.9,
                                                    want_w=True)
        assert torch.equal(acc, torch.zeros_like(acc)) and not bool(w.any()) and bool(torch.isfinite(w_agent).all())
        assert bool(any_valid.any()) == bool(pv.any())


def _dists(tb, g, name, dev):
    D = import_module("trafficbots_amd.models.modules.distributions")
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"]).to(dev)
    rows, A = g[f"{name}/post_valid"].shape
    return (D.DestCategorical(logits=t("navi_logits"), valid=t("navi_valid")), D.DiagGaussian(t("post_mean"), t("post_log_std"), valid=t("post_valid")),
            D.DiagGaussian(torch.zeros(rows, A, 16, device=dev), torch.zeros(16, device=dev), valid=t("prior_valid")))


@pytest.mark.parametrize("name", CASES)
def test_training_metrics_vs_reference(tb, fixture, name):
    """TrainingMetrics.update / compute with the recorded pick injected against the reference's compute() dict: every key, rtol 1e-5; the
    buffer in both axis orders. A setting without a switch on takes the class's present path (no kernel call)."""
    TM = import_module("trafficbots_amd.models.metrics.training")
    g = fixture
    arrs = {k: _layouts(g[f"{name}/{k}"]) for k in ("pred_valid", "tf", "reward_valid", "reward")}
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"]).to(DEV)
    navi, post, prior = _dists(tb, g, name, DEV)
    worst = 0.0
    for i, s in case_settings(g, name):
        want = {k: v for k, v in zip(LR.OUT_KEYS, g[f"{name}/out"][i]) if not np.isnan(v)}
        for lay in ("chain", "buffer"):
            buf = SimpleNamespace(pred_valid=arrs["pred_valid"][lay], mask_teacher_forcing=arrs["tf"][lay], tl_state_nll=t("tl_nll"),
                                  tl_state_nll_invalid=t("tl_nll_invalid"),
                                  diffbar_reward={"diffbar_reward_valid": arrs["reward_valid"][lay], "diffbar_reward": arrs["reward"][lay]})
            m = TM.TrainingMetrics(prefix="training", train_navi=True, train_latent=True, w_vae_kl=1.0, kl_balance_scale=0.2, kl_free_nats=1.0,
                                   kl_for_unseen_agent=True, w_diffbar_reward=1.0, w_navi=1.0, w_tl_state=1.0, w_relevant_agent=s["w_relevant_agent"],
                                   p_loss_for_irrelevant=s["p_loss_for_irrelevant"], step_training_start=s["step_training_start"],
                                   temporal_discount=s["temporal_discount"], loss_for_teacher_forcing=s["loss_for_teacher_forcing"])
            m.update(buf, t("ag_role"), navi, t("navi_gt"), post, prior, pick=torch.from_numpy(g[f"{name}/pick"][i]).to(DEV))
            got = m.compute()
            assert {k.split("/")[1] for k in got} == set(want), (name, s, lay, sorted(got), sorted(want))
            for k, v in want.items():
                x = float(got[f"training/{k}"])
                assert abs(x - v) <= 1e-5 * abs(v), (name, s, lay, k, x, v)
                worst = max(worst, abs(x - v) / max(abs(v), 1e-30))
    print(f"[TrainingMetrics vs reference, {name}] worst relative difference {worst:.3g} (bound 1e-5)")


# ------------------------------------------------------------------------------------------------------------------ training step
def _train_wm(tb, **metrics):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    cfg = tb.config.default_model_cfg(n_tgt_knn=4)
    cfg["tf_cfg"]["dropout_p"] = 0.0
    cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    over = metrics.pop("sim", {})
    scfg = tb.config.default_sim_cfg(**over)
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["teacher_forcing_training"]["gt_sdc"] = True
    scfg["training_metrics"].update(metrics)
    return W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg)


def _damped(tb, wm):
    tb.utils.det_fill(wm.model, 0)
    with torch.no_grad():
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    return wm


def _gnorms(wm):
    gn = {}
    for k, p in wm.model.named_parameters():
        if p.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(p.grad.double().pow(2).sum())
    return {k: v ** 0.5 for k, v in gn.items()}


@pytest.mark.parametrize("prec,time_batched", [("fp32", True), ("bf16", True), ("fp32", False), ("bf16", False)])
def test_training_step_shaped_vs_reference(tb, golden_dir, prec, time_batched):
    """test_training_step_vs_oracle_and_reference's procedure (every RNG site neutralised, damped action head) at the c1 sizes with
    gt_sdc, temporal_discount = 0.9 and p_loss_for_irrelevant = 0.5, the reference's recorded draw through wm.loss_irrelevant_pick."""
    dev = torch.device(DEV)
    g = np.load(golden_dir / "train_c1_shaped.npz")
    wm = _damped(tb, _train_wm(tb, temporal_discount=float(g["temporal_discount"]), p_loss_for_irrelevant=float(g["p_loss_for_irrelevant"]),
                               sim=dict(p_training_rollout_prior=0.0))).to(dev).train()
    wm.train_precision, wm.time_batched_training = prec, time_batched
    wm.loss_irrelevant_pick = torch.from_numpy(g["pick"]).to(dev)
    tol = TRAIN_TOL[prec]
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    torch.manual_seed(7)
    loss = wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
    loss.backward()
    keys = ("loss", "vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss")
    gn = _gnorms(wm)
    named = dict(wm.model.named_parameters())
    spots = [x for x in g.files if x.startswith("dgrad_")]
    rel = lambda x, r, floor: abs(x - r) / max(abs(r), floor)
    meas = {"loss": max(rel(float(wm.last_metrics[k].detach()), float(g[f"dtrain_{k}"]), 1e-1) for k in keys),
            "gnorm": max(rel(v, float(g[f"dgradnorm_{top}"]), 1e-6) for top, v in gn.items()),
            "spot": max(float((named[k[6:]].grad[:8, :16].cpu() - torch.from_numpy(g[k])).abs().max()) / max(float(np.abs(g[k]).max()), 1e-12) for k in spots)}
    print(f"[training step, shaped, {prec}, time_batched={time_batched}] loss {float(loss):.6g} (reference {float(g['dtrain_loss']):.6g}, unshaped "
          f"{float(g['unshaped/dtrain_loss']):.6g}); loss terms max rel diff {meas['loss']:.3g}, gradient norms {meas['gnorm']:.3g}, spot blocks max |d| / "
          f"max |ref| {meas['spot']:.3g}")
    for k in keys:
        torch.testing.assert_close(wm.last_metrics[k].detach().cpu().float(), torch.from_numpy(np.asarray(g[f"dtrain_{k}"])).float(),
                                   rtol=tol["loss"], atol=1e-1 * tol["loss"])
    assert len(gn) >= 6
    for top, v in gn.items():
        ref = float(g[f"dgradnorm_{top}"])
        assert abs(v - ref) <= tol["gnorm"] * max(ref, 1e-6), (top, v, ref)
    for k in spots:
        ref = torch.from_numpy(g[k])
        torch.testing.assert_close(named[k[6:]].grad[:8, :16].cpu(), ref, rtol=tol["spot_rtol"], atol=1e-5 + tol["spot_atol_rel"] * float(ref.abs().max()))


def test_relevance_weight_end_to_end(tb):
    """Every agent of the batch relevant, w_relevant_agent = 2: the KL, reward and navigation terms and their gradients are three times the
    w = 0 run's (w_agent = 1 + 2 on every agent that has a loss at all); the light term is untouched."""
    dev = torch.device(DEV)
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    batch["agent/role"] = torch.ones_like(batch["agent/role"])
    res = {}
    for w in (0.0, 2.0):
        wm = _damped(tb, _train_wm(tb, w_relevant_agent=w, sim=dict(p_training_rollout_prior=0.0))).to(dev).train()
        wm.train_precision = "fp32"
        torch.manual_seed(7)
        loss = wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
        loss.backward()
        res[w] = (float(wm.last_metrics["loss"]) - float(wm.last_metrics["tl_state_loss"]), _gnorms(wm)["action_head"], float(wm.last_metrics["tl_state_loss"]))
    tol = TRAIN_TOL["fp32"]
    print(f"[relevance weight] loss - tl_state_loss {res[2.0][0]:.6g} vs 3 x {res[0.0][0]:.6g}; action head gradient norm {res[2.0][1]:.6g} vs 3 x {res[0.0][1]:.6g}")
    assert abs(res[2.0][0] - 3 * res[0.0][0]) <= tol["loss"] * abs(3 * res[0.0][0])
    assert abs(res[2.0][1] - 3 * res[0.0][1]) <= tol["gnorm"] * 3 * res[0.0][1]
    assert res[2.0][2] == res[0.0][2]


def test_graphed_train_step_with_the_switches_on(tb):
    """GraphedTrainStep with temporal_discount and p_loss_for_irrelevant on: the replayed loss and gradients are the eager step's on the
    current weights (the bounds of test_graphed_train_step_with_the_term_equals_eager), and a replay after wm.loss_irrelevant_pick was
    refilled in place follows the new mask."""
    dev = torch.device(DEV)
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    torch.manual_seed(0)
    wm = _train_wm(tb, temporal_discount=0.9, p_loss_for_irrelevant=0.5, sim=dict(time_step_end=30)).to(dev).train()
    wm.loss_irrelevant_pick = torch.zeros(2, 8, dtype=torch.bool, device=dev)
    wm.loss_irrelevant_pick[:, 4:6] = True
    (opt,), _ = wm.configure_optimizers()
    batches = [{k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=s).items()} for s in (0, 2)]
    gs = DP.GraphedTrainStep(wm, opt, batches[0], warmup=1)
    for i in range(2):
        gs(batches[i % 2])
    gs.opt, gs.clip = torch.optim.SGD(gs.live, lr=0.0), 0
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-6)
    names = {id(p): k for k, p in wm.model.named_parameters()}
    losses = []
    for refill in (False, True):
        if refill:
            wm.loss_irrelevant_pick.copy_(torch.tensor([[0, 0, 0, 0, 0, 0, 1, 1]] * 2, dtype=torch.bool, device=dev))  # in place: the graph reads it
        m = gs(batches[1])
        loss_g = float(m["loss"].detach())
        g1 = [g.clone() for g in gs.grads]
        for p in gs.live:
            p.grad = None
        loss = wm.training_step({k: v.clone() for k, v in batches[1].items()}, 0, noise=gs.noise, use_prior=gs.use_prior)
        loss.backward()
        assert abs(float(loss.detach()) - loss_g) <= 1e-5 * abs(loss_g), (refill, float(loss.detach()), loss_g)
        for a, p in zip(g1, gs.live):
            assert close(a, p.grad, 1e-3), (refill, names[id(p)])
        losses.append(loss_g)
    print(f"[captured step, shaped] replayed loss {losses[0]:.6g}; after the pick was refilled in place {losses[1]:.6g}")
    assert abs(losses[1] - losses[0]) > 1e-4 * abs(losses[0])


def test_default_switches_launch_nothing_new(tb, fixture, monkeypatch):
    """A counting stub around hip.loss_shape sees zero calls in training_step, validation_step and TrainingMetrics.update under the default
    configuration - and is reached with a switch on (the stub is in the path it claims to watch)."""
    dev = torch.device(DEV)
    hip = import_module("trafficbots_amd.hip")
    TM = import_module("trafficbots_amd.models.metrics.training")
    real, calls = hip.loss_shape, []
    monkeypatch.setattr(hip, "loss_shape", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    raw = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    batch = {k: v.to(dev) for k, v in raw.items()}
    val = {**raw, **tb.synthetic.to_history_batch(raw), **tb.synthetic.make_wosac_keys(1, 8, seed=0)}
    val = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in val.items()}
    name, g = "r3_a5_t12", fixture
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"]).to(dev)
    buf = SimpleNamespace(pred_valid=t("pred_valid"), mask_teacher_forcing=t("tf"), tl_state_nll=t("tl_nll"), tl_state_nll_invalid=t("tl_nll_invalid"),
                          diffbar_reward={"diffbar_reward_valid": t("reward_valid"), "diffbar_reward": t("reward")})
    navi, post, prior = _dists(tb, g, name, dev)
    seen = {}
    for over in ({}, dict(temporal_discount=0.9)):
        del calls[:]
        wm = _train_wm(tb, sim=dict(n_joint_future_wosac=4), **over).to(dev).train()
        wm.training_step(dict(batch), 0).backward()
        n_train = len(calls)
        wm.eval()
        wm.validation_step(dict(val), 0)
        n_val = len(calls) - n_train
        cfg = tb.config.default_sim_cfg()["training_metrics"]
        cfg.update(over)
        TM.TrainingMetrics(prefix="training", train_navi=True, train_latent=True, **cfg).update(buf, t("ag_role"), navi, t("navi_gt"), post, prior)
        seen[bool(over)] = (n_train, n_val, len(calls) - n_train - n_val)
    assert seen[False] == (0, 0, 0), seen
    assert seen[True] == (1, 1, 1), seen
