"""GPU checks of the collision term of the differentiable reward (w_collision > 0) above the kernel level: tbx_train_chain_bwd_pose,
the fused training chain and the torch state machine with the term on, `training_step` against the reference's recorded step
(tests/golden/train_c1_collision.npz), the captured step, and the rollout engine / `validation_step`.

The chain tests use the shapes and tolerances of tests/test_hip_training.py::test_train_chain_kernels_vs_torch_state_machine (rtol 1e-3,
atol 1e-5 max|grad|), the training step the fp32 class's TRAIN_TOL of that file, the rollout the bound of tests/test_hip_collision.py."""
import sys
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import collision_ref as CR  # noqa: E402
from test_hip_training import TRAIN_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _fp32_class_by_default():
    TG = import_module("trafficbots_amd.train_graph")
    prev = TG.state.DEFAULT_PRECISION
    TG.state.DEFAULT_PRECISION = "fp32"
    yield
    TG.state.DEFAULT_PRECISION = prev


def _sim_cfg(tb, w_collision, reduce_max, **over):
    scfg = tb.config.default_sim_cfg(**over)
    scfg["differentiable_reward"]["w_collision"] = w_collision
    scfg["differentiable_reward"]["reduce_collsion_with_max"] = reduce_max
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    return scfg


def _chain_setup(tb, w_collision, reduce_max, pull=None):
    """test_train_chain_kernels_vs_torch_state_machine's inputs (3 scenes x 40 agents x 90 steps, tight map boundary, holes in the ground
    truth, extra forcing, random action means); pull: the agents' starts crowded (synthetic.crowd_scene) so that footprints overlap."""
    dev = torch.device(DEV)
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **_sim_cfg(tb, w_collision, reduce_max)).to(dev)
    n, A, T = 3, 40, 90
    raw = tb.synthetic.make_scene(n, A, 64, 8, seed=3)
    if pull is not None:
        raw = tb.synthetic.crowd_scene(raw, pull=pull)
    with torch.no_grad():
        b = wm.pre_processing({k: v.to(dev) for k, v in raw.items()})
    b["map/boundary"] = torch.tensor([[-60.0, 60.0, -60.0, 60.0]], device=dev).repeat(n, 1)
    torch.manual_seed(11)
    b["gt/ag_valid"] = b["gt/ag_valid"] & (torch.rand(b["gt/ag_valid"].shape, device=dev) > 0.1)
    tf = wm.teacher_forcing_training
    tf.init(ag_valid=b["gt/ag_valid"], ag_pose=b["gt/ag_pose"], ag_motion=b["gt/ag_motion"], tl_state=b["gt/tl_state"], current_epoch=0)
    tf_mask = tf.ag_teacher_forcing | (torch.rand(b["gt/ag_valid"].shape, device=dev) < 0.05) & b["gt/ag_valid"]
    g = torch.Generator().manual_seed(2)
    mean0 = (torch.randn(n, T, A, 2, generator=g) * 1.5).to(dev)
    w_r = torch.randn(n, A, T, generator=g).to(dev)
    d_pp = torch.randn(n, A, T, 3, generator=g).to(dev)
    L = b["gt/tl_state"].shape[1]
    tl = {"tl_token_invalid": torch.zeros(n, L, dtype=torch.bool, device=dev)}
    logits = torch.zeros(n, L, 5, device=dev)
    return wm, b, tf_mask, mean0, w_r, d_pp, tl, logits, (n, A, T)


def test_train_chain_bwd_pose_vs_torch_state_machine(tb):
    """d_pred_pose = NULL: tbx_train_chain_bwd, bit for bit. A random d_pred_pose: autograd through the torch state machine with the same
    adjoint injected at the predictions (the loss gets + sum(pred_pose * d_pred_pose))."""
    hip = import_module("trafficbots_amd.hip")
    TG = import_module("trafficbots_amd.train_graph")
    wm, b, tf_mask, mean0, w_r, d_pp, tl, logits, (n, A, T) = _chain_setup(tb, 0, True)
    m1 = mean0.clone().requires_grad_(True)
    ro = TG.training_rollout(wm, b, None, tl, None, None, tf_mask, T, need_hist=False, policy=lambda s, h, v, p, nv: (m1[:, s - 1], logits))
    ((ro["reward"] * w_r).sum() + (ro["pred_pose"] * d_pp).sum()).backward()
    chain = TG.TrainChain(wm, b, tf_mask, T)
    assert chain.collision is None
    m2 = mean0.clone().requires_grad_(True)
    TG.TrainChainFn.apply(m2, chain)
    d_reward = w_r.permute(0, 2, 1).contiguous()
    strides = (T * A * 2, A * 2)
    got, plain, null = (torch.full_like(mean0, float("nan")) for _ in range(3))
    hip.train_chain_bwd(chain.args, mean0, *strides, d_reward, plain)
    hip.train_chain_bwd_pose(chain.args, mean0, *strides, d_reward, None, null)
    assert torch.equal(null.view(torch.int32), plain.view(torch.int32))
    hip.train_chain_bwd_pose(chain.args, mean0, *strides, d_reward, d_pp.permute(0, 2, 1, 3).contiguous(), got)
    scale = float(m1.grad.abs().max())
    print(f"[tbx_train_chain_bwd_pose vs autograd] max |d| {float((got - m1.grad).abs().max()):.3g}, max |grad| {scale:.3g}; "
          f"the injected adjoint moves d(mean) by {float((got - plain).abs().max()):.3g}")
    torch.testing.assert_close(got, m1.grad, rtol=1e-3, atol=1e-5 * scale)
    assert float((got - plain).abs().max()) > 1e-2 * scale  # the extra input matters


@pytest.mark.parametrize("reduce_max", [True, False], ids=["max", "sum"])
def test_fused_chain_with_the_term_equals_torch_state_machine(tb, reduce_max):
    TG = import_module("trafficbots_amd.train_graph")
    wm, b, tf_mask, mean0, w_r, _, tl, logits, (n, A, T) = _chain_setup(tb, 1.0, reduce_max, pull=0.3)
    m1 = mean0.clone().requires_grad_(True)
    ro = TG.training_rollout(wm, b, None, tl, None, None, tf_mask, T, need_hist=False, policy=lambda s, h, v, p, nv: (m1[:, s - 1], logits))
    (ro["reward"] * w_r).sum().backward()
    m2 = mean0.clone().requires_grad_(True)
    chain = TG.TrainChain(wm, b, tf_mask, T)
    out = chain.outputs(TG.TrainChainFn.apply(m2, chain))
    (out["reward"] * w_r).sum().backward()
    for k in ("pred_valid", "reward_valid", "tf"):
        assert torch.equal(out[k], ro[k]), k
    assert torch.equal(out["reward_valid"], out["pred_valid"])  # rewards.py:77
    hit = float((ro["rule_apx"] < 0).float().mean())
    scale = float(m1.grad.abs().max())
    print(f"[fused chain vs torch state machine, w_collision = 1, {'max' if reduce_max else 'sum'}] {100 * hit:.1f} % of the agent-steps collide; reward max |d| "
          f"{float((out['reward'] - ro['reward']).detach().abs().max()):.3g}; d(mean) max |d| {float((m2.grad - m1.grad).abs().max()):.3g} of max |grad| {scale:.3g}")
    assert hit > 0.01
    for k in ("pred_pose", "pred_motion", "reward", "rule_apx"):
        torch.testing.assert_close(out[k], ro[k], rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(m2.grad, m1.grad, rtol=1e-3, atol=1e-5 * scale)
    # the term reaches d(mean): the same chain with the term's weight at zero gives another gradient
    m3 = mean0.clone().requires_grad_(True)
    chain.collision = (0.0,) + chain.collision[1:]
    (chain.outputs(TG.TrainChainFn.apply(m3, chain))["reward"] * w_r).sum().backward()
    assert float((m3.grad - m2.grad).abs().max()) > 1e-3 * scale
    # the no-grad stepping pass (record=...) computes nothing of the term
    rec = {}
    with torch.no_grad():
        ro1 = TG.training_rollout(wm, b, None, tl, None, None, tf_mask, 3, record=rec, policy=lambda s, h, v, p, nv: (mean0[:, s - 1], logits))
    assert "rule_apx" not in ro1


def _train_wm(tb, reduce_max, w_collision=1.0, **over):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    cfg = tb.config.default_model_cfg(n_tgt_knn=4)
    cfg["tf_cfg"]["dropout_p"] = 0.0
    cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = _sim_cfg(tb, w_collision, reduce_max, **over)
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    return W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg)


@pytest.mark.parametrize("reduce_max", [True, False], ids=["max", "sum"])
def test_training_step_with_the_term_vs_reference(tb, golden_dir, reduce_max):
    """test_training_step_vs_oracle_and_reference's procedure (every RNG site neutralised, damped action head) at the c1 sizes on the
    crowded scene, w_collision = 1, fp32 class: loss terms incl. dr_rule_apx, per-module gradient norms, spot gradients."""
    dev = torch.device(DEV)
    g = np.load(golden_dir / "train_c1_collision.npz")
    tag = "max" if reduce_max else "sum"
    wm = _train_wm(tb, reduce_max, float(g["w_collision"]), p_training_rollout_prior=0.0)
    tb.utils.det_fill(wm.model, 0)
    with torch.no_grad():
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    wm = wm.to(dev).train()
    wm.train_precision = "fp32"
    tol = TRAIN_TOL["fp32"]
    batch = tb.synthetic.crowd_scene(tb.synthetic.make_scene(1, 8, 64, 8, seed=0), pull=float(g["crowd_pull"]), size_scale=float(g["crowd_size_scale"]))
    torch.manual_seed(7)
    loss = wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
    loss.backward()
    keys = ("loss", "vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss", "dr_rule_apx")
    gn = {}
    for k, p in wm.model.named_parameters():
        if p.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(p.grad.double().pow(2).sum())
    named = dict(wm.model.named_parameters())
    spots = [x.split("/", 1)[1] for x in g.files if x.startswith(f"{tag}/dgrad_")]
    meas = {"loss": max(abs(float(wm.last_metrics[k]) - float(g[f"{tag}/dtrain_{k}"])) / max(abs(float(g[f"{tag}/dtrain_{k}"])), 1e-1) for k in keys),
            "gnorm": max(abs(v ** 0.5 - float(g[f"{tag}/dgradnorm_{top}"])) / max(float(g[f"{tag}/dgradnorm_{top}"]), 1e-6) for top, v in gn.items()),
            "spot": max(float((named[k[6:]].grad[:8, :16].cpu() - torch.from_numpy(g[f"{tag}/{k}"])).abs().max()) / max(float(np.abs(g[f"{tag}/{k}"]).max()), 1e-12)
                        for k in spots)}
    print(f"[training step, w_collision = 1, {tag}] dr_rule_apx {float(wm.last_metrics['dr_rule_apx']):.6g} (reference {float(g[f'{tag}/dtrain_dr_rule_apx']):.6g}); "
          f"loss terms max rel diff {meas['loss']:.3g}, gradient norms {meas['gnorm']:.3g}, spot blocks max |d| / max |ref| {meas['spot']:.3g}")
    assert float(g[f"{tag}/dtrain_dr_rule_apx"]) < 0
    for k in keys:
        torch.testing.assert_close(wm.last_metrics[k].detach().cpu().float(), torch.from_numpy(np.asarray(g[f"{tag}/dtrain_{k}"])).float(),
                                   rtol=tol["loss"], atol=1e-1 * tol["loss"])
    assert len(gn) >= 6
    for top, v in gn.items():
        ref = float(g[f"{tag}/dgradnorm_{top}"])
        assert abs(v ** 0.5 - ref) <= tol["gnorm"] * max(ref, 1e-6), (top, v ** 0.5, ref)
    for k in spots:
        ref = torch.from_numpy(g[f"{tag}/{k}"])
        torch.testing.assert_close(named[k[6:]].grad[:8, :16].cpu(), ref, rtol=tol["spot_rtol"], atol=1e-5 + tol["spot_atol_rel"] * float(ref.abs().max()))


def test_graphed_train_step_with_the_term_equals_eager(tb):
    """GraphedTrainStep with the term on (its two launches inside the captured forward / backward): after two optimizer steps the replayed
    loss and gradients are the eager step's on the current weights - the tolerances of
    test_graphed_train_step_equals_eager_across_optimizer_steps."""
    dev = torch.device(DEV)
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    torch.manual_seed(0)
    wm = _train_wm(tb, True, 1.0, time_step_end=30).to(dev).train()
    (opt,), _ = wm.configure_optimizers()
    batches = [{k: v.to(dev) for k, v in tb.synthetic.crowd_scene(tb.synthetic.make_scene(2, 8, 64, 8, seed=s), pull=0.06).items()} for s in (0, 2)]
    gs = DP.GraphedTrainStep(wm, opt, batches[0], warmup=1)
    for i in range(2):
        m = gs(batches[i % 2])
        assert "dr_rule_apx" in m and float(m["dr_rule_apx"]) < 0
    gs.opt, gs.clip = torch.optim.SGD(gs.live, lr=0.0), 0
    m = gs(batches[1])
    loss_g, apx_g = float(m["loss"].detach()), float(m["dr_rule_apx"])
    g1 = [g.clone() for g in gs.grads]
    for p in gs.live:
        p.grad = None
    loss = wm.training_step({k: v.clone() for k, v in batches[1].items()}, 0, noise=gs.noise, use_prior=gs.use_prior)
    loss.backward()
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-6)
    assert abs(float(loss.detach()) - loss_g) <= 1e-5 * abs(loss_g)
    assert abs(float(wm.last_metrics["dr_rule_apx"]) - apx_g) <= 1e-5 * abs(apx_g)
    names = {id(p): k for k, p in wm.model.named_parameters()}
    for a, p in zip(g1, gs.live):
        assert close(a, p.grad, 1e-3), names[id(p)]


# ------------------------------------------------------------------------------------------------------------------ rollout
def _rollout_setup(tb, w_collision, reduce_max):
    dev = torch.device(DEV)
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg(n_joint_future_wosac=4)
    scfg["differentiable_reward"]["w_collision"] = w_collision
    scfg["differentiable_reward"]["reduce_collsion_with_max"] = reduce_max
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    return wm.to(dev).eval()


def _crowded_batch(tb, dev, n_sc=1, wosac=False):
    raw = tb.synthetic.crowd_scene(tb.synthetic.make_scene(n_sc, 8, 64, 8, seed=0), pull=0.06)
    full = {**raw, **tb.synthetic.to_history_batch(raw), **(tb.synthetic.make_wosac_keys(n_sc, 8, seed=0) if wosac else {})}
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in full.items()}


def _replay(wm, batch, **kw):
    b = wm.pre_processing(dict(batch))
    mp, tl = wm.encode_scene(b, tl_valid_key="gt/tl_valid")
    valid = b["gt/ag_valid"].any(-1)
    g = torch.Generator().manual_seed(2)
    z = torch.randn(valid.shape[0], 8, 16, generator=g).to(valid.device)
    return b, wm.reactive_replay(b, mp, tl, z, valid, b["gt/ag_navi"], valid, wm.teacher_forcing_reactive_replay, True, **kw)


@pytest.mark.parametrize("reduce_max", [True, False], ids=["max", "sum"])
def test_rollout_logs_the_term(tb, golden_dir, reduce_max):
    """`reactive_replay` on a crowded c1 scene with w_collision = 0.7: the engine's one launch over its finished pose log against the
    restatement of that log; the sum, the mask; and with the weight at 0 the default configuration's buffers, bit for bit."""
    dev = torch.device(DEV)
    g = np.load(golden_dir / "collision_reward.npz")
    tol_c = 8 * float(g["bound_c"]) + 1e-7
    wm = _rollout_setup(tb, 0.7, reduce_max)
    batch = _crowded_batch(tb, dev)
    b, buf = _replay(wm, batch)
    dr = {k: v[:, 0] for k, v in buf.diffbar_reward.items()}  # [1, A, T]
    pv, pp = buf.pred_valid[:, 0].cpu(), buf.pred_pose[:, 0].cpu()
    ref = -0.7 * CR.term_log(pv.permute(0, 2, 1), pp.permute(0, 2, 1, 3), b["ref/ag_size"].cpu(), reduce_max).permute(0, 2, 1)
    err = float((dr["r_traffic_rule_approx"].cpu().double() - ref).abs().max())
    print(f"[rollout, w_collision = 0.7, {'max' if reduce_max else 'sum'}] {100 * float((ref < 0).double().mean()):.1f} % of the agent-steps collide; "
          f"r_traffic_rule_approx vs restatement max |d| {err:.3g} (bound {tol_c:.3g})")
    assert float((ref < 0).double().mean()) > 0.01 and err <= tol_c
    four = dr["r_imitation_pos"] + dr["r_imitation_rot"] + dr["r_imitation_spd"] + dr["r_traffic_rule_approx"]
    torch.testing.assert_close(dr["diffbar_reward"], four, rtol=1e-6, atol=1e-6)
    assert torch.equal(dr["diffbar_reward_valid"], buf.pred_valid[:, 0])
    # with the weight at 0 the same module launches nothing new: hard zeros, the default configuration's log bit for bit
    wm.diffbar_reward.w_collision = 0
    _, buf0 = _replay(wm, batch)
    wm_default = _rollout_setup(tb, 0, True)
    _, buf_d = _replay(wm_default, batch)
    assert torch.equal(buf0.pred_pose, buf.pred_pose) and torch.equal(buf_d.pred_pose, buf.pred_pose)
    assert set(buf0.diffbar_reward) == set(buf_d.diffbar_reward) == set(buf.diffbar_reward)
    for k, v in buf_d.diffbar_reward.items():
        assert torch.equal(buf0.diffbar_reward[k], v), k
    assert not bool(buf0.diffbar_reward["r_traffic_rule_approx"].any())
    # (with the term on the mask is the prediction's validity: wider than pred & gt valid on this scene)
    assert int(buf.diffbar_reward["diffbar_reward_valid"].sum()) >= int(buf_d.diffbar_reward["diffbar_reward_valid"].sum())


def test_stepwise_rollout_logs_the_same_term(tb):
    """`rollout(stepwise=True)` - the reference's Python loop, one `forward` per step - applies the term when its buffer is finished:
    the same reward log as the engine's own loop, bit for bit (the same launch on the same pose log)."""
    dev = torch.device(DEV)
    wm = _rollout_setup(tb, 0.7, True)
    batch = _crowded_batch(tb, dev)
    b, buf = _replay(wm, batch, step_end=20)
    mp, tl = wm.encode_scene(b, tl_valid_key="gt/tl_valid")
    valid = b["gt/ag_valid"].any(-1)
    z = torch.randn(1, 8, 16, generator=torch.Generator().manual_seed(2)).to(dev)
    ag = {"ag_type": b["ref/ag_type"], "ag_size": b["ref/ag_size"], "ag_attr": b["sc/ag_attr"], "gt_valid": b["gt/ag_valid"], "gt_pose": b["gt/ag_pose"],
          "gt_motion": b["gt/ag_motion"], "ag_latent": z, "ag_latent_valid": valid, "ag_navi": b["gt/ag_navi"], "ag_navi_valid": valid}
    step = wm.rollout(ag, mp, tl, b["gt/tl_state"], wm.teacher_forcing_reactive_replay, wm._rule_checker(b, b["gt/ag_navi"], tl), 20, True, stepwise=True)
    assert torch.equal(step.pred_pose, buf.pred_pose[:, 0])
    assert bool((step.diffbar_reward["r_traffic_rule_approx"] < 0).any())
    for k, v in step.diffbar_reward.items():
        assert torch.equal(v, buf.diffbar_reward[k][:, 0]), k


def test_validation_step_includes_the_term(tb):
    dev = torch.device(DEV)
    batch = _crowded_batch(tb, dev, n_sc=2, wosac=True)
    losses = {}
    for w in (0.7, 0):
        wm = _rollout_setup(tb, w, True)
        torch.manual_seed(11)
        assert wm.validation_step(batch, 0) is None
        wm.validation_epoch_end([None])
        losses[w] = (float(wm.logged["val/loss"]), float(wm.logged["reactive_replay/dr_rule_apx"]))
    print(f"[validation_step] val/loss {losses[0.7][0]:.6g} with w_collision = 0.7 (dr_rule_apx {losses[0.7][1]:.6g}), {losses[0][0]:.6g} without")
    assert np.isfinite(losses[0.7][0]) and np.isfinite(losses[0][0]) and losses[0.7][0] != losses[0][0]
    assert losses[0.7][1] < 0 and losses[0][1] == 0
