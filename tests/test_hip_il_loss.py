"""GPU checks of the configurable imitation terms of the differentiable reward (include/tbx_hip_il.h, libtbx_il.so): the kernel pair
tbx_il_reward_fwd / _bwd against the float64 restatement tests/il_loss_ref.py for every configuration of tests/golden/il_loss.npz,
tbx_train_chain_bwd_state against tbx_train_chain_bwd and autograd through the torch state machine, the rollout engine's log, and the
training step against the reference's recorded steps (tests/golden/train_c1_il.npz), across its three schedules and captured.

Tolerance of the kernel comparison: 4 x the configuration's bound_r / bound_g of the fixture - the reference's own largest float32 -
float64 difference relative to the case's largest magnitude; the kernel's sinf / cosf / fmodf differ from torch's CPU routines by a few
ulp each and up to four such terms add. Measured on MI355X: the test prints the ratio to the bound (profiles/MEASUREMENT_LOG.md)."""
import sys
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import il_loss_ref as IL  # noqa: E402
from test_hip_collision_training import _chain_setup  # noqa: E402
from test_hip_training import TRAIN_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (rows, A, T, n_step_gt, n_k, gt_offset): one step against one step; one agent; slots past the ground truth (and more than one 64-lane
# row of agents); rollouts that share a scene's ground truth
SHAPES = [(3, 17, 1, 1, 1, 0), (2, 1, 5, 6, 1, 1), (2, 65, 7, 4, 1, 1), (4, 33, 3, 4, 2, 1)]
_CASES = {}


@pytest.fixture(autouse=True)
def _fp32_class_by_default():
    TG = import_module("trafficbots_amd.train_graph")
    prev = TG.state.DEFAULT_PRECISION
    TG.state.DEFAULT_PRECISION = "fp32"
    yield
    TG.state.DEFAULT_PRECISION = prev


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load(), h.load_il()
    return h


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "il_loss.npz")


def _case(shape):
    """The seeded inputs of a shape and, per configuration, the float64 restatement: computed once, shared, never written to."""
    if shape not in _CASES:
        rows, A, T, Tg, n_k, off = shape
        case = IL.make_case(rows, A, T, Tg, n_k, off, seed=2)
        w = IL.upstream_weight(rows, T, A)
        _CASES[shape] = (case, w, {name: IL.reward(case, cfg, upstream=w) for name, cfg in IL.CONFIGS.items()})
    return _CASES[shape]


def _views(case, g, layout, dev):
    """The case's log as NON-CONTIGUOUS [rows, T, A(, 3)] views of agent-major / time-major storage with padding, plus like-laid-out
    views for the four output planes and the upstream weight."""
    rows, T, A = case["pred_valid"].shape

    def lay(x):  # x [rows, T, A, ...] -> the same values in a padded buffer of the layout
        tail = x.shape[3:]
        if layout == "agent_major":
            buf = torch.zeros(rows, A, T + 2, *tail, dtype=x.dtype, device=dev)
            v = buf[:, :, 1:T + 1].transpose(1, 2)
        else:
            buf = torch.zeros(rows, T, A + 3, *tail, dtype=x.dtype, device=dev)
            v = buf[:, :, 2:A + 2]
        v.copy_(x.to(dev))
        assert v.data_ptr() != buf.data_ptr() and tuple(v.shape[:3]) == (rows, T, A)  # an offset view of padded storage
        return v

    out4 = lay(torch.full((rows, T, A, 4), float("nan")))
    return (lay(case["pred_valid"].to(torch.uint8)), lay(case["pred_pose"]), lay(case["pred_motion"]), case["gt_valid"].to(torch.uint8).to(dev),
            case["gt_pose"].to(dev), case["gt_motion"].to(dev)), out4, lay(g.float())


@pytest.mark.parametrize("layout", ["agent_major", "time_major"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64_restatement(tb, hip, golden, shape, layout):
    dev = torch.device(DEV)
    rows, A, T, Tg, n_k, off = shape
    case, w, refs = _case(shape)
    views, out4, g = _views(case, w, layout, dev)
    worst = {"r": (0.0, ""), "g": (0.0, "")}
    for name, cfg in IL.CONFIGS.items():
        codes = (hip.IL_CRITERIA[cfg[0]], hip.IL_CRITERIA[cfg[1]], hip.IL_CRITERIA[cfg[2]], hip.IL_ANGULAR[cfg[3]])
        ref = refs[name]
        out4.fill_(float("nan"))
        hip.il_reward_fwd(*views, codes, IL.WEIGHTS, gt_offset=off, n_k=n_k, out4=out4)
        total = hip.il_reward_fwd(*views, codes, IL.WEIGHTS, gt_offset=off, n_k=n_k)  # the sum plane alone
        d_pose, d_spd = hip.il_reward_bwd(*views, codes, IL.WEIGHTS, gt_offset=off, g=g, n_k=n_k)
        got4 = out4.cpu().double()
        assert torch.equal(total.cpu(), out4[..., 3].cpu()) and d_pose.is_contiguous() and d_spd.is_contiguous()
        # masked elements and slots past the ground truth: hard zeros, forward and backward
        dead = ~ref["valid"]
        assert not bool(got4[dead].any()) and not bool(d_pose.cpu()[dead].any()) and not bool(d_spd.cpu()[dead].any())
        if T + off > Tg:
            assert bool(dead[:, Tg - off:].all())
        r_scale = float(ref["r4"].abs().max())
        err_r = float((got4 - ref["r4"]).abs().max()) / r_scale
        ex = IL.excluded(case, cfg)
        assert float(ex.double().mean()) <= IL.MAX_EXCLUDED, name
        keep = ~ex
        gp, gs = d_pose.cpu().double(), d_spd.cpu().double()
        g_scale = max(float(ref["d_pose"][keep].abs().max()), float(ref["d_spd"][keep].abs().max()))
        err_g = max(float((gp - ref["d_pose"])[keep].abs().max()), float((gs - ref["d_spd"])[keep].abs().max())) / g_scale
        br, bg = 4 * float(golden[f"{name}/bound_r"]), 4 * float(golden[f"{name}/bound_g"])
        print(f"[il kernels {shape} {layout} {name}] value err / max |r| {err_r:.3g} = {err_r / br:.2f} x the bound {br:.3g}; "
              f"gradient err / max |g| {err_g:.3g} = {err_g / bg:.2f} x the bound {bg:.3g}; {int(ex.sum())} elements excluded")
        worst["r"], worst["g"] = max(worst["r"], (err_r / br, name)), max(worst["g"], (err_g / bg, name))
        assert err_r <= br, (name, err_r, br)
        assert err_g <= bg, (name, err_g, bg)
        # the planted exact zeros give gradient exactly 0
        live = ref["valid"].unsqueeze(-1) & case["planted"]
        grads = torch.cat([gp, gs.unsqueeze(-1)], -1)
        assert not bool(grads[live].any()), name
        if rows * T * A >= 50:
            assert bool(live.any())
    print(f"[il kernels {shape} {layout}] worst ratio to the bound: value {worst['r'][0]:.2f} ({worst['r'][1]}), gradient {worst['g'][0]:.2f} ({worst['g'][1]})")


def test_all_codes_zero_is_tbx_diffbar_reward(tb, hip):
    dev = torch.device(DEV)
    case = IL.make_case(3, 70, 1, 1, 1, 0, seed=4)
    pv, pp, pm = case["pred_valid"][:, 0].to(torch.uint8).to(dev), case["pred_pose"][:, 0].contiguous().to(dev), case["pred_motion"][:, 0].contiguous().to(dev)
    gv, gp, gm = case["gt_valid"][:, :, 0].to(torch.uint8).to(dev), case["gt_pose"][:, :, 0].contiguous().to(dev), case["gt_motion"][:, :, 0].contiguous().to(dev)
    want, _ = hip.diffbar_reward(pv, pp, pm, gv, gp, gm, *IL.WEIGHTS)
    n, A = pv.shape
    got = torch.empty(n, 1, A, 4, device=dev)
    hip.il_reward_fwd(pv.view(n, 1, A), pp.view(n, 1, A, 3), pm.view(n, 1, A, 3), gv.view(n, A, 1), gp.view(n, A, 1, 3), gm.view(n, A, 1, 3), (0, 0, 0, 0),
                      IL.WEIGHTS, gt_offset=0, out4=got)
    assert bool((want != 0).any())
    torch.testing.assert_close(got[:, 0], want, rtol=1e-6, atol=1e-6)
    # ... and the module: Huber is SmoothL1 under another name, through the new kernel
    R = import_module("trafficbots_amd.utils.rewards")
    mk = lambda cfg: R.DifferentiableReward(**IL.reward_cfg(cfg), w_collision=0, use_il_loss=True, reduce_collsion_with_max=True)
    a = mk(IL.CONFIGS["SmoothL1Loss_cosine"]).get(pv, pp, pm, gv, gp, gm)
    b = mk(IL.CONFIGS["HuberLoss_cosine"]).get(pv, pp, pm, gv, gp, gm)
    assert a.keys() == b.keys() and torch.equal(a["diffbar_reward_valid"], b["diffbar_reward_valid"])
    for k in a:
        torch.testing.assert_close(b[k].float(), a[k].float(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", ["rot_None_L1Loss", "rot_cast_MSELoss", "rot_vector_SmoothL1Loss", "SmoothL1Loss_cosine"])
def test_angular_error_on_device_tensors(tb, hip, golden, name):
    L = import_module("trafficbots_amd.models.metrics.loss")
    cfg = IL.CONFIGS[name]
    gw, pw = torch.from_numpy(golden["gt_pose"])[:, :, 0, 2], torch.from_numpy(golden["pred_pose"])[:, 0, :, 2]
    got = L.AngularError(cfg[1], cfg[3]).compute(gw.to(DEV), pw.to(DEV))
    ref = torch.from_numpy(golden[f"{name}/ang"])
    # The rotation term alone at weight 1 (the fixture's bound_r is relative to the largest |r| of ALL terms at the fixture's weights, so
    # it does not apply). Bound from the number format: the float32 argument of the criterion carries at most three roundings of half an
    # ulp at magnitudes below 16 (gw - pw, + pi, - pi: 3 x 4.8e-7 = 1.5e-6 rad), the steepest criterion here is MSE with |crit'| <= 2 x
    # 2 pi, so |error| <= 1.9e-5 against a largest error of at least pi^2 (cast) : 2e-6 of the largest value, the same for the other types.
    err = float((got.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print(f"[AngularError {name}] err / max |e| {err:.3g}")
    assert got.shape == gw.shape and err <= 2e-6


# ------------------------------------------------------------------------------------------------------------------ the chain
def test_train_chain_bwd_state_vs_torch_state_machine(tb, hip):
    """Both adjoints NULL: tbx_train_chain_bwd, bit for bit. Random d_pred_pose and d_pred_spd: autograd through the torch state machine
    with the same adjoints injected at the predictions (the loss gets + sum(pred_pose * d_pred_pose) + sum(pred_speed * d_pred_spd))."""
    TG = import_module("trafficbots_amd.train_graph")
    wm, b, tf_mask, mean0, w_r, d_pp, tl, logits, (n, A, T) = _chain_setup(tb, 0, True)
    d_sp = torch.randn(n, A, T, generator=torch.Generator().manual_seed(3)).to(DEV)
    m1 = mean0.clone().requires_grad_(True)
    ro = TG.training_rollout(wm, b, None, tl, None, None, tf_mask, T, need_hist=False, policy=lambda s, h, v, p, nv: (m1[:, s - 1], logits))
    ((ro["reward"] * w_r).sum() + (ro["pred_pose"] * d_pp).sum() + (ro["pred_motion"][..., 0] * d_sp).sum()).backward()
    chain = TG.TrainChain(wm, b, tf_mask, T)
    assert chain.collision is None and chain.il is None
    TG.TrainChainFn.apply(mean0.clone().requires_grad_(True), chain)
    d_reward = w_r.permute(0, 2, 1).contiguous()
    strides = (T * A * 2, A * 2)
    got, plain, null, pose_only, pose_ref = (torch.full_like(mean0, float("nan")) for _ in range(5))
    hip.train_chain_bwd(chain.args, mean0, *strides, d_reward, plain)
    hip.train_chain_bwd_state(chain.args, mean0, *strides, d_reward, None, None, null)
    assert torch.equal(null.view(torch.int32), plain.view(torch.int32))
    dp, ds = d_pp.permute(0, 2, 1, 3).contiguous(), d_sp.permute(0, 2, 1).contiguous()
    hip.train_chain_bwd_pose(chain.args, mean0, *strides, d_reward, dp, pose_ref)
    hip.train_chain_bwd_state(chain.args, mean0, *strides, d_reward, dp, None, pose_only)
    assert torch.equal(pose_only.view(torch.int32), pose_ref.view(torch.int32))
    hip.train_chain_bwd_state(chain.args, mean0, *strides, d_reward, dp, ds, got)
    scale = float(m1.grad.abs().max())
    print(f"[tbx_train_chain_bwd_state vs autograd] max |d| {float((got - m1.grad).abs().max()):.3g}, max |grad| {scale:.3g}; "
          f"the speed adjoint moves d(mean) by {float((got - pose_only).abs().max()):.3g}")
    torch.testing.assert_close(got, m1.grad, rtol=1e-3, atol=1e-5 * scale)
    assert float((got - pose_only).abs().max()) > 1e-2 * scale  # the extra input matters


# ------------------------------------------------------------------------------------------------------------------ rollout
def _rollout_wm(tb, cfg):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg(n_joint_future_wosac=4)
    if cfg is not None:
        scfg["differentiable_reward"].update(IL.reward_cfg(cfg))
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    return wm.to(torch.device(DEV)).eval()


def _replay(wm, batch, **kw):
    b = wm.pre_processing(dict(batch))
    mp, tl = wm.encode_scene(b, tl_valid_key="gt/tl_valid")
    valid = b["gt/ag_valid"].any(-1)
    z = torch.randn(valid.shape[0], 8, 16, generator=torch.Generator().manual_seed(2)).to(valid.device)
    return b, mp, tl, z, wm.reactive_replay(b, mp, tl, z, valid, b["gt/ag_navi"], valid, wm.teacher_forcing_reactive_replay, True, **kw)


def _count_il_calls(monkeypatch):
    """Every call into libtbx_il.so goes through hip_train.load_il(): count them by entry point."""
    HT = import_module("trafficbots_amd.hip_train")
    real, calls = HT.load_il, []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real(), name)

            def call(*a):
                calls.append(name)
                return fn(*a)
            return call

    monkeypatch.setattr(HT, "load_il", lambda: Counting())
    return calls


def test_rollout_logs_the_configured_terms(tb, hip, monkeypatch):
    """`reactive_replay` on a c1 scene with MSE position / L1 speed / cast + SmoothL1 heading: the engine's one launch over its finished
    log gives, slot by slot, what `DifferentiableReward.get` gives on that slot's logged prediction and ground truth; the mask is the
    default configuration's; the step-wise driver logs the same; the default configuration never calls into libtbx_il.so."""
    dev = torch.device(DEV)
    cfg = IL.TRAIN_CONFIGS["mse_l1_cast"]
    raw = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in {**raw, **tb.synthetic.to_history_batch(raw)}.items()}
    calls = _count_il_calls(monkeypatch)
    wm_d = _rollout_wm(tb, None)
    _, _, _, _, buf_d = _replay(wm_d, batch)
    assert calls == [] and wm_d.diffbar_reward.il_default
    wm = _rollout_wm(tb, cfg)
    b, mp, tl, z, buf = _replay(wm, batch)
    assert calls == ["tbx_il_reward_fwd"]  # ONE launch over the finished log
    assert torch.equal(buf.pred_pose, buf_d.pred_pose) and torch.equal(buf.pred_valid, buf_d.pred_valid)  # the reward never feeds back
    dr, dr_d = {k: v[:, 0] for k, v in buf.diffbar_reward.items()}, {k: v[:, 0] for k, v in buf_d.diffbar_reward.items()}  # [1, A, T]
    assert torch.equal(dr["diffbar_reward_valid"], dr_d["diffbar_reward_valid"])
    assert not torch.equal(dr["diffbar_reward"], dr_d["diffbar_reward"]) and not bool(dr["r_traffic_rule_approx"].any())
    T, Tg = buf.pred_valid.shape[-1], b["gt/ag_valid"].shape[-1]
    pv, pp, pm = buf.pred_valid[:, 0], buf.pred_pose[:, 0], buf.pred_motion[:, 0]
    keys = ("r_imitation_pos", "r_imitation_rot", "r_imitation_spd", "diffbar_reward")
    for t in range(T):
        s = t + 1
        gt = (b["gt/ag_valid"][:, :, s], b["gt/ag_pose"][:, :, s], b["gt/ag_motion"][:, :, s]) if s < Tg else (None, None, None)
        one = wm.diffbar_reward.get(pv[:, :, t], pp[:, :, t], pm[:, :, t], *gt)
        for k in keys:
            assert torch.equal(dr[k][:, :, t], one[k]), (k, t)
        assert torch.equal(dr["diffbar_reward_valid"][:, :, t], one["diffbar_reward_valid"]), t
    four = dr["r_imitation_pos"] + dr["r_imitation_rot"] + dr["r_imitation_spd"]
    torch.testing.assert_close(dr["diffbar_reward"], four, rtol=1e-6, atol=1e-6)
    # against the float64 restatement of the logged slots
    case = dict(pred_valid=pv.permute(0, 2, 1).cpu(), pred_pose=pp.permute(0, 2, 1, 3).cpu(), pred_motion=pm.permute(0, 2, 1, 3).cpu(),
                gt_valid=b["gt/ag_valid"].cpu(), gt_pose=b["gt/ag_pose"].float().cpu(), gt_motion=b["gt/ag_motion"].float().cpu(), n_k=1, gt_offset=1)
    ref = IL.reward(case, cfg)["r4"].permute(0, 2, 1, 3)
    got = torch.stack([dr[k] for k in keys], -1).cpu().double()
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) and float(ref.abs().max()) > 0
    # the step-wise driver (the reference's Python loop, one `forward` per step) takes the same values through DifferentiableReward
    valid = b["gt/ag_valid"].any(-1)
    ag = {"ag_type": b["ref/ag_type"], "ag_size": b["ref/ag_size"], "ag_attr": b["sc/ag_attr"], "gt_valid": b["gt/ag_valid"], "gt_pose": b["gt/ag_pose"],
          "gt_motion": b["gt/ag_motion"], "ag_latent": z, "ag_latent_valid": valid, "ag_navi": b["gt/ag_navi"], "ag_navi_valid": valid}
    _, _, _, _, buf12 = _replay(wm, batch, step_end=12)
    step = wm.rollout(ag, mp, tl, b["gt/tl_state"], wm.teacher_forcing_reactive_replay, wm._rule_checker(b, b["gt/ag_navi"], tl), 12, True, stepwise=True)
    assert torch.equal(step.pred_pose, buf12.pred_pose[:, 0])
    assert not torch.equal(buf12.diffbar_reward["diffbar_reward"][..., :12], buf_d.diffbar_reward["diffbar_reward"][..., :12])
    for k, v in step.diffbar_reward.items():
        assert torch.equal(v, buf12.diffbar_reward[k][:, 0]), k


# ------------------------------------------------------------------------------------------------------------------ training
def _train_wm(tb, cfg, **over):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    mcfg = tb.config.default_model_cfg(n_tgt_knn=4)
    mcfg["tf_cfg"]["dropout_p"] = 0.0
    mcfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    mcfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg(**over)
    scfg["differentiable_reward"].update(IL.reward_cfg(cfg))
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    wm = W.WaymoMotion(model=mcfg, data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    with torch.no_grad():
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    return wm


@pytest.mark.parametrize("tag", list(IL.TRAIN_CONFIGS))
def test_training_step_vs_reference(tb, golden_dir, tag, monkeypatch):
    """test_training_step_vs_oracle_and_reference's procedure (every RNG site neutralised, damped action head) at the c1 sizes with the
    configuration's criteria, fp32 class: loss terms, per-module gradient norms, spot gradients against the reference's recorded step."""
    dev = torch.device(DEV)
    g = np.load(golden_dir / "train_c1_il.npz")
    calls = _count_il_calls(monkeypatch)
    wm = _train_wm(tb, IL.TRAIN_CONFIGS[tag], p_training_rollout_prior=0.0).to(dev).train()
    wm.train_precision = "fp32"
    tol = TRAIN_TOL["fp32"]
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    torch.manual_seed(7)
    loss = wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
    loss.backward()
    assert sorted(calls) == ["tbx_il_reward_bwd", "tbx_il_reward_fwd", "tbx_train_chain_bwd_state"]  # two launches more than the default's step
    keys = ("loss", "vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss")
    gn = {}
    for k, p in wm.model.named_parameters():
        if p.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(p.grad.double().pow(2).sum())
    named = dict(wm.model.named_parameters())
    spots = [x.split("/", 1)[1] for x in g.files if x.startswith(f"{tag}/dgrad_")]
    meas = {"loss": max(abs(float(wm.last_metrics[k].detach()) - float(g[f"{tag}/dtrain_{k}"])) / max(abs(float(g[f"{tag}/dtrain_{k}"])), 1e-1) for k in keys),
            "gnorm": max(abs(v ** 0.5 - float(g[f"{tag}/dgradnorm_{top}"])) / max(float(g[f"{tag}/dgradnorm_{top}"]), 1e-6) for top, v in gn.items()),
            "spot": max(float((named[k[6:]].grad[:8, :16].cpu() - torch.from_numpy(g[f"{tag}/{k}"])).abs().max()) / max(float(np.abs(g[f"{tag}/{k}"]).max()), 1e-12)
                        for k in spots)}
    print(f"[training step, {tag}] diffbar_reward {float(wm.last_metrics['diffbar_reward']):.6g} (reference {float(g[f'{tag}/dtrain_diffbar_reward']):.6g}); "
          f"loss terms max rel diff {meas['loss']:.3g}, gradient norms {meas['gnorm']:.3g}, spot blocks max |d| / max |ref| {meas['spot']:.3g}")
    for k in keys:
        torch.testing.assert_close(wm.last_metrics[k].detach().cpu().float(), torch.from_numpy(np.asarray(g[f"{tag}/dtrain_{k}"])).float(),
                                   rtol=tol["loss"], atol=1e-1 * tol["loss"])
    assert len(gn) >= 6 and len(spots) == 6
    for top, v in gn.items():
        ref = float(g[f"{tag}/dgradnorm_{top}"])
        assert abs(v ** 0.5 - ref) <= tol["gnorm"] * max(ref, 1e-6), (top, v ** 0.5, ref)
    for k in spots:
        ref = torch.from_numpy(g[f"{tag}/{k}"])
        torch.testing.assert_close(named[k[6:]].grad[:8, :16].cpu(), ref, rtol=tol["spot_rtol"], atol=1e-5 + tol["spot_atol_rel"] * float(ref.abs().max()))


@pytest.mark.parametrize("tag", list(IL.TRAIN_CONFIGS))
def test_fused_chain_equals_the_torch_schedules(tb, tag):
    """The fused chain (tbx_il_reward_fwd / _bwd + tbx_train_chain_bwd_state) against the torch state machine behind fused_train_chain =
    False and against the plain step-by-step loop (time_batched_training = False), which use the torch criteria and the AngularError
    expressions: the metrics and tolerances of test_time_batched_training_rollout_equals_step_by_step_autograd (C1_SHAPE, no dropout)."""
    dev = torch.device(DEV)
    wm = _train_wm(tb, IL.TRAIN_CONFIGS[tag], p_training_rollout_prior=0.0, time_step_end=30).to(dev).train()
    wm.attn_dropout_seed = torch.tensor([4242], dtype=torch.int64, device=dev)
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=1).items()}
    noise = torch.randn(2, 8, wm.model.latent_encoder.out_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    use_prior = torch.zeros((), dtype=torch.bool, device=dev)
    res = {}
    for mode, (batched, fused) in {"fused": (True, True), "torch_chain": (True, False), "stepwise": (False, True)}.items():
        wm.time_batched_training, wm.fused_train_chain = batched, fused
        wm.zero_grad(set_to_none=True)
        loss = wm.training_step({k: v.clone() for k, v in batch.items()}, 0, noise=noise, use_prior=use_prior)
        loss.backward()
        res[mode] = ({k: float(v.detach()) for k, v in wm.last_metrics.items()}, {k: p.grad.clone() for k, p in wm.model.named_parameters() if p.grad is not None})
    for other in ("torch_chain", "stepwise"):
        worst = 0.0
        for k, v in res[other][0].items():
            assert abs(res["fused"][0][k] - v) <= 2e-5 * max(abs(v), 1e-3), (other, k, res["fused"][0][k], v)
        assert res["fused"][1].keys() == res[other][1].keys()
        for k, gs in res[other][1].items():
            err = (res["fused"][1][k] - gs).double()
            rel_l2 = float(err.norm()) / max(float(gs.double().norm()), 1e-6 * gs.numel() ** 0.5)
            relu_fed = any(t in k for t in (".linear1.", ".norm2.", "log_std"))
            worst = max(worst, rel_l2)
            assert rel_l2 <= (1e-2 if relu_fed else 2e-3), (other, k, rel_l2, float(err.abs().max()), float(gs.abs().max()))
            n_big = int((err.abs() > 1e-3 * max(float(gs.abs().max()), 1e-6)).sum())
            assert relu_fed or n_big <= max(2, gs.numel() // 200), (other, k, n_big, gs.numel())
        print(f"[fused chain vs {other}, {tag}] loss {res['fused'][0]['loss']:.6g} / {res[other][0]['loss']:.6g}; worst parameter-gradient rel L2 {worst:.3g}")


def test_graphed_train_step_equals_eager(tb):
    """GraphedTrainStep with the first configuration (the new launches inside the captured forward / backward): after one optimizer step
    the replayed loss and gradients are the eager step's on the current weights - the tolerances of
    test_graphed_train_step_equals_eager_across_optimizer_steps."""
    dev = torch.device(DEV)
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    torch.manual_seed(0)
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    mcfg = tb.config.default_model_cfg(n_tgt_knn=4)
    mcfg["tf_cfg"]["dropout_p"] = 0.0
    mcfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    mcfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg(time_step_end=30)
    scfg["differentiable_reward"].update(IL.reward_cfg(IL.TRAIN_CONFIGS["mse_l1_cast"]))
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    wm = W.WaymoMotion(model=mcfg, data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
    (opt,), _ = wm.configure_optimizers()
    batches = [{k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=s).items()} for s in (0, 2)]
    gs = DP.GraphedTrainStep(wm, opt, batches[0], warmup=1)
    gs(batches[0])  # replay + clip + AdamW: the weights move
    gs.opt, gs.clip = torch.optim.SGD(gs.live, lr=0.0), 0
    m = gs(batches[1])
    loss_g = float(m["loss"].detach())
    g1 = [g.clone() for g in gs.grads]
    for p in gs.live:
        p.grad = None
    loss = wm.training_step({k: v.clone() for k, v in batches[1].items()}, 0, noise=gs.noise, use_prior=gs.use_prior)
    loss.backward()
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-6)
    print(f"[graphed step, mse_l1_cast] replayed loss {loss_g:.6g}, eager {float(loss.detach()):.6g}")
    assert abs(float(loss.detach()) - loss_g) <= 1e-5 * abs(loss_g)
    names = {id(p): k for k, p in wm.model.named_parameters()}
    for a, p in zip(g1, gs.live):
        assert close(a, p.grad, 1e-3), names[id(p)]
