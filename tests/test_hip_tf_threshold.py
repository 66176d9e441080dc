"""GPU checks of error-threshold teacher forcing (TeacherForcing's threshold_xy / threshold_yaw / threshold_spd): tbx_tf_threshold against
the reference's own results (tests/golden/tf_threshold.npz), the rollout engine's closed loop against the reference's reactive_replay
(rollout_c1_tfthr.npz) in both schedules and through the reference-order loop, the pristine table of a cached engine, independent
decisions of a scene's K rollouts, thresholds off = nothing new, and the training step (train_c1_tfthr.npz) in its three forms and captured."""
import sys
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tf_threshold_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# tests/test_hip_training.py TRAIN_TOL, test_time_batched_training_rollout_equals_step_by_step_autograd's bounds
TRAIN_TOL = {"fp32": dict(loss=1e-3, gnorm=1e-2, spot_rtol=2e-2, spot_atol_rel=0.0), "bf16": dict(loss=5e-4, gnorm=2e-2, spot_rtol=0.0, spot_atol_rel=6e-2)}


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def cases():
    return TR.load_cases()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("step_on_device", [False, True])
def test_kernel_equals_the_reference_exactly(hip, cases, step_on_device):
    """Per case and setting: column s and out_reset equal the reference's, every other column keeps the pattern it was filled with, a second
    call leaves the same bytes, a step outside (0, Tg) writes nothing (out_reset included)."""
    dev = torch.device(DEV)
    for name, step, inp, want in cases:
        d = {k: v.to(dev) for k, v in inp.items()}
        rows, A, Tg = inp["gt_valid"].shape
        pattern = (2 + torch.arange(rows * A * Tg, dtype=torch.int64).reshape(rows, A, Tg) % 7).to(torch.uint8)  # never 0 / 1
        for i, thr in enumerate(TR.SETTINGS):
            table = pattern.clone()
            inside = 0 < step < Tg
            if inside:
                table[:, :, step] = inp["tf_init"][:, :, step].to(torch.uint8)
            start = table.clone()
            table = table.to(dev)
            out_reset = torch.full((rows, A), 7, dtype=torch.uint8, device=dev)
            s_arg = torch.tensor([step, 0], dtype=torch.int32, device=dev) if step_on_device else step
            args = (thr, s_arg, d["pred_valid"], d["pred_pose"], d["pred_motion"], d["gt_valid"], d["gt_pose"], d["gt_motion"], table, out_reset)
            hip.tf_threshold(*args)
            first = (table.cpu(), out_reset.cpu())
            hip.tf_threshold(*args)
            assert torch.equal(table.cpu(), first[0]) and torch.equal(out_reset.cpu(), first[1]), (name, thr)
            expect = start.clone()
            if inside:
                expect[:, :, step] = want["tf_after"][i][:, :, step].to(torch.uint8)
                reset = TR.resets(thr, step, inp["pred_valid"], inp["pred_pose"], inp["pred_motion"], inp["gt_valid"], inp["gt_pose"], inp["gt_motion"])
                assert torch.equal(first[1].bool(), reset) and int(first[1].max()) <= 1, (name, thr)
                assert torch.equal(first[1].bool() | inp["tf_init"][:, :, step], want["tf_after"][i][:, :, step]), (name, thr)
            else:
                assert bool((first[1] == 7).all()), (name, thr)
            assert torch.equal(first[0], expect), (name, thr)  # column s the reference's, every other column untouched
    # step 0 (and a negative one) through the device counter: nothing is written
    name, step, inp, want = cases[1]
    d = {k: v.to(dev) for k, v in inp.items()}
    for s in (0, -3):
        table = torch.full(inp["gt_valid"].shape, 5, dtype=torch.uint8, device=dev)
        s_arg = torch.tensor([s], dtype=torch.int32, device=dev) if step_on_device else s
        hip.tf_threshold(TR.SETTINGS[-1], s_arg, d["pred_valid"], d["pred_pose"], d["pred_motion"], d["gt_valid"], d["gt_pose"], d["gt_motion"], table)
        assert bool((table == 5).all())


def test_get_on_device_tensors_is_one_launch_on_the_table_in_place(tb, hip, cases, monkeypatch):
    TF = import_module("trafficbots_amd.utils.teacher_forcing")
    dev = torch.device(DEV)
    real, calls = hip.tf_threshold_launch, []
    monkeypatch.setattr(hip, "tf_threshold_launch", lambda a: (calls.append(1), real(a))[1])
    for name, step, inp, want in cases:
        d = {k: v.to(dev) for k, v in inp.items()}
        for i, thr in enumerate(TR.SETTINGS):
            tf = TF.TeacherForcing(step_spawn_agent=10, step_warm_start=2, threshold_xy=thr[0], threshold_yaw=thr[1], threshold_spd=thr[2])
            tf.init(d["gt_valid"], d["gt_pose"], d["gt_motion"], d["tl_state"], 0)
            tf.ag_teacher_forcing.copy_(d["tf_init"])
            del calls[:]
            ag, _ = tf.get(step, d["pred_valid"], d["pred_pose"], d["pred_motion"])
            assert len(calls) == (1 if 0 < step < inp["gt_valid"].shape[-1] else 0)
            assert torch.equal(ag["valid"].cpu(), want["ov_valid"][i]) and torch.equal(tf.ag_teacher_forcing.cpu(), want["tf_after"][i]), (name, thr)
            assert torch.equal(ag["pose"].cpu(), want["ov_pose"]) and torch.equal(ag["motion"].cpu(), want["ov_motion"])


# ------------------------------------------------------------------------------------------------ the engine's closed loop
def _damp(wm):
    with torch.no_grad():
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    return wm


def _rollout_setup(tb, thr, sizes=(8, 64, 8), **tf_over):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg()
    if thr is not None:
        for k in ("teacher_forcing_reactive_replay", "teacher_forcing_joint_future_pred"):
            scfg[k] = dict(scfg[k], threshold_xy=thr[0], threshold_yaw=thr[1], threshold_spd=thr[2], **tf_over)
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    wm = _damp(wm).to(DEV).eval()
    batch = tb.synthetic.make_scene(1, *sizes, seed=0)
    bd = wm.pre_processing({k: v.to(DEV) for k, v in {**batch, **tb.synthetic.to_history_batch(batch)}.items()})
    return wm, bd


@pytest.fixture(scope="module")
def golden_rollout(golden_dir):
    return np.load(golden_dir / "rollout_c1_tfthr.npz")


def _replay(wm, bd, g, tokens, **kw):
    mp, tl = tokens
    z, zv = torch.from_numpy(g["latent"]).to(DEV), torch.from_numpy(g["latent_valid"]).to(DEV)
    return wm.reactive_replay(bd, mp, tl, z, zv, bd["gt/ag_navi"], bd["gt/ag_valid"].any(-1), wm.teacher_forcing_reactive_replay, True,
                              step_end=int(g["n_step"]), **kw)


def test_reactive_replay_equals_the_reference_in_both_schedules_and_orders(tb, hip, golden_rollout, monkeypatch):
    """Flag log and pred_valid exactly, poses at the c1 closed-loop tolerance (tests/test_hip_rollout.py: rtol 1e-4, atol 5e-3): the
    one-queue and the two-stream schedule, eager and captured; the reference-order loop (teacher_forcing.get -> forward -> rule_checker.check)
    logs the same flags; a second rollout on the cached engine (refill) and a restore() of it reproduce the first bit for bit."""
    g = golden_rollout
    thr = tuple(float(t) for t in g["thresholds"])
    wm, bd = _rollout_setup(tb, thr)
    E = import_module("trafficbots_amd.engine")
    new = torch.from_numpy(g["new_bits"])
    assert int(new[:, :, 11:].any(-1).sum()) >= 2  # the fixture has resets after the warm start, on several agents
    real, calls = hip.tf_threshold_launch, []
    monkeypatch.setattr(hip, "tf_threshold_launch", lambda a: (calls.append(1), real(a))[1])
    T = int(g["n_step"])
    outs = {}
    for one in (True, False):
        wm.schedule = E.DEFAULT.replace(one_queue=one)
        tokens = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")
        for use_graph in (False, True):
            del calls[:]
            buf = _replay(wm, bd, g, tokens, use_graph=use_graph)
            eng = wm._engine
            assert eng.one_queue == one and eng.tf_thresholds == thr
            if not use_graph:
                assert len(calls) == T  # one launch per step
            outs[one, use_graph] = buf
            flags = buf.mask_teacher_forcing[:, 0].cpu()
            worst = float((buf.pred_pose[:, 0].cpu() - torch.from_numpy(g["pred_pose"])).abs().max())
            print(f"[reactive_replay with thresholds {thr}, one_queue={one}, graph={use_graph}] {int(new.sum())} resets; max |pose - reference| {worst:.3g}")
            assert torch.equal(flags, torch.from_numpy(g["mask_teacher_forcing"])), (one, use_graph)
            assert torch.equal(buf.pred_valid[:, 0].cpu(), torch.from_numpy(g["pred_valid"])), (one, use_graph)
            np.testing.assert_allclose(buf.pred_pose[:, 0].cpu().numpy(), g["pred_pose"], rtol=1e-4, atol=5e-3)
            # the engine's table holds the schedule's bits + the resets, its pristine copy the schedule's alone
            assert torch.equal(eng.S["tf_mask"].bool().cpu(), torch.from_numpy(g["tf_table"]))
            assert torch.equal(eng.init_state["tf_mask"].bool().cpu(), torch.from_numpy(g["tf_table"] & ~g["new_bits"]))
        # the cached engine again: a refill with the same scene, then restore() + run() - the table starts from the schedule's both times
        eng = wm._engine
        again = _replay(wm, bd, g, tokens, use_graph=True)
        assert wm._engine is eng
        eng.restore()
        eng.run(T)
        third = eng.buffer(wm.hp.time_step_current)
        for b2 in (again, third):
            b2_flags = b2.mask_teacher_forcing.reshape(outs[one, True].mask_teacher_forcing.shape)
            assert torch.equal(b2_flags, outs[one, True].mask_teacher_forcing)
            assert torch.equal(b2.pred_pose.reshape(outs[one, True].pred_pose.shape), outs[one, True].pred_pose)
    ref = outs[True, False]
    for k, o in outs.items():  # the same arithmetic in every form: one more launch in front of the step changes no other
        assert torch.equal(o.pred_pose, ref.pred_pose) and torch.equal(o.mask_teacher_forcing, ref.mask_teacher_forcing), k
    # the reference's own calling order: TeacherForcing.get decides (one launch per step with the host's step), forward applies
    wm.schedule = E.DEFAULT
    tokens = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")
    del calls[:]
    z, zv = torch.from_numpy(g["latent"]).to(DEV), torch.from_numpy(g["latent_valid"]).to(DEV)
    ag_tokens = {"ag_type": bd["ref/ag_type"], "ag_size": bd["ref/ag_size"], "ag_attr": bd["sc/ag_attr"], "gt_valid": bd["gt/ag_valid"],
                 "gt_pose": bd["gt/ag_pose"], "gt_motion": bd["gt/ag_motion"], "ag_latent": z, "ag_latent_valid": zv, "ag_navi": bd["gt/ag_navi"],
                 "ag_navi_valid": bd["gt/ag_valid"].any(-1)}
    tf = wm.teacher_forcing_reactive_replay
    buf = wm.rollout(ag_tokens, tokens[0], tokens[1], bd["gt/tl_state"], tf, wm._rule_checker(bd, bd["gt/ag_navi"], tokens[1]), T, True, stepwise=True)
    assert len(calls) == T and wm._engine.tf_thresholds is None  # decided by get(), not by the engine
    assert torch.equal(buf.mask_teacher_forcing.cpu().reshape(1, 8, T), torch.from_numpy(g["mask_teacher_forcing"]))
    assert torch.equal(tf.ag_teacher_forcing.cpu(), torch.from_numpy(g["tf_table"]))  # the table itself keeps the bits


def test_sampled_rollouts_of_a_scene_decide_independently(tb):
    """joint_future_pred with K = 3 sampled rollouts (deterministic_action=False): the engine's table has one row per rollout, and the
    resets differ between the rollouts of the scene. joint_future_pred's ground truth is the history (11 steps), so the warm start is
    cut to 2 steps here: steps 3 .. 10 are free and have ground truth to drift from."""
    wm, bd = _rollout_setup(tb, (0.3, 60.0, 0.3), step_warm_start=2)
    D = import_module("trafficbots_amd.models.modules.distributions")
    with torch.no_grad():  # (the samples spread with the head's log_std: wide enough for the rollouts to part within a few steps)
        for p in wm.model.action_head.log_std:
            p.fill_(0.0)
    K, T = 3, 16
    valid = bd["sc/ag_valid"].any(-1)
    n, A = valid.shape
    Tg = bd["sc/ag_valid"].shape[-1]
    mp, tl = wm.encode_scene(bd, n_rollout=K)
    lat = D.DiagGaussian(torch.zeros(n, A, 16, device=DEV), torch.full((16,), -200.0, device=DEV), valid=valid)
    nav = D.DestCategorical(probs=torch.nn.functional.one_hot(bd["gt/ag_navi"], bd["sc/mp_valid"].shape[1]).float(), valid=valid)
    wm.hp.joint_future_pred_deterministic_k0 = False
    torch.manual_seed(11)
    buf = wm.joint_future_pred(bd, mp, tl, lat, nav, wm.teacher_forcing_joint_future_pred, K, step_end=T, deterministic_action=False)
    eng = wm._engine
    assert eng.S["tf_mask"].shape == (n * K, A, Tg)
    table, pristine = eng.S["tf_mask"].bool().view(n, K, A, Tg), eng.init_state["tf_mask"].bool().view(n, K, A, Tg)
    assert all(torch.equal(pristine[:, 0], pristine[:, k]) for k in range(1, K))  # one schedule for the K rollouts
    new = table & ~pristine
    print(f"[K = {K} sampled rollouts] resets per rollout: {[int(new[:, k].sum()) for k in range(K)]}")
    assert bool(new.any()) and any(not torch.equal(new[:, 0], new[:, k]) for k in range(1, K))
    flags = buf.mask_teacher_forcing  # [n, K, A, T]
    assert torch.equal(flags[..., :Tg - 1], table[..., 1:]) and not flags[..., Tg - 1:].any()


def test_thresholds_off_launch_nothing_and_change_nothing(tb, hip, monkeypatch):
    """Thresholds at -1: nothing of the threshold path is called - the rollout runs with hip.tf_threshold_launch, hip.tf_threshold_args and
    hip.tf_threshold all made to raise, so nothing builds the arguments either -, the eager one-queue step is its five launches, and the
    log equals the one of an engine built before the three may be used again. With a threshold on the same step is those five launches +
    one."""
    E = import_module("trafficbots_amd.engine")
    counts = {"pair": 0, "tf": 0}
    real_front, real_layer, real_tf = hip.launch_front_pair, hip.launch_dec_layer_pair, hip.tf_threshold_launch
    real_args, real_whole = hip.tf_threshold_args, hip.tf_threshold
    monkeypatch.setattr(hip, "launch_front_pair", lambda *a: (counts.__setitem__("pair", counts["pair"] + 1), real_front(*a))[1])
    monkeypatch.setattr(hip, "launch_dec_layer_pair", lambda *a: (counts.__setitem__("pair", counts["pair"] + 1), real_layer(*a))[1])
    T = 20
    res = {}
    for thr in (None, (3.0, 60.0, 3.0)):
        wm, bd = _rollout_setup(tb, thr)
        wm.schedule, wm.engine_cache = E.DEFAULT, 0
        tokens = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")
        z = torch.randn(1, 8, 16, generator=torch.Generator().manual_seed(6)).to(DEV)
        v = bd["gt/ag_valid"].any(-1)
        run = lambda g_: wm.reactive_replay(bd, tokens[0], tokens[1], z, v, bd["gt/ag_navi"], v, wm.teacher_forcing_reactive_replay, True, step_end=T,
                                            use_graph=g_)
        if thr is None:
            def refuse(*a, **k):
                raise AssertionError("the threshold path was entered with every threshold off")
            for name in ("tf_threshold_launch", "tf_threshold_args", "tf_threshold"):
                monkeypatch.setattr(hip, name, refuse)
        else:
            monkeypatch.setattr(hip, "tf_threshold_launch", lambda a: (counts.__setitem__("tf", counts["tf"] + 1), real_tf(a))[1])
            monkeypatch.setattr(hip, "tf_threshold_args", real_args), monkeypatch.setattr(hip, "tf_threshold", real_whole)
        counts.update(pair=0, tf=0)
        eager = run(False)
        assert wm._engine.one_queue and (wm._engine._tf_args is None) == (thr is None)
        # five paired launches per step (the very first step of a fresh engine runs its halves unpaired), and the sixth only with a threshold
        assert counts["pair"] in ((T - 1) * 5, T * 5) and counts["tf"] == (0 if thr is None else T), (thr, counts)
        res["pairs", thr is None] = counts["pair"]
        graphed = run(True)
        assert "tf_mask" not in wm._engine.init_state if thr is None else "tf_mask" in wm._engine.init_state
        assert torch.equal(eager.pred_pose, graphed.pred_pose) and torch.equal(eager.mask_teacher_forcing, graphed.mask_teacher_forcing)
        res[thr is None] = graphed
    assert res["pairs", True] == res["pairs", False]  # every other launch of the step is there, on or off
    # the first 10 steps are the warm start in both: the same log whether the extra launch runs or not
    off, on = res[True], res[False]
    assert torch.equal(off.pred_pose[..., :10, :], on.pred_pose[..., :10, :])
    assert torch.equal(off.mask_teacher_forcing[..., :10], on.mask_teacher_forcing[..., :10])


# ------------------------------------------------------------------------------------------------ training
def _train_wm(tb, thr, n_step, dropout=False):
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    cfg = tb.config.default_model_cfg(n_tgt_knn=4)
    if not dropout:
        cfg["tf_cfg"]["dropout_p"] = 0.0
        cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
        cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg(p_training_rollout_prior=0.0, time_step_end=n_step)
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    if thr is not None:
        scfg["teacher_forcing_training"].update(threshold_xy=thr[0], threshold_yaw=thr[1], threshold_spd=thr[2])
    wm = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    return _damp(wm)


def _gnorms(wm):
    gn = {}
    for k, p in wm.model.named_parameters():
        if p.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(p.grad.double().pow(2).sum())
    return {k: v ** 0.5 for k, v in gn.items()}


@pytest.fixture(scope="module")
def golden_train(golden_dir):
    return np.load(golden_dir / "train_c1_tfthr.npz")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_training_step_with_thresholds_vs_reference(tb, golden_train, prec):
    """test_training_step_vs_oracle_and_reference's procedure (every RNG site neutralised, damped action head) at the c1 sizes with
    thresholds in teacher_forcing_training: loss terms, gradient norms and spot gradients at TRAIN_TOL, the flag log exactly."""
    g = golden_train
    thr = tuple(float(t) for t in g["thresholds"])
    wm = _train_wm(tb, thr, int(g["n_step"])).to(DEV).train()
    wm.train_precision = prec
    tol = TRAIN_TOL[prec]
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    torch.manual_seed(7)
    loss = wm.training_step({k: v.to(DEV) for k, v in batch.items()}, 0)
    loss.backward()
    table = wm.teacher_forcing_training.ag_teacher_forcing.cpu()
    assert torch.equal(table, torch.from_numpy(g["tf_table"]))  # column s is step s's logged flag: the flag log, and the table keeps the bits
    assert bool(torch.from_numpy(g["new_bits"])[:, :, 11:].any())
    keys = ("loss", "vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss")
    gn = _gnorms(wm)
    named = dict(wm.model.named_parameters())
    spots = [x for x in g.files if x.startswith("dgrad_")]
    rel = lambda x, r, floor: abs(x - r) / max(abs(r), floor)
    meas = {"loss": max(rel(float(wm.last_metrics[k].detach()), float(g[f"dtrain_{k}"]), 1e-1) for k in keys),
            "gnorm": max(rel(v, float(g[f"dgradnorm_{top}"]), 1e-6) for top, v in gn.items()),
            "spot": max(float((named[k[6:]].grad[:8, :16].cpu() - torch.from_numpy(g[k])).abs().max()) / max(float(np.abs(g[k]).max()), 1e-12) for k in spots)}
    print(f"[training step, thresholds {thr}, {prec}] loss {float(loss.detach()):.6g} (reference {float(g['dtrain_loss']):.6g}, without thresholds "
          f"{float(g['off/dtrain_loss']):.6g}); loss terms max rel diff {meas['loss']:.3g}, gradient norms {meas['gnorm']:.3g}, spot blocks max |d| / "
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


def test_the_three_training_rollouts_take_the_same_resets(tb):
    """The fused chain, fused_train_chain=False (the recording pass decides, the replay on batched means reads) and
    time_batched_training=False (autograd through the steps) agree on the flag log exactly and on loss and gradients at
    test_time_batched_training_rollout_equals_step_by_step_autograd's bounds, on that test's small shape (2 scenes x 8 agents, 30 steps:
    the bounds were measured there) with thresholds low enough for resets within the 20 free steps, from each of the three terms' range."""
    thr, (n_sc, sizes, n_steps) = (1.0, 10.0, 0.5), (2, (8, 64, 8), 30)
    wm = _train_wm(tb, thr, n_steps).to(DEV).train()
    wm.train_precision = "fp32"  # (the class that test runs in - its file's autouse fixture - and its bounds belong to)
    batch = {k: v.to(DEV) for k, v in tb.synthetic.make_scene(n_sc, *sizes, seed=1).items()}
    noise = torch.randn(n_sc, sizes[0], wm.model.latent_encoder.out_dim, generator=torch.Generator().manual_seed(5)).to(DEV)
    use_prior = torch.zeros((), dtype=torch.bool, device=DEV)
    res = {}
    for mode, (batched, fused) in dict(chain=(True, True), torch_batched=(True, False), stepwise=(False, True)).items():
        wm.time_batched_training, wm.fused_train_chain = batched, fused
        wm.zero_grad(set_to_none=True)
        loss = wm.training_step({k: v.clone() for k, v in batch.items()}, 0, noise=noise, use_prior=use_prior)
        loss.backward()
        res[mode] = ({k: float(v.detach()) for k, v in wm.last_metrics.items()}, {k: p.grad.clone() for k, p in wm.model.named_parameters() if p.grad is not None},
                     wm.teacher_forcing_training.ag_teacher_forcing.clone())
    ref = res["stepwise"]
    # (the schedule - warm start 10, spawns up to step 10, no random forcing - has no bit past column 10: every one there is a reset)
    late = ref[2][:, :, 11:n_steps + 1]
    print(f"[three training rollouts, thresholds {thr}] {int(late.sum())} resets on {int(late.any(-1).sum())} agents within {n_steps} steps")
    assert int(late.any(-1).sum()) >= 2
    for mode in ("chain", "torch_batched"):
        got = res[mode]
        assert torch.equal(got[2], ref[2]), mode
        for k, v in ref[0].items():
            assert abs(got[0][k] - v) <= 2e-5 * max(abs(v), 1e-3), (mode, k, got[0][k], v)
        assert got[1].keys() == ref[1].keys()
        for k, gs in ref[1].items():
            err = (got[1][k] - gs).double()
            rel_l2 = float(err.norm()) / max(float(gs.double().norm()), 1e-6 * gs.numel() ** 0.5)
            relu_fed = any(t in k for t in (".linear1.", ".norm2.", "log_std"))
            assert rel_l2 <= (1e-2 if relu_fed else 2e-3), (mode, k, rel_l2)
            n_big = int((err.abs() > 1e-3 * max(float(gs.abs().max()), 1e-6)).sum())
            assert relu_fed or n_big <= max(2, gs.numel() // 200), (mode, k, n_big, gs.numel())


def test_graphed_train_step_starts_every_replay_from_a_clean_table(tb, golden_train):
    """GraphedTrainStep captures the tbx_tf_threshold calls; TeacherForcing.init rebuilds the table inside every replay: two replays of
    the same batch with the same host draws (learning rate 0) give identical losses and flag logs, and equal the eager step."""
    g = golden_train
    thr = tuple(float(t) for t in g["thresholds"])
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    torch.manual_seed(0)
    wm = _train_wm(tb, thr, int(g["n_step"])).to(DEV).train()
    batch = {k: v.to(DEV) for k, v in tb.synthetic.make_scene(1, 8, 64, 8, seed=0).items()}
    (opt,), _ = wm.configure_optimizers()
    gs = DP.GraphedTrainStep(wm, opt, batch, warmup=1)
    gs.opt, gs.clip = torch.optim.SGD(gs.live, lr=0.0), 0
    tf = wm.teacher_forcing_training
    seen = []
    for _ in range(2):
        torch.manual_seed(3)  # (the latent noise of a call is drawn from the host generator)
        m = gs(batch)
        seen.append((float(m["loss"].detach()), tf.ag_teacher_forcing.clone()))
    assert seen[0][0] == seen[1][0] and torch.equal(seen[0][1], seen[1][1])
    new = seen[0][1].cpu() & ~torch.from_numpy(g["off/tf_table"])
    assert bool(new[:, :, 11:].any())  # resets happened, and the second replay did not start from them
    for p in gs.live:
        p.grad = None
    loss = wm.training_step({k: v.clone() for k, v in batch.items()}, 0, noise=gs.noise, use_prior=gs.use_prior)
    assert torch.equal(wm.teacher_forcing_training.ag_teacher_forcing, seen[0][1])
    assert abs(float(loss.detach()) - seen[0][0]) <= 1e-5 * abs(seen[0][0]), (float(loss.detach()), seen[0][0])
