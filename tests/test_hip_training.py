"""GPU parity of the training path: KNARPE attention backward kernel vs autograd of the oracle
formulation, and WaymoMotion.training_step loss / gradients vs the oracle and vs the REFERENCE's golden values."""
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import hptr_ops as H
from oracle import trafficbots_oracle as O
from test_hip_attn_backward import reference as attn_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fp32_class_by_default(tb):
    """The tests of this file that do not say otherwise pin the fp32-CLASS training arithmetic (train_graph.precision() == "fp32": split-bf16 /
    exact-fp32 products, VALU attention) at its tight tolerances; the bf16-class default (autocast-class contractions, the schedule the
    `training` bench figure runs on) is checked by the tests with `bf16` in their name / parameters, at stated tolerances."""
    TG = import_module("trafficbots_amd.train_graph")
    prev = TG.state.DEFAULT_PRECISION
    TG.state.DEFAULT_PRECISION = "fp32"
    yield
    TG.state.DEFAULT_PRECISION = prev


def test_attention_backward_vs_oracle_autograd(tb):
    dev = torch.device("cuda:0")
    M = import_module("trafficbots_amd.models.modules")
    TG = import_module("trafficbots_amd.train_graph")
    g = torch.Generator().manual_seed(4)
    n, S, T, K, d = 2, 19, 23, 7, 128
    att = M.attention_rpe.AttentionRPE(d_model=d, n_head=4, dropout_p=0.0, d_rpe=d)
    tb.utils.det_fill(att, 15)
    P = {"a." + k: v.detach().clone().requires_grad_(True) for k, v in att.state_dict().items()}
    src = torch.randn(n, S, d, generator=g)
    tokens = torch.randn(n, T, d, generator=g)  # target tokens (shared table), gathered by idx
    idx = torch.randint(0, T, (n, S, K), generator=g)
    emb = torch.randn(n, S, K, d, generator=g)
    m = torch.rand(n, S, K, generator=g) < 0.3
    m[0, 2] = True
    w_out = torch.randn(n, S, d, generator=g)
    # oracle: reference formulation (gather -> per-pair projection), autograd on CPU
    src_o, tok_o = src.clone().requires_grad_(True), tokens.clone().requires_grad_(True)
    y_o = H.attention_rpe(P, "a", 4, src_o, H.gather_tokens(tok_o, idx), m, emb)
    (y_o * w_out).sum().backward()
    # HIP: table form
    att = att.to(dev)
    src_h, tok_h = src.to(dev).requires_grad_(True), tokens.to(dev).requires_grad_(True)
    t = TG.Targets(tok_h.reshape(n * T, d), idx.to(torch.int32).to(dev).contiguous(), m.to(torch.uint8).to(dev).contiguous(),
                   emb.to(dev).contiguous(), n_tgt=T)  # materialised-embedding form of the kernel pair
    y_h = TG.attention(att, src_h.reshape(n * S, d), [t], [TG.kv_table(att, None, t)], n, S).view(n, S, d)
    (y_h * w_out.to(dev)).sum().backward()
    tol = dict(rtol=2e-3, atol=2e-4)
    torch.testing.assert_close(y_h.detach().cpu(), y_o.detach(), rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(src_h.grad.cpu(), src_o.grad, **tol)
    torch.testing.assert_close(tok_h.grad.cpu(), tok_o.grad, **tol)
    for k, p in att.named_parameters():
        torch.testing.assert_close(p.grad.cpu(), P["a." + k].grad, **tol)


# Tolerances of the training step against the REFERENCE's golden values per arithmetic class: (loss terms rtol, per-module gradient-norm
# rel, spot gradients rtol / atol relative to the largest reference entry of the block). "bf16" = the autocast-class contractions
# (train_graph.py: one bf16 product per term in the tall LINEARs, their weight gradients and the attention forward): <= 2 x the largest
# difference measured on MI355X (printed by the test; profiles/r05_train_bf16_tolerances.txt).
TRAIN_TOL = {"fp32": dict(loss=1e-3, gnorm=1e-2, spot_rtol=2e-2, spot_atol_rel=0.0),
             "bf16": dict(loss=5e-4, gnorm=2e-2, spot_rtol=0.0, spot_atol_rel=6e-2)}  # measured: 2.1e-4 / 1.0e-2 / 3.0e-2
# The batch with the domain's empty inputs (train_c1_edge.npz) is ILL-CONDITIONED for a few parameter blocks: its lights' window rows are
# replicated (55 distinct attribute rows over 23,760 window rows) in front of LayerNorms and a max-pool, and in the scene without a map the
# gradient that reaches them is 20 x larger than in a plain batch. Measured (profiles/MEASUREMENT_LOG.md, round 5): replacing
# tbx_tall_linear's products (within their stated 5e-6 of sum |x||w|: no ReLU sign changes) by the EXACT fp32 products brings every
# gradient back to the plain batches' agreement with the oracle; exact products + Gaussian noise of 1e-6 / 5e-6 move the lights' input
# encoder's gradients by 3e-3 / 8e-3 of their largest entry. The fp32 class's spot bound for this fixture is therefore relative to the
# block's largest entry: measured 3.6e-3, bound 2 x; loss and gradient-norm bounds as everywhere.
TRAIN_TOL_EDGE_FP32_SPOT = 7.5e-3
# A 16-scene step against the count-weighted recombination of its four 4-scene quarters: the same arithmetic on the same rows in a
# different summation order (weight gradients summed over 4 x the rows in one reduction vs 4 partial reductions added up; atomics
# in the attention backward). Bounds <= 2 x measured on MI355X (printed by the test).
RECOMBINE_TOL = {"fp32": dict(loss=2e-5, gnorm=1e-3, grad=5e-3), "bf16": dict(loss=1e-4, gnorm=5e-3, grad=2e-2)}
# The bf16 class where the tall LINEARs / weight gradients actually run (>= 16,384 rows: batch 4 of the full-size scene; or the row
# threshold lowered at the 8-agent size - then EVERY Linear of >= 256 rows is one bf16 product per term): the class's own rounding
# (each operand to 8 mantissa bits, ~50 LINEARs deep, 90 closed-loop steps), not a defect of a kernel - the fp32 class through the SAME
# launches agrees with the reference to 3e-6 / 3e-5 / 7e-4, and the kernels are pinned op by op (test_tall_linear_bf16_vs_float64,
# test_linear_wgrad_bf16_vs_float64). Measured on MI355X: b4 6.0e-3 / 8.5e-3 / 5.1e-2; c1_b3 at 256 rows 3.7e-3 / 3.5e-2 / 9.9e-2.
TRAIN_TOL_BF16_TALL = {"train_c2_b4.npz": dict(loss=1.2e-2, gnorm=2e-2, spot_rtol=0.0, spot_atol_rel=0.1),
                       "train_c1_b3.npz": dict(loss=8e-3, gnorm=7e-2, spot_rtol=0.0, spot_atol_rel=0.2)}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("sizes,knn,fixture,n_sc", [((8, 64, 8), 4, "model_c1.npz", 1), ((64, 1024, 128), 32, "train_c2.npz", 1),
                                                    # a BATCH of 4 full-size scenes (~8 min of reference CPU in
                                                    # make_golden.py): 4 x 90 x 64 = 23,040 agent rows per LINEAR - the >= 16,384-row
                                                    # branch (tbx_tall_linear / tbx_linear_wgrad and their bf16 forms, the dual-output
                                                    # K/V tables) and the loss normalisers over several full-size scenes
                                                    ((64, 1024, 128), 32, "train_c2_b4.npz", 4),
                                                    # ... the same branch at the 8-agent size: the row threshold lowered to 256
                                                    ((8, 64, 8), 4, "train_c1_b3.npz|min_rows=256", 3),
                                                    ((8, 64, 8), 4, "train_c1_b3.npz", 3),  # a BATCH of 3 scenes (the reference's own numbers)
                                                    # ... and a batch with the domain's empty inputs: a scene without a valid light, one with two
                                                    # agents, one without a valid polyline (synthetic.make_edge_batch)
                                                    ((8, 64, 8), 4, "train_c1_edge.npz", 3),
                                                    # ... and ONE scene without a valid light: the light-state term's counter is zero, the
                                                    # reference leaves the term out (metrics/training.py:184) and no gradient reaches the lights
                                                    ((8, 64, 8), 4, "train_c1_nolights.npz", 1)])
def test_training_step_vs_oracle_and_reference(tb, golden_dir, sizes, knn, fixture, n_sc, prec, monkeypatch):
    """One training_step with every RNG site neutralised (dropout 0, posterior latent, no random forcing) at C1 and at the
    scene size of BASELINE config 3 (64 agents / 1024 polylines / 128 lights, default K-nearest sizes: the shape behind the
    training scenes/s figure): loss terms vs the reference's golden values; per-module gradient norms vs the reference's; spot
    gradients vs the reference's."""
    dev = torch.device("cuda:0")
    fixture, _, opt = fixture.partition("|")
    min_rows = int(opt.split("=")[1]) if opt else None
    if min_rows is not None:  # (train_ops.linear / linear_kv read the module global at call time)
        monkeypatch.setattr(import_module("trafficbots_amd.train_ops"), "WGRAD_MIN_ROWS", min_rows)
    cfg = tb.config.default_model_cfg(n_tgt_knn=knn)
    cfg["tf_cfg"]["dropout_p"] = 0.0
    cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg(p_training_rollout_prior=0.0)
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    wm = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    # damped action head (x0.02): without it the 80 free-running steps are chaotic and the loss itself moves by ~0.2 %
    # between fp32 summation orders (measured); the reference's golden values for this variant are `dtrain_*`
    with torch.no_grad():
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    wm = wm.to(dev).train()
    wm.train_precision = prec
    tol = TRAIN_TOL[prec]
    batch = (tb.synthetic.make_edge_batch(*sizes, seed=0, kind="mixed" if "edge" in fixture else "no_lights") if ("edge" in fixture or "nolights" in fixture)
             else tb.synthetic.make_scene(n_sc, *sizes, seed=0))
    torch.manual_seed(7)
    calls = {"mfma": 0, "wgrad_bf16": 0, "wgrad": 0, "tall": 0, "tall_bf16": 0, "tall_dual16": 0}
    hip = import_module("trafficbots_amd.hip")
    orig = (hip.knarpe_attn_mfma, hip.linear_wgrad, hip.tall_linear)

    def mf(*a, **kw):
        calls["mfma"] += 1
        return orig[0](*a, **kw)

    def wg(*a, **kw):
        calls["wgrad_bf16"] += int(bool(kw.get("bf16")))
        calls["wgrad"] += 1
        return orig[1](*a, **kw)

    def tall(*a, **kw):
        if kw.get("out") is not None and kw["out"].stride(0) != kw["out"].shape[1]:
            # the no-grad stepping pass's K/V tables (train_graph._kv_tables_tall: column blocks of one table): the inference schedule's
            # fp32-equivalent products in BOTH classes - the closed loop's states do not depend on the training class
            assert not kw.get("bf16") and not torch.is_grad_enabled()
            return orig[2](*a, **kw)
        calls["tall"] += 1
        calls["tall_bf16"] += int(bool(kw.get("bf16")))
        calls["tall_dual16"] += int(kw.get("out16") is not None)
        return orig[2](*a, **kw)

    hip.knarpe_attn_mfma, hip.linear_wgrad, hip.tall_linear = mf, wg, tall
    try:
        loss = wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
        loss.backward()
    finally:
        hip.knarpe_attn_mfma, hip.linear_wgrad, hip.tall_linear = orig
    # the class that was asked for is what ran (tbx_linear_wgrad only serves the LINEARs of >= 16384 rows: none at the 8-agent size)
    assert (calls["mfma"] > 0) == (prec == "bf16") and calls["wgrad_bf16"] == (calls["wgrad"] if prec == "bf16" else 0)
    assert calls["tall_bf16"] == (calls["tall"] if prec == "bf16" else 0)
    if min_rows is not None or n_sc * sizes[0] * 90 >= 16384:
        # the tall branch end to end inside a reference-checked step (the 8-agent fixtures alone never reached it): the tall
        # LINEARs forward + input gradient, the weight gradients, and under the bf16 class the K/V tables written as bfloat16 beside fp32
        assert calls["wgrad"] > 10 and calls["tall"] > 10, calls
        assert (calls["tall_dual16"] > 0) == (prec == "bf16"), calls
    print(f"[training step, {fixture}{' ' + opt if opt else ''}, {prec}] kernel calls: {calls}")
    g = np.load(golden_dir / fixture)
    gv = lambda key: g[key] if key in g.files else np.zeros((), np.float32)  # (a term / module the reference left out: counter 0, no gradient)
    tol = dict(tol, spot_atol_rel=max(tol["spot_atol_rel"], TRAIN_TOL_EDGE_FP32_SPOT)) if "edge" in fixture else tol
    if prec == "bf16" and calls["wgrad_bf16"] > 10 and fixture in TRAIN_TOL_BF16_TALL:
        tol = TRAIN_TOL_BF16_TALL[fixture]
    meas = {"loss": 0.0, "gnorm": 0.0, "spot": 0.0}
    for k in ("loss", "vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss"):
        got, ref = float(wm.last_metrics[k].detach().cpu()), float(gv("dtrain_" + k))
        meas["loss"] = max(meas["loss"], abs(got - ref) / max(abs(ref), 1e-1))
    gn = {}
    for k, p in wm.model.named_parameters():
        if p.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(p.grad.double().pow(2).sum())
    for top, v in gn.items():
        ref = float(gv("dgradnorm_" + top))
        meas["gnorm"] = max(meas["gnorm"], abs(v**0.5 - ref) / max(ref, 1e-6))
    named = dict(wm.model.named_parameters())
    spot = lambda key: (torch.zeros(8, 16) if named[key].grad is None else named[key].grad[:8, :16].cpu())  # (None: no gradient reached the module)
    for k in [x for x in g.files if x.startswith("dgrad_")]:
        got, ref = spot(k[6:]), torch.from_numpy(g[k])
        meas["spot"] = max(meas["spot"], float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12))
    print(f"[training step vs reference golden, {fixture}, {prec}] loss terms: max rel diff {meas['loss']:.3g}; per-module gradient norms: max rel diff "
          f"{meas['gnorm']:.3g}; spot gradient blocks: max |d| / max |ref| {meas['spot']:.3g}")
    for k in ("loss", "vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss"):
        torch.testing.assert_close(wm.last_metrics[k].detach().cpu(), torch.from_numpy(np.asarray(gv("dtrain_" + k))), rtol=tol["loss"], atol=1e-1 * tol["loss"])
    for top, v in gn.items():
        ref = float(gv("dgradnorm_" + top))
        assert abs(v**0.5 - ref) <= tol["gnorm"] * max(ref, 1e-6), (top, v**0.5, ref)
    for k in [x for x in g.files if x.startswith("dgrad_")]:
        ref = torch.from_numpy(g[k])
        torch.testing.assert_close(spot(k[6:]), ref, rtol=tol["spot_rtol"], atol=1e-5 + tol["spot_atol_rel"] * float(ref.abs().max()))
    dead = set((golden_dir / "params_without_grad.txt").read_text().split())
    for k, p in wm.model.named_parameters():
        if k in dead:
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0, k


@pytest.mark.parametrize("tall_rows", [None, 256])
def test_graphed_train_step_equals_eager_across_optimizer_steps(tb, monkeypatch, tall_rows):
    """GraphedTrainStep (fwd + bwd replayed as one hipGraph) vs the eager step: after real AdamW updates between replays the
    replayed loss / gradients must be those of the CURRENT weights and inputs (a stale replay - see the ROCm caveat in
    data_parallel.py - passes a same-weights comparison), and two replays of the same inputs must agree.
    tall_rows = 256: the row threshold of the tall LINEAR path lowered so that TallLinearFn runs at this size - its BACKWARD packs the
    W^T image of every such weight, and a captured backward that found the warm-up passes' image in the per-parameter cache replayed
    the capture-time W^T forever: the input gradients of every replay after the first optimizer step were wrong.
    ... and a new epoch re-captures (TeacherForcing's schedules read current_epoch on the host) instead of asserting."""
    dev = torch.device("cuda:0")
    if tall_rows is not None:
        monkeypatch.setattr(import_module("trafficbots_amd.train_ops"), "WGRAD_MIN_ROWS", tall_rows)
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    cfg = tb.config.default_model_cfg(n_tgt_knn=4)
    cfg["tf_cfg"]["dropout_p"] = 0.0
    cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg()
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    scfg["time_step_end"] = 30
    torch.manual_seed(0)
    wm = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
    (opt,), _ = wm.configure_optimizers()
    batches = [{k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=s).items()} for s in (0, 2)]
    gs = DP.GraphedTrainStep(wm, opt, batches[0], warmup=2 if tall_rows else 1)  # (2 warm-up passes: the default, and what left the stale cache)
    for i in range(3):  # replay + clip + AdamW: the weights move
        gs(batches[i % 2])
    if tall_rows is None:  # an epoch change: the step is re-captured (the forcing schedule of the new epoch), the optimizer state kept
        g0, state0 = gs.graph, len(opt.state)
        wm.current_epoch += 1
        gs(batches[0])
        assert gs.graph is not g0 and gs.epoch == wm.current_epoch and len(opt.state) == state0 > 0
    gs.opt, gs.clip = torch.optim.SGD(gs.live, lr=0.0), 0
    m = gs(batches[1])
    loss_g = float(m["loss"].detach())
    g1 = [g.clone() for g in gs.grads]
    gs.graph.replay()
    torch.cuda.synchronize()
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-6)
    for a, b in zip(g1, gs.grads):
        assert close(a, b, 1e-4)  # atomics in the attention backward: not bitwise
    for p in gs.live:
        p.grad = None
    loss = wm.training_step({k: v.clone() for k, v in batches[1].items()}, 0, noise=gs.noise, use_prior=gs.use_prior)
    loss.backward()
    assert abs(float(loss.detach()) - loss_g) <= 1e-5 * abs(loss_g)
    names = {id(p): k for k, p in wm.model.named_parameters()}
    for a, p in zip(g1, gs.live):
        assert close(a, p.grad, 1e-3), names[id(p)]


def test_rollout_after_flat_adamw_steps_runs_on_the_trained_weights(tb):
    """Validation between training steps of GraphedTrainStep (FlatAdamW: the update goes through ONE flat buffer, not through the
    parameters' own version counters): the rollout after two more steps must run on the trained weights - a new engine, bit for bit
    the rollout of a fresh module loaded with the same state dict (no caches). Every derived weight image and engine is stamped with
    the parameters' versions (hip_base.weights_stamp); without FlatAdamW.step bumping them the second validation reused the first one's
    engine and images: stale weights, no error."""
    dev = torch.device("cuda:0")
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    cfg = tb.config.default_model_cfg(n_tgt_knn=4)
    cfg["tf_cfg"]["dropout_p"] = 0.0
    cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg()
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    scfg["time_step_end"] = 30
    torch.manual_seed(0)
    wm = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
    (opt,), _ = wm.configure_optimizers()
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=0).items()}
    gs = DP.GraphedTrainStep(wm, opt, batch)
    assert gs.flat_opt is not None  # (the default: FlatAdamW)
    scene = tb.synthetic.make_scene(1, 8, 64, 8, seed=11)
    full = {k: v.to(dev) for k, v in {**scene, **tb.synthetic.to_history_batch(scene)}.items()}

    def roll(m):
        m.eval()
        bd = m.pre_processing({k: v.clone() for k, v in full.items()})
        mp, tl = m.encode_scene(bd, tl_valid_key="gt/tl_valid")
        valid = bd["gt/ag_valid"].any(-1)
        z = torch.randn(1, valid.shape[1], 16, generator=torch.Generator().manual_seed(1)).to(dev)
        buf = m.reactive_replay(bd, mp, tl, z, valid, bd["gt/ag_navi"], valid, m.teacher_forcing_joint_future_pred, True, step_end=24)
        return buf, m._engine

    for _ in range(2):
        gs(batch)
    first, eng0 = roll(wm)
    wm.train()
    for _ in range(2):
        gs(batch)
    got, eng1 = roll(wm)
    fresh = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev)
    fresh.load_state_dict(wm.state_dict())
    ref, _ = roll(fresh)
    assert not torch.equal(first.pred_pose, ref.pred_pose)  # the training steps did move the rollout
    assert torch.equal(got.pred_pose, ref.pred_pose) and torch.equal(got.vis_dict["action"], ref.vis_dict["action"])
    assert torch.equal(got.vis_dict["tl_state"], ref.vis_dict["tl_state"]) and torch.equal(got.tl_state_nll, ref.tl_state_nll)
    assert eng1 is not eng0


def test_attention_probability_dropout_vs_explicit_mask(tb):
    """tbx_knarpe_attn_fwd / _bwd with p_drop > 0 (attention_rpe.py:171-172 inside the kernels) against explicit torch math with
    the mask the (seed, call) pair produces (hip.dropout_keep_mask restates the kernels' counter hash): forward outputs and
    every gradient; two target segments so that the second segment's slots continue the first's."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    TG = import_module("trafficbots_amd.train_graph")
    g = torch.Generator().manual_seed(9)
    n, S, T1, T2, K1, K2, p, call = 2, 19, 23, 11, 7, 5, 0.25, 3
    rows = n * S
    qbuf = torch.randn(rows, 640, generator=g)
    bias_k = torch.randn(128, generator=g)
    kvs = [torch.randn(n * T1, 256, generator=g), torch.randn(n * T2, 256, generator=g)]
    idx = [torch.randint(0, T1, (n, S, K1), generator=g), torch.randint(0, T2, (n, S, K2), generator=g)]
    inv = [torch.rand(n, S, K1, generator=g) < 0.3, torch.rand(n, S, K2, generator=g) < 0.3]
    inv[0][0, 2] = True
    inv[1][0, 2] = True  # a row without any valid target
    emb = [torch.randn(n, S, K1, 128, generator=g), torch.randn(n, S, K2, 128, generator=g)]
    w_out = torch.randn(rows, 640, generator=g)
    seed = torch.tensor([0x1234_5678_9ABC_DEF1], dtype=torch.int64)
    keep = hip.dropout_keep_mask(int(seed[0]), call, rows, K1 + K2, p).float()  # [rows, 4, K]
    assert 0.6 < float(keep.mean()) < 0.9

    def reference(qbuf, bias_k, kv1, kv2):  # the float64 evaluation shared with tests/test_hip_attn_backward.py
        return attn_reference(qbuf, bias_k, [kv1, kv2], idx, inv, emb, (T1, T2), (1, 1), n, S, keep=keep, p=p)

    leaves_c = [t.clone().requires_grad_(True) for t in (qbuf, bias_k, *kvs)]
    out_c, dead = reference(*leaves_c)
    (out_c * w_out).sum().backward()
    leaves_h = [t.clone().to(dev).requires_grad_(True) for t in (qbuf, bias_k, *kvs)]
    meta = [(idx[i].to(torch.int32).to(dev).contiguous(), inv[i].to(torch.uint8).to(dev).contiguous(), emb[i].to(dev).contiguous(), None,
             (T1, T2)[i], 1) for i in range(2)]
    out_h, flag = TG.KnarpeAttnFn.apply(leaves_h[0], leaves_h[1], n, S, meta, (None, None), (p, seed.to(dev), call), *leaves_h[2:])
    assert torch.equal(flag.bool().cpu(), dead)
    out_h = out_h.masked_fill(flag.bool().unsqueeze(-1), 0.0)
    (out_h * w_out.to(dev)).sum().backward()
    torch.testing.assert_close(out_h.detach().cpu(), out_c.detach(), rtol=2e-4, atol=2e-5)
    for a, b in zip(leaves_h, leaves_c):
        torch.testing.assert_close(a.grad.cpu(), b.grad, rtol=2e-3, atol=2e-4)
    # the same backward through inverse K-nearest lists (tbx_knn_inverse + tbx_knarpe_attn_bwd with coef): no dK / dV atomics
    lists = [hip.knn_inverse(meta[i][0], meta[i][1], (T1, T2)[i]) for i in range(2)]
    for i, (T, K) in enumerate(((T1, K1), (T2, K2))):  # the lists are the un-masked pairs grouped by target token
        ptr, lst = lists[i][0].cpu(), lists[i][1].cpu()
        ix, iv = idx[i].reshape(n, -1), inv[i].reshape(n, -1)
        for b_ in range(n):
            for j in (0, 3, T - 1):
                want = sorted((b_ * S * K + torch.nonzero((ix[b_] == j) & ~iv[b_]).flatten()).tolist())
                assert sorted(lst[b_, ptr[b_, j]:ptr[b_, j + 1]].tolist()) == want
            assert int(ptr[b_, T]) == int((~iv[b_]).sum())
    leaves_g = [t.clone().to(dev).requires_grad_(True) for t in (qbuf, bias_k, *kvs)]
    meta_g = [m + (lists[i],) for i, m in enumerate(meta)]
    out_g, _ = TG.KnarpeAttnFn.apply(leaves_g[0], leaves_g[1], n, S, meta_g, (None, None), (p, seed.to(dev), call), *leaves_g[2:])
    (out_g.masked_fill(flag.bool().unsqueeze(-1), 0.0) * w_out.to(dev)).sum().backward()
    for a, b in zip(leaves_g, leaves_h):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-4, atol=1e-5)
    # p = 0 through the same entry points is the plain kernel pair
    o0, _ = TG.KnarpeAttnFn.apply(leaves_h[0].detach(), leaves_h[1].detach(), n, S, meta, (None, None), None, *[t.detach() for t in leaves_h[2:]])
    o1, _ = TG.KnarpeAttnFn.apply(leaves_h[0].detach(), leaves_h[1].detach(), n, S, meta, (None, None), (0.0, None, 0), *[t.detach() for t in leaves_h[2:]])
    assert torch.equal(o0, o1)


def test_keyed_dropout_time_batched_masks_equal_per_step_masks(tb):
    """tbx_keyed_dropout: the call over T time-batched entries per scene ([scene][step] order) draws exactly the masks of T
    per-step calls keyed with (time_batch = 1, time0 = step); rate ~ p, scale 1 / (1 - p), the backward re-applies the mask,
    other sites / seeds give other masks."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    TG = import_module("trafficbots_amd.train_graph")
    n, T, R, cols, p = 3, 5, 14, 36, 0.2
    seed = torch.tensor([0x0123_4567_89AB_CDEF], dtype=torch.int64, device=dev)
    x = torch.randn(n, T, R, cols, device=dev)
    yb = hip.keyed_dropout(x.reshape(n * T * R, cols), p, seed, 7, R, T, 1).view(n, T, R, cols)
    for t in range(T):
        yt = hip.keyed_dropout(x[:, t].reshape(n * R, cols).contiguous(), p, seed, 7, R, 1, 1 + t).view(n, R, cols)
        assert torch.equal(yt, yb[:, t])
    kept = yb != 0
    assert abs(float(kept.float().mean()) - (1 - p)) < 0.02
    torch.testing.assert_close(yb[kept], x[kept] / (1 - p))
    assert not torch.equal(kept[:, 0], kept[:, 1])  # steps differ
    assert not torch.equal(kept, hip.keyed_dropout(x.reshape(-1, cols), p, seed, 8, R, T, 1).view(n, T, R, cols) != 0)
    assert not torch.equal(kept, hip.keyed_dropout(x.reshape(-1, cols), p, seed + 1, 7, R, T, 1).view(n, T, R, cols) != 0)
    odd = torch.randn(6, 7, device=dev)  # scalar path (cols % 4 != 0)
    assert abs(float((hip.keyed_dropout(odd, 0.5, seed, 1, 2) != 0).float().mean()) - 0.5) < 0.3
    xg = x.reshape(-1, cols).clone().requires_grad_(True)
    y = TG.KeyedDropoutFn.apply(xg, p, seed, 7, R, T, 1)
    y.sum().backward()
    torch.testing.assert_close(xg.grad, kept.reshape(-1, cols).float() / (1 - p))


def test_attention_dropout_time_batched_call_equals_per_step_calls(tb):
    """tbx_knarpe_attn_fwd with time_batch = T: one call over n x T entries (a scene's T steps consecutive, the scene's table shared
    through batch_div = T) == T calls of n entries keyed (1, step), forward and backward."""
    dev = torch.device("cuda:0")
    TG = import_module("trafficbots_amd.train_graph")
    g = torch.Generator().manual_seed(3)
    n, T, S, Tt, K, p, call = 2, 3, 9, 13, 5, 0.3, 11
    qbuf = torch.randn(n, T, S, 640, generator=g).to(dev)
    bias_k = torch.randn(128, generator=g).to(dev)
    kv = torch.randn(n * Tt, 256, generator=g).to(dev)  # one table per scene
    idx = torch.randint(0, Tt, (n, T, S, K), generator=g).to(torch.int32).to(dev)
    inv = (torch.rand(n, T, S, K, generator=g) < 0.2).to(torch.uint8).to(dev)
    emb = torch.randn(n, T, S, K, 128, generator=g).to(dev)
    seed = torch.tensor([77], dtype=torch.int64, device=dev)
    w = torch.randn(n, T, S, 640, generator=g).to(dev)
    qb, kvb = qbuf.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    meta = [(idx.reshape(n * T, S, K).contiguous(), inv.reshape(n * T, S, K).contiguous(), emb.reshape(n * T, S, K, 128).contiguous(), None, Tt, T)]
    out_b, _ = TG.KnarpeAttnFn.apply(qb.reshape(n * T * S, 640), bias_k, n * T, S, meta, (None, None), (p, seed, call, T, 1), kvb)
    (out_b * w.reshape(-1, 640)).sum().backward()
    gq, gkv = torch.zeros_like(qbuf), torch.zeros_like(kv)
    for t in range(T):
        qs, kvs = qbuf[:, t].clone().requires_grad_(True), kv.clone().requires_grad_(True)
        m = [(idx[:, t].contiguous(), inv[:, t].contiguous(), emb[:, t].contiguous(), None, Tt, 1)]
        out_s, _ = TG.KnarpeAttnFn.apply(qs.reshape(n * S, 640), bias_k, n, S, m, (None, None), (p, seed, call, 1, 1 + t), kvs)
        assert torch.equal(out_s.view(n, S, 640), out_b.view(n, T, S, 640)[:, t])
        (out_s * w[:, t].reshape(-1, 640)).sum().backward()
        gq[:, t], gkv = qs.grad, gkv + kvs.grad
    torch.testing.assert_close(qb.grad, gq, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(kvb.grad, gkv, rtol=1e-4, atol=1e-5)


C1_SHAPE, C3_SHAPE = (2, (8, 64, 8), 4, 30), (16, (64, 1024, 128), 32, 14)  # (scenes, sizes, n_tgt_knn, steps)


@pytest.mark.parametrize("dropout,tl_ahead,fused,shape", [(False, True, True, C1_SHAPE), (True, True, True, C1_SHAPE), (True, False, True, C1_SHAPE),
                                                          (True, True, False, C1_SHAPE), (True, True, True, C3_SHAPE)])
def test_time_batched_training_rollout_equals_step_by_step_autograd(tb, dropout, tl_ahead, fused, shape):
    """training_rollout_batched (no-grad stepping pass + ONE differentiated policy batch over all steps + the dynamics chain) vs
    training_rollout (autograd through 30 sequential policy steps): same loss terms and parameter gradients - also in train mode
    with every dropout live, since the keyed masks of the batched pass are those of the per-step pass. tl_ahead: the light encoder
    of all steps evaluated once ahead of the stepping pass (lights are teacher-forced while ground truth lasts) or inside it;
    fused: the per-step state machine (dynamics, forcing, rule flags, reward) as tbx_train_chain_fwd / _bwd or as torch ops.
    C3_SHAPE: the batch of BASELINE config 3 (16 scenes x 64 agents / 1024 polylines / 128 lights, default K-nearest sizes), 14
    closed-loop steps (10 warm-start steps, which carry no loss: training.py step_training_start, + 4 free-running ones)."""
    dev = torch.device("cuda:0")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    n_sc, sizes, knn, n_steps = shape
    cfg = tb.config.default_model_cfg(n_tgt_knn=knn)
    if not dropout:
        cfg["tf_cfg"]["dropout_p"] = 0.0
        cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
        cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg(p_training_rollout_prior=0.0)
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    scfg["time_step_end"] = n_steps
    wm = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    with torch.no_grad():  # damped action head: the free-running closed loop is chaotic otherwise
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    wm = wm.to(dev).train()
    wm.attn_dropout_seed = torch.tensor([4242], dtype=torch.int64, device=dev)
    wm.tl_encoder_ahead, wm.fused_train_chain = tl_ahead, fused
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(n_sc, *sizes, seed=1).items()}
    noise = torch.randn(n_sc, sizes[0], wm.model.latent_encoder.out_dim, generator=torch.Generator().manual_seed(5)).to(dev)
    use_prior = torch.zeros((), dtype=torch.bool, device=dev)
    res = {}
    for mode in (True, False):
        wm.time_batched_training = mode
        wm.zero_grad(set_to_none=True)
        loss = wm.training_step({k: v.clone() for k, v in batch.items()}, 0, noise=noise, use_prior=use_prior)
        loss.backward()
        res[mode] = ({k: float(v.detach()) for k, v in wm.last_metrics.items()}, {k: p.grad.clone() for k, p in wm.model.named_parameters() if p.grad is not None})
    for k, v in res[False][0].items():
        assert abs(res[True][0][k] - v) <= 2e-5 * max(abs(v), 1e-3), (k, res[True][0][k], v)
    assert res[True][1].keys() == res[False][1].keys()
    for k, gs in res[False][1].items():
        gb = res[True][1][k]
        # Robust metric: the relative L2 error of the whole parameter gradient at 2e-3 (measured on the C3 shape:
        # every parameter <= 1.0e-3, the worst being a LayerNorm weight whose gradient - 3e-4 at its largest entry - is a sum of 2e5
        # cancelling per-row terms; the old per-entry bound was 1e-2 of the largest entry with a 3e-5 floor). The two schedules sum the
        # same per-row terms in different orders (fp32 atomics, split-K weight gradients): measured 2e-6 .. 5e-6 per entry
        # (tools/scratch/batched_vs_stepwise_spread.py). The only known legitimate outliers are the weights feeding a ReLU
        # (transformer linear1 / its bias / the norm in front of it) when ONE unit's pre-activation changes sign between the two
        # schedules: those - and only those - get the looser per-entry bound; a parameter whose whole gradient is a ~1e-6 residue
        # of cancelling terms (the posterior's log_std) is compared on the absolute scale of those terms. A wrong mask or a missing
        # term is an O(0.1 .. 1) difference in either metric.
        err = (gb - gs).double()
        rel_l2 = float(err.norm()) / max(float(gs.double().norm()), 1e-6 * gs.numel() ** 0.5)
        relu_fed = any(t in k for t in (".linear1.", ".norm2.", "log_std"))
        assert rel_l2 <= (1e-2 if relu_fed else 2e-3), (k, rel_l2, float(err.abs().max()), float(gs.abs().max()))
        n_big = int((err.abs() > 1e-3 * max(float(gs.abs().max()), 1e-6)).sum())
        assert relu_fed or n_big <= max(2, gs.numel() // 200), (k, n_big, gs.numel())


@pytest.mark.parametrize("rows,n,k,ld_pad", [(20000, 128, 128, 0), (70001, 640, 128, 0), (33333, 128, 640, 0), (16390, 64, 20, 12), (50000, 4, 256, 0),
                                            (17, 128, 64, 0), (300000, 256, 128, 0)])
def test_linear_wgrad_vs_float64(tb, rows, n, k, ld_pad):
    """tbx_linear_wgrad (dW = dY^T X, db = sum dY over 10^4..10^5 rows; exact-fp32 MFMA, fixed summation order) vs float64:
    relative to sum |dy||x| the error stays at fp32 accumulation level; deterministic across calls; strided x (a column slice)."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    g = torch.Generator().manual_seed(rows + n + k)
    dy = torch.randn(rows, n, generator=g).to(dev)
    xs = torch.randn(rows, k + ld_pad, generator=g).to(dev)
    x = xs[:, :k]
    assert hip.linear_wgrad_ok(dy, x)
    dw, db = hip.linear_wgrad(dy, x, True)
    dw2, db2 = hip.linear_wgrad(dy, x, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    ref = dy.double().t() @ x.double()
    mag = dy.double().abs().t() @ x.double().abs()
    assert float(((dw.double() - ref).abs() / mag).max()) < 2e-6
    torch.testing.assert_close(db.double(), dy.double().sum(0), rtol=1e-5, atol=1e-5 * rows ** 0.5)
    dw3, none = hip.linear_wgrad(dy, x, False)
    assert none is None and torch.equal(dw3, dw)


def test_tall_linear_fn_gradients(tb):
    """TallLinearFn (library GEMMs for y and dx, tbx_linear_wgrad for dW / db) vs autograd of F.linear."""
    dev = torch.device("cuda:0")
    TG = import_module("trafficbots_amd.train_graph")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 500, 128, generator=g).to(dev)
    w, b = (torch.randn(256, 128, generator=g) * 0.1).to(dev), torch.randn(256, generator=g).to(dev)
    go = torch.randn(40, 500, 256, generator=g).to(dev)
    outs = []
    for kk, nn in ((128, 256), (128, 64), (121, 5), (31, 121), (128, 1)):  # the odd widths go through zero-padded copies; 64-wide: tbx_tall_linear on the padded image
        xk, wk, bk, gk = x[..., :kk].contiguous(), w[:nn, :kk].contiguous(), b[:nn].contiguous(), go[..., :nn].contiguous()
        outs = []
        for fn in (TG.linear, torch.nn.functional.linear):
            xx, ww, bb = xk.clone().requires_grad_(True), wk.clone().requires_grad_(True), bk.clone().requires_grad_(True)
            y = fn(xx, ww, bb)
            (y * gk).sum().backward()
            outs.append((y.detach(), xx.grad, ww.grad, bb.grad))
        for a, r in zip(*outs):
            torch.testing.assert_close(a, r, rtol=2e-4, atol=2e-4 * float(r.abs().max()))
    assert isinstance(TG.linear(x.requires_grad_(True), w, b).grad_fn, TG.TallLinearFn._backward_cls)


def test_train_chain_kernels_vs_torch_state_machine(tb):
    """tbx_train_chain_fwd / _bwd vs `training_rollout`'s elementwise torch state machine + autograd on random action means that
    make agents leave the map, reach destinations, get disabled and re-spawned by forcing: every logged tensor and d(mean)."""
    dev = torch.device("cuda:0")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    TG = import_module("trafficbots_amd.train_graph")
    scfg = tb.config.default_sim_cfg()
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(n_tgt_knn=4), data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev)
    n, A, T = 3, 40, 90
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(n, A, 64, 8, seed=3).items()}
    with torch.no_grad():
        b = wm.pre_processing(batch)
    b["map/boundary"] = torch.tensor([[-60.0, 60.0, -60.0, 60.0]], device=dev).repeat(n, 1)  # tight: many agents leave
    torch.manual_seed(11)
    b["gt/ag_valid"] = b["gt/ag_valid"] & (torch.rand(b["gt/ag_valid"].shape, device=dev) > 0.1)  # holes in the ground truth
    tf = wm.teacher_forcing_training
    tf.init(ag_valid=b["gt/ag_valid"], ag_pose=b["gt/ag_pose"], ag_motion=b["gt/ag_motion"], tl_state=b["gt/tl_state"], current_epoch=0)
    tf_mask = tf.ag_teacher_forcing | (torch.rand(b["gt/ag_valid"].shape, device=dev) < 0.05) & b["gt/ag_valid"]
    g = torch.Generator().manual_seed(2)
    mean0 = (torch.randn(n, T, A, 2, generator=g) * 1.5).to(dev)
    w_r = torch.randn(n, A, T, generator=g).to(dev)
    L = b["gt/tl_state"].shape[1]
    logits = torch.zeros(n, L, 5, device=dev)
    m1 = mean0.clone().requires_grad_(True)
    ro = TG.training_rollout(wm, b, None, {"tl_token_invalid": torch.zeros(n, L, dtype=torch.bool, device=dev)}, None, None, tf_mask, T,
                             need_hist=False, policy=lambda s, h, v, p, nv: (m1[:, s - 1], logits))
    (ro["reward"] * w_r).sum().backward()
    m2 = mean0.clone().requires_grad_(True)
    chain = TG.TrainChain(wm, b, tf_mask, T)
    out = chain.outputs(TG.TrainChainFn.apply(m2, chain))
    (out["reward"] * w_r).sum().backward()
    for k in ("pred_valid", "reward_valid", "tf"):
        assert torch.equal(out[k], ro[k]), k
    assert 0.05 < float(ro["pred_valid"].float().mean()) < 0.98
    assert bool((~ro["pred_valid"][:, :, -1] & ro["pred_valid"][:, :, 0]).any())  # some agents were disabled on the way
    for k in ("pred_pose", "pred_motion", "reward"):
        torch.testing.assert_close(out[k], ro[k], rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(m2.grad, m1.grad, rtol=1e-3, atol=1e-5 * float(m1.grad.abs().max()))
    assert float(m1.grad.abs().max()) > 0
    # one step at a time == all steps at once
    chain.reset()
    for s in range(1, T + 1):
        chain.step(s, mean0[:, s - 1])
    for k in ("pred_pose", "reward"):
        assert torch.equal(chain.outputs(chain.t["reward"])[k], out[k].detach()), k
    # the recorded pre-step states are the windows the torch loop builds
    rec = {}
    TG.training_rollout(wm, b, None, {"tl_token_invalid": torch.zeros(n, L, dtype=torch.bool, device=dev)}, None, None, tf_mask, T,
                        record=rec, policy=lambda s, h, v, p, nv: (mean0[:, s - 1], logits))
    hv, hp, hm, valid, pose, navi = chain.windows()
    assert torch.equal(hv.view(n, T, A, -1), torch.stack(rec["hv"], 1))
    torch.testing.assert_close(hp.view(n, T, A, -1, 3), torch.stack(rec["hp"], 1), rtol=1e-4, atol=2e-4)
    assert torch.equal(navi.view(n, T, A), torch.stack(rec["navi_valid"], 1))
    assert bool((~navi.view(n, T, A)[:, -1] & navi.view(n, T, A)[:, 0]).any())  # some destinations were reached


@pytest.mark.parametrize("sizes,knn", [((2, 8, 64, 8), 4), ((1, 64, 1024, 128), None), ((16, 64, 64, 8), 4)])  # last: 1024 agent rows -> tbx_layer_tile with its keyed dropouts
def test_nograd_policy_step_on_chain_kernels_equals_torch_ops_with_dropout(tb, sizes, knn):
    """The stepping pass of the time-batched rollout: with autograd off, train_graph runs whole layers as the inference engine's
    chain kernels (keyed dropouts as DROPOUT stages / inside the attention kernels). Same action means and light logits as the
    torch-op path with every dropout live (p = 0.1; the masks agree or the results would differ at the 10 % level)."""
    dev = torch.device("cuda:0")
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    TG = import_module("trafficbots_amd.train_graph")
    scfg = tb.config.default_sim_cfg()
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    cfg = tb.config.default_model_cfg(n_tgt_knn=knn) if knn else tb.config.default_model_cfg()
    wm = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    wm = wm.to(dev).train()
    model = wm.model
    n, A, M, L = sizes
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(n, A, M, L, seed=4).items()}
    outs = {}
    with torch.no_grad():
        b = wm.pre_processing(batch)
        for chains in (False, True):
            TG.state.NOGRAD_CHAINS = chains
            TG.state._DROP = {"seed": torch.tensor([99], dtype=torch.int64, device=dev), "call": 0, "site": 0, "n_batch": n, "tb": 1, "t0": 0}
            TG.state._FOLD_CACHE = {}
            try:
                mp = TG.map_encoder(model.mp_encoder, b["sc/mp_valid"], b["sc/mp_attr"], b["sc/mp_pose"], b["ref/mp_type"], True)
                tl = TG.tl_pre_compute(model.tl_encoder, b["gt/tl_valid"], b["sc/tl_attr"], b["sc/tl_pose"], mp)
                mp["_kv_cache"], tl["_kv_cache"] = {}, {}
                Wn = model.temp_window_size
                hv, hp, hm = model.ag_encoder.pad_hist(b["sc/ag_valid"], b["sc/ag_pose"], b["sc/ag_motion"], Wn)
                ht = model.tl_encoder.states_to_hist(b["gt/tl_state"][:, :, :Wn], Wn)
                z = torch.randn(n, A, model.latent_encoder.out_dim, generator=torch.Generator().manual_seed(1)).to(dev)
                valid = b["sc/ag_valid"][:, :, -1]
                res = []
                for step in (1, 2):  # two steps: the masks move with the step, the static map tables are cached
                    with TG._DropScope(n, 1, step, restart=TG._POLICY_SITE0):
                        res.append(TG.policy_step(model, (hv, hp, hm, ht), b["sc/ag_attr"].float().contiguous(), b["ref/ag_type"], valid,
                                                  b["sc/ag_pose"][:, :, -1], z, valid, b["gt/ag_navi"], valid, tl, mp, True))
                outs[chains] = res
                # light tokens encoded ahead (tl_pre): the agents' half alone - on the engine's schedule when chains are on
                eng = []
                for step in (1, 2):
                    with TG._DropScope(n, 1, step, restart=TG._POLICY_SITE0):
                        tl_feat = TG.tl_encoder(model.tl_encoder, ht, tl, True)
                        ids = (TG.state._DROP["site"], TG.state._DROP["call"])
                    with TG._DropScope(n, 1, step, restart=TG._POLICY_SITE0):
                        eng.append(TG.policy_step(model, (hv, hp, hm, ht), b["sc/ag_attr"].float().contiguous(), b["ref/ag_type"], valid,
                                                  b["sc/ag_pose"][:, :, -1], z, valid, b["gt/ag_navi"], valid, tl, mp, True,
                                                  tl_pre=(tl_feat, ids), want_logits=False)[0])
                outs[("engine", chains)] = eng
            finally:
                TG.state._DROP, TG.state._FOLD_CACHE, TG.state.NOGRAD_CHAINS = None, None, True
    for (m0, l0), (m1, l1) in zip(outs[False], outs[True]):
        torch.testing.assert_close(m1, m0, rtol=2e-4, atol=2e-5 + 2e-4 * float(m0.abs().max()))
        torch.testing.assert_close(l1, l0, rtol=2e-4, atol=2e-5 + 2e-4 * float(l0.abs().max()))
    assert not torch.equal(outs[False][0][0], outs[False][1][0])
    for step in range(2):  # agents' half: torch ops == engine chains == the full torch step
        ref = outs[False][step][0]
        for k in (("engine", False), ("engine", True)):
            torch.testing.assert_close(outs[k][step], ref, rtol=2e-4, atol=2e-5 + 2e-4 * float(ref.abs().max()))


def test_navi_pair_first_layer_is_the_concat_linear_without_the_concat(tb):
    """NaviPredictor's first pair Linear (navigation.py:245-262) split into per-agent + per-polyline + per-pair terms
    (train_graph.NaviPairFirstLayer): output and the gradients of all four inputs equal the reference formulation's
    `F.linear(cat([f_a, f_m, e]), W, b)` built with autograd, while what autograd keeps per (agent, polyline) pair is the 12-byte
    relative pose instead of the 1,536-byte concatenated row (+ 512 B of embedding): > 5x less, as SURVEY.md 8f-2 asks."""
    dev = torch.device("cuda:0")
    TG = import_module("trafficbots_amd.train_graph")
    hip = import_module("trafficbots_amd.hip")
    P = import_module("trafficbots_amd.utils.pose_emb")
    g = torch.Generator().manual_seed(3)
    n, A, M, d = 2, 9, 70, 128
    pe = P.PoseEmb("pe_xy_yaw", pe_dim=d, theta_xy=1e3).to(dev)
    rel = torch.cat([(torch.rand(n, A, M, 2, generator=g) - 0.5) * 150, (torch.rand(n, A, M, 1, generator=g) - 0.5) * 6], -1).to(dev)
    W = (torch.randn(d, 3 * d, generator=g) * 0.05).to(dev).requires_grad_(True)
    bias = torch.randn(d, generator=g).to(dev).requires_grad_(True)
    fa = torch.randn(n, A, d, generator=g).to(dev).requires_grad_(True)
    fm = torch.randn(n, M, d, generator=g).to(dev).requires_grad_(True)
    wout = torch.randn(n, A, M, d, generator=g).to(dev)
    # reference formulation
    emb = hip.pose_embed(rel.reshape(-1, 3).contiguous(), pe.pe_xy.freqs, pe.pe_yaw.freqs, d).view(n, A, M, d)
    zc = torch.cat([fa[:, :, None].expand(-1, -1, M, -1), fm[:, None].expand(-1, A, -1, -1), emb], -1)
    y_ref = torch.nn.functional.linear(zc, W, bias)
    (y_ref * wout).sum().backward()
    ref = [t.grad.clone() for t in (W, bias, fa, fm)]
    for t in (W, bias, fa, fm):
        t.grad = None
    # factorised
    pa = torch.nn.functional.linear(fa, W[:, :d])
    pm = torch.nn.functional.linear(fm, W[:, d:2 * d], bias)
    y = TG.NaviPairFirstLayer.apply(rel.contiguous(), W[:, 2 * d:], pa, pm, pe.pe_xy.freqs, pe.pe_yaw.freqs)
    kept = sum(t.numel() * t.element_size() for t in y.grad_fn.saved_tensors if t.shape[:3] == (n, A, M))
    assert kept == n * A * M * 12 and kept * 5 < zc.numel() * 4
    (y * wout).sum().backward()
    torch.testing.assert_close(y, y_ref, rtol=1e-4, atol=1e-4)
    for got, want, name in zip((W, bias, fa, fm), ref, ("W", "bias", "f_a", "f_m")):
        torch.testing.assert_close(got.grad, want, rtol=2e-4, atol=2e-4, msg=lambda m, name=name: f"{name}: {m}")


@pytest.mark.parametrize("shape", [(1, 128), (7, 9, 128), (70001, 128), (16, 64, 300, 128)])
def test_layernorm_backward_vs_float64_autograd(tb, shape):
    """tbx_layernorm_bwd behind train_graph.layer_norm (rows of 128; forward and backward) vs float64 autograd of F.layer_norm:
    dx per element, dgamma / dbeta relative to the sum of magnitudes they accumulate; deterministic across calls."""
    dev = torch.device("cuda:0")
    TG = import_module("trafficbots_amd.train_graph")
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(*shape, generator=g) * 3.0 + 0.5).to(dev)
    go = torch.randn(*shape, generator=g).to(dev)
    m = torch.nn.LayerNorm(128).to(dev)
    with torch.no_grad():
        m.weight.copy_(torch.randn(128, generator=g) * 0.5 + 1.0)
        m.bias.copy_(torch.randn(128, generator=g))
    res = []
    for _ in range(2):
        xx = x.clone().requires_grad_(True)
        m.zero_grad()
        y = TG.layer_norm(xx, m)
        assert isinstance(y.grad_fn, TG.LayerNormFn._backward_cls)
        (y * go).sum().backward()
        res.append((y.detach(), xx.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    xd = x.double().requires_grad_(True)
    wd, bd = m.weight.detach().double().requires_grad_(True), m.bias.detach().double().requires_grad_(True)
    yd = torch.nn.functional.layer_norm(xd, (128,), wd, bd, m.eps)
    (yd * go.double()).sum().backward()
    y, dx, dw, db = res[0]
    torch.testing.assert_close(y.double(), yd.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dx.double(), xd.grad, rtol=1e-4, atol=1e-5 * float(xd.grad.abs().max()))
    rows = x.numel() // 128
    xh = ((xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + m.eps)).detach()
    mag_w = (go.double().abs() * xh.abs()).reshape(rows, 128).sum(0)
    mag_b = go.double().abs().reshape(rows, 128).sum(0)
    assert float(((dw.double() - wd.grad).abs() / mag_w.clamp_min(1e-30)).max()) < 2e-6
    assert float(((db.double() - bd.grad).abs() / mag_b.clamp_min(1e-30)).max()) < 2e-6


@pytest.mark.parametrize("rows", [37, 20000])
def test_layer_norm_join_backward_is_the_sum_autograd_forms(tb, rows):
    """train_ops.layer_norm_join (LayerNormJoinFn: x handed back beside LayerNorm(x), ONE backward pass dx = d_residual + LayerNorm'(dy),
    tbx_layernorm_bwd_add) in the pre-norm residual form x' = x + f(LayerNorm(x)) vs layer_norm + autograd's own sum of the two gradients
    of x: outputs and every gradient bit-identical; a LayerNorm whose output is not used, and one whose x is not, included."""
    dev = torch.device("cuda:0")
    TG = import_module("trafficbots_amd.train_graph")
    g = torch.Generator().manual_seed(rows)
    m = torch.nn.LayerNorm(128).to(dev)
    with torch.no_grad():
        m.weight.copy_(torch.randn(128, generator=g)), m.bias.copy_(torch.randn(128, generator=g))
    x0 = torch.randn(rows, 128, generator=g).to(dev)
    wf = torch.randn(128, 128, generator=g).to(dev)
    go = torch.randn(rows, 128, generator=g).to(dev)
    res = {}
    for join in (True, False):
        x = x0.clone().requires_grad_(True)
        m.zero_grad()
        xa, xb = x * 1.0, x * 1.0  # (non-leaves, as in the block; every junction sums TWO gradients, as there - three would associate differently)
        if join:
            xr, s = TG.layer_norm_join(xa, m)
            assert isinstance(s.grad_fn, TG.LayerNormJoinFn._backward_cls) and xr.grad_fn is s.grad_fn
            _, unused = TG.layer_norm_join(xr, m)  # its LayerNorm output takes no gradient: the residual's passes through
            only_ln = TG.layer_norm_join(xb, m)[1]  # its x takes none
        else:
            xr, s = xa, TG.layer_norm(xa, m)
            only_ln = TG.layer_norm(xb, m)
        y = xr + torch.tanh(s @ wf) + 0.5 * only_ln
        (y * go).sum().backward()
        res[join] = (y.detach(), x.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone())
    for a_, b_ in zip(res[True], res[False]):
        assert torch.equal(a_, b_)


@pytest.mark.parametrize("relu", [False, True])
def test_pair_bias_relu_equals_the_broadcast_adds(tb, relu):
    """tbx_pair_bias_relu (NaviPredictor's first Linear, train_ops.NaviPairFirstLayer): h[n, a, m] += pa[n, a] + pm[n, m] (+ relu) in one
    in-place pass vs the torch broadcast ops it replaces - bit-identical (h + (pa + pm), the same association)."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    g = torch.Generator().manual_seed(11)
    n, A, M, d = 3, 7, 33, 128
    h = torch.randn(n, A, M, d, generator=g).to(dev)
    pa, pm = torch.randn(n, A, d, generator=g).to(dev), torch.randn(n, M, d, generator=g).to(dev)
    ref = h + (pa.unsqueeze(2) + pm.unsqueeze(1))
    ref = torch.relu(ref) if relu else ref
    out = hip.pair_bias_relu(h.clone(), pa, pm, relu)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("G,W,dropout", [(5, 11, False), (3000, 11, True), (777, 16, True), (64, 1, False), (1500, 20, True), (300, 19, False), (9, 32, True)])
def test_fused_pointnet_glue_equals_the_aten_ops(tb, G, W, dropout):
    """train_graph.pointnet with tbx_pointnet_tail_* / tbx_masked_maxpool_* (one launch per layer for relu / keyed dropout / masked max /
    concat / zeroing, one for their backward) vs the same function on aten ops: forward bit-identical (same masks: the dropout ids
    agree), input and parameter gradients at fp32 summation level - with ties (ReLU zeros, repeated rows), invalid rows and groups
    without a valid row."""
    dev = torch.device("cuda:0")
    W_ = import_module("trafficbots_amd.pl_modules.waymo_motion")
    TG = import_module("trafficbots_amd.train_graph")
    wm = W_.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg())
    tb.utils.det_fill(wm.model, 0)
    enc = wm.model.ag_encoder.temp_encoder.to(dev)
    g = torch.Generator().manual_seed(G + W)
    x = torch.randn(G, W, 128, generator=g)
    if W > 2:
        x[:, 2] = x[:, 1]  # tied maxima
    invalid = torch.rand(G, W, generator=g) < 0.3
    invalid[0] = True  # a group without a valid row
    go = torch.randn(G, 128, generator=g).to(dev)
    x, invalid = x.to(dev), invalid.to(dev)
    res = {}
    saved = (TG.state.POINTNET_FUSED, TG.state._DROP)
    try:
        for fused in (True, False):
            TG.state.POINTNET_FUSED = fused
            TG.state._DROP = {"seed": torch.tensor([1234], dtype=torch.int64, device=dev), "call": 0, "site": 7, "n_batch": 1, "tb": 1, "t0": 3}
            xx = x.clone().requires_grad_(True)
            enc.zero_grad()
            y = TG.pointnet(enc, xx, invalid, training=dropout)
            assert isinstance(y.grad_fn, TG.MaskedMaxPoolFn._backward_cls) == fused
            (y * go).sum().backward()
            res[fused] = (y.detach(), xx.grad.clone(), [p.grad.clone() for p in enc.parameters()], TG.state._DROP["site"])
    finally:
        TG.state.POINTNET_FUSED, TG.state._DROP = saved
    (ya, dxa, dpa, sa), (yb, dxb, dpb, sb) = res[True], res[False]
    assert sa == sb  # the dropout site ids advance alike
    assert torch.equal(ya, yb) and float(ya[0].abs().max()) == 0.0
    if dropout:
        assert bool((ya == 0).any())
    torch.testing.assert_close(dxa, dxb, rtol=1e-4, atol=1e-5 * float(dxb.abs().max()))
    for a, b in zip(dpa, dpb):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=2e-5 * float(b.abs().max()) + 1e-12)


@pytest.mark.parametrize("rows,cols,dropout", [(1000, 128, True), (3, 512, True), (50000, 128, False), (4097, 512, True)])
def test_fused_transformer_glue_equals_the_aten_ops(tb, rows, cols, dropout):
    """train_graph.residual / relu_drop as tbx_residual_drop_* / tbx_relu_drop_* (one pass per tensor) vs the aten sequence they replace
    (masked_fill, keyed dropout, add, masked_fill; relu, keyed dropout): values and input gradients bit-identical - the same keyed masks
    (site ids advance alike), the same products."""
    dev = torch.device("cuda:0")
    TG = import_module("trafficbots_amd.train_graph")
    g = torch.Generator().manual_seed(rows + cols)
    x, y = torch.randn(rows, cols, generator=g).to(dev), torch.randn(rows, cols, generator=g).to(dev)
    zy = (torch.rand(rows, generator=g) < 0.2).to(torch.uint8).to(dev)
    zo = (torch.rand(rows, generator=g) < 0.2).to(dev)
    go = torch.randn(rows, cols, generator=g).to(dev)
    p = 0.1
    res = {}
    saved = (TG.state.GLUE_FUSED, TG.state._DROP)
    try:
        for fused in (True, False):
            TG.state.GLUE_FUSED = fused
            TG.state._DROP = {"seed": torch.tensor([77], dtype=torch.int64, device=dev), "call": 0, "site": 3, "n_batch": 1, "tb": 1, "t0": 5}
            xx, yy = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            a = TG.residual(xx, yy, p, dropout, zero_y=zy)                  # attention residual
            b = TG.residual(a, TG.relu_drop(yy, p, dropout), p, dropout, zero_out=zo)   # FFN tail with the closing row mask
            assert isinstance(b.grad_fn, TG.ResidualDropFn._backward_cls) == fused
            (b * go).sum().backward()
            res[fused] = (a.detach(), b.detach(), xx.grad.clone(), yy.grad.clone(), TG.state._DROP["site"])
    finally:
        TG.state.GLUE_FUSED, TG.state._DROP = saved
    assert res[True][4] == res[False][4] == (6 if dropout else 3)
    for u, v in zip(res[True][:4], res[False][:4]):
        assert torch.equal(u, v)
    assert bool((res[True][1][zo] == 0).all())


def test_modules_in_train_mode_run_the_differentiable_path(tb):
    """The reference's modules run in train() with their default dropouts (transformer_rpe.py:207-245, mlp.py:58-72,
    polyline_encoder.py:49-61, add_navi_latent.py:52-65): here `TransformerBlockRPE / AttentionRPE / MLP / PolylineEncoder /
    AddNaviLatent.forward` in train mode take the training path (HIP attention forward / backward, keyed dropout, autograd).
    Checked through the reference signatures: p = 0 in train mode == eval mode (values), gradients == the oracle's autograd;
    p = 0.1: masks are live (outputs differ from eval, about 10 % of an MLP's outputs are zeroed), reproducible under
    torch.manual_seed, gradients finite and flowing to every parameter."""
    from oracle import hptr_ops as H

    dev = torch.device("cuda:0")
    M = import_module("trafficbots_amd.models.modules")
    g = torch.Generator().manual_seed(3)
    n, S, K, Ks, d = 2, 19, 9, 5, 128
    src = torch.randn(n, S, d, generator=g)
    tgt = torch.randn(n, S, K, d, generator=g)
    rpe = torch.randn(n, S, K, d, generator=g)
    m = torch.rand(n, S, K, generator=g) < 0.3
    src_inv = torch.rand(n, S, generator=g) < 0.2
    m[src_inv] = True
    idx_self = torch.randint(0, S, (n, S, Ks), generator=g)
    m_self = torch.rand(n, S, Ks, generator=g) < 0.3
    m_self[src_inv] = True
    rpe_self = torch.randn(n, S, Ks, d, generator=g)
    to = lambda t: t.to(dev)

    def build(p):
        blk = M.transformer_rpe.TransformerBlockRPE(n_layer=2, mode="dec_cross_attn", d_rpe=128, d_model=128, n_head=4, k_feedforward=4,
                                                    dropout_p=p, bias=True, activation="relu", out_layernorm=False, apply_q_rpe=False)
        tb.utils.det_fill(blk, 5)
        return blk.to(dev)

    def call(blk, x):
        return blk(src=x, src_padding_mask=to(src_inv), tgt=to(tgt), tgt_padding_mask=to(m), rpe=to(rpe), decoder_tgt=to(idx_self),
                   decoder_tgt_padding_mask=to(m_self), decoder_rpe=to(rpe_self))[0]

    blk0 = build(0.0)
    y_eval = call(blk0.eval(), to(src))
    x = to(src).requires_grad_(True)
    y_tr = call(blk0.train(), x)
    torch.testing.assert_close(y_tr.detach(), y_eval, rtol=2e-4, atol=2e-5 + 2e-4 * float(y_eval.abs().max()))
    y_tr.square().sum().backward()
    # oracle autograd on the CPU
    P = {"t." + k: v.detach().cpu().clone().requires_grad_(True) for k, v in blk0.state_dict().items()}
    xs = src.clone().requires_grad_(True)
    ref = H.transformer_block(P, "t", "dec_cross_attn", 2, 4, xs, src_inv, tgt, m, rpe, idx_self, m_self, rpe_self)
    ref.square().sum().backward()
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-6)
    assert close(x.grad.cpu(), xs.grad, 2e-3)
    for k, p_ in blk0.named_parameters():
        gref = P["t." + k].grad
        if gref is None:
            assert p_.grad is None or float(p_.grad.abs().max()) == 0.0, k
        else:
            assert close(p_.grad.cpu(), gref, 2e-3), k
    # p = 0.1: live, reproducible masks
    blk = build(0.1).train()
    torch.manual_seed(7)
    y1 = call(blk, to(src))
    torch.manual_seed(7)
    y2 = call(blk, to(src))
    torch.manual_seed(8)
    y3 = call(blk, to(src))
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    assert float((y1 - call(blk.eval(), to(src))).abs().max()) > 1e-3
    blk.train()
    xg = to(src).requires_grad_(True)
    call(blk, xg).square().sum().backward()
    assert torch.isfinite(xg.grad).all() and all(p_.grad is None or torch.isfinite(p_.grad).all() for p_ in blk.parameters())

    # AttentionRPE / MLP / PolylineEncoder / AddNaviLatent in train mode
    att = M.attention_rpe.AttentionRPE(d_model=128, n_head=4, dropout_p=0.1, d_rpe=128)
    tb.utils.det_fill(att, 6)
    att = att.to(dev).train()
    xa = to(src).requires_grad_(True)
    ya = att(xa, to(tgt), tgt_padding_mask=to(m), rpe=to(rpe))[0]
    ya.sum().backward()
    assert torch.isfinite(ya).all() and torch.isfinite(xa.grad).all() and att.in_proj_weight.grad is not None
    assert float((ya - att.eval()(to(src), to(tgt), tgt_padding_mask=to(m), rpe=to(rpe))[0]).abs().max()) > 1e-4
    mlp = M.mlp.MLP([64, 128, 128], dropout_p=0.1).to(dev).train()
    xm = torch.randn(500, 64, generator=g).to(dev).requires_grad_(True)
    ym = mlp(xm)
    frac0 = float((ym == 0).float().mean())
    assert 0.05 < frac0 < 0.75  # relu zeros + ~10 % dropped
    ym.sum().backward()
    assert torch.isfinite(xm.grad).all()
    pe = M.polyline_encoder.PolylineEncoder(hidden_dim=128, tf_cfg=None, n_layer=3, mlp_use_layernorm=False, mlp_dropout_p=0.1, use_pointnet=True,
                                            pooling_mode="max_valid").to(dev).train()
    xp = torch.randn(2, 30, 11, 128, generator=g).to(dev).requires_grad_(True)
    ip = (torch.rand(2, 30, 11, generator=g) < 0.3).to(dev)
    yp = pe(xp, ip)
    yp.sum().backward()
    assert yp.shape == (2, 30, 128) and torch.isfinite(xp.grad).all()
    an = M.add_navi_latent.AddNaviLatent(hidden_dim=128, in_dim=16, dummy=False, mode="cat", n_layer=3, mlp_use_layernorm=False,
                                         mlp_dropout_p=0.1, res_add=True).to(dev).train()
    xn = torch.randn(2, 9, 128, generator=g).to(dev).requires_grad_(True)
    zn = torch.randn(2, 9, 16, generator=g).to(dev)
    zv = (torch.rand(2, 9, generator=g) < 0.8).to(dev)
    yn = an(xn, zn, zv)
    yn.sum().backward()
    assert torch.isfinite(yn).all() and torch.isfinite(xn.grad).all()
    torch.testing.assert_close(yn[~zv], xn.detach()[~zv])  # rows without a valid z pass through


# ---------------------------------------------------------------------------------------------------- the bf16 (autocast-class) contractions
@pytest.mark.parametrize("rows,n,k,ld_pad", [(20000, 128, 128, 0), (70001, 640, 128, 0), (33333, 128, 640, 0), (16390, 64, 20, 12), (17, 128, 64, 0),
                                            (300000, 256, 128, 0)])
def test_linear_wgrad_bf16_vs_float64(tb, rows, n, k, ld_pad):
    """tbx_linear_wgrad_bf16 (dW = dY^T X with dY, X rounded to bfloat16 in registers, fp32 accumulation over the rows; db exact) vs
    float64: every term carries two 2^-9 roundings, so |dW - ref| <= 2^-8 sum |dy||x| is the worst case; with random signs the error of
    a sum of R terms is ~2^-8.5 sqrt(sum (dy x)^2): stated as 3e-3 of sqrt(sum dy^2 x^2) per entry (measured ~1.1e-3 x that, printed)
    and always inside the worst-case bound; equal to the fp32 kernel on inputs that ARE bfloat16 values; deterministic."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    g = torch.Generator().manual_seed(rows + n + k)
    dy = torch.randn(rows, n, generator=g).to(dev)
    xs = torch.randn(rows, k + ld_pad, generator=g).to(dev)
    x = xs[:, :k]
    dw, db = hip.linear_wgrad(dy, x, True, bf16=True)
    dw2, db2 = hip.linear_wgrad(dy, x, True, bf16=True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    ref = dy.double().t() @ x.double()
    worst = dy.double().abs().t() @ x.double().abs()
    rms = ((dy.double() ** 2).t() @ (x.double() ** 2)).sqrt()
    err = (dw.double() - ref).abs()
    print(f"[wgrad bf16 vs float64] rows={rows} n={n} k={k}: max err / worst-case bound {float((err / worst).max()):.3g} (bound 2^-8 = 3.9e-3), "
          f"max err / sqrt(sum dy^2 x^2) {float((err / rms).max()):.3g}")
    assert float((err / worst).max()) < 2.0 ** -8 and float((err / rms).max()) < 3e-3 * 4  # (4 sigma-ish over n * k entries)
    torch.testing.assert_close(db.double(), dy.double().sum(0), rtol=1e-5, atol=1e-5 * rows ** 0.5)
    assert float((err / rms).max()) > 1e-5  # the operands really were rounded
    # inputs that are exactly representable in bfloat16: the one-product kernel and the exact-fp32 kernel agree to accumulation order
    dyb, xb = dy.to(torch.bfloat16).float(), x.to(torch.bfloat16).float().contiguous()
    a, _ = hip.linear_wgrad(dyb, xb, False, bf16=True)
    b, _ = hip.linear_wgrad(dyb, xb, False, bf16=False)
    magb = dyb.double().abs().t() @ xb.double().abs()
    assert float(((a.double() - b.double()).abs() / magb).max()) < 2e-6


@pytest.mark.parametrize("m,k,n,wt,bias", [(1000, 128, 128, False, True), (70001, 128, 640, False, True), (4097, 640, 128, False, False), (20000, 128, 256, True, False),
                                           # the 64-wide PointNet layers (round 6): forward 128 -> 64 and its input gradient 64 -> 128 (wt) on the
                                           # zero-padded image, loads / stores masked by column
                                           (30011, 128, 64, False, True), (30011, 64, 128, True, False), (5000, 192, 64, False, True)])
def test_tall_linear_bf16_vs_float64(tb, m, k, n, wt, bias):
    """tbx_tall_linear_bf16 (y = x W^T + b with x and W rounded to bfloat16, fp32 accumulation) vs float64: within 2^-8 sum |x||w| (worst
    case of two 2^-9 roundings per term); exactly the fp32-class kernel's result up to accumulation when x and W are bfloat16 values."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    g = torch.Generator().manual_seed(m + k + n)
    x = torch.randn(m, k, generator=g).to(dev)
    w = (torch.randn(k, n, generator=g) if wt else torch.randn(n, k, generator=g)).to(dev) * 0.1
    b = torch.randn(n, generator=g).to(dev) if bias else None
    y = hip.tall_linear(x, w, b, wt=wt, bf16=True)
    wd = w.double() if wt else w.double().t()
    ref = x.double() @ wd + (b.double() if bias else 0.0)
    worst = x.double().abs() @ wd.abs()
    err = (y.double() - ref).abs()
    print(f"[tall linear bf16 vs float64] m={m} k={k} n={n}: max err / sum |x||w| {float((err / worst).max()):.3g}")
    assert float((err / worst).max()) < 2.0 ** -8 and float((err / worst).max()) > 1e-6
    # the dual-output form (tbx_linear_t.y16: the K/V tables' bfloat16 copy written by the producing launch): the same fp32 rows, and
    # their round-to-nearest-even bfloat16 values
    for cls in (True, False):
        y16 = torch.empty(m, n, dtype=torch.bfloat16, device=dev)
        yd = hip.tall_linear(x, w, b, wt=wt, bf16=cls, out16=y16)
        assert torch.equal(yd, hip.tall_linear(x, w, b, wt=wt, bf16=cls)) and torch.equal(y16, yd.to(torch.bfloat16))
    xb, wb = x.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
    y1, y3 = hip.tall_linear(xb, wb, b, wt=wt, bf16=True), hip.tall_linear(xb, wb, b, wt=wt, bf16=False)
    assert float(((y1 - y3).abs().double() / (xb.double().abs() @ (wb.double() if wt else wb.double().t()).abs() + 1e-30)).max()) < 2e-6


def test_mfma_attention_forward_draws_the_valu_kernels_dropout_mask(tb):
    """tbx_knarpe_attn_fwd_mfma with dropout must drop exactly the (row, target slot, head) probabilities the VALU forward / backward kernels
    drop for the same key (the fp32 backward regenerates the mask from it). V tables are one-hot rows - V[j][32 h + j] = 1 for every head
    h, K <= 32 distinct targets per row - so out[row][32 h + j] IS head h's dropped-and-rescaled probability of target j: the zero
    pattern of the two kernels must be identical (two segments, time-batched key), the kept probabilities agree to the bf16 operand
    tolerance, and the pattern changes with the call id."""
    dev = torch.device("cuda:0")
    hip = import_module("trafficbots_amd.hip")
    PE = import_module("trafficbots_amd.utils.pose_emb")
    g = torch.Generator().manual_seed(5)
    n, S, T0, K0, T1, K1, tb_, t0 = 6, 67, 24, 20, 40, 12, 3, 4
    pe = PE.PoseEmb("pe_xy_yaw", pe_dim=128, theta_xy=1e3).to(dev)
    fxy, fyw = pe.pe_xy.freqs, pe.pe_yaw.freqs
    q = (torch.randn(n * S, 640, generator=g) * 0.3).to(dev)

    def seg(T, K, col0):  # tokens 0 .. K - 1 of every table are the ones indexed: token j shows in column col0 + j of every head
        kv = torch.zeros(n * T, 256)
        kv[:, :128] = torch.randn(n * T, 128, generator=g) * 0.3
        for j in range(K):
            for h in range(4):
                kv[j::T, 128 + 32 * h + col0 + j] = 1.0
        idx = torch.stack([torch.stack([torch.randperm(K, generator=g) for _ in range(S)]) for _ in range(n)]).to(torch.int32)
        inv = (torch.rand(n, S, K, generator=g) < 0.2).to(torch.uint8)
        rel = torch.cat([(torch.rand(n, S, K, 2, generator=g) - 0.5) * 80, (torch.rand(n, S, K, 1, generator=g) - 0.5) * 6], -1)
        return hip.Seg(kv.to(dev), 0, 128, T, idx.to(dev), inv.to(dev), None, 1, rel=rel.to(dev).contiguous())

    segs = [seg(T0, K0, 0), seg(T1, K1, 20)]  # segment 0's targets show in columns 0..19, segment 1's in 20..31 of every head
    bias = torch.zeros(128, device=dev)
    seed = torch.tensor([0x1234567887654321 & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64, device=dev)
    outs = {}
    for name, call in (("valu", 7), ("mfma", 7), ("mfma_other_call", 8)):
        out = torch.empty(n * S, 640, device=dev)
        flag = torch.empty(n * S, dtype=torch.uint8, device=dev)
        drop = (0.25, seed, call, tb_, t0)
        if name == "valu":
            hip.knarpe_attn(q, 0, 128, bias, n, S, segs, out, flag, fxy, fyw, drop=drop)
        else:
            hip.knarpe_attn_mfma(q, 0, 128, n, S, segs, out, flag, fxy, fyw, drop=drop)
        torch.cuda.synchronize()
        outs[name] = out[:, :128].clone()
    a, b, c = outs["valu"], outs["mfma"], outs["mfma_other_call"]
    assert torch.equal(a == 0, b == 0)  # the same probabilities were dropped (masked targets are zeros in both)
    frac = float(((a == 0) & (c != 0)).float().mean())
    assert 0.01 < frac  # ... and they depend on the call id
    assert float((a - b).abs().max()) <= 2e-2 * float(a.abs().max()) and float((a - b).abs().max()) > 0.0
    kept = float((a != 0).float().mean())
    assert 0.3 < kept < 0.9


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sixteen_scene_step_is_the_count_weighted_recombination_of_its_quarters(tb, prec, monkeypatch):
    """BASELINE config 3 at its own batch size (batch 16 was benchmarked, never checked): one training step on 16
    scenes of 64 agents / 1024 polylines / 128 lights against the EXACT recombination of four 4-scene steps - the first of which is the
    batch the reference itself ran (tests/golden/train_c2_b4.npz: scenes 0..3 of the same generator). Every loss term of the reference
    is a ratio of sums over the whole batch (metrics/training.py:166-186), so with c_i the term's counter in sub-batch i:
        term(batch) = sum_i c_i term_i / sum_i c_i,      d term(batch) / d theta = sum_i (c_i / sum_j c_j) d term_i / d theta.
    Scenes do not interact anywhere else (every kernel works row by row / scene by scene), so the 16-scene launches - 92,160 agent
    rows per LINEAR: tbx_tall_linear / tbx_linear_wgrad and their bf16 forms at the benchmarked size, the time-batched attention and
    chain kernels over 16 x 90 batch entries - must reproduce the 4-scene results up to summation order (weight gradients reduced over
    4 x the rows at once; atomics in the attention backward). RNG sites neutralised as in the fixtures.
    Why quarters and not single scenes: the schedule picks kernels by row count (tile kernels from 193 rows, tall LINEARs from 16,384,
    matrix-core attention from 193), and a single 64-agent scene falls on the other side of all three - a different arithmetic class
    in the bf16 case, not a different summation order (measured: 2.8e-3 on the loss). A quarter sits on the batch's side of every
    threshold once the tall LINEAR's is lowered to 4,096 rows (a quarter's map rows: 4 x 1024; the batch's population of tall LINEARs is
    unchanged by that - each has >= 16,384 rows)."""
    dev = torch.device("cuda:0")
    monkeypatch.setattr(import_module("trafficbots_amd.train_ops"), "WGRAD_MIN_ROWS", 4096)
    n_sc, n_sub, sizes = 16, 4, (64, 1024, 128)
    cfg = tb.config.default_model_cfg(n_tgt_knn=32)
    cfg["tf_cfg"]["dropout_p"] = 0.0
    cfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
    cfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    scfg = tb.config.default_sim_cfg(p_training_rollout_prior=0.0)
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    wm = W.WaymoMotion(model=cfg, data_size=tb.synthetic.DATA_SIZE, **scfg)
    tb.utils.det_fill(wm.model, 0)
    with torch.no_grad():
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    wm = wm.to(dev).train()
    wm.train_precision = prec
    cpu_batch = tb.synthetic.make_scene(n_sc, *sizes, seed=0)
    fixture_batch = tb.synthetic.make_scene(n_sub, *sizes, seed=0)
    for k, v in fixture_batch.items():  # the first quarter is the batch the reference ran for train_c2_b4.npz
        assert torch.equal(cpu_batch[k][:n_sub], v), k
    batch = {k: v.to(dev) for k, v in cpu_batch.items()}
    noise = torch.randn(n_sc, sizes[0], 16, generator=torch.Generator().manual_seed(3)).to(dev)
    use_prior = torch.zeros((), dtype=torch.bool, device=dev)
    terms = ("vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss")
    sign = {"vae_kl": 1.0, "diffbar_reward": -1.0, "navi_loss": 1.0, "tl_state_loss": 1.0}
    # ---- the 16-scene step
    loss = wm.training_step({k: v.clone() for k, v in batch.items()}, 0, noise=noise, use_prior=use_prior)
    loss.backward()
    big = {k: float(v.detach()) for k, v in wm.last_metrics.items()}
    C = {k: float(wm.last_counts[k]) for k in terms}
    assert all(c > 0 for c in C.values())
    named = [(k, p) for k, p in wm.model.named_parameters() if p.grad is not None]
    g_big = {k: p.grad.detach().double().clone() for k, p in named}
    for _, p in named:
        p.grad = None
    # ---- four 4-scene steps, each term weighted by its share of the batch's counter
    rec, c_sum = {k: 0.0 for k in terms}, {k: 0.0 for k in terms}
    for i in range(0, n_sc, n_sub):
        part = {k: v[i:i + n_sub].clone() for k, v in batch.items()}
        wm.training_step(part, 0, noise=noise[i:i + n_sub], use_prior=use_prior)
        m, c = wm.last_metrics, wm.last_counts
        comb = 0.0
        for k in terms:
            w = float(c[k]) / C[k]
            c_sum[k] += float(c[k])
            rec[k] += w * float(m[k].detach())
            comb = comb + sign[k] * w * m[k]
        comb.backward()  # (gradients accumulate over the sub-batches)
    assert c_sum == C  # the counters themselves add up exactly
    rec["loss"] = sum(sign[k] * rec[k] for k in terms)
    meas = {"loss": 0.0, "gnorm": 0.0, "grad": 0.0}
    for k in ("loss",) + terms:
        meas["loss"] = max(meas["loss"], abs(big[k] - rec[k]) / max(abs(rec[k]), 1e-1))
    gn_b, gn_r, gmax, dmax = {}, {}, {}, {}
    for k, p in named:
        top = k.split(".")[0]
        g = p.grad.detach().double()
        gn_b[top] = gn_b.get(top, 0.0) + float(g_big[k].pow(2).sum())
        gn_r[top] = gn_r.get(top, 0.0) + float(g.pow(2).sum())
        gmax[top] = max(gmax.get(top, 0.0), float(g.abs().max()))
        dmax[top] = max(dmax.get(top, 0.0), float((g_big[k] - g).abs().max()))
    for top in gn_b:
        meas["gnorm"] = max(meas["gnorm"], abs(gn_b[top] ** 0.5 - gn_r[top] ** 0.5) / max(gn_r[top] ** 0.5, 1e-12))
        meas["grad"] = max(meas["grad"], dmax[top] / max(gmax[top], 1e-12))  # largest entry-wise difference over the module's largest entry
    print(f"[16-scene step vs recombined 4-scene steps, {prec}] loss terms: max rel diff {meas['loss']:.3g}; per-module gradient norms: max rel diff "
          f"{meas['gnorm']:.3g}; gradients entry-wise: max |d| / max |g| of the module {meas['grad']:.3g}; counters {C}")
    tol = RECOMBINE_TOL[prec]
    assert meas["loss"] <= tol["loss"] and meas["gnorm"] <= tol["gnorm"] and meas["grad"] <= tol["grad"], meas


def test_attention_fold_kernels_equal_the_torch_algebra(tb):
    """tbx_attn_fold_fwd / _bwd (one launch each per AttentionRPE module) against the slice / bmm / cat algebra they replace
    (train_ops.fold_attention_weights_torch) and its autograd: the seven folded tensors and the gradients of all six
    parameters, with every output used and with outputs left unused (their gradient arrives as None)."""
    dev = torch.device("cuda:0")
    TO = import_module("trafficbots_amd.train_ops")
    A = import_module("trafficbots_amd.models.modules.attention_rpe")
    torch.manual_seed(0)
    att = A.AttentionRPE(d_model=128, n_head=4, dropout_p=0.0, bias=True, d_rpe=128, apply_q_rpe=False).to(dev)
    with torch.no_grad():
        for p in att.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    names = ("w_in", "b_in", "w_kv", "b_kv", "bias_k", "w_out", "b_out")
    params = (att.in_proj_weight, att.in_proj_bias, att.linear_rpe.weight, att.linear_rpe.bias, att.out_proj_weight, att.out_proj_bias)
    g = torch.Generator().manual_seed(1)
    ref = TO.fold_attention_weights_torch(att)
    cot = {k: torch.randn(ref[k].shape, generator=g).to(dev) for k in names}
    for used in (names, ("w_in", "b_in"), ("w_kv", "b_out"), ("bias_k", "w_out")):
        ref = TO.fold_attention_weights_torch(att)
        got = dict(zip(names, TO.AttnFoldFn.apply(*params)))
        for k in names:
            torch.testing.assert_close(got[k], ref[k], rtol=1e-5, atol=1e-5)
        g_ref = torch.autograd.grad(sum((ref[k] * cot[k]).sum() for k in used), params, allow_unused=True)
        g_got = torch.autograd.grad(sum((got[k] * cot[k]).sum() for k in used), params, allow_unused=True)
        for p_ref, p_got, p in zip(g_ref, g_got, params):
            want = torch.zeros_like(p) if p_ref is None else p_ref
            torch.testing.assert_close(p_got, want, rtol=1e-4, atol=1e-4)
    # and inside a training step the Function is what runs (the fold's launches are the ones it replaced)
    assert TO.ATTN_FOLD_KERNEL


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("rows,k,n,nb,dropout", [(20480, 128, 512, 4, True), (16450, 128, 128, 1, True), (18000, 256, 128, 2, False)])
def test_linear_relu_drop_one_launch_equals_two(tb, rows, k, n, nb, dropout, prec):
    """train_ops.linear_relu_drop (tbx_tall_linear with tbx_linear_t.drop: LINEAR + relu + keyed dropout in the launch's epilogue; the FFN's hidden
    activation / an MLP layer over the time-batched rows) against the two launches it replaces (TallLinearFn, then ReluDropFn): values and
    all three gradients bit-identical - the same products, the same keyed mask (site ids advance alike; row count not a multiple of 64,
    several scenes per batch, a time batch with an offset)."""
    dev = torch.device("cuda:0")
    TO = import_module("trafficbots_amd.train_ops")
    ST = import_module("trafficbots_amd.train_state")
    g = torch.Generator().manual_seed(rows + n)
    x0 = torch.randn(rows, k, generator=g).to(dev)
    w0, b0 = (torch.randn(n, k, generator=g) * 0.1).to(dev), torch.randn(n, generator=g).to(dev)
    go = torch.randn(rows, n, generator=g).to(dev)
    p = 0.1
    res = {}
    saved = (TO.LINEAR_RELU_DROP, ST._DROP, ST._PREC)
    try:
        ST._PREC = prec
        for fused in (True, False):
            TO.LINEAR_RELU_DROP = fused
            ST._DROP = {"seed": torch.tensor([91], dtype=torch.int64, device=dev), "call": 0, "site": 7, "n_batch": nb, "tb": 2 if nb % 2 == 0 else 1, "t0": 3}
            x, w, b = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            h = TO.linear_relu_drop(x, w, b, p, dropout)
            assert isinstance(h.grad_fn, TO.TallLinearReluDropFn._backward_cls) == fused
            (h * go).sum().backward()
            res[fused] = (h.detach(), x.grad.clone(), w.grad.clone(), b.grad.clone(), ST._DROP["site"])
    finally:
        TO.LINEAR_RELU_DROP, ST._DROP, ST._PREC = saved
    assert res[True][4] == res[False][4] == (8 if dropout else 7)
    for u, v in zip(res[True][:4], res[False][:4]):
        assert torch.equal(u, v)
    frac0 = float((res[True][0] == 0).float().mean())
    assert (0.5 < frac0 < 0.65) if dropout else (0.4 < frac0 < 0.6)  # relu zeroes ~half, the dropout a tenth of the rest
