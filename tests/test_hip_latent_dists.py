"""GPU checks of the learned latent distributions (conditional prior, per-type branches, learned log_std, categorical family) at the
c1 sizes against the reference's recorded runs (tests/golden/latent_c1.npz, train_c1_latent.npz; tests/golden/make_golden_latent.py):
the eval-mode distributions of both sides, joint_future_pred and validation_step on them, and the training step - against the
reference, across its three schedules, captured, and untouched for the default configuration.

The scene is latent_ref.c1_batch: make_scene with two planted agents - one seen in the history only between the down-sampled steps, one
seen in the future only - whose learned prior is invalid while their posterior is valid."""
import sys
from collections import Counter
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import latent_ref as LR  # noqa: E402
from test_hip_training import TRAIN_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(autouse=True)
def _fp32_class_by_default():
    TG = import_module("trafficbots_amd.train_graph")
    prev = TG.state.DEFAULT_PRECISION
    TG.state.DEFAULT_PRECISION = "fp32"
    yield
    TG.state.DEFAULT_PRECISION = prev


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "latent_c1.npz")


@pytest.fixture(scope="module")
def golden_train(golden_dir):
    return np.load(golden_dir / "train_c1_latent.npz")


def _wm(tb, tag, free_nats=1.0, **over):
    """The module of a tag with the fixtures' weights (det_fill, damped action head) and every random site of a step neutralised."""
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg(**over)
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["training_metrics"]["kl_free_nats"] = free_nats
    wm = W.WaymoMotion(model=LR.model_cfg(tb, tag), data_size=tb.synthetic.DATA_SIZE, **scfg)
    LR.det_fill(tb, wm.model)
    with torch.no_grad():
        for k, p in wm.model.named_parameters():
            if k.startswith("action_head.mlp_mean") and ".fc_layers.4." in k:
                p.mul_(0.02)
    return wm


def _eval_dists(tb, wm, batch, dev):
    """(pre-processed batch, map tokens, light tokens, posterior, prior) as validation_step makes them."""
    full = {**batch, **tb.synthetic.to_history_batch(batch)}
    bd = wm.pre_processing({k: v.to(dev) for k, v in full.items()})
    mp, tl = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")
    kw = dict(ag_attr=bd["sc/ag_attr"], ag_type=bd["ref/ag_type"], mp_tokens=mp, tl_tokens=tl)
    post = wm.model.latent_encoder(ag_valid=bd["gt/ag_valid"], ag_motion=bd["gt/ag_motion"], ag_pose=bd["gt/ag_pose"], tl_state=bd["gt/tl_state"],
                                   posterior=True, **kw)
    prior = wm.model.latent_encoder(ag_valid=bd["sc/ag_valid"], ag_motion=bd["sc/ag_motion"], ag_pose=bd["sc/ag_pose"], tl_state=bd["sc/tl_state"],
                                    posterior=False, **kw)
    return bd, mp, tl, post, prior


def _params(d):
    if hasattr(d, "logits"):
        return {"logits": d.logits}
    return {"mean": d.mean, "log_std": d.stddev.expand_as(d.mean).log()}


# ------------------------------------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("tag", list(LR.TAGS))
def test_eval_distributions_vs_reference(tb, golden, tag):
    """Both sides' parameters at the bound tests/test_hip_rollout.py holds the posterior mean to, on the exact-fp32 schedule; `valid`
    equal; rows with valid false hold exactly the reference's masked values; the planted agents as recorded."""
    dev = torch.device(DEV)
    E = import_module("trafficbots_amd.engine")
    wm = _wm(tb, tag).to(dev).eval()
    wm.schedule = E.DEFAULT.replace(dec_tail_mfma=False, tile_small=False, navi_rider=False)
    batch = LR.c1_batch(tb, golden["agent/valid"])
    with torch.no_grad(), E.use(wm.schedule):
        _, _, _, post, prior = _eval_dists(tb, wm, batch, dev)
    learned = not wm.model.latent_encoder.latent_dist_prior.skip_forward
    for side, d in (("post", post), ("prior", prior)):
        valid = _T(golden[f"{tag}/{side}_valid"])
        assert torch.equal(d.valid.cpu(), valid), side
        for k, v in _params(d).items():
            ref = _T(golden[f"{tag}/{side}_{k}"])
            print(f"[{tag} {side} {k}] max |d| {float((v.cpu() - ref).abs().max()):.3g} of max |ref| {float(ref.abs().max()):.3g}")
            torch.testing.assert_close(v.cpu(), ref, rtol=2e-3, atol=2e-4)
            assert torch.equal(v.cpu()[~valid], ref[~valid]), (side, k)  # the masked rows: exactly the reference's fill
        s = d.sample(True)
        if tag in LR.CATEGORICAL:  # (a one-hot: equal unless two logits of the reference lie within the tolerance of each other)
            lg = _T(golden[f"{tag}/{side}_logits"])
            top2 = lg.topk(2, -1).values
            clear = ((top2[..., 0] - top2[..., 1]) > 2 * (2e-3 * lg.abs().max() + 2e-4)).all(-1)
            clear |= (d.logits.cpu() == lg).flatten(-2, -1).all(-1)  # (... or the logits are the reference's to the bit: the fixed prior's zeros)
            assert torch.equal(s.cpu()[clear], _T(golden[f"{tag}/{side}_det_sample"])[clear]) and bool(clear.any())
        else:
            torch.testing.assert_close(s.cpu(), _T(golden[f"{tag}/{side}_det_sample"]), rtol=2e-3, atol=2e-4)
            torch.testing.assert_close(d.log_prob(s).cpu(), _T(golden[f"{tag}/{side}_det_log_prob"]), rtol=2e-3, atol=2e-4)
    assert bool(post.valid[0, LR.AG_BETWEEN]) and bool(post.valid[0, LR.AG_FUTURE])
    assert bool(prior.valid[0, LR.AG_BETWEEN]) == (not learned) and not bool(prior.valid[0, LR.AG_FUTURE])


HEADS = {"gaus_ln_learned_std": dict(dist_type="diag_gaus", branch_type=False, mlp_use_layernorm=True, log_std=None),
         "gaus_learned_std": dict(dist_type="diag_gaus", branch_type=False, mlp_use_layernorm=False, log_std=None),
         "cat_ln": dict(dist_type="cat", branch_type=False, mlp_use_layernorm=True, log_std=0.0),
         "gaus_branch_fixed_std": dict(dist_type="diag_gaus", branch_type=True, mlp_use_layernorm=False, log_std=-0.5),
         "cat_branch_ln": dict(dist_type="cat", branch_type=True, mlp_use_layernorm=True, log_std=0.0)}


@pytest.mark.parametrize("name", list(HEADS))
def test_heads_on_the_device_equal_the_torch_form(tb, name):
    """The heads the fixtures do not reach in eval mode on the device - un-branched with LayerNorm or with an `mlp_log_std` head
    (MLP.forward + row mask), branched without LayerNorm and with the log_std list - against the same module's torch form on the CPU
    (train_graph.dist_head), on 2 x 37 agents (five 16-row tiles, the last one partial) with invalid rows of every type. Bound: the
    eval comparison's rtol 2e-3, atol 2e-4 (exact-fp32 products against the CPU's); masked rows exactly equal."""
    LE = import_module("trafficbots_amd.models.latent_encoder")
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 37, 128, generator=g)
    valid = torch.rand(2, 37, generator=g) > 0.25
    ag_type = torch.nn.functional.one_hot(torch.randint(0, 3, (2, 37), generator=g), 3).bool()
    torch.manual_seed(4)
    de = LE.DistEncoder(128, 16, n_cat=4, n_layer=3, **HEADS[name]).eval()
    with torch.no_grad():
        for q in de.parameters():
            if q.dim() == 1:
                q.add_(0.1 * torch.randn(q.shape, generator=g))
        want = de(x, valid, ag_type)
        got = de.to(dev)(x.to(dev), valid.to(dev), ag_type.to(dev))
    assert torch.equal(got.valid.cpu(), valid) and not bool(valid.all())
    for (k, a), b in zip(_params(got).items(), _params(want).values()):
        print(f"[{name} {k}] max |d| {float((a.cpu() - b).abs().max()):.3g} of max |ref| {float(b.abs().max()):.3g}")
        torch.testing.assert_close(a.cpu(), b.expand_as(a), rtol=2e-3, atol=2e-4)
        assert torch.equal(a.cpu()[~valid], b.expand_as(a)[~valid]), k


@pytest.mark.parametrize("tag", ["prior_gaus", "cat_cat"])
def test_joint_future_pred_on_a_learned_prior(tb, golden, tag):
    """K = 4 futures of 12 steps from the learned prior: rollout 0 under joint_future_pred_deterministic_k0 carries the deterministic
    sample, the same seed gives the same bits, another seed another latent."""
    dev = torch.device(DEV)
    wm = _wm(tb, tag, joint_future_pred_deterministic_k0=True, time_step_end=12).to(dev).eval()
    batch = LR.c1_batch(tb, golden["agent/valid"])
    seen = []
    real = wm.rollout
    wm.rollout = lambda ag_tokens, *a, **k: (seen.append(ag_tokens["ag_latent"].clone()), real(ag_tokens, *a, **k))[1]

    def run(seed):
        with torch.no_grad():
            bd, mp, tl, _, prior = _eval_dists(tb, wm, batch, dev)
            det = prior.sample(True).clone()
            navi = wm.model.navi_predictor(ag_valid=bd["sc/ag_valid"], ag_attr=bd["sc/ag_attr"], ag_motion=bd["sc/ag_motion"], ag_pose=bd["sc/ag_pose"],
                                           ag_type=bd["ref/ag_type"], **mp)
            torch.manual_seed(seed)
            buf = wm.joint_future_pred(batch=bd, mp_tokens=mp, tl_tokens=tl, ag_latent_dist=prior, ag_navi_dist=navi,
                                       teacher_forcing=wm.teacher_forcing_joint_future_pred, n_joint_future=4)
        return det, seen[-1], buf

    det, z_a, buf_a = run(3)
    _, z_b, buf_b = run(3)
    _, z_c, buf_c = run(4)
    assert z_a.shape == (4, 8, 16) and torch.equal(z_a[0], det[0])
    assert not torch.equal(z_a[1], det[0])
    assert torch.equal(z_a, z_b) and torch.equal(buf_a.pred_pose, buf_b.pred_pose) and torch.equal(buf_a.log_prob, buf_b.log_prob)
    assert not torch.equal(z_a, z_c) and torch.equal(z_c[0], det[0])
    assert buf_a.pred_pose.shape[:3] == (1, 4, 8) and bool(torch.isfinite(buf_a.log_prob).all())
    if tag in LR.CATEGORICAL:
        assert bool((z_a.view(4, 8, LR.N_CAT, -1).sum(-1) == 1).all()) and bool(((z_a == 0) | (z_a == 1)).all())


@pytest.mark.parametrize("tag", ["prior_gaus", "cat_cat"])
def test_validation_step_takes_the_distributions(tb, golden, tag):
    """One validation batch: val/loss is finite, is the sum of its logged terms, and its KL term is the balanced KL of the fixture's
    distributions over the KL-valid agents. Bound of the KL term: 1e-2 relative - the parameters are held to 2e-3 of the reference's, a
    KL is quadratic in the mean differences (twice the relative error) and two sides enter."""
    dev = torch.device(DEV)
    wm = _wm(tb, tag, n_joint_future_wosac=2).to(dev).eval()
    raw = LR.c1_batch(tb, golden["agent/valid"])
    batch = {**raw, **tb.synthetic.to_history_batch(raw), **tb.synthetic.make_wosac_keys(1, 8, seed=0)}
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    captured = []
    real = wm.reactive_replay
    wm.reactive_replay = lambda *a, **k: (captured.append(real(*a, **k)), captured[-1])[1]
    torch.manual_seed(0)
    wm.validation_step(batch, 0)
    wm.validation_epoch_end([None])
    lg = {k: float(v) for k, v in wm.logged.items()}
    assert np.isfinite(lg["val/loss"]) and lg["val/loss"] == lg["reactive_replay/loss"]
    parts = lg["reactive_replay/vae_kl"] - lg["reactive_replay/diffbar_reward"] + lg["reactive_replay/navi_loss"] + lg["reactive_replay/tl_state_loss"]
    assert abs(lg["val/loss"] - parts) <= 1e-5 * max(abs(parts), 1.0)
    lv = captured[0].pred_valid[:, 0].clone()
    lv[:, :, :10] = False
    kv = _T(golden[f"{tag}/post_valid"]) & lv.any(-1).cpu()
    want = float(_T(golden[f"{tag}/kl64_a0.2_f1.0"])[kv].sum() / kv.sum())
    print(f"[validation_step, {tag}] val/loss {lg['val/loss']:.6g}, vae_kl {lg['reactive_replay/vae_kl']:.6g} (fixture's distributions {want:.6g}, {int(kv.sum())} agents)")
    assert int(kv.sum()) >= 4 and abs(lg["reactive_replay/vae_kl"] - want) <= 1e-2 * want


# --------------------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("tag,p", LR.TRAIN_RUNS)
def test_training_step_vs_reference(tb, golden_train, tag, p):
    """test_hip_il_loss.py::test_training_step_vs_reference's procedure on every recorded run: fp32 class, TRAIN_TOL["fp32"], loss terms,
    per-module gradient norms, the six spot blocks and the two in the prior encoder and the prior head. The categorical runs are handed
    the recorded uniform noise."""
    dev = torch.device(DEV)
    g, key = golden_train, f"{tag}_p{p}"
    wm = _wm(tb, tag, free_nats=float(g[f"{key}/kl_free_nats"]), p_training_rollout_prior=float(p)).to(dev).train()
    wm.train_precision = "fp32"
    tol = TRAIN_TOL["fp32"]
    batch = LR.c1_batch(tb, g[f"{key}/agent/valid"])
    noise = _T(g[f"{key}/u"]).to(dev) if tag in LR.CATEGORICAL else None
    torch.manual_seed(7)
    loss = wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0, noise=noise)
    loss.backward()
    keys = ("loss", "vae_kl", "diffbar_reward", "navi_loss", "tl_state_loss")
    gn = {}
    for k, q in wm.model.named_parameters():
        if q.grad is not None:
            gn[k.split(".")[0]] = gn.get(k.split(".")[0], 0.0) + float(q.grad.double().pow(2).sum())
    spots = [x.split("/", 1)[1] for x in g.files if x.startswith(f"{key}/dgrad_")]
    grad = lambda name: wm.model.get_parameter(name).grad[:8, :16].cpu()  # (by path: shared encoders are listed once)
    meas = {"loss": max(abs(float(wm.last_metrics[k].detach()) - float(g[f"{key}/dtrain_{k}"])) / max(abs(float(g[f"{key}/dtrain_{k}"])), 1e-1) for k in keys),
            "gnorm": max(abs(v ** 0.5 - float(g[f"{key}/dgradnorm_{top}"])) / max(float(g[f"{key}/dgradnorm_{top}"]), 1e-6) for top, v in gn.items()),
            "spot": max(float((grad(k[6:]) - _T(g[f"{key}/{k}"])).abs().max()) / max(float(np.abs(g[f"{key}/{k}"]).max()), 1e-12) for k in spots)}
    print(f"[training step, {key}] loss {float(loss.detach()):.6g} (reference {float(g[f'{key}/dtrain_loss']):.6g}), vae_kl {float(wm.last_metrics['vae_kl']):.6g} "
          f"({float(g[f'{key}/dtrain_vae_kl']):.6g}); loss terms max rel diff {meas['loss']:.3g}, gradient norms {meas['gnorm']:.3g}, spot blocks max |d| / max |ref| {meas['spot']:.3g}")
    for k in keys:
        torch.testing.assert_close(wm.last_metrics[k].detach().cpu().float(), _T(g[f"{key}/dtrain_{k}"]).float(), rtol=tol["loss"], atol=1e-1 * tol["loss"])
    assert len(gn) >= 6 and len(spots) == 8 and f"dgrad_{LR.SPOT_PRIOR_ENC}" in spots and f"dgrad_{LR.prior_head_spot(tag)}" in spots
    assert {top for top in gn} == {x.split("dgradnorm_")[1] for x in g.files if x.startswith(f"{key}/dgradnorm_")}
    for top, v in gn.items():
        ref = float(g[f"{key}/dgradnorm_{top}"])
        assert abs(v ** 0.5 - ref) <= tol["gnorm"] * max(ref, 1e-6), (top, v ** 0.5, ref)
    for k in spots:
        ref = _T(g[f"{key}/{k}"])
        torch.testing.assert_close(grad(k[6:]), ref, rtol=tol["spot_rtol"], atol=1e-5 + tol["spot_atol_rel"] * float(ref.abs().max()))
    # every prior-side parameter took part
    assert all(q.grad is not None for k, q in wm.model.named_parameters() if ("_encoder_prior." in k or ".latent_dist_prior." in k) and q.requires_grad)


def _noise(wm, n, A, dev, seed=5):
    le = wm.model.latent_encoder
    g = torch.Generator().manual_seed(seed)
    if le.categorical:
        return torch.rand(n, A, le.latent_dist_post.n_cat, le.latent_dist_post.n_class, generator=g).clamp_(min=1e-30).to(dev)
    return torch.randn(n, A, le.out_dim, generator=g).to(dev)


@pytest.mark.parametrize("tag", ["prior_gaus", "cat_cat"])
def test_fused_chain_equals_the_torch_schedules(tb, tag):
    """Fused chain + time-batched against fused_train_chain = False and time_batched_training = False, 2 scenes of 30 steps, rolled out
    from the prior: the metrics and bounds of test_hip_il_loss.py::test_fused_chain_equals_the_torch_schedules."""
    dev = torch.device(DEV)
    wm = _wm(tb, tag, p_training_rollout_prior=0.0, time_step_end=30).to(dev).train()
    wm.attn_dropout_seed = torch.tensor([4242], dtype=torch.int64, device=dev)
    batch = {k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=1).items()}
    noise = _noise(wm, 2, 8, dev)
    use_prior = torch.ones((), dtype=torch.bool, device=dev)
    res = {}
    for mode, (batched, fused) in {"fused": (True, True), "torch_chain": (True, False), "stepwise": (False, True)}.items():
        wm.time_batched_training, wm.fused_train_chain = batched, fused
        wm.zero_grad(set_to_none=True)
        loss = wm.training_step({k: v.clone() for k, v in batch.items()}, 0, noise=noise, use_prior=use_prior)
        loss.backward()
        res[mode] = ({k: float(v.detach()) for k, v in wm.last_metrics.items()}, {k: q.grad.clone() for k, q in wm.model.named_parameters() if q.grad is not None})
    assert any("_encoder_prior." in k for k in res["fused"][1])
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


@pytest.mark.parametrize("tag", ["prior_gaus", "cat_cat"])
def test_graphed_train_step_with_a_learned_prior(tb, tag):
    """GraphedTrainStep for prior_gaus and for the categorical family (whose distributions must be built without a host read): after one optimizer step the replayed loss and gradients are the eager step's on the current
    weights (the bounds of test_hip_il_loss.py::test_graphed_train_step_equals_eager); the prior encoders' parameters are among the
    live ones, in the flat buffer and in FlatAdamW's main group; `use_prior`, toggled between two replays, changes the loss."""
    dev = torch.device(DEV)
    DP = import_module("trafficbots_amd.pl_modules.data_parallel")
    torch.manual_seed(0)
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    scfg = tb.config.default_sim_cfg(time_step_end=30)
    scfg["teacher_forcing_training"]["prob_forcing_agent"] = 0.0
    scfg["pre_processing"]["scene_centric"]["dropout_p_history"] = -1.0
    wm = W.WaymoMotion(model=LR.model_cfg(tb, tag), data_size=tb.synthetic.DATA_SIZE, **scfg).to(dev).train()
    (opt,), _ = wm.configure_optimizers()
    batches = [{k: v.to(dev) for k, v in tb.synthetic.make_scene(2, 8, 64, 8, seed=s).items()} for s in (0, 2)]
    gs = DP.GraphedTrainStep(wm, opt, batches[0], warmup=1)
    names = {id(q): k for k, q in wm.model.named_parameters()}
    live = {names[id(q)] for q in gs.live}
    prior_side = {k for k, q in wm.model.named_parameters() if ("_encoder_prior." in k or ".latent_dist_prior." in k) and q.requires_grad}
    assert len(prior_side) > 200 and prior_side <= live
    assert len(gs.flat.params) == len(gs.live) and gs.flat_opt is not None
    # ... in the flat gradient buffer, in FlatAdamW's run of the main parameter group (group 0; navi_predictor is group 1), and among the
    # gradient-norm names
    index = {id(q): i for i, q in enumerate(gs.flat.params)}
    main = {id(q) for q in opt.param_groups[0]["params"]}
    runs = gs.flat_opt.runs
    for k in prior_side:
        q = wm.model.get_parameter(k)
        i = index[id(q)]
        assert id(q) in main and q.data_ptr() == gs.flat_opt.p.data_ptr() + 4 * gs.flat.offsets[i], k
        assert any(gi == 0 and a <= gs.flat.offsets[i] and gs.flat.offsets[i] + q.numel() <= b for gi, a, b, _ in runs), k
    norm_names = set(gs.flat.norm_plan(wm).names)
    assert {"model." + k for k in prior_side} <= norm_names and len(norm_names) == len(gs.live)
    gs(batches[0])  # replay + clip + AdamW: the weights move
    gs.opt, gs.clip = torch.optim.SGD(gs.live, lr=0.0), 0
    m = gs(batches[1])
    loss_g = float(m["loss"].detach())
    g1 = [g.clone() for g in gs.grads]
    for q in gs.live:
        q.grad = None
    loss = wm.training_step({k: v.clone() for k, v in batches[1].items()}, 0, noise=gs.noise, use_prior=gs.use_prior)
    loss.backward()
    close = lambda a, b, tol: float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-6)
    print(f"[graphed step, {tag}] replayed loss {loss_g:.6g}, eager {float(loss.detach()):.6g}")
    assert abs(float(loss.detach()) - loss_g) <= 1e-5 * abs(loss_g)
    for a, q in zip(g1, gs.live):
        assert close(a, q.grad, 1e-3), names[id(q)]
    # the choice of the rolled-out side is a device-side select inside the graph
    losses = []
    for flag in (False, True):
        gs.use_prior.fill_(flag)
        gs.graph.replay()
        losses.append(float(gs.metrics["loss"].detach()))
    assert losses[0] != losses[1], losses


def _count_library_calls(monkeypatch):
    """Every call into the main library goes through a module's `load()`: count them by entry point."""
    lib, calls = import_module("trafficbots_amd.abi").load(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)

            def call(*a):
                calls.append(name)
                return fn(*a)
            return call

    counting = Counting()
    for mod in ("hip_base", "hip_chain", "hip_rules", "hip", "hip_train"):
        monkeypatch.setattr(import_module("trafficbots_amd." + mod), "load", lambda: counting)
    return calls


def test_default_configuration_runs_no_prior_pass(tb, monkeypatch):
    """The default configuration's training step: the multiset of library calls equals that of a second module built the same way, the
    prior's distribution is the fixed one (skip_forward), no latent pass over the history is made and no prior encoder is entered."""
    dev = torch.device(DEV)
    TG = import_module("trafficbots_amd.train_graph")
    sides = []
    real_dist = TG.latent_dist
    monkeypatch.setattr(TG, "latent_dist", lambda *a, posterior=True, **k: (sides.append(posterior), real_dist(*a, posterior=posterior, **k))[1])
    calls = _count_library_calls(monkeypatch)
    counted = []
    batch = tb.synthetic.make_scene(1, 8, 64, 8, seed=0)
    for _ in range(2):
        wm = _wm(tb, None, time_step_end=20).to(dev).train()
        le = wm.model.latent_encoder
        assert le.latent_dist_prior.skip_forward and le.latent_dist_prior.dist_type == "std_gaus"
        entered = []
        for m in (le.tl_encoder_prior, le.ag_encoder_prior):
            m.register_forward_pre_hook(lambda *_: entered.append(1))
        wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0).backward()  # (un-counted: lazy initialisations, caches)
        calls.clear()
        torch.manual_seed(7)
        wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0).backward()
        counted.append(Counter(calls))
        assert not entered
    assert sides == [True] * 4, sides
    assert counted[0] == counted[1] and sum(counted[0].values()) > 100
    # ... and a learned prior does make the second pass, with more launches
    sides.clear()
    wm = _wm(tb, "prior_gaus", time_step_end=20).to(dev).train()
    wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0).backward()
    calls.clear()
    wm.training_step({k: v.to(dev) for k, v in batch.items()}, 0).backward()
    assert sides == [True, False] * 2
    assert sum(Counter(calls).values()) > sum(counted[0].values())
