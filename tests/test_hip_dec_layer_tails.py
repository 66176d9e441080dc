"""The one-launch decoder layer with its tail kind and its half as compile-time choices (csrc/dec_layer_mf.inc: one kernel
instantiation per tail - nothing, the next layer's projections, the lights' tail, the agents' heads - and, in a paired launch, one
inlined body per half): every kind as a PAIRED launch (tbx_knarpe_dec_layer_pair) against its two single launches
(tbx_knarpe_dec_layer), bit for bit, from the same descriptors (hip.defer). The heads also against the stand-alone heads launch."""
from importlib import import_module

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip(tb):
    h = import_module("trafficbots_amd.hip")
    h.load()
    return h


@pytest.fixture(scope="module")
def model(tb, dev):
    """The default model's heads and light tail (weights only: det_fill)."""
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg())
    tb.utils.det_fill(wm.model, 3)
    return wm.to(dev).eval().model


def _pair_xcd(na: int, nb: int) -> int:
    """tbx_knarpe_dec_layer_pair's default split of the 8 XCDs between the halves (0: the halves follow each other in block order)."""
    xa = (16 * na + (na + nb)) // (2 * (na + nb))
    xa = min(max(xa, 1), 7)
    return 0 if ((na + xa - 1) // xa > 32 or (nb + 7 - xa) // (8 - xa) > 32) else xa


class _Half:
    """One row set of a paired launch: a 2-layer dec_cross_attn block on n x S rows (self K-nearest Ks, cross T / K), layer 0's
    projections made ahead, so that run_block issues tbx_knarpe_dec_layer launches only (layer 0: next-layer projections, layer 1: `tails`)."""

    def __init__(self, tb, hip, eng, dev, seed, n, S, Ks, T, K, bf16):
        M = import_module("trafficbots_amd.models.modules.transformer_rpe")
        g = torch.Generator().manual_seed(seed)
        self.hip, self.eng, self.n, self.S, self.rows = hip, eng, n, S, n * S
        self.blk = M.TransformerBlockRPE(n_layer=2, mode="dec_cross_attn", d_rpe=128, d_model=128, n_head=4, k_feedforward=4, dropout_p=0.1,
                                         bias=True, activation="relu", out_layernorm=False, apply_q_rpe=False)
        tb.utils.det_fill(self.blk, seed)
        self.blk = self.blk.to(dev).eval()
        rows = self.rows
        self.x0 = torch.randn(rows, D, generator=g).to(dev)
        inv = torch.rand(rows, generator=g) < 0.2
        inv[0] = False
        self.src_invalid = inv.to(torch.uint8).to(dev)
        self.x0[inv.to(dev)] = 0.0

        def knn(T_, K_):
            rel = torch.cat([(torch.rand(n, S, K_, 2, generator=g) - 0.5) * 100, (torch.rand(n, S, K_, 1, generator=g) - 0.5) * 6], -1)
            idx = torch.randint(0, T_, (n, S, K_), generator=g).to(torch.int32).to(dev)
            m = (torch.rand(n, S, K_, generator=g) < 0.3).to(torch.uint8).to(dev)
            m[self.src_invalid.view(n, S).bool()] = 1  # an invalid source has no valid pair (as the K-nearest kernel produces)
            return idx, m, rel.to(dev).contiguous()

        self.self_knn = knn(S, Ks)
        self.cross_knn = knn(T, K)
        kv = torch.randn(n * T, 2 * 256, generator=g).to(dev)
        self.kv = kv.to(torch.bfloat16) if bf16 else kv
        self.T = T
        self.x = self.x0.clone()
        # layer 0's q | k | v | W_k^T q (the launch that produces x makes them in the closed loop)
        self.qkv = torch.empty(rows, eng.QKV_LD, device=dev)
        self.kv16 = torch.empty(rows, 2 * D, dtype=torch.bfloat16, device=dev) if bf16 else None
        l0 = self.blk.layers[0]
        hip.layer_tile(self.x, proj=eng.tile_proj_part(l0.norm_src, l0.attn_src, self.qkv, True, self.kv16), store_x=False)

    def run(self, pe, heads=None, lights=None):
        """run_block on the current x (launches, or - inside hip.defer() - appends its launch descriptors)."""
        i0, m0, r0 = self.self_knn
        ic, mc, rc = self.cross_knn
        self.eng.run_block(self.blk, self.x, self.src_invalid, self.n, self.S, self.eng.SelfKnn(i0, m0, rel=r0),
                           cross=lambda l: [self.hip.Seg(self.kv, l * 256, l * 256 + D, self.T, ic, mc, None, 1, rel=rc)], pose_rpe=pe,
                           first_proj=dict(qkv=self.qkv, kv16=self.kv16), heads_tail=heads, tail_mf=lights)


def _heads(hip, model, g, rows, dev):
    """tbx_heads_tail_t fields on the default model's adders / action head: one row of each agent type, one without a type (action
    exactly 0), one with two type bits (two trips of the branch loop), the rest random."""
    navi_emb, lat_emb = torch.relu(torch.randn(rows, D, generator=g)).to(dev), torch.relu(torch.randn(rows, D, generator=g)).to(dev)
    navi_valid = (torch.rand(rows, generator=g) < 0.8).to(torch.uint8).to(dev)
    lat_inv = (torch.rand(rows, generator=g) < 0.2).to(torch.uint8).to(dev)
    navi_emb[navi_valid == 0] = 0.0
    lat_emb[lat_inv != 0] = 0.0
    ty = torch.randint(0, 4, (rows,), generator=g)  # 3: no type
    ty[:5] = torch.tensor([0, 1, 2, 3, 0])
    type_mask = torch.stack([(ty != i) for i in range(3)]).to(torch.uint8)
    type_mask[2, 4] = 0  # row 4: branches 0 and 2
    pw = lambda w, b, **kw: hip.packed_weight(w, b, mfma32=True, **kw)
    lins = [[t[0] for t in mlp.linear_layers()] for mlp in model.action_head.mlp_mean]
    w1, b1 = hip.stacked_linear([l[0] for l in lins])
    w2, b2 = hip.stacked_linear([l[1] for l in lins])
    w3, b3 = hip.stacked_linear([l[2] for l in lins], pad_out_to=16)
    imgs = [pw(t[0].weight, t[0].bias) for t in model.add_navi.mlp.linear_layers()] + [pw(t[0].weight, t[0].bias) for t in model.add_latent.mlp.linear_layers()]
    imgs += [pw(w1, b1), pw(w2, b2, groups=3), pw(w3, b3, groups=3)]
    return dict(images=imgs, navi_emb=navi_emb, latent_emb=lat_emb, navi_valid=navi_valid, latent_invalid=lat_inv,
                type_mask=type_mask.contiguous().to(dev), action_out=torch.full((rows, 2), 7.0, device=dev)), ty


def _lights(hip, model, g, rows, bf16, dev):
    """tbx_tl_tail_t fields on the default model's K/V projections of the agents' 4 layers and its next-state predictor."""
    layers = model.ag_encoder.tl_kv_layers()
    lins = [t[0] for t in model.tl_state_predictor.mlp.linear_layers()]
    assert len(layers) == 4 and len(lins) == 3
    pw = lambda w, b: hip.packed_weight(w, b, mfma32=True)
    w3, b3 = hip.stacked_linear([lins[2]], pad_out_to=16)
    inv = (torch.rand(rows, generator=g) < 0.3).to(torch.uint8).to(dev)
    return dict(kv_images=[pw(at.in_proj_weight[D:], at.in_proj_bias[D:]) for _, at in layers], norms=[(nm.weight, nm.bias, nm.eps) for nm, _ in layers],
                kv_out=torch.full((rows, 8 * D), 7.0, device=dev).to(torch.bfloat16 if bf16 else torch.float32),
                mlp_images=[pw(lins[0].weight, lins[0].bias), pw(lins[1].weight, lins[1].bias), pw(w3, b3)], tl_invalid=inv,
                logits_out=torch.full((rows, 5), 7.0, device=dev), clamp=(-3.0, 3.0), sim=None)


# lights per scene: 5 and 13 rows -> the halves on disjoint XCDs (xcd_a = 5 and 3) with surplus blocks in both halves' slots and row counts
# (10, 26) that are no multiple of 8; 120 -> a half with more rows than its XCDs have CUs: xcd_a = 0, the halves in block order
@pytest.mark.parametrize("L,bf16", [(5, False), (13, True), (120, False), (5, True)])
def test_every_tail_kind_paired_equals_its_two_single_launches(tb, hip, dev, model, L, bf16):
    """Agents 2 x 8 rows (Ks 4) with lights 2 x L rows, cross T 64 / K 8, both 2-layer blocks: layer 0 has the next layer's projections
    as its tail, layer 1 nothing or the agents' heads / the lights' tail (fp32 and bf16 tables). Every launch as a pair
    (tbx_knarpe_dec_layer_pair: the half and both tails resolved at compile time) writes what its two single launches write, bit for
    bit; a pair of kinds no caller launches is refused, not misrun; the heads inside the launch equal the stand-alone heads launch
    (tbx_heads_tile on the rows the layer stored: the same split-bf16 stages in the same summation order, as 16-row tiles) bit for
    bit, and a row without an agent type gets action exactly 0."""
    eng = import_module("trafficbots_amd.engine")
    P = import_module("trafficbots_amd.utils.pose_emb")
    pe = P.PoseEmb("pe_xy_yaw", pe_dim=128, theta_xy=1e3).to(dev)
    g = torch.Generator().manual_seed(100 + L)
    na, nb = 2 * 8, 2 * L
    assert (_pair_xcd(na, nb) == 0) == (L == 120)
    if L != 120:  # surplus blocks: the grid is 8 x the larger half's slots
        xa = _pair_xcd(na, nb)
        assert 8 * max((na + xa - 1) // xa, (nb + 7 - xa) // (8 - xa)) > na + nb and nb % 8 != 0
    sched = eng.DEFAULT.replace(live_rows=1, attn_fold=True, dec_mid=True, dec_layer=True, kv_bf16=bf16, split_bf16=False, dec_tail_mfma=True)
    with eng.use(sched):
        ag = _Half(tb, hip, eng, dev, 21, 2, 8, 4, 64, 8, bf16)
        tl = _Half(tb, hip, eng, dev, 22, 2, L, min(4, L - 1), 64, 8, bf16)
        hd, ty = _heads(hip, model, g, na, dev)
        lt = _lights(hip, model, g, nb, bf16, dev)
        outs = {}
        for tails in (False, True):
            kw_a, kw_l = (dict(heads=hd), dict(lights=lt)) if tails else ({}, {})
            watch = dict(x_a=ag.x, x_l=tl.x, action=hd["action_out"], kv=lt["kv_out"], logits=lt["logits_out"])

            def reset():
                ag.x.copy_(ag.x0), tl.x.copy_(tl.x0)
                hd["action_out"].fill_(7.0), lt["kv_out"].fill_(7.0), lt["logits_out"].fill_(7.0)

            reset()
            ag.run(pe, **kw_a), tl.run(pe, **kw_l)  # single launches (and every weight image packed)
            torch.cuda.synchronize()
            single = {k: v.clone() for k, v in watch.items()}
            reset()
            with hip.defer() as ca:
                ag.run(pe, **kw_a)
            with hip.defer() as cl:
                tl.run(pe, **kw_l)
            assert [c[0] for c in ca] == [c[0] for c in cl] == ["tbx_knarpe_dec_layer"] * 2
            for a_, l_ in zip(ca, cl):
                hip.launch_dec_layer_pair(a_, l_)
            torch.cuda.synchronize()
            for k, v in watch.items():
                assert torch.equal(v, single[k]), (tails, k, float((v.float() - single[k].float()).abs().max()))
            outs[tails] = single
            if tails:  # the agents' heads next to a half without a tail: no caller pairs these, and no kernel is instantiated for them
                with hip.defer() as plain:
                    tl.run(pe)
                with pytest.raises(RuntimeError):
                    hip.launch_dec_layer_pair(ca[1], plain[1])
    plain, full = outs[False], outs[True]
    assert torch.isfinite(full["x_a"]).all() and float((full["x_a"] - ag.x0).abs().max()) > 1e-3
    assert torch.equal(full["x_a"], plain["x_a"]) and torch.equal(full["x_l"], plain["x_l"])  # the tails leave the stored rows alone
    assert float(full["x_a"][ag.src_invalid.bool()].abs().max()) == 0.0
    # the lights' tail wrote every table row and every logit, clamped, invalid lights' logits 0; without it nothing is written
    assert float(plain["logits"].min()) == 7.0 and float(plain["action"].min()) == 7.0
    assert float(full["logits"].abs().max()) <= 3.0 and float(full["logits"][lt["tl_invalid"].bool()].abs().max()) == 0.0
    assert torch.isfinite(full["kv"].float()).all() and not bool((full["kv"].float() == 7.0).all(1).any())
    # the heads: against the stand-alone launch on the stored rows
    ref = torch.full((na, 2), 7.0, device=dev)
    with eng.use(sched):
        hip.heads_tile(plain["x_a"].clone(), dict(hd, action_out=ref))
    torch.cuda.synchronize()
    act = full["action"]
    none = (ty == 3).to(dev)
    none[4] = False
    assert bool(none[3]) and float(act[none].abs().max()) == 0.0 and float(ref[none].abs().max()) == 0.0
    assert float(ref.abs().max()) > 1e-3 and torch.equal(act, ref), float((act - ref).abs().max())
    assert float(act[4].abs().max()) > 0.0 and float(act[:3].abs().min()) > 0.0


@pytest.mark.parametrize("sizes", [(16, 64, 13), (8, 64, 5)])
def test_fused_tails_paired_equal_the_two_stream_step(tb, sizes):
    """The last layers' tails WITH their steps in the launch (the agents' fused step tail, the lights' own step: tbx_heads_tail_t /
    tbx_tl_tail_t sim_state) as the paired launch of the one-queue closed-loop step against the two-stream step's single launches, at
    light counts that are no multiple of 8: the rollout log over teacher-forced and free steps does not differ by a bit."""
    from test_hip_rollout import _setup

    dev = torch.device("cuda:0")
    wm, P, b, bd = _setup(tb, dev, sizes, 4)
    E = import_module("trafficbots_amd.engine")
    mp, tl = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")
    z = torch.randn(1, sizes[0], 16, generator=torch.Generator().manual_seed(6)).to(dev)
    valid = bd["gt/ag_valid"].any(-1)
    outs = {}
    for one in (False, True):
        wm.schedule = E.DEFAULT.replace(one_queue=one)
        outs[one] = wm.reactive_replay(bd, mp, tl, z, valid, bd["gt/ag_navi"], valid, wm.teacher_forcing_joint_future_pred, True, step_end=16,
                                       use_graph=False)
        assert wm._engine.one_queue == one
    ref, o = outs[False], outs[True]
    for name in ("pred_pose", "pred_valid", "pred_motion", "action_log_prob"):
        assert torch.equal(getattr(o, name), getattr(ref, name)), name
    for name in ("action", "tl_state"):
        assert torch.equal(o.vis_dict[name], ref.vis_dict[name]), name


def test_fused_tail_heads_on_crafted_type_masks(tb, hip):
    """The heads WITH the fused step tail (the separately compiled bodies: tbx_heads_tail_t.sim_state) on type masks a scene never has:
    before each of three steps of a restored engine the first rows' masks are overwritten - all three branches (three trips of the
    branch loop), branches 0 and 1, none, branches 0 and 2 (the next branch is not the following one) - behind the preparation that
    the previous launch's tail ran. The fused PAIRED launches of the one-queue step against the fused SINGLE launches of the two-stream
    step over the three steps, and the first step against the heads without the step behind them plus the stand-alone tbx_sim_step
    (that launch's heads are compared with the stand-alone heads launch above): actions and the agents' windows bit for bit, the row
    without a type gets action exactly 0 with the step behind it, and the crafted rows really are sums of several branches."""
    from test_hip_rollout import _setup

    dev = torch.device("cuda:0")
    sizes = (16, 64, 13)
    wm, P, b, bd = _setup(tb, dev, sizes, 4)
    E = import_module("trafficbots_amd.engine")
    mp, tl = wm.encode_scene(bd, tl_valid_key="gt/tl_valid")
    z = torch.randn(1, sizes[0], 16, generator=torch.Generator().manual_seed(6)).to(dev)
    valid = bd["gt/ag_valid"].any(-1)
    names = ("hist_pose", "hist_motion", "hist_valid")

    def craft(eng):
        tm = eng.policy_out["prep"]["type_mask"]
        tm[:, 0] = 0  # all three branches
        tm[:2, 1], tm[2, 1] = 0, 1  # branches 0 and 1
        tm[:, 2] = 1  # none
        tm[0, 3], tm[1, 3], tm[2, 3] = 0, 1, 0  # branches 0 and 2

    def snap(eng):
        torch.cuda.synchronize()
        return [eng.policy_out["action_mean"].clone()] + [eng.S[k].clone() for k in names]

    logs, plain = {}, {}
    for one in (False, True):
        wm.schedule = E.DEFAULT.replace(one_queue=one)
        wm.reactive_replay(bd, mp, tl, z, valid, bd["gt/ag_navi"], valid, wm.teacher_forcing_joint_future_pred, True, step_end=4, use_graph=False)
        eng = wm._engine
        assert eng.one_queue == one
        for crafted in (True, False):
            eng.restore()
            assert eng._prep_ready  # (the first step's preparation ran: the heads take the masks as they stand)
            log = []
            for _ in range(3):
                if crafted:
                    craft(eng)
                eng.step()
                assert eng.policy_out["prep"].get("_tail_fused")
                log.append(snap(eng))
            (logs if crafted else plain)[one] = log
    for s in range(3):
        for x, y in zip(logs[True][s], logs[False][s]):
            assert torch.equal(x, y), s
    act, act_plain = logs[True][0][0], plain[True][0][0]
    assert float(act[2].abs().max()) == 0.0 and float(act_plain.abs().max()) > 1e-2
    for r in (0, 1, 3):  # several branches: not the one-hot row's action
        assert float((act[r] - act_plain[r]).abs().max()) > 1e-4, r
    assert torch.equal(act[4:], act_plain[4:])  # the ordinary rows do not see the crafted ones
    # the first step once more on the two-stream engine's state: heads in the launch, the agents' step as a launch of its own
    wm.schedule = E.DEFAULT.replace(one_queue=False)
    wm.reactive_replay(bd, mp, tl, z, valid, bd["gt/ag_navi"], valid, wm.teacher_forcing_joint_future_pred, True, step_end=4, use_graph=False)
    eng = wm._engine
    eng.restore()
    craft(eng)
    S = eng.S
    with E.use(eng.sched):
        wm.model.agent_policy(S["hist_valid"], S["hist_pose"], S["hist_motion"], eng.ag_attr6, S["ag_type_idx"], eng.ag_latent, eng.latent_invalid,
                              eng.dest, S["navi_valid"], eng.tl_tokens, eng.mp_tokens, eng.tl_kv[0], eng.policy_out, rollout_consts=eng.consts,
                              prep_ready=True)
        assert not eng.policy_out["prep"].get("_tail_fused")
        hip.sim_step(eng.sim_state, hip.SIM_AGENTS | hip.SIM_ADVANCE)
    for x, y in zip(snap(eng), logs[False][0]):
        assert torch.equal(x, y)
