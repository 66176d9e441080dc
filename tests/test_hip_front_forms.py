"""tbx_front / tbx_front_pair (csrc/front.hip) form by form, bit for bit (torch.equal everywhere).

The front kernels resolve the half, the block kind and the search job once, from the head of their argument block, and branch into one
inlined body per form: window + projection ("cat" 64 / "add" 128), rider, one body per search job and per candidates-per-lane count
(n_tgt <= 128, <= 1024, and - only in the kernels picked when a job needs it - above), pose embedding. The oracle for every form is
the launch the front replaced, which takes its arguments the plain way (one struct, no dispatch): tbx_window_tile -> tbx_layer_tile
(first projection + rider) and tbx_knn_embed_multi; the paired launch is compared with its two tbx_front halves. That oracle is NOT
independent in its values: those launches instantiate the same window_body, rider_tile and knn_rows templates (clamped early loads,
the one-clause search), so a mistake in the shared bodies shows on both sides alike. What this file checks is the dispatch and the
argument groups - the right body on the right arguments for every form; the values themselves rest on the torch- and chain-referenced
tests of tests/test_hip_parity.py (test_window_tile_equals_grouped_chain, test_window_tile_add_mode_equals_grouped_chain,
test_knn_embed, the rider's chain test), which run the same bodies, and on the benchmark's outputs being byte-equal to the parent's
(profiles/front_args_bench_ab.txt); the ragged ends - odd window counts, window length 1, a 17-row rider - are also compared
with tbx_rowchain programs here (test_ragged_windows_against_the_row_chain, test_rider_17_rows_against_the_row_chain). The shapes sit on
both sides of every threshold a body is chosen by, and on the ragged ends: an odd window count (the last workgroup's second row is
empty), window lengths 1 / 11 / 16, windows without a valid step, 4 and 32 attribute columns, 0 / 1 / 16 / 17 rider rows from poses
and from rows, n_tgt 3 .. 1025 with k 1 .. 64, an invalid source row, a job whose targets are all invalid, lattice poses (ties),
tgt_batch_div 1 and 2, 1 to 4 jobs with and without the pose-embedding job, a paired launch above 256 workgroups and with either half
without searches. Argument errors return what they returned before the argument block was regrouped (-1 ARG, -2 UNSUPPORTED)."""
import ctypes as C
from importlib import import_module

import pytest
import torch

from oracle import hptr_ops as H

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
def ctx(tb, hip, dev):
    """The weights every case shares: the default model's two window encoders, one first-projection layer, one rider MLP."""
    W = import_module("trafficbots_amd.pl_modules.waymo_motion")
    M = import_module("trafficbots_amd.models.modules.transformer_rpe")
    wm = W.WaymoMotion(model=tb.config.default_model_cfg(), data_size=tb.synthetic.DATA_SIZE, **tb.config.default_sim_cfg())
    tb.utils.det_fill(wm.model, 3)
    wm = wm.to(dev).eval()
    blk = M.TransformerBlockRPE(n_layer=1, mode="enc_self_attn", d_rpe=128, d_model=128, n_head=4, k_feedforward=4, dropout_p=0.0,
                                bias=True, activation="relu", out_layernorm=False, apply_q_rpe=False)
    tb.utils.det_fill(blk, 6)
    g = torch.Generator().manual_seed(11)
    Ws = [(torch.randn(D, D, generator=g) / 8).to(dev) for _ in range(4)]
    bs = [torch.randn(D, generator=g).to(dev) for _ in range(4)]
    return dict(eng=import_module("trafficbots_amd.engine"), l0=blk.to(dev).eval().layers[0], model=wm.model, rider_wb=(Ws, bs),
                imgs={False: wm.model.ag_encoder._window_tile_images(32), True: wm.model.tl_encoder._window_tile_images()},
                rider_images=[hip.packed_weight(w, b, mfma32=True) for w, b in zip(Ws, bs)],
                fxy=H.make_freqs_xy(32, 1e3).to(dev), fyw=H.make_freqs_rad(64).to(dev))


def _poses(g, n, S, lattice=False):
    if lattice:  # (every distance exact in fp32, many of them equal: the ties' order is the kernels' own rule)
        return torch.cat([torch.randint(-6, 6, (n, S, 2), generator=g).float() * 0.25, torch.zeros(n, S, 1)], -1)
    return torch.cat([(torch.rand(n, S, 2, generator=g) - 0.5) * 200, (torch.rand(n, S, 1, generator=g) - 0.5) * 6], -1)


class Half:
    """The inputs of one tbx_front call and its three un-fused launches. searches: (n_tgt, k) per job; all_inv: index of the job whose
    targets are all invalid; pose_job: the searches' pose-embedding job (only with searches)."""

    def __init__(self, ctx, dev, seed, G, W, add, attr_cols=32, rider_rows=0, rider_pose=True, searches=(), n=2, S=5, div=1, lattice=False,
                 all_inv=None, pose_job=False, kv16=False):
        g = torch.Generator().manual_seed(seed)
        self.ctx, self.dev, self.G, self.add, self.rider_rows, self.kv16 = ctx, dev, G, add, rider_rows, kv16
        attr = torch.randn(G * W, attr_cols, generator=g).to(dev)
        pe = torch.randn(G, D, generator=g).to(dev) if add else torch.randn(G * W, 64, generator=g).to(dev)
        inv = torch.rand(G, W, generator=g) < 0.3
        self.no_valid = 1 if G > 1 else None  # a window without a valid step (not the only one: the oracle must be seen to have run)
        if G > 1:
            inv[1] = True
        self.win = dict(attr=attr, pe=pe, row_invalid=inv.reshape(-1).to(torch.uint8).to(dev), in_images=ctx["imgs"][add][0],
                        pn_images=ctx["imgs"][add][1], window=W, add_mode=add)
        self.rider = None
        if rider_rows:
            self.rider = dict(add=torch.randn(rider_rows, D, generator=g).to(dev), valid=(torch.rand(rider_rows, generator=g) < 0.7).to(torch.uint8).to(dev),
                              images=ctx["rider_images"])
            if rider_pose:
                p3 = torch.cat([(torch.rand(rider_rows, 2, generator=g) - 0.5) * 300, (torch.rand(rider_rows, 1, generator=g) - 0.5) * 6], -1)
                self.rider.update(pose3=p3.to(dev).contiguous(), freqs=(ctx["fxy"], ctx["fyw"]))
            else:
                self.rider.update(inp=torch.randn(rider_rows, D, generator=g).to(dev))
        self.jobs = []
        sp = _poses(g, n, S, lattice).to(dev).contiguous()
        si = torch.zeros(n, S, dtype=torch.uint8)
        si[0, S // 2] = 1  # an invalid source row
        for j, (T, k) in enumerate(searches):
            assert k < T
            tp = _poses(g, n // div, T, lattice).to(dev).contiguous()
            ti = (torch.rand(n // div, T, generator=g) < 0.2).to(torch.uint8)
            if j == all_inv:
                ti[:] = 1
            self.jobs.append(dict(src_pose=sp, src_invalid=si.to(dev), tgt_pose=tp, tgt_invalid=ti.to(dev), k=k, dist_limit=60.0 if j & 1 else 1e9,
                                  tgt_batch_div=div, want_rel_pose=True, want_emb=False))
        self.q3 = torch.randn(7, 3, generator=g).to(dev) if pose_job else None
        assert not pose_job or searches

    def outputs(self):
        dev, G = self.dev, self.G
        return dict(x=torch.full((G, D), 7.0, device=dev), qkv=torch.zeros(G, self.ctx["eng"].QKV_LD, device=dev),
                    kv16=torch.zeros(G, 256, dtype=torch.bfloat16, device=dev) if self.kv16 else None,
                    rider=torch.full((max(self.rider_rows, 1), D), 5.0, device=dev), pj=torch.full((7, D), 3.0, device=dev))

    def args(self, o):
        eng, l0 = self.ctx["eng"], self.ctx["l0"]
        return dict(window=dict(self.win, out=o["x"]), proj=eng.tile_proj_part(l0.norm1, l0.attn, o["qkv"], True, o["kv16"]),
                    rider=dict(self.rider, out=o["rider"]) if self.rider else None, jobs=[dict(q) for q in self.jobs] or None,
                    pose_embed_job=dict(pose3=self.q3, freqs_xy=self.ctx["fxy"], freqs_yaw=self.ctx["fyw"], pe_dim=128, out=o["pj"]) if self.q3 is not None else None)

    def unfused(self, hip):
        o = self.outputs()
        a = self.args(o)
        with self.ctx["eng"].use(self.ctx["eng"].DEFAULT):
            hip.window_tile(**a["window"])
            hip.layer_tile(o["x"], proj=a["proj"], store_x=False, rider=a["rider"])
            o["knn"] = hip.knn_embed_multi(a["jobs"], pose_embed_job=a["pose_embed_job"]) if a["jobs"] else []
        return o

    def fused(self, hip):
        o = self.outputs()
        with self.ctx["eng"].use(self.ctx["eng"].DEFAULT):
            o["knn"] = hip.front(**self.args(o))
        return o

    def deferred(self, hip):
        """-> (outputs, the ("tbx_front", Front, keep) entry of a deferred list: what launch_front_pair takes)"""
        o = self.outputs()
        with self.ctx["eng"].use(self.ctx["eng"].DEFAULT), hip.defer() as calls:
            o["knn"] = hip.front(**self.args(o))
        return o, calls[0]


def _same(a, b, what="", kv_fp32=True):
    """kv_fp32 = False: the fp32 k | v columns are left out (with the bfloat16 table tbx_layer_tile writes k | v there INSTEAD, the
    front there AS WELL - as it always has; the table itself and q, W_k^T q are compared)"""
    for k in ("x", "kv16", "rider", "pj"):
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (what, k)
    for lo, hi in ((0, D), (D, 3 * D), (3 * D, a["qkv"].shape[1])):
        if kv_fp32 or lo != D:
            assert torch.equal(a["qkv"][:, lo:hi], b["qkv"][:, lo:hi]), (what, "qkv", lo)
    assert len(a["knn"]) == len(b["knn"])
    for j, ((i0, m0, r0, _), (i1, m1, r1, _)) in enumerate(zip(a["knn"], b["knn"])):
        assert torch.equal(i0, i1) and torch.equal(m0, m1) and torch.equal(r0, r1), (what, "job", j)


def _check_half(hip, h):
    a, b = h.unfused(hip), h.fused(hip)
    torch.cuda.synchronize()
    assert float(a["x"].abs().max()) > 1e-3 and float(a["qkv"].abs().max()) > 0  # (the oracle ran)
    if h.no_valid is not None:
        assert float(a["x"][h.no_valid].abs().max()) == 0.0 and float(b["x"][h.no_valid].abs().max()) == 0.0
    _same(a, b, kv_fp32=not h.kv16)
    if h.kv16:  # the front's fp32 k | v columns next to the table: the same values before rounding
        assert torch.equal(b["qkv"][:, D:3 * D].to(torch.bfloat16), b["kv16"])
    for (idx, _, _, _), q in zip(b["knn"], h.jobs):
        assert int(idx.min()) >= 0 and int(idx.max()) < q["tgt_pose"].shape[1]
    return b


@pytest.mark.parametrize("G,W,add,attr_cols", [(1, 1, False, 4), (2, 11, False, 32), (3, 16, False, 4), (5, 11, False, 32), (5, 1, False, 32),
                                               (1, 11, True, 4), (2, 16, True, 32), (3, 1, True, 32), (5, 11, True, 4), (3, 16, True, 32)])
def test_window_forms(ctx, hip, dev, G, W, add, attr_cols):
    """Both window + projection bodies: 1 / 2 / 3 / 5 windows (odd counts: the last workgroup's second row is empty), window lengths
    1 / 11 / 16, a window without a valid step, 4 and 32 attribute columns; k | v also as the bfloat16 table."""
    _check_half(hip, Half(ctx, dev, 100 * G + W, G, W, add, attr_cols=attr_cols, kv16=(G & 1) == 1))


@pytest.mark.parametrize("rows,pose", [(1, True), (1, False), (16, True), (16, False), (17, True), (17, False)])
def test_rider_forms(ctx, hip, dev, rows, pose):
    """The rider body at 1, 16 and 17 rows (a full tile; a second tile of one row), from poses and from rows (0 rows: every window case)."""
    o = _check_half(hip, Half(ctx, dev, rows, 3, 11, False, rider_rows=rows, rider_pose=pose))
    assert float(o["rider"].abs().max()) > 0


@pytest.mark.parametrize("searches,div,lattice,all_inv,pose_job", [
    (((3, 1), (64, 25), (65, 64), (128, 2)), 1, False, None, True),       # 4 jobs; both bodies, on both sides of 64 (one lane round) and at 128
    (((129, 64), (1024, 25), (128, 64), (64, 1)), 2, True, 2, False),     # 129 / 1024: the 16-candidate body's ends; ties; a job without a valid target
    (((1025, 64), (1024, 2), (3, 2)), 1, False, None, True),              # 3 jobs, one above 1024: the kernel with the third body
    (((1025, 1),), 2, True, None, False),                                  # 1 job, the third body alone
    (((128, 25), (129, 25)), 1, True, 0, True),                            # 2 jobs on the two sides of 128
    (((65, 2),), 1, False, None, False),                                   # 1 job
])
def test_search_forms(ctx, hip, dev, searches, div, lattice, all_inv, pose_job):
    """Every search body (candidates per lane for n_tgt <= 128, <= 1024, above) as job 0, 1, 2 and 3 of a launch, k 1 / 2 / 25 / 64, an invalid
    source row, a job whose targets are all invalid, lattice poses, tgt_batch_div 1 / 2, with and without the pose-embedding job."""
    h = Half(ctx, dev, len(searches) * 10 + div, 2, 11, False, searches=searches, div=div, lattice=lattice, all_inv=all_inv, pose_job=pose_job)
    o = _check_half(hip, h)
    for (idx, m, _, _), (T, k) in zip(o["knn"], searches):
        assert idx.shape[-1] == k
    if all_inv is not None:
        assert bool((o["knn"][all_inv][1] == 1).all())
    assert bool((o["knn"][0][1][0, 5 // 2] == 1).all())  # the invalid source row
    if pose_job:
        assert float((o["pj"] - 3.0).abs().max()) > 0


@pytest.mark.parametrize("G,W,add", [(3, 1, False), (5, 11, False), (3, 1, True), (5, 16, True)])
def test_ragged_windows_against_the_row_chain(ctx, hip, dev, G, W, add):
    """The front's pooled rows on the ragged ends - an odd window count, window length 1 (every clamp of the early input loads is
    taken), a window without a valid step - against the grouped tbx_rowchain program (exact fp32 stages: a reference that shares no
    code with window_body), within tests/test_hip_parity.py's bound for this comparison, 2e-4 of the largest pooled entry (split-bf16
    stages against fp32); the all-invalid window exactly 0."""
    eng, m = ctx["eng"], ctx["model"]
    h = Half(ctx, dev, 500 + 10 * G + W, G, W, add, attr_cols=16 if add else 32)
    if not add:
        h.win["attr"][:, 20:] = 0.0  # (the producer zero-pads the 20 attributes to 32 columns)
    o = h.fused(hip)
    ref = torch.empty(G, D, device=dev)
    ch = hip.Chain(hip.group_tile_rows(W, G), 132)
    if add:
        cur = m.tl_encoder.input_encoder.emit(ch, h.win["attr"], h.win["pe"], pe_row_div=W)
        eng.emit_pointnet(ch, m.tl_encoder.temp_encoder, h.win["row_invalid"], ref, x_buf=cur)
    else:
        ch.load2(h.win["attr"], hip.BUF0, 0, h.win["pe"], hip.BUF1, 64)
        cur = eng.emit_mlp(ch, m.ag_encoder.input_encoder.mlp, hip.BUF0, 0)
        eng.emit_pointnet(ch, m.ag_encoder.temp_encoder, h.win["row_invalid"], ref, x_buf=cur)
    ch.run(G * W, group_rows=W)
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    assert scale > 1e-2 and float(ref[1].abs().max()) == 0.0 and float(o["x"][1].abs().max()) == 0.0
    assert float((o["x"] - ref).abs().max()) <= 2e-4 * scale, (float((o["x"] - ref).abs().max()), scale)


@pytest.mark.parametrize("pose", [True, False])
def test_rider_17_rows_against_the_row_chain(ctx, hip, dev, pose):
    """The front's rider at 17 rows (a full tile and a tile of one row: the clamped input rows) against the 4-stage tbx_rowchain program,
    within tests/test_hip_parity.py's bound for this comparison (1e-4 of the largest entry); invalid rows exactly 0."""
    h = Half(ctx, dev, 600 + pose, 3, 11, False, rider_rows=17, rider_pose=pose)
    o = h.fused(hip)
    Ws, bs = ctx["rider_wb"]
    inp = hip.pose_embed(h.rider["pose3"], ctx["fxy"], ctx["fyw"], D) if pose else h.rider["inp"]
    ref = torch.empty(17, D, device=dev)
    B0 = hip.BUF0
    ch = hip.Chain(16, 4 * D + 4)
    ch.load2(inp, B0, 0, h.rider["add"], B0, D)
    ch.linear(B0, 0, B0, D, Ws[0], bs[0], accum=True)
    ch.linear(B0, D, B0, 2 * D, Ws[1], bs[1], relu=True)
    ch.linear(B0, 2 * D, B0, D, Ws[2], bs[2], relu=True)
    ch.linear(B0, D, B0, 2 * D, Ws[3], bs[3], relu=True, skip_rows=h.rider["valid"], skip_is_valid=True, zero_skipped=True)
    ch.store(B0, 2 * D, D, ref)
    ch.run(17)
    torch.cuda.synchronize()
    out, bad = o["rider"], ~h.rider["valid"].bool()
    assert bool(bad.any()) and float(out[bad].abs().max()) == 0.0 and float(ref[bad].abs().max()) == 0.0
    err, scale = float((out - ref).abs().max()), float(ref.abs().max())
    assert scale > 1e-2 and err <= 1e-4 * scale, (err, scale)


PAIRS = {
    # agents' half, lights' half (G, searches, rider rows)
    "agents search, lights none, > 256 workgroups": (dict(G=100, rider_rows=17, searches=((200, 16), (40, 4)), S=20), dict(G=401)),
    "lights search, agents none": (dict(G=5, rider_rows=16), dict(G=3, searches=((65, 25),), pose_job=True)),
    "both search, one job above 1024": (dict(G=3, searches=((3, 2), (1025, 64)), pose_job=True), dict(G=7, searches=((128, 64), (129, 1), (64, 2)), div=2)),
}


@pytest.mark.parametrize("case", list(PAIRS))
def test_pair_equals_its_halves(ctx, hip, dev, case):
    """tbx_front_pair = its two tbx_front halves: halves of different sizes, a grid above 256 workgroups (more than one round on 256
    CUs), either half without searches, the kernel with and without the third search body."""
    ka, kb = PAIRS[case]
    ha = Half(ctx, dev, 1, W=11, add=False, **ka)
    hb = Half(ctx, dev, 2, W=5, add=True, attr_cols=16, **kb)
    sa, sb = ha.fused(hip), hb.fused(hip)
    (pa, ea), (pb, eb) = ha.deferred(hip), hb.deferred(hip)
    hip.launch_front_pair(ea, eb)
    torch.cuda.synchronize()
    assert float(sa["x"].abs().max()) > 1e-3 and float(sb["x"].abs().max()) > 1e-3
    _same(sa, pa, "agents")
    _same(sb, pb, "lights")


def test_argument_errors(ctx, hip, dev):
    """What tbx_front / tbx_front_pair return for a NULL image (-1, TBX_ERR_ARG), drop_thresh != 0 and a job with emb != NULL (-2,
    TBX_ERR_UNSUPPORTED: front_fill's checks, unchanged), and for the halves the wrong way round (-2); nothing is launched."""
    lib = hip.load()
    ha = Half(ctx, dev, 3, 4, 11, False, searches=((40, 4),))
    hb = Half(ctx, dev, 4, 4, 5, True, attr_cols=16)
    (_, ea), (_, eb) = ha.deferred(hip), hb.deferred(hip)
    fa, fb = ea[1], eb[1]
    both = lambda: (lib.tbx_front(C.byref(fa), None), lib.tbx_front_pair(C.byref(fa), C.byref(fb), None))
    assert lib.tbx_front_pair(C.byref(fb), C.byref(fa), None) == -2
    img = fa.win.in_images[1]
    fa.win.in_images[1] = None
    assert both() == (-1, -1)
    fa.win.in_images[1] = img
    fa.win.drop_thresh = 1
    assert both() == (-2, -2)
    fa.win.drop_thresh = 0
    jobs = C.cast(C.c_void_p(fa.jobs), C.POINTER(hip.KnnJob))
    jobs[0].emb = jobs[0].rel_pose
    assert both() == (-2, -2)
    jobs[0].emb = None
    fb.win.pn_images[2] = None
    assert lib.tbx_front_pair(C.byref(fa), C.byref(fb), None) == -1
    torch.cuda.synchronize()
