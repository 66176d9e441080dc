"""GPU sweep of the kernels that close every step of the rollout - tbx_sim_step (csrc/sim.hip, bodies in csrc/step_core.h), tbx_agent_prep /
tbx_tl_prep / tbx_map_prep (csrc/prep.hip) and tbx_diffbar_reward - against their float64 reference (tests/sim_step_ref.py) at the shapes
where the kernels take another path: more than 32 destination nodes, windows of more than 33 steps and of one, light windows of 8 / 9,
grids sized by the lights, workgroups of 256..1024 threads and the second launch above 256 workgroups, the parts one by one, the step-wise
driver's modifiers, steps past the log, window floats past index 64, the wavefront-per-agent form.

Method (tbx_sim_step): the state and the logs are cloned before every launch, and everything the launch leaves is compared with
sim_step_ref.step applied to the clone - one step from the kernel's own state, so nothing drifts. Masks, bytes, one-hots and counters
must be equal, floats lie within c * 2^-23 * scale (sim_step_cases.C: 4 x the float32 CPU evaluation's error, pinned on the CPU by
test_sim_step_ref.py); every tensor the reference leaves alone and every log column but step - 1 are unchanged bit for bit. Agents with a
float64 decision margin inside the band (32 float32 ulps of 50 m for the two distances, 32 * 2^-23 for the dot product) are skipped; at
most 0.5 % of a case's agent-steps (never fewer than one allowed) may be. Every buffer handed to a kernel is a view into a larger
allocation filled with a sentinel, and the margins are untouched after every call."""
import ctypes as C
from importlib import import_module

import pytest
import torch

import sim_step_cases as K
import sim_step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = {k: float("inf") for k in K.C}


class Arena:
    """One device allocation per element type, filled with a sentinel; the named tensors are views into it, a guard of G sentinels before,
    between and behind them. snapshot() brings everything to the host and checks the guards."""
    G = 64
    SENT = {torch.uint8: 0xA5, torch.float32: -12345.5, torch.int32: -77, torch.int64: -77}

    def __init__(self, tensors, dev):
        self.slots, self.flat, self.guard = {}, {}, {}
        by = {}
        for name, t in tensors.items():
            by.setdefault(t.dtype, []).append((name, t))
        for dt, items in by.items():
            off = self.G
            for name, t in items:
                self.slots[name] = (dt, off, tuple(t.shape))
                off += -(-t.numel() // self.G) * self.G + self.G
            flat, guard = torch.full((off,), self.SENT[dt], dtype=dt), torch.ones(off, dtype=torch.bool)
            for name, t in items:
                o = self.slots[name][1]
                flat[o:o + t.numel()], guard[o:o + t.numel()] = t.reshape(-1), False
            self.flat[dt], self.guard[dt] = flat.to(dev), guard

    def view(self, name):
        dt, o, shape = self.slots[name]
        return self.flat[dt][o:o + int(torch.Size(shape).numel())].view(shape)

    def snapshot(self, what=""):
        torch.cuda.synchronize()
        host = {dt: f.to("cpu", copy=True) for dt, f in self.flat.items()}
        for dt, h in host.items():
            assert bool((h[self.guard[dt]] == self.SENT[dt]).all()), f"{what}: a {dt} guard was written"
        return {name: host[dt][o:o + int(torch.Size(shape).numel())].view(shape) for name, (dt, o, shape) in self.slots.items()}


def _sim_struct(hip, arena, case):
    n, A, L, W, n_node, T, n_gt, n_tl_gt = case["dims"]
    S = case["S"]
    st = hip.SimState()
    st.n_batch, st.n_ag, st.n_tl, st.window, st.n_step_gt, st.n_step_tl_gt, st.n_step_out, st.n_node = n, A, L, W, n_gt, n_tl_gt, T, n_node
    for name, _ in hip.SimState._fields_:
        if name in arena.slots:
            setattr(st, name, arena.view(name).data_ptr())
    st.max_acc, st.max_yaw_rate, st.dt = (C.c_float * 3)(*S["max_acc"]), (C.c_float * 3)(*S["max_yaw_rate"]), S["dt"]
    st.w_pos, st.w_rot, st.w_spd = S["w_pos"], S["w_rot"], S["w_spd"]
    for ty in range(3):
        for d in range(2):
            st.act_log_std[ty][d] = S["act_log_std"][ty][d]
    return st


def _run_sim_case(hip, case, launches=None, compare=True):
    """-> (the snapshots after every step, kernel stats, yardstick stats, agent-steps in the band, agent-steps in all)."""
    dev = torch.device(DEV)
    S = case["S"]
    n, A, L, W = case["dims"][:4]
    tensors = {k: v for k, v in S.items() if torch.is_tensor(v)}
    lds = sorted({ld for st in case["steps"] for _, ld in st["launches"] if ld})
    extra = {}
    if lds:
        g = torch.Generator().manual_seed(5)
        extra["tl_invalid"] = (torch.rand(n * L, generator=g) < 0.3).to(torch.uint8)
        for tag in ("ride", "alone"):
            extra[f"{tag}_attr"] = torch.full((n * L * W, lds[0]), 7777.0)
            extra[f"{tag}_row_invalid"] = torch.full((n * L * W,), 99, dtype=torch.uint8)
    arena = Arena({**tensors, **extra}, dev)
    st = _sim_struct(hip, arena, case)
    kstats, ystats, n_band, n_pair, after_steps = {}, {}, 0, 0, []
    name = case["name"]
    for i, step in enumerate(case["steps"]):
        for k, v in step["set"].items():
            arena.view(k).copy_(v)
        for parts, ld in (launches or step["launches"]):
            what = f"{name} step {i + 1} parts {parts}"
            snap = arena.snapshot(what + " (before)")
            before = {**{k: snap[k] for k in tensors}, **{k: v for k, v in S.items() if not torch.is_tensor(v)}}
            hip.sim_step(st, parts, tl_prep=(arena.view("tl_invalid"), arena.view("ride_attr"), arena.view("ride_row_invalid")) if ld else None)
            snap2 = arena.snapshot(what)
            if not compare:
                continue
            after = {k: snap2[k] for k in tensors}
            t = int(before["step"][0])
            eps = after["out_act_noise"][:, :, t - 1] if ("act_seed" in tensors and parts & R.AGENTS and t - 1 < case["dims"][5]) else None
            if "act_seed" in tensors and parts & R.AGENTS:
                assert eps is not None, "the sampled case stays inside its log"
            new, log, scale, mg = R.step(before, before["action_mean"], before["tl_logits"], parts, eps=eps)
            band = K.band_of(mg)
            if band is not None:
                n_band, n_pair = n_band + int(band.sum()), n_pair + band.numel()
            bad = K.check_launch(before, after, new, log, scale, band, kstats, what)
            assert not bad, "\n".join(bad)
            new32, log32, _, _ = R.step(before, before["action_mean"], before["tl_logits"], parts, eps=eps, dtype=torch.float32)
            K.check_launch(before, K.commit(before, new32, log32), new, log, scale, band, ystats, what, INF)
            if ld:  # the rows riding on the lights' update: the reference's and the stand-alone kernel's on the new windows
                want = R.tl_rows(new["hist_tl"], snap2["tl_invalid"].view(n, L), ld)
                assert torch.equal(snap2["ride_attr"].double(), want["attr"]) and torch.equal(snap2["ride_row_invalid"] != 0, want["row_invalid"]), what
                hip.tl_prep(arena.view("hist_tl"), arena.view("tl_invalid"), arena.view("alone_attr"), arena.view("alone_row_invalid"))
                snap3 = arena.snapshot(what + " (tbx_tl_prep)")
                assert torch.equal(snap3["alone_attr"], snap3["ride_attr"]) and torch.equal(snap3["alone_row_invalid"], snap3["ride_row_invalid"]), what
                assert all(torch.equal(K._bits(snap3[k]), K._bits(snap2[k])) for k in tensors), what
        after_steps.append(arena.snapshot(name))
    return after_steps, kstats, ystats, n_band, n_pair


def _report(name, kstats, ystats):
    print(f"[{name}] worst err / bound, kernel (float32 yardstick): " +
          ", ".join(f"{g} {v / K.C[g]:.3g} ({ystats.get(g, 0.0) / K.C[g]:.3g})" for g, v in kstats.items()))


@pytest.mark.parametrize("name", list(K.sim_cases()))
def test_sim_step_against_the_float64_reference(tb, name):
    """One case of sim_step_cases.sim_cases() (their docstrings say which path each reaches), launch by launch, by the module's method.
    `parts`: AGENTS, then LIGHTS, then ADVANCE in launches of their own - and the state and logs after every step equal the one-launch
    step's bit for bit. grid1100 / grid8200: the counter reads [t + 1, 0] after every step (part of the comparison of `step`)."""
    hip = import_module("trafficbots_amd.hip")
    case = K.sim_cases()[name]
    steps, kstats, ystats, n_band, n_pair = _run_sim_case(hip, case)
    print(f"[{name}] {n_band} of {n_pair} agent-steps inside the decision band, skipped (allowed {K.band_allowed(n_pair)})")
    _report(name, kstats, ystats)
    assert n_band <= K.band_allowed(n_pair)
    if name.startswith("grid"):
        assert [snap["step"].tolist() for snap in steps] == [[i + 2, 0] for i in range(len(steps))]
    if name == "parts":
        whole, *_ = _run_sim_case(hip, case, launches=[(K.FULL, None)], compare=False)
        for i, (a, b) in enumerate(zip(steps, whole)):
            for k in a:
                assert torch.equal(K._bits(a[k]), K._bits(b[k])), (k, i)


def test_agent_prep_against_the_float64_reference(tb):
    """tbx_agent_prep over sim_step_cases.agent_prep_cases(): W in {1, 11, 21, 22, 23} (3 W floats pass index 64 at 22 and 23), 3 and 515
    rows (the wavefront-per-agent form at its built-in switch of 512 rows, 515 % 4 != 0), pe_dim 64 and 128, type_mask and dest on and
    off, mp_batch_div 1 and 3, every validity pattern. Copies, one-hots, masks and navi_row equal; pe and navi_pose3 within their bounds;
    the inputs and the guards around every buffer untouched."""
    hip = import_module("trafficbots_amd.hip")
    dev = torch.device(DEV)
    for name, c in K.agent_prep_cases().items():
        ref = K.agent_rows_of(c)
        n, A, W = c["hist_valid"].shape
        full = c["dest"] is not None
        ins = {k: c[k] for k in ("hist_valid", "hist_pose", "hist_motion", "ag_attr6", "freqs_xy", "freqs_yaw")}
        if full:
            ins.update(ag_type_idx=c["ag_type_idx"], dest=c["dest"], mp_tok_pose=c["mp_tok_pose"])
        outs = dict(tok_pose=torch.full((n, A, 3), 7777.0), tok_invalid=torch.full((n, A), 99, dtype=torch.uint8), attr=torch.full((n * A * W, 32), 7777.0),
                    pe=torch.full((n * A * W, c["pe_dim"]), 7777.0), row_invalid=torch.full((n * A * W,), 99, dtype=torch.uint8))
        if full:
            outs.update(type_mask=torch.full((3, n * A), 99, dtype=torch.uint8), navi_pose3=torch.full((n * A, 3), 7777.0),
                        navi_row=torch.full((n * A,), -5, dtype=torch.int32))
        arena = Arena({**ins, **outs}, dev)
        v = arena.view
        hip.agent_prep(v("hist_valid"), v("hist_pose"), v("hist_motion"), v("ag_attr6"), v("ag_type_idx") if full else None, v("freqs_xy"),
                       v("freqs_yaw"), c["pe_dim"], {k: v(k) for k in outs}, dest=v("dest") if full else None,
                       mp_tok_pose=v("mp_tok_pose") if full else None, n_mp=c["mp_tok_pose"].shape[1] if full else 0, mp_batch_div=c["mp_batch_div"])
        snap = arena.snapshot(name)
        assert all(torch.equal(K._bits(snap[k]), K._bits(t)) for k, t in ins.items()), name
        kstats, ystats = {}, {}
        bad = K.check_rows(snap, ref, K.PREP_GROUPS, kstats, name)
        assert not bad, "\n".join(bad)
        K.check_rows(K.agent_rows_of(c, dtype=torch.float32), ref, K.PREP_GROUPS, ystats, name, INF)
        _report("agent_prep " + name, kstats, ystats)


def test_map_prep_against_the_float64_reference(tb):
    """tbx_map_prep at n_node 1 / 20 / 21 on 2 x 7 polylines (a row count that fills no workgroup; more than one), nodes behind, beside and
    ahead of the first node (the clamp of the projection at 1, inside, at 0) and a node on the frame's origin."""
    hip = import_module("trafficbots_amd.hip")
    for name, c in K.map_prep_cases().items():
        ref = R.map_rows(**c)
        n, M, N = c["mp_valid"].shape
        outs = dict(attr=torch.full((n * M * N, 32), 7777.0), pe=torch.full((n * M * N, 8), 7777.0), row_invalid=torch.full((n * M * N,), 99, dtype=torch.uint8),
                    tok_pose=torch.full((n, M, 3), 7777.0), tok_invalid=torch.full((n, M), 99, dtype=torch.uint8))
        arena = Arena({**c, **outs}, torch.device(DEV))
        v = arena.view
        hip.map_prep(v("mp_valid"), v("mp_type11"), v("mp_pose"), v("attr"), v("pe"), v("row_invalid"), v("tok_pose"), v("tok_invalid"))
        snap = arena.snapshot(name)
        assert all(torch.equal(K._bits(snap[k]), K._bits(t)) for k, t in c.items()), name
        kstats, ystats = {}, {}
        bad = K.check_rows(snap, ref, K.MAP_GROUPS, kstats, name)
        assert not bad, "\n".join(bad)
        K.check_rows(R.map_rows(**c, dtype=torch.float32), ref, K.MAP_GROUPS, ystats, name, INF)
        _report("map_prep " + name, kstats, ystats)


def test_tl_prep_against_the_reference(tb):
    """tbx_tl_prep at W in {1, 11, 27} x ld_attr in {8, 16, 32, 64} where the row holds the window: one-hots, padding and masks equal."""
    hip = import_module("trafficbots_amd.hip")
    for name, c in K.tl_prep_cases().items():
        n, L, W = c["hist_tl"].shape
        ref = R.tl_rows(c["hist_tl"], c["tl_invalid"], c["ld_attr"])
        arena = Arena(dict(hist_tl=c["hist_tl"], tl_invalid=c["tl_invalid"].reshape(-1), attr=torch.full((n * L * W, c["ld_attr"]), 7777.0),
                           row_invalid=torch.full((n * L * W,), 99, dtype=torch.uint8)), torch.device(DEV))
        hip.tl_prep(arena.view("hist_tl"), arena.view("tl_invalid"), arena.view("attr"), arena.view("row_invalid"))
        snap = arena.snapshot(name)
        assert torch.equal(snap["hist_tl"], c["hist_tl"]) and torch.equal(snap["tl_invalid"], c["tl_invalid"].reshape(-1)), name
        assert torch.equal(snap["attr"].double(), ref["attr"]) and torch.equal(snap["row_invalid"] != 0, ref["row_invalid"]), name


def test_diffbar_reward_against_the_float64_reference(tb):
    """tbx_diffbar_reward with differences at 1 +- 1e-3 and exactly 1 (smooth L1's switch), yaw differences across +-pi, and gt_valid
    NULL (valid = pred_valid, every term 0)."""
    hip = import_module("trafficbots_amd.hip")
    c = K.reward_case()
    keys = ("pred_valid", "pred_pose", "pred_motion", "gt_valid", "gt_pose", "gt_motion")
    arena = Arena({k: c[k] for k in keys}, torch.device(DEV))
    v = arena.view
    w = (c["w_pos"], c["w_rot"], c["w_spd"])
    out4, ov = hip.diffbar_reward(*(v(k) for k in keys), *w)
    out4_0, ov_0 = hip.diffbar_reward(v("pred_valid"), v("pred_pose"), v("pred_motion"), None, None, None, *w)
    snap = arena.snapshot("diffbar_reward")
    assert all(torch.equal(K._bits(snap[k]), K._bits(c[k])) for k in keys)
    r4, r_valid, s4 = R.reward(**c)
    kstats, ystats = {}, {}
    bad = K._float_check("out4", out4.cpu(), r4, s4, "reward", None, kstats, "diffbar_reward")
    assert not bad, "\n".join(bad)
    assert torch.equal(ov.cpu() != 0, r_valid)
    K._float_check("out4", R.reward(**c, dtype=torch.float32)[0], r4, s4, "reward", None, ystats, "diffbar_reward", INF)
    _report("diffbar_reward", kstats, ystats)
    assert not bool(out4_0.any()) and torch.equal(ov_0.cpu(), c["pred_valid"])
    near = (c["gt_pose"][:40, 0] - c["pred_pose"][:40, 0]).abs()
    assert bool((near == 1).any()) and bool((near < 1).any()) and bool((near > 1).any())  # the inputs do sit on the switch
