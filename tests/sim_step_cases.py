"""Inputs, tolerances and the comparison of the float64 reference sweep of the closed-loop step and the feature preparation
(tests/sim_step_ref.py): shared by the CPU tests that pin them (test_sim_step_ref.py) and the GPU tests that use them
(test_hip_sim_step.py). Nothing here runs on a GPU.

A case = a state (CPU tensors named like tbx_sim_state_t's fields + the scalar fields) and a list of steps; a step = the model outputs of
the step, the fields rewritten before it (explicit overrides, player actions) and the launches (parts, ld_attr of riding light rows | None)
it is made of. Inputs: boundary +-50 m, positions uniform in +-48 m, speeds 0..15 m/s, destination nodes 1 m apart starting 2..12 m
ahead, 30 % of the nodes invalid, thresholds 3 / 10 m, tanh actions from N(0, 1.5)."""
import math

import torch

import sim_step_ref as R

U8, F32 = torch.uint8, torch.float32
ULP = 2.0 ** -23
COORD = 50.0                                  # the cases' largest coordinate magnitude (the boundary)
BAND_DIST = 32 * 2.0 ** (math.floor(math.log2(COORD)) - 23)  # 32 float32 ulps of it: the two distances
BAND_DOT = 32 * ULP                           # the dot product against cos 30 deg
BAND_CAP = 0.005                              # share of a case's agent-steps that may lie in the band (never fewer than one allowed)

# c of the bound c * 2^-23 * scale per output group: 4 x the worst figure of the float32 CPU evaluation of the reference against its
# float64 evaluation on these very inputs (test_sim_step_ref.py::test_float32_yardstick measures them again and holds them to C / 4;
# the figures are in profiles/MEASUREMENT_LOG.md), rounded up to a whole number of at most two significant digits. Not taken from any
# kernel's output. Measured: pose 1.02, motion 0.83, reward 0.43, nll 0.44, log_prob 0.51, pe 33.5 (1 + |argument| does not see the
# cancellation of a rotated offset of tens of metres: 4 x is still 1.7e-5 of the scale), navi 1.34, map_pe 0.85.
C = {"pose": 5.0, "motion": 4.0, "reward": 2.0, "nll": 2.0, "log_prob": 3.0, "pe": 140.0, "navi": 6.0, "map_pe": 4.0}
# ... capped at what the rollout tests state for the quantity (test_hip_rollout._compare): (rtol, atol)
CAP = {"pose": (1e-4, 1e-3)}
CAP_REST = (1e-3, 1e-3)

AG_KEYS = {"ag_valid", "ag_disabled", "ag_pose", "ag_motion", "navi_valid", "outside_map", "dest_reached", "hist_valid", "hist_pose",
           "hist_motion", "now_outside", "now_reached", "out_valid", "out_pose", "out_motion", "out_action", "out_outside_map",
           "out_dest_reached", "out_reward", "out_reward_valid", "out_tf", "out_act_noise", "out_act_log_prob"}
GROUP = {"ag_pose": "pose", "hist_pose": "pose", "out_pose": "pose", "ag_motion": "motion", "hist_motion": "motion", "out_motion": "motion",
         "out_action": "motion", "out_reward": "reward", "out_tl_nll": "nll", "out_act_log_prob": "log_prob", "out_act_noise": "log_prob"}
LOG_STEP_DIM = 2  # out_* are [n, A | L, T, ..]

FULL = R.AGENTS | R.LIGHTS | R.ADVANCE
LIMITS = dict(max_acc=[4.0, 2.0, 3.0], max_yaw_rate=[1.0, 1.5, 1.2], dt=0.1, w_pos=0.1, w_rot=10.0, w_spd=0.1,
              act_log_std=[[-2.0, -1.5], [-1.0, -2.5], [-0.5, -3.0]])
SCALARS = tuple(LIMITS)


def _rand(g, *shape, lo=0.0, hi=1.0):
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(F32)


def _pose(g, *shape):
    return torch.cat([_rand(g, *shape, 2, lo=-48, hi=48), _rand(g, *shape, 1, lo=-math.pi, hi=math.pi)], -1)


def make_state(n, A, L, W, n_node, T, n_gt, n_tl_gt, seed, far_nodes=False, optional=True, sampled=False, now=False):
    """far_nodes: for every second agent the nodes below index 32 are invalid and the polyline runs TOWARDS the agent, so the only valid
    node within the threshold / within 30 degrees has index >= 32."""
    g = torch.Generator().manual_seed(seed)
    bern = lambda p, *s: (torch.rand(*s, generator=g) < p).to(U8)
    S = dict(LIMITS)
    S["step"] = torch.tensor([1, 0], dtype=torch.int32)
    never = bern(0.1, n, A)  # never valid: invalid now, in the window, and no ground truth
    S["ag_valid"] = bern(0.8, n, A) * (1 - never)
    S["ag_disabled"] = bern(0.1, n, A) * (1 - S["ag_valid"])
    S["ag_pose"] = torch.cat([_rand(g, n, A, 2, lo=-48, hi=48), _rand(g, n, A, 1, lo=-math.pi, hi=math.pi)], -1)
    S["ag_pose"][:, 0, 2] = math.pi - 1e-3  # yaws next to +-pi
    if A > 1:
        S["ag_pose"][:, 1, 2] = -math.pi + 1e-3
    S["ag_motion"] = torch.cat([_rand(g, n, A, 1, hi=15), _rand(g, n, A, 1, lo=-3, hi=3), _rand(g, n, A, 1, lo=-1, hi=1)], -1)
    S["ag_pose"] *= S["ag_valid"].unsqueeze(-1)  # an invalid agent's state is 0 (dynamics.py masks it)
    S["ag_motion"] *= S["ag_valid"].unsqueeze(-1)
    S["navi_valid"] = bern(0.9, n, A)
    S["outside_map"], S["dest_reached"] = bern(0.05, n, A), bern(0.1, n, A)
    S["tl_state"] = (1 << torch.randint(0, 5, (n, L), generator=g)).to(U8)
    S["hist_valid"] = bern(0.7, n, A, W) * (1 - never).unsqueeze(-1)
    S["hist_pose"] = torch.cat([_rand(g, n, A, W, 2, lo=-48, hi=48), _rand(g, n, A, W, 1, lo=-math.pi, hi=math.pi)], -1)
    S["hist_motion"] = _rand(g, n, A, W, 3, lo=-3, hi=15)
    S["hist_tl"] = (1 << torch.randint(0, 5, (n, L, W), generator=g)).to(U8)
    S["hist_tl"][bern(0.2, n, L, W).bool()] = 0xFF  # missing steps
    S["ag_type_idx"] = torch.randint(0, 3, (n, A), generator=g).to(U8)
    # ground truth with holes; forced (every step), spawned (the first step ground truth turns valid) and free (step 0 only) agents
    S["gt_valid"] = bern(0.8, n, A, n_gt) * (1 - never).unsqueeze(-1)
    role = torch.randint(0, 3, (n, A), generator=g)
    tf = torch.zeros(n, A, n_gt, dtype=U8)
    tf[:, :, 0] = S["gt_valid"][:, :, 0]
    tf[role == 0] = S["gt_valid"][role == 0]
    spawn = torch.zeros_like(tf)
    spawn[:, :, 1:] = (1 - S["gt_valid"][:, :, :-1]) * S["gt_valid"][:, :, 1:]
    tf[role == 1] |= spawn[role == 1]
    S["tf_mask"] = tf
    S["gt_pose"] = torch.cat([_rand(g, n, A, n_gt, 2, lo=-48, hi=48), _rand(g, n, A, n_gt, 1, lo=-math.pi, hi=math.pi)], -1)
    S["gt_motion"] = torch.cat([_rand(g, n, A, n_gt, 1, hi=15), _rand(g, n, A, n_gt, 1, lo=-3, hi=3), _rand(g, n, A, n_gt, 1, lo=-1, hi=1)], -1)
    S["tl_gt"] = (1 << torch.randint(0, 5, (n, L, n_tl_gt), generator=g)).to(U8)
    S["boundary"] = torch.tensor([-COORD, COORD, -COORD, COORD], dtype=F32).repeat(n, 1)
    # destination polylines: nodes 1 m apart along the agent's heading turned by up to +-50 degrees, the first 2..12 m ahead
    yaw = S["ag_pose"][..., 2].double()
    head = torch.stack([yaw.cos(), yaw.sin()], -1)
    turn = yaw + _rand(g, n, A, lo=-0.87, hi=0.87).double()
    d = torch.stack([turn.cos(), turn.sin()], -1)
    k = torch.arange(n_node, dtype=torch.float64)
    far = torch.zeros(n, A, dtype=torch.bool)
    if far_nodes:
        far[:, ::2] = True
    along = torch.where(far.unsqueeze(-1), (n_node - 1 - k).expand(n, A, -1), k.expand(n, A, -1))
    start = S["ag_pose"][..., :2].double() + head * _rand(g, n, A, 1, lo=2, hi=12).double()
    S["dest_pos"] = (start.unsqueeze(2) + along.unsqueeze(-1) * d.unsqueeze(2)).to(F32)
    S["dest_dir"] = d.unsqueeze(2).expand(-1, -1, n_node, -1).to(F32).contiguous()
    S["dest_invalid"] = bern(0.3, n, A, n_node)
    if far_nodes:
        S["dest_invalid"][:, ::2, :32] = 1
        S["dest_invalid"][:, ::2, 32:] = 0
    S["dest_kind"] = torch.randint(0, 4, (n, A), generator=g).to(U8)
    S["dest_thresh"] = torch.where(torch.rand(n, A, generator=g) < 0.5, 3.0, 10.0).to(F32)
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt)
    S.update(out_valid=z(n, A, T, dt=U8), out_pose=z(n, A, T, 3), out_motion=z(n, A, T, 3), out_action=z(n, A, T, 2),
             out_tl_state=z(n, L, T, dt=U8), out_outside_map=z(n, A, T, dt=U8), out_dest_reached=z(n, A, T, dt=U8))
    if optional:
        S.update(out_reward=z(n, A, T, 4), out_reward_valid=z(n, A, T, dt=U8), out_tf=z(n, A, T, dt=U8), out_tl_nll=z(n, L, T))
    if sampled:
        S.update(act_seed=torch.tensor([0x1234567 + seed], dtype=torch.int64), out_act_noise=z(n, A, T, 2), out_act_log_prob=z(n, A, T))
    if now:
        S.update(now_outside=z(n, A, dt=U8), now_reached=z(n, A, dt=U8))
    return S, g


def model_outputs(g, n, A, L):
    """tanh actions from N(0, 1.5), light logits from N(0, 2)."""
    return {"action_mean": (torch.randn(n * A, 2, generator=g, dtype=torch.float64) * 1.5).to(F32),
            "tl_logits": (torch.randn(n, L, 5, generator=g, dtype=torch.float64) * 2).to(F32)}


def _plain_steps(g, n, A, L, n_step, launches=((FULL, None),)):
    return [dict(set=model_outputs(g, n, A, L), launches=list(launches)) for _ in range(n_step)]


def _case(name, dims, n_step, seed, launches=((FULL, None),), **kw):
    n, A, L, W, n_node, T, n_gt, n_tl_gt = dims
    S, g = make_state(n, A, L, W, n_node, T, n_gt, n_tl_gt, seed, **kw)
    S.update(model_outputs(g, n, A, L))
    return dict(name=name, S=S, steps=_plain_steps(g, n, A, L, n_step, launches), dims=dims)


def _stepwise(seed):
    """A step-wise driver: explicit overrides of agents and lights, player actions, NO_DISABLE | NO_APPEND with now_*, then APPEND."""
    dims = n, A, L, W, n_node, T, n_gt, n_tl_gt = 3, 6, 3, 11, 20, 8, 5, 4
    S, g = make_state(*dims, seed, now=True)
    S.update(model_outputs(g, n, A, L))
    bern = lambda p, *s: (torch.rand(*s, generator=g) < p).to(U8)
    S.update(player_valid=bern(0.3, n, A), player_action=_rand(g, n, A, 2, lo=-2, hi=2), ov_valid=bern(0.3, n, A),
             ov_pose=_pose(g, n, A), ov_motion=_rand(g, n, A, 3, lo=-3, hi=15), ov_tl_valid=bern(0.5, n, L),
             ov_tl_state=(1 << torch.randint(0, 5, (n, L), generator=g)).to(U8))
    S["ag_disabled"][0, 2], S["ag_valid"][0, 2] = 1, 0  # an override on a disabled agent, at every step
    steps = []
    for _ in range(6):
        st = model_outputs(g, n, A, L)
        st.update(player_valid=bern(0.3, n, A), player_action=_rand(g, n, A, 2, lo=-2, hi=2), ov_valid=bern(0.3, n, A),
                  ov_pose=_pose(g, n, A), ov_motion=_rand(g, n, A, 3, lo=-3, hi=15), ov_tl_valid=bern(0.5, n, L),
                  ov_tl_state=(1 << torch.randint(0, 5, (n, L), generator=g)).to(U8))
        st["ov_valid"][0, 2] = 1
        st["player_valid"][:, 3] = 1  # (agents invalid at some step among them: the player's action is for valid agents)
        steps.append(dict(set=st, launches=[(FULL | R.NO_DISABLE | R.NO_APPEND, None), (R.APPEND, None)]))
    return dict(name="stepwise", S=S, steps=steps, dims=dims)


def _lights_edge(seed):
    """Tied logits (all five, the first two, the last two), logits of +-80, tl_gt masks 0 and 0xFF."""
    dims = n, A, L, W, n_node, T, n_gt, n_tl_gt = 2, 3, 8, 9, 20, 6, 4, 3
    c = _case("lights_edge", dims, 6, seed)
    S = c["S"]
    S["tl_gt"][:, 0, :], S["tl_gt"][:, 1, :] = 0, 0xFF
    for st in [dict(set=S)] + c["steps"]:
        lg = st["set"]["tl_logits"]
        lg[:, 0], lg[:, 1, :2], lg[:, 2, 3:] = 0.25, 3.5, 4.0
        lg[:, 3], lg[:, 4] = torch.tensor([80.0, -80.0, 79.0, -80.0, 0.0]), torch.tensor([-80.0, -80.0, -80.0, -79.5, -80.0])
        lg[0, 5] = torch.tensor([-80.0, 80.0, 80.0, -80.0, 80.0])
    return c


def sim_cases():
    """name -> case. Each runs a dozen steps or fewer, at the smallest shapes that reach the paths named in the module docstrings."""
    split = ((R.AGENTS, None), (R.LIGHTS, None), (R.ADVANCE, None))
    cases = [
        _case("base", (3, 5, 3, 11, 20, 12, 8, 6), 12, 1),
        _case("nodes33", (2, 5, 2, 11, 33, 6, 4, 3), 6, 2, far_nodes=True),
        _case("nodes70", (2, 5, 2, 11, 70, 6, 4, 3), 6, 3, far_nodes=True),
        _case("win34", (2, 3, 2, 34, 20, 5, 3, 3), 5, 4),
        _case("win70", (2, 3, 2, 70, 20, 5, 3, 3), 5, 5),
        _case("win1", (2, 3, 2, 1, 20, 5, 3, 3), 5, 6),
        _case("win2", (2, 3, 2, 2, 20, 5, 3, 3), 5, 7),
        _case("win8", (2, 3, 3, 8, 20, 5, 3, 3), 5, 8),
        _case("win9", (2, 3, 3, 9, 20, 5, 3, 3), 5, 9),
        _case("lights_grid", (2, 1, 9, 11, 20, 5, 3, 3), 5, 10),
        _case("parts", (3, 5, 3, 11, 20, 8, 5, 4), 8, 11, launches=split),
        _stepwise(12),
        _case("past_log", (2, 5, 2, 11, 20, 4, 3, 3), 7, 13),
        _case("riding_rows16", (2, 3, 5, 11, 20, 5, 3, 3), 5, 14, launches=((FULL, 16),)),
        _case("riding_rows32", (2, 3, 5, 11, 20, 5, 3, 3), 5, 15, launches=((FULL, 32),)),
        _lights_edge(16),
        _case("sampled", (3, 5, 2, 11, 20, 8, 5, 4), 8, 17, sampled=True),
        _case("grid1100", (11, 100, 2, 2, 1, 3, 2, 2), 3, 18, optional=False),
        _case("grid8200", (82, 100, 2, 2, 1, 3, 2, 2), 3, 19, optional=False),
    ]
    return {c["name"]: c for c in cases}


def band_of(margins):
    """[n, A] bool: the (agent, step) pairs with a float64 decision margin inside the band."""
    if not margins:
        return None
    return (margins["bnd"] < BAND_DIST) | (margins["dist"] < BAND_DIST) | (margins["dot"] < BAND_DOT)


def band_allowed(n_agent_steps):
    return max(1, int(BAND_CAP * n_agent_steps))


def _bits(x):
    return x if x.dtype == U8 else x.contiguous().view(U8)


def _float_check(name, got, ref, scale, group, skip, stats, what, c_of=C):
    err = (got.double() - ref.double()).abs()
    unit = ULP * scale.double()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / unit)  # (scale 0 = an exact copy or an exact 0: any error is infinite)
    if skip is not None:
        ratio = ratio.masked_fill(skip.view(skip.shape + (1,) * (ratio.dim() - skip.dim())), 0)
    rtol, atol = CAP.get(group, CAP_REST)
    capped = torch.minimum(c_of[group] * unit, atol + rtol * ref.double().abs())
    bad = (err > capped) & (ratio > 0)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    stats[group] = max(stats.get(group, 0.0), worst)
    return [f"{what} {name}: {int(bad.sum())} elements beyond the bound, worst err / (2^-23 scale) = {worst:.3g} (c = {c_of[group]})"] if bool(bad.any()) else []


def check_launch(before, after, new, log, scale, band, stats, what, c_of=C):
    """One launch: `after` (name -> tensor, as the kernel left it or as another evaluation of the reference gives it) against the
    reference's (new, log, scale) for the state `before`. Masks, bytes and counters equal, floats within c * 2^-23 * scale (capped);
    every tensor the reference does not name, and every log column but step - 1, unchanged bit for bit; agents in `band` are skipped.
    -> the list of mismatches (empty = equal); stats[group] = worst err / (2^-23 scale)."""
    bad = []
    t = int(before["step"][0])
    for name, b in before.items():
        if not torch.is_tensor(b):
            continue
        a = after[name]
        skip = band if (band is not None and name in AG_KEYS) else None
        if name in new:
            ref, got = new[name], a
        elif name in log:
            col = torch.zeros(b.shape[LOG_STEP_DIM], dtype=torch.bool)
            col[t - 1] = True
            if not torch.equal(_bits(a[:, :, ~col]), _bits(b[:, :, ~col])):
                bad.append(f"{what} {name}: a log column other than step - 1 = {t - 1} changed")
            ref, got = log[name], a[:, :, t - 1]
        else:
            if not torch.equal(_bits(a), _bits(b)):
                bad.append(f"{what} {name}: changed, and the reference leaves it alone")
            continue
        if ref.dtype.is_floating_point:
            bad += _float_check(name, got, ref, scale[name], GROUP[name], skip, stats, what, c_of)
        else:
            ne = got.to(torch.int64) != ref.to(torch.int64)
            if skip is not None:
                ne = ne.masked_fill(skip.view(skip.shape + (1,) * (ne.dim() - skip.dim())), False)
            if bool(ne.any()):
                bad.append(f"{what} {name}: {int(ne.sum())} entries differ (first at {ne.nonzero()[0].tolist()})")
    return bad


def commit(S, new, log):
    """The state after a launch as the device holds it: the reference's results stored in the tensors' own types."""
    t = int(S["step"][0])
    out = dict(S)
    for name, v in new.items():
        out[name] = v.to(S[name].dtype)
    for name, v in log.items():
        x = S[name].clone()
        x[:, :, t - 1] = v.to(x.dtype)
        out[name] = x
    return out


def step_noise(S, action_noise):
    """The step's eps [n, A, 2] for the state's seed: hip_base.action_noise, the Python restatement of the generator."""
    if S.get("act_seed") is None:
        return None
    n, A = S["ag_valid"].shape
    e = action_noise(int(S["act_seed"][0]) % (1 << 64), int(S["step"][0]), torch.arange(n * A).numpy())
    return torch.from_numpy(e).to(F32).view(n, A, 2)


def walk(case, action_noise=None, dtype=torch.float64, defects=()):
    """The reference on its own through the case: yields (before, parts, ld, new, log, scale, margins) per launch, committing the clean
    float64 results (so an evaluation with defects, or in float32, is always ONE launch away from the clean trajectory, as the kernel is
    from its own state in the GPU test)."""
    S = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in case["S"].items()}
    for st in case["steps"]:
        S = dict(S)
        S.update({k: v.clone() for k, v in st["set"].items()})
        for parts, ld in st["launches"]:
            eps = step_noise(S, action_noise) if parts & R.AGENTS else None
            clean = R.step(S, S["action_mean"], S["tl_logits"], parts, eps=eps)
            other = clean if (dtype == torch.float64 and not defects) else R.step(S, S["action_mean"], S["tl_logits"], parts, eps=eps, dtype=dtype, defects=defects)
            yield S, parts, ld, clean, other
            S = commit(S, clean[0], clean[1])


# ---------------------------------------------------------------------------------------------------------------- feature preparation
def _freqs(pe_dim):
    """pe_xy.freqs / pe_yaw.freqs as the model holds them (repeat-interleaved): pe_dim / 4 and pe_dim / 2 entries."""
    return R.H.make_freqs_xy(pe_dim // 4, 1000.0), R.H.make_freqs_rad(pe_dim // 2)


def agent_prep_cases():
    """W in {1, 11, 21, 22, 23} x n_tok in {3, 515} (the wavefront form from 512 rows on; 515 % 4 != 0) x pe_dim 64 with type_mask and
    dest / 128 without, + mp_batch_div 3 and pe_dim 128 with dest; per agent one of the validity patterns none / first only / last only /
    a hole / last valid before the end / all; yaws next to +-pi, coordinates up to 2e3 m (a window is a trajectory: its steps lie
    within tens of metres of each other)."""
    cfgs = [(W, n, A, pe, full, 1) for W in (1, 11, 21, 22, 23) for n, A in ((1, 3), (5, 103)) for pe, full in ((64, True), (128, False))]
    cfgs += [(11, 6, 3, 64, True, 3), (23, 6, 3, 128, True, 3), (22, 1, 3, 128, True, 1)]
    out = []
    for W, n, A, pe_dim, full, div in cfgs:
        g = torch.Generator().manual_seed(1000 + W * 7 + n + pe_dim + div)
        valid = torch.zeros(n, A, W, dtype=U8)
        pat = torch.arange(n * A).view(n, A) % 6
        valid[pat == 1, 0] = 1
        valid[pat == 2, W - 1] = 1
        valid[pat == 3] = 1
        valid[pat == 3, W // 2] = 0
        valid[pat == 4, : max(1, W - 2)] = 1
        valid[pat == 5] = 1
        base = torch.cat([_rand(g, n, A, 1, 2, lo=-2e3, hi=2e3), _rand(g, n, A, 1, 1, lo=-math.pi, hi=math.pi)], -1)
        base[:, 0, 0, 2] = math.pi - 1e-3
        base[:, 1, 0, 2] = -math.pi + 1e-3
        pose = base + torch.cat([_rand(g, n, A, W, 2, lo=-30, hi=30), _rand(g, n, A, W, 1, lo=-0.5, hi=0.5)], -1)
        M, n_map = 7, n // div
        c = dict(name=f"W{W}_tok{n * A}_pe{pe_dim}_{'full' if full else 'bare'}_div{div}", hist_valid=valid, hist_pose=pose,
                 hist_motion=_rand(g, n, A, W, 3, lo=-3, hi=15), ag_attr6=_rand(g, n, A, 6, hi=5), pe_dim=pe_dim,
                 ag_type_idx=torch.randint(0, 3, (n, A), generator=g).to(U8) if full else None,
                 dest=torch.randint(0, M, (n, A), generator=g) if full else None, mp_batch_div=div,
                 mp_tok_pose=torch.cat([_rand(g, n_map, M, 2, lo=-2e3, hi=2e3), _rand(g, n_map, M, 1, lo=-math.pi, hi=math.pi)], -1) if full else None)
        c["freqs_xy"], c["freqs_yaw"] = _freqs(pe_dim)
        out.append(c)
    return {c["name"]: c for c in out}


def agent_rows_of(c, **kw):
    return R.agent_rows(c["hist_valid"], c["hist_pose"], c["hist_motion"], c["ag_attr6"], c["ag_type_idx"], c["freqs_xy"], c["freqs_yaw"],
                        c["pe_dim"], c["dest"], c["mp_tok_pose"], c["mp_batch_div"], **kw)


def map_prep_cases():
    """n_node in {1, 20, 21}, 7 polylines (x 2 scenes: 14 * n_node rows fill no workgroup of 256 at n_node 1, more than one at 20 / 21):
    nodes behind, beside and ahead of the first node - the clamp of the projection at 0 (ahead), inside (0, 1) and at 1 (behind) - at
    least half a metre off the first node's axis or more than a metre along it (the closest point's distance is then no cancellation),
    and a node ON the origin (the first node's pose again)."""
    out = {}
    for N in (1, 20, 21):
        g = torch.Generator().manual_seed(2000 + N)
        n, M = 2, 7
        first = torch.cat([_rand(g, n, M, 1, 2, lo=-2e3, hi=2e3), _rand(g, n, M, 1, 1, lo=-math.pi, hi=math.pi)], -1)
        first[0, 0, 0, 2], first[0, 1, 0, 2] = math.pi - 1e-3, -math.pi + 1e-3
        along = _rand(g, n, M, N, lo=-20, hi=20)
        side = _rand(g, n, M, N, lo=0.5, hi=6) * torch.where(torch.rand(n, M, N, generator=g) < 0.5, -1.0, 1.0)
        if N > 3:
            along[:, :, 1], side[:, :, 1] = -0.5, 0.75   # the projection inside (0, 1)
            along[:, :, 2], side[:, :, 2] = -7.0, 0.0    # straight behind: the clamp at 1
            along[:, :, 3], side[:, :, 3] = 7.0, 0.0     # straight ahead: the clamp at 0
        c0, s0 = first[..., 2].double().cos(), first[..., 2].double().sin()
        xy = first[..., :2].double() + torch.stack([along.double() * c0 - side.double() * s0, along.double() * s0 + side.double() * c0], -1)
        pose = torch.cat([xy.to(F32), first[..., 2:] + _rand(g, n, M, N, 1, lo=-0.6, hi=0.6)], -1)
        pose[:, :, 0] = first[:, :, 0]
        if N > 4:
            pose[:, :, 4] = first[:, :, 0]  # a node on the frame's origin
        valid = (torch.rand(n, M, N, generator=g) < 0.8).to(U8)
        valid[0, 2, 0] = 0  # an invalid first node: an invalid token
        out[f"nodes{N}"] = dict(mp_valid=valid, mp_type11=torch.nn.functional.one_hot(torch.randint(0, 11, (n, M), generator=g), 11).to(F32), mp_pose=pose)
    return out


def tl_prep_cases():
    out = {}
    for W in (1, 11, 27):
        for ld in (8, 16, 32, 64):
            if ld < 5 + W:
                continue
            g = torch.Generator().manual_seed(3000 + W + ld)
            n, L = 2, 5
            ht = (1 << torch.randint(0, 5, (n, L, W), generator=g)).to(U8)
            ht[torch.rand(n, L, W, generator=g) < 0.2] = 0xFF
            ht[0, 0, 0] = 0
            out[f"W{W}_ld{ld}"] = dict(hist_tl=ht, tl_invalid=(torch.rand(n, L, generator=g) < 0.3).to(U8), ld_attr=ld)
    return out


def reward_case():
    """Differences at 1 +- 1e-3 and exactly 1 (smooth L1's switch), yaw differences across +-pi."""
    g = torch.Generator().manual_seed(4000)
    n = 300
    pp = torch.cat([_rand(g, n, 2, lo=-48, hi=48), _rand(g, n, 1, lo=-math.pi, hi=math.pi)], -1)
    pm = _rand(g, n, 3, lo=0, hi=15)
    pp[:40], pm[:40] = (pp[:40] * 64).round() / 64, (pm[:40] * 64).round() / 64  # (p + 1 is then exact)
    d = _rand(g, n, 3, lo=-3, hi=3)
    d[:40] = torch.tensor([1.0, -1.0, 1.0]) + torch.tensor([1e-3, -1e-3, 1e-3]) * torch.tensor([[-1.0], [0.0], [1.0], [0.0]]).repeat(10, 1)
    gp, gm = pp + d, pm + _rand(g, n, 3, lo=-2, hi=2)
    gm[:40, 0] = pm[:40, 0] + d[:40, 0]
    pp[40:60, 2], gp[40:60, 2] = math.pi - 0.05, -math.pi + 0.05  # across +-pi
    pp[60:80, 2], gp[60:80, 2] = -math.pi + 1e-3, math.pi - 1e-3
    return dict(pred_valid=(torch.rand(n, generator=g) < 0.8).to(U8), pred_pose=pp, pred_motion=pm, gt_valid=(torch.rand(n, generator=g) < 0.8).to(U8),
                gt_pose=gp, gt_motion=gm, w_pos=0.1, w_rot=10.0, w_spd=0.1)


PREP_GROUPS = {"pe": "pe", "navi_pose3": "navi"}
MAP_GROUPS = {"pe": "map_pe"}


def check_rows(got, ref, groups, stats, what, c_of=C):
    """Rows of a preparation kernel (or of another evaluation of the reference) against the reference's: the floats named in `groups`
    within c * 2^-23 * scale (capped), everything else - copies, one-hots, masks, row indices - equal. -> the list of mismatches."""
    bad = []
    for name, r in ref.items():
        if name.endswith("__scale") or name == "proj":
            continue
        g = got[name]
        if name in groups:
            bad += _float_check(name, g.reshape(r.shape), r, ref[name + "__scale"], groups[name], None, stats, what, c_of)
        elif not torch.equal(g.reshape(r.shape).double(), r.double()):
            bad.append(f"{what} {name}: {int((g.reshape(r.shape).double() != r.double()).sum())} entries differ")
    return bad
