"""REFERENCE (test infrastructure, not product): the closed-loop step and the per-step feature preparation as plain vectorised torch,
float64 on the CPU - what tbx_sim_step, tbx_agent_prep / tbx_tl_prep / tbx_map_prep and tbx_diffbar_reward (include/tbx_hip.h) compute.

Written from the statements that oracle/trafficbots_oracle.py restates (Sim.rollout's loop body, Sim.feedback_checks, _append_hist,
ag_encoder's and mp_encoder's input rows), not from the kernels: no lanes, no chunks, no split of the nodes. Float inputs of any type are
promoted to `dtype` (float64; float32 gives the yardstick of the tolerances: the same statements in the kernels' own precision), byte masks
are read as the header documents them (0 = false; tl state = 5-bit mask, 0xFF in a window = missing step).

Every float output comes with its `scale` - the sum of the magnitudes of the terms added to form it (1 + |argument| for a pose-embedding
element) - so that a test bounds the error by c * 2^-23 * scale (the convention of test_hip_sampled_actions._check_log_prob).

`defects`: names of deliberate mistakes (DEFECTS), injected HERE only, for test_inputs_discriminate_the_defects: each of them must be
visible in what the GPU tests compare.
"""
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as Fn

from oracle import hptr_ops as H

AGENTS, LIGHTS, ADVANCE, NO_DISABLE, NO_APPEND, APPEND = 1, 2, 4, 8, 16, 32
COS30 = math.cos(math.radians(30))
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)
FLT_EPSILON = 2.0 ** -23

DEFECTS = (
    "nodes32",          # destination nodes >= 32 ignored
    "win33",            # window entries from 32 on keep their old content (their sources, entries >= 33, are not shifted)
    "tlwin8",           # the light window's entry 8 not shifted
    "ov_disabled",      # the override applied to disabled agents
    "dis_ignore_gt",    # disable ignoring gt_valid
    "dis_past_gt",      # past n_step_gt the disable behaves as if ground truth were valid
    "reach_post",       # reach decided on the post-override pose
    "kind2_rot",        # dest_kind bit 1 requiring rot_ok
    "navi_nodisable",   # navi_valid cleared under NO_DISABLE
    "valid_post",       # out_valid logged after the override
    "reward_post",      # the reward taken on the post-override state
    "nll_argmax",       # NLL against the argmax instead of the ground truth
    "nll_past",         # NLL not zero past n_step_tl_gt
    "tie_last",         # a tie resolved to the last index
    "player_invalid",   # the player action applied to invalid agents
    "no_eps",           # sampled std * eps dropped
    "last_step",        # agent_rows taking the last step instead of the last valid step
    "win64",            # agent_rows reading 0 for window floats at index >= 64
    "dest_tok_frame",   # the destination's pose relative to the token pose instead of the current pose
    "no_batch_div",     # mp_batch_div ignored
    "no_clamp",         # map_rows without the clamp
)

STATE_KEYS = ("ag_valid", "ag_disabled", "ag_pose", "ag_motion", "navi_valid", "outside_map", "dest_reached", "tl_state", "hist_valid",
              "hist_pose", "hist_motion", "hist_tl", "now_outside", "now_reached")


def _c32(v, dtype):
    """A constant that crosses the C ABI as float: rounded to float32 first."""
    return torch.tensor(v, dtype=torch.float32).to(dtype)


def _append(hist, new):
    return torch.cat([hist[:, :, 1:], new.unsqueeze(2)], 2)


def _agents(S, t, parts, action_mean, eps, dtype, D):
    F = lambda x: x.to(dtype)
    n, A, W = S["hist_valid"].shape
    n_gt = S["gt_valid"].shape[2]
    valid0, dis0, reached0 = S["ag_valid"] != 0, S["ag_disabled"] != 0, S["dest_reached"] != 0
    pose0, mot0 = F(S["ag_pose"]), F(S["ag_motion"])
    ty = S["ag_type_idx"].long()
    lim = torch.stack([_c32(S["max_acc"], dtype)[ty], _c32(S["max_yaw_rate"], dtype)[ty]], -1)
    dt = _c32(S["dt"], dtype)
    inv1 = ~valid0.unsqueeze(-1)
    log, scale = {}, {}
    # Dynamics.update_ag + MultiPathPP
    mean = F(action_mean).view(n, A, 2)
    um = mean
    if eps is not None:
        ls, e = _c32(S["act_log_std"], dtype)[ty], F(eps).view(n, A, 2)
        if "no_eps" not in D:
            um = mean + ls.exp() * e
        log["out_act_log_prob"] = (-(0.5 * e * e + ls + LOG_SQRT_2PI).sum(-1)).masked_fill(~valid0, 0)
        scale["out_act_log_prob"] = (0.5 * e * e).sum(-1) + ls.abs().sum(-1) + 2 * LOG_SQRT_2PI
    action = (torch.tanh(um) * lim).masked_fill(inv1, 0)
    if S.get("player_valid") is not None:
        pm = S["player_valid"] != 0
        if "player_invalid" not in D:
            pm = pm & valid0
        action = torch.where(pm.unsqueeze(-1), F(S["player_action"]), action)
    acc, yr = action[..., 0], action[..., 1]
    v_t = mot0[..., 0] + 0.5 * dt * acc
    th_t = pose0[..., 2] + 0.5 * dt * yr
    new_pose = pose0 + dt * torch.stack([v_t * torch.cos(th_t), v_t * torch.sin(th_t), yr], -1)
    new_motion = torch.stack([mot0[..., 0] + dt * acc, acc, yr], -1)
    pred_pose, pred_motion = new_pose.masked_fill(inv1, 0), new_motion.masked_fill(inv1, 0)
    s_xy = dt * (mot0[..., 0].abs() + 0.5 * dt * acc.abs())
    s_act = lim * (1 + um.abs())
    s_pose = torch.stack([pose0[..., 0].abs() + s_xy, pose0[..., 1].abs() + s_xy, pose0[..., 2].abs() + dt * yr.abs()], -1)
    s_motion = torch.stack([mot0[..., 0].abs() + dt * acc.abs(), s_act[..., 0], s_act[..., 1]], -1)
    # TeacherForcing.get + override_ag
    has_gt = t < n_gt
    if S.get("ov_valid") is not None:
        tf_now, ov_pose, ov_motion = S["ov_valid"] != 0, F(S["ov_pose"]), F(S["ov_motion"])
    elif has_gt:
        tf_now, ov_pose, ov_motion = S["tf_mask"][:, :, t] != 0, F(S["gt_pose"][:, :, t]), F(S["gt_motion"][:, :, t])
    else:
        tf_now, ov_pose, ov_motion = torch.zeros_like(valid0), torch.zeros_like(pose0), torch.zeros_like(mot0)
    ov = tf_now if "ov_disabled" in D else tf_now & ~dis0
    valid = valid0 | ov
    ov1 = ov.unsqueeze(-1)
    pose, motion = torch.where(ov1, ov_pose, pred_pose), torch.where(ov1, ov_motion, pred_motion)
    # the two rule checks that feed back, on the prediction
    chk_pose = pose if "reach_post" in D else pred_pose
    x, y = pred_pose[..., 0], pred_pose[..., 1]
    bnd = F(S["boundary"])
    out_now = ((x > bnd[:, [1]]) | (x < bnd[:, [0]]) | (y > bnd[:, [3]]) | (y < bnd[:, [2]])) & valid0
    m_bnd = torch.stack([(x - bnd[:, [1]]).abs(), (x - bnd[:, [0]]).abs(), (y - bnd[:, [3]]).abs(), (y - bnd[:, [2]]).abs()], -1).amin(-1)
    d_inv = S["dest_invalid"] != 0
    if "nodes32" in D:
        d_inv = d_inv.clone()
        d_inv[:, :, 32:] = True
    dd = torch.norm(chk_pose[:, :, None, :2] - F(S["dest_pos"]), dim=-1).masked_fill(d_inv, float("inf"))
    thresh = F(S["dest_thresh"])
    pos_ok = (dd < thresh.unsqueeze(-1)).any(-1)
    hf = torch.stack([torch.cos(chk_pose[..., 2]), torch.sin(chk_pose[..., 2])], -1)
    rot = (hf.unsqueeze(2) * F(S["dest_dir"])).sum(-1).masked_fill(d_inv, 0)
    rot_ok = (rot > COS30).any(-1)
    kind = S["dest_kind"]
    k_lane, k_edge = (kind & 1) != 0, (kind & 2) != 0
    edge_ok = pos_ok & rot_ok if "kind2_rot" in D else pos_ok
    reach_now = ~reached0 & valid0 & ((k_lane & pos_ok & rot_ok) | (k_edge & edge_ok))
    # float64 margins of the thresholded decisions (inf where the decision cannot matter)
    inf = torch.full_like(m_bnd, float("inf"))
    live = valid0 & ~reached0
    m_dist = torch.where(live & (k_lane | k_edge), (dd.amin(-1) - thresh).abs(), inf)
    m_dot = torch.where(live & k_lane & ~d_inv.all(-1), (rot.masked_fill(d_inv, -2.0).amax(-1) - COS30).abs(), inf)
    margins = {"bnd": torch.where(valid0, m_bnd, inf), "dist": m_dist, "dot": m_dot}
    # disable_ag / disable_navi
    g_valid = S["gt_valid"][:, :, t] != 0 if has_gt else torch.zeros_like(valid0)
    no_disable = bool(parts & NO_DISABLE)
    if "dis_ignore_gt" in D:
        dis = out_now
    elif "dis_past_gt" in D and not has_gt:
        dis = torch.zeros_like(out_now)
    else:
        dis = out_now & ~g_valid
    if no_disable:
        dis = torch.zeros_like(dis)
    new = {"ag_valid": valid & ~dis, "ag_disabled": dis0 | dis, "ag_pose": pose, "ag_motion": motion,
           "outside_map": (S["outside_map"] != 0) | out_now, "dest_reached": reached0 | reach_now,
           "navi_valid": (S["navi_valid"] != 0) & ~reach_now if (not no_disable or "navi_nodisable" in D) else S["navi_valid"] != 0}
    scale["ag_pose"], scale["ag_motion"] = torch.where(ov1, ov_pose.abs(), s_pose), torch.where(ov1, ov_motion.abs(), s_motion)
    if S.get("now_outside") is not None:
        new["now_outside"], new["now_reached"] = out_now, reach_now
    if not parts & NO_APPEND:
        hv, hp, hm = _append(S["hist_valid"] != 0, new["ag_valid"]), _append(F(S["hist_pose"]), pose), _append(F(S["hist_motion"]), motion)
        if "win33" in D and W > 33:
            hv[:, :, 32:W - 1], hp[:, :, 32:W - 1], hm[:, :, 32:W - 1] = (S["hist_valid"] != 0)[:, :, 32:W - 1], F(S["hist_pose"])[:, :, 32:W - 1], F(S["hist_motion"])[:, :, 32:W - 1]
        new["hist_valid"], new["hist_pose"], new["hist_motion"] = hv, hp, hm
        scale["hist_pose"], scale["hist_motion"] = _append(F(S["hist_pose"]).abs(), scale["ag_pose"]), _append(F(S["hist_motion"]).abs(), scale["ag_motion"])
    # the log column
    log.update(out_valid=(valid if "valid_post" in D else valid0), out_pose=pred_pose, out_motion=pred_motion, out_action=action,
               out_outside_map=new["outside_map"], out_dest_reached=new["dest_reached"])
    scale.update(out_pose=s_pose, out_motion=s_motion, out_action=s_act)
    if S.get("out_tf") is not None:
        log["out_tf"] = tf_now
    if eps is not None:
        log["out_act_noise"] = F(eps).view(n, A, 2)
        scale["out_act_noise"] = log["out_act_noise"].abs()
    if S.get("out_reward") is not None:
        r_pose, r_motion = (pose, motion) if "reward_post" in D else (pred_pose, pred_motion)
        if has_gt:
            gp, gm = F(S["gt_pose"][:, :, t]), F(S["gt_motion"][:, :, t])
            r4, r_valid, s4 = reward(valid0, r_pose, r_motion, g_valid, gp, gm, S["w_pos"], S["w_rot"], S["w_spd"], dtype, s_pose, s_motion[..., 0])
        else:
            r4, r_valid, s4 = reward(valid0, r_pose, r_motion, None, None, None, S["w_pos"], S["w_rot"], S["w_spd"], dtype)
        log["out_reward"], scale["out_reward"] = r4, s4
        if S.get("out_reward_valid") is not None:
            log["out_reward_valid"] = r_valid
    return new, log, scale, margins


def reward(pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion, w_pos, w_rot, w_spd, dtype=torch.float64, s_pose=None, s_spd=None):
    """DifferentiableReward.get for one step, default configuration (Sim.rollout's reward lines; tbx_diffbar_reward) ->
    (out4 [..., 4] = pos, rot, spd, (pos + rot) + spd; valid [...] bool; scale [..., 4]). gt_valid None: valid = pred_valid, all terms 0.
    s_pose / s_spd: the scales of a prediction that was itself computed (tbx_sim_step); given inputs count with their magnitude."""
    F = lambda x: x.to(dtype)
    pv = pred_valid != 0
    pp, pm = F(pred_pose), F(pred_motion)
    if gt_valid is None:
        z = torch.zeros(*pv.shape, 4, dtype=dtype)
        return z, pv, z.clone()
    gp, gm = F(gt_pose), F(gt_motion)
    s_pose = pp.abs() if s_pose is None else s_pose
    s_spd = pm[..., 0].abs() if s_spd is None else s_spd
    wp, wr, ws = _c32(w_pos, dtype), _c32(w_rot, dtype), _c32(w_spd, dtype)
    r_valid = pv & (gt_valid != 0)
    e_xy = Fn.smooth_l1_loss(gp[..., :2], pp[..., :2], reduction="none")
    e_rot = 0.5 * (1 - torch.cos(gp[..., 2] - pp[..., 2]))
    e_spd = Fn.smooth_l1_loss(gm[..., 0], pm[..., 0], reduction="none")
    r = torch.stack([-wp * e_xy.sum(-1), -wr * e_rot, -ws * e_spd], -1).masked_fill(~r_valid.unsqueeze(-1), 0)
    s = torch.stack([wp * (e_xy + gp[..., :2].abs() + s_pose[..., :2]).sum(-1), wr * 0.5 * (2 + gp[..., 2].abs() + s_pose[..., 2]),
                     ws * (e_spd + gm[..., 0].abs() + s_spd)], -1)
    r4 = torch.cat([r, ((r[..., 0] + r[..., 1]) + r[..., 2]).unsqueeze(-1)], -1)
    return r4, r_valid, torch.cat([s, s.sum(-1, keepdim=True)], -1)


def _lights(S, t, parts, tl_logits, dtype, D):
    F = lambda x: x.to(dtype)
    n, L, W = S["hist_tl"].shape
    n_tl_gt = S["tl_gt"].shape[2]
    lg = F(tl_logits).view(n, L, 5)
    is_max, idx = lg == lg.amax(-1, keepdim=True), torch.arange(5).expand(n, L, 5)
    am = torch.where(is_max, idx, 5).amin(-1)  # argmax: the first maximum
    if "tie_last" in D:
        am = torch.where(is_max, idx, -1).amax(-1)
    st = (1 << am).to(torch.uint8)
    if S.get("ov_valid") is not None:
        st = torch.where(S["ov_tl_valid"] != 0, S["ov_tl_state"], st)
    elif t < n_tl_gt:
        st = S["tl_gt"][:, :, t].clone()
    new, log, scale = {"tl_state": st}, {"out_tl_state": st}, {}
    if S.get("out_tl_nll") is not None:
        lse = torch.logsumexp(lg, -1)
        if t < n_tl_gt and "nll_argmax" not in D:
            gm = S["tl_gt"][:, :, t].long()
            bits = torch.stack([(gm >> c) & 1 for c in range(8)], -1)
            gi = bits.argmax(-1)  # lowest set bit, 0 for an empty mask (the argmax of the all-false one-hot)
            gi = torch.where(gi < 5, gi, torch.zeros_like(gi))
            nll = lse - lg.gather(-1, gi.unsqueeze(-1)).squeeze(-1)
        elif t < n_tl_gt or "nll_past" in D:
            gi = am
            nll = lse - lg.gather(-1, gi.unsqueeze(-1)).squeeze(-1)
        else:
            gi, nll = am, torch.zeros_like(lse)
        best = lg.amax(-1)
        log["out_tl_nll"] = nll
        scale["out_tl_nll"] = best.abs() + (lse - best) + lg.gather(-1, gi.unsqueeze(-1)).squeeze(-1).abs() + (lg.abs() + best.abs().unsqueeze(-1)).amax(-1)
    if not parts & NO_APPEND:
        ht = _append(S["hist_tl"], st)
        if "tlwin8" in D and W > 8:
            ht[:, :, 8] = S["hist_tl"][:, :, 8]
        new["hist_tl"] = ht
    return new, log, scale


def step(S: Dict, action_mean, tl_logits, parts: int = AGENTS | LIGHTS | ADVANCE, eps: Optional[torch.Tensor] = None,
         dtype=torch.float64, defects=()):
    """One launch of tbx_sim_step(parts) on the state S: a dict of CPU tensors named like tbx_sim_state_t's fields (sizes are the
    tensors' shapes; optional fields absent or None = off; max_acc / max_yaw_rate / dt / w_* / act_log_std as Python numbers), S["step"] =
    the device counter [t, 0]. eps [n, A, 2]: the step's noise, given (sampled actions).
    -> new: the state tensors the launch rewrites (masks as bool, floats in `dtype`, "step" as [t', 0]),
       log: the column t - 1 of every out_* the launch writes ({} once t - 1 >= n_step_out),
       scale: per float tensor of new / log, the sum of magnitudes its error bound is relative to,
       margins: float64 distance of every thresholded decision from its threshold, [n, A] each: "bnd", "dist", "dot"."""
    D = frozenset(defects)
    assert not D - set(DEFECTS), D - set(DEFECTS)
    t = int(S["step"][0])
    T = S["out_valid"].shape[2]
    new, log, scale, margins = {}, {}, {}, {}
    if parts == APPEND:
        new["hist_valid"] = _append(S["hist_valid"] != 0, S["ag_valid"] != 0)
        new["hist_pose"], new["hist_motion"] = _append(S["hist_pose"].to(dtype), S["ag_pose"].to(dtype)), _append(S["hist_motion"].to(dtype), S["ag_motion"].to(dtype))
        new["hist_tl"] = _append(S["hist_tl"], S["tl_state"])
        scale["hist_pose"], scale["hist_motion"] = new["hist_pose"].abs(), new["hist_motion"].abs()
        return new, log, scale, margins
    if parts & AGENTS:
        new, log, scale, margins = _agents(S, t, parts, action_mean, eps, dtype, D)
    if parts & LIGHTS:
        n2, l2, s2 = _lights(S, t, parts, tl_logits, dtype, D)
        new.update(n2), log.update(l2), scale.update(s2)
    if t - 1 >= T:
        log = {}
    new["step"] = torch.tensor([t + 1 if parts & ADVANCE else t, 0], dtype=torch.int32)
    return new, log, scale, margins


def agent_rows(hist_valid, hist_pose, hist_motion, ag_attr6, ag_type_idx, freqs_xy, freqs_yaw, pe_dim, dest=None, mp_tok_pose=None,
               mp_batch_div=1, dtype=torch.float64, defects=()):
    """What tbx_agent_prep writes: ag_encoder's token pose ("last_valid"), attribute rows, pose embeddings in the token frame, the type
    masks of the action head and navi_encoder's relative pose of the destination. hist_* [n, A, W, ..]; mp_tok_pose [n / div, M, 3]."""
    D = frozenset(defects)
    F = lambda x: x.to(dtype)
    n, A, W = hist_valid.shape
    valid = hist_valid != 0
    pose, motion = F(hist_pose), F(hist_motion)
    if "win64" in D:
        keep = (torch.arange(W * 3) < 64).view(W, 3)
        pose, motion = pose * keep, motion * keep
    inv = ~valid
    tok_inv = ~valid.any(-1)
    tok_pose = H.seq_pool(pose, inv, "last" if "last_step" in D else "last_valid")
    d_xy = pose[..., :2] - tok_pose[:, :, None, :2]
    xy = H.rot_local(d_xy, tok_pose[..., 2])
    yaw = pose[..., 2] - tok_pose[:, :, None, 2]
    attr = torch.cat([F(ag_attr6)[:, :, None].expand(-1, -1, W, -1), motion, torch.eye(W, dtype=dtype).expand(n, A, -1, -1),
                      torch.zeros(n, A, W, 32 - 9 - W, dtype=dtype)], -1)
    fx, fy = F(freqs_xy)[: pe_dim // 4], F(freqs_yaw)[: pe_dim // 2]
    pe = H.pe_xy_yaw(xy, yaw, fx, fy)
    arg = torch.cat([xy[..., [0]] * fx[::2], xy[..., [1]] * fx[::2], yaw.unsqueeze(-1) * fy[::2]], -1).abs()
    nxy, nyw = pe_dim // 8, pe_dim // 4
    s_pe = 1 + torch.cat([arg[..., :nxy], arg[..., :nxy], arg[..., nxy:2 * nxy], arg[..., nxy:2 * nxy], arg[..., 2 * nxy:], arg[..., 2 * nxy:]], -1)
    out = {"tok_pose": tok_pose, "tok_invalid": tok_inv, "attr": attr.reshape(n * A * W, 32), "pe": pe.reshape(n * A * W, pe_dim),
           "row_invalid": inv.reshape(-1), "pe__scale": s_pe.reshape(n * A * W, pe_dim)}
    if ag_type_idx is not None:
        ty = ag_type_idx.long()
        out["type_mask"] = torch.stack([~((ty == i) & valid[:, :, -1]) for i in range(3)], 0).reshape(3, n * A)
    if dest is not None:
        M = mp_tok_pose.shape[1]
        b_map = torch.arange(n) // mp_batch_div if "no_batch_div" not in D else torch.arange(n).clamp(max=mp_tok_pose.shape[0] - 1)
        gp = F(mp_tok_pose)[b_map.unsqueeze(1), dest]
        cur = tok_pose if "dest_tok_frame" in D else pose[:, :, -1]
        d = gp[:, :, None, :2] - cur[:, :, None, :2]
        nxy_ = H.rot_local(d, cur[:, :, 2]).squeeze(2)
        out["navi_pose3"] = torch.cat([nxy_, (gp[:, :, 2] - cur[:, :, 2]).unsqueeze(-1)], -1).reshape(n * A, 3)
        s_d = d.abs().sum(-1).squeeze(2)
        out["navi_pose3__scale"] = torch.stack([s_d, s_d, gp[:, :, 2].abs() + cur[:, :, 2].abs()], -1).reshape(n * A, 3)
        out["navi_row"] = (b_map.unsqueeze(1) * M + dest).reshape(-1).to(torch.int32)
    return out


def tl_rows(hist_tl, tl_invalid, ld_attr, dtype=torch.float64):
    """What tbx_tl_prep (and the rows riding on tbx_sim_step) write: tl_encoder's input rows, one-hot5(state) | one-hot_W(position) | 0."""
    n, L, W = hist_tl.shape
    missing = hist_tl == 0xFF
    state = torch.stack([((hist_tl >> c) & 1) != 0 for c in range(5)], -1) & ~missing.unsqueeze(-1)
    attr = torch.cat([state.to(dtype), torch.eye(W, dtype=dtype).expand(n, L, -1, -1), torch.zeros(n, L, W, ld_attr - 5 - W, dtype=dtype)], -1)
    return {"attr": attr.reshape(n * L * W, ld_attr), "row_invalid": (missing | (tl_invalid != 0).view(n, L, 1)).reshape(-1)}


def mpa_pl(pos, yaw, eps, clamp=True):
    """utils/pose_emb.py's 7-d MultiPath++ polyline feature as hptr_ops.mpa_pl states it, with the epsilon as an argument (the kernel's
    FLT_EPSILON is part of the operation; hptr_ops.mpa_pl would take float64's on float64 input) -> (feature [..., 7], the projection
    before the clamp [...], the distance of the closest point [..., 1])."""
    dirv = torch.cat([yaw.cos(), yaw.sin()], -1)
    proj = (-pos * dirv).sum(-1) / ((dirv * dirv).sum(-1) + eps)
    closest = pos + (torch.clamp(proj, min=0, max=1) if clamp else proj).unsqueeze(-1) * dirv
    r = torch.norm(closest, dim=-1, keepdim=True)
    dn = torch.norm(dirv, dim=-1, keepdim=True)
    return torch.cat([r, closest / (r + eps), dirv / (dn + eps), dn, torch.norm(pos + dirv - closest, dim=-1, keepdim=True)], -1), proj, r


def map_rows(mp_valid, mp_type11, mp_pose, eps=FLT_EPSILON, dtype=torch.float64, defects=()):
    """What tbx_map_prep writes: mp_encoder's token pose (first node), attribute rows and the polyline feature | 0 of every node."""
    D = frozenset(defects)
    F = lambda x: x.to(dtype)
    valid, pose = mp_valid != 0, F(mp_pose)
    n, M, N = valid.shape
    tok_pose, tok_inv = pose[:, :, 0], ~valid[:, :, 0]
    pos = H.rot_local(pose[..., :2] - tok_pose[:, :, None, :2], tok_pose[..., 2])
    yaw = pose[..., 2:3] - tok_pose[:, :, None, 2:3]
    feat, proj, r = mpa_pl(pos, yaw, eps, clamp="no_clamp" not in D)
    pe = torch.cat([feat, torch.zeros_like(r)], -1)
    mag = (1 + pos.abs().sum(-1, keepdim=True)) * (1 + yaw.abs())  # the terms of the rotated offset and of its projection
    s = torch.cat([mag, (mag / (r + eps)).expand(-1, -1, -1, 2), (1 + yaw.abs()).expand(-1, -1, -1, 3), mag, torch.ones_like(r)], -1)
    attr = torch.cat([F(mp_type11)[:, :, None].expand(-1, -1, N, -1), torch.eye(N, dtype=dtype).expand(n, M, -1, -1),
                      torch.zeros(n, M, N, 32 - 11 - N, dtype=dtype)], -1)
    return {"attr": attr.reshape(-1, 32), "pe": pe.reshape(-1, 8), "pe__scale": s.reshape(-1, 8), "row_invalid": (~valid).reshape(-1),
            "tok_pose": tok_pose, "tok_invalid": tok_inv, "proj": proj}
