"""ctypes binding of libtbx_hip.so (include/tbx_hip.h and the topical tbx_hip_*.h headers it includes) + the `Chain` builder for tbx_rowchain programs.

The HIP library IS the product path: there is no CPU or PyTorch fallback. `load()` raises if the shared object is
missing, and every wrapper raises on a non-zero tbx return code or on tensors that are not on a HIP device.
"""
import ctypes as C
import os
import re
from pathlib import Path
from typing import List, Optional, Sequence

import torch

from . import abi, hip_base
from .abi import *  # noqa: F401,F403  (constants, structures, load, declared_symbols: the C-ABI mirror)
from .abi import AGGR_LIB_PATH, GRAD_LIB_PATH, HEADER_PATH, IL_LIB_PATH, LIB_PATH, SUB_LIB_PATH, load, load_aggr, load_grad, load_il, load_sub  # noqa: F401
from .hip_base import *  # noqa: F401,F403  (Seg, stream_ptr, packed_weight / stacked_linear / padded_weight)
from .hip_base import _attn_args, _check, _cptr, _fill_drop, _ptr  # noqa: F401
from .hip_chain import *  # noqa: F401,F403  (Chain, group_tile_rows)
from .hip_rules import *  # noqa: F401,F403  (rule_tables, rule_check, rule_accumulate, filter_futures, womd_modes, womd_aggr, pose_to_global, rollout_metrics)
from .hip_train import *  # noqa: F401,F403  (the training entry points)


# ------------------------------------------------------------------------------------------------ wrappers
def knn_embed(src_pose, src_invalid, tgt_pose, tgt_invalid, k: int, dist_limit: float, freqs_xy=None, freqs_yaw=None,
              pe_dim: int = 128, tgt_batch_div: int = 1, want_rel_pose: bool = False, want_emb: bool = True, out=None):
    """-> idx i32 [n,S,k], invalid u8 [n,S,k], rel_pose f32 [n,S,k,3] | None, emb f32 [n,S,k,pe_dim] | None.
    out = (idx, invalid, rel_pose) of a previous call: written in place (buffers shared across streams / steps)."""
    n, S, _ = src_pose.shape
    T = tgt_pose.shape[1]
    dev = src_pose.device
    if out is not None:
        idx, inv, rel = out
        assert idx.shape == (n, S, k) and inv.shape == (n, S, k) and (rel is not None) == want_rel_pose
    else:
        idx = torch.empty(n, S, k, dtype=torch.int32, device=dev)
        inv = torch.empty(n, S, k, dtype=torch.uint8, device=dev)
        rel = torch.empty(n, S, k, 3, dtype=torch.float32, device=dev) if want_rel_pose else None
    emb = torch.empty(n, S, k, pe_dim, dtype=torch.float32, device=dev) if want_emb else None
    rc = load().tbx_knn_embed(_cptr(src_pose, torch.float32), _cptr(src_invalid, torch.uint8), _cptr(tgt_pose, torch.float32),
                              _cptr(tgt_invalid, torch.uint8), n, S, T, tgt_batch_div, k, float(dist_limit), _ptr(idx),
                              _ptr(inv), _ptr(rel), _ptr(emb), _cptr(freqs_xy), _cptr(freqs_yaw), pe_dim, stream_ptr())
    _check(rc, "tbx_knn_embed")
    return idx, inv, rel, emb


def knn_embed_multi(jobs, freqs_xy=None, freqs_yaw=None, pe_dim: int = 128, pose_embed_job=None):
    """Several `knn_embed` searches in one launch. jobs: dicts with knn_embed's arguments (src_pose, src_invalid, tgt_pose,
    tgt_invalid, k, dist_limit, tgt_batch_div, want_rel_pose, want_emb, out) -> list of (idx, invalid, rel_pose, emb).
    pose_embed_job = dict(pose3, freqs_xy, freqs_yaw, pe_dim, out[, col_off]): a `pose_embed` in the same launch."""
    outs, cj = _knn_jobs(jobs, pe_dim)
    pj = _pose_job(pose_embed_job) if pose_embed_job is not None else None
    _check(load().tbx_knn_embed_multi(cj, len(jobs), _cptr(freqs_xy), _cptr(freqs_yaw), pe_dim, pj, stream_ptr()), "tbx_knn_embed_multi")
    return outs


def _pose_job(q) -> "PoseEmbedJob":
    out = q["out"]
    return PoseEmbedJob(_cptr(q["pose3"], torch.float32), _cptr(q["freqs_xy"]), _cptr(q["freqs_yaw"]), _ptr(out, torch.float32),
                        q["pose3"].numel() // 3, int(q["pe_dim"]), out.stride(0), int(q.get("col_off", 0)), 0)


def _knn_jobs(jobs, pe_dim: int = 128):
    """-> ([(idx, invalid, rel_pose, emb)], tbx_knn_job_t array) for knn_embed_multi's job dicts."""
    outs, cj = [], (KnnJob * len(jobs))()
    for j, q in enumerate(jobs):
        n, S, _ = q["src_pose"].shape
        T, k, dev = q["tgt_pose"].shape[1], q["k"], q["src_pose"].device
        want_rel, want_emb = q.get("want_rel_pose", False), q.get("want_emb", True)
        if q.get("out") is not None:
            idx, inv, rel = q["out"]
            assert idx.shape == (n, S, k) and inv.shape == (n, S, k) and (rel is not None) == want_rel
        else:
            idx = torch.empty(n, S, k, dtype=torch.int32, device=dev)
            inv = torch.empty(n, S, k, dtype=torch.uint8, device=dev)
            rel = torch.empty(n, S, k, 3, dtype=torch.float32, device=dev) if want_rel else None
        emb = torch.empty(n, S, k, pe_dim, dtype=torch.float32, device=dev) if want_emb else None
        cj[j] = KnnJob(_cptr(q["src_pose"], torch.float32), _cptr(q["src_invalid"], torch.uint8), _cptr(q["tgt_pose"], torch.float32),
                       _cptr(q["tgt_invalid"], torch.uint8), _ptr(idx), _ptr(inv), _ptr(rel), _ptr(emb), n, S, T,
                       q.get("tgt_batch_div", 1), k, float(q["dist_limit"]))
        outs.append((idx, inv, rel, emb))
    return outs, cj


def rel_pose_dense(src_pose, src_invalid, tgt_pose, tgt_invalid, tgt_batch_div: int = 1, want_rel_pose: bool = True, want_dist: bool = True):
    """utils/rpe.py:8-58 as dense tensors -> rel_pose f32 [n,S,T,3] | None, rel_dist f32 [n,S,T] | None (+inf on invalid pairs)."""
    n, S, _ = src_pose.shape
    T = tgt_pose.shape[1]
    dev = src_pose.device
    rel = torch.empty(n, S, T, 3, dtype=torch.float32, device=dev) if want_rel_pose else None
    dist = torch.empty(n, S, T, dtype=torch.float32, device=dev) if want_dist else None
    _check(load().tbx_rel_pose_dense(_cptr(src_pose, torch.float32), _cptr(src_invalid, torch.uint8), _cptr(tgt_pose, torch.float32),
                                     _cptr(tgt_invalid, torch.uint8), n, S, T, tgt_batch_div, _ptr(rel), _ptr(dist), stream_ptr()),
           "tbx_rel_pose_dense")
    return rel, dist


def diffbar_reward(pred_valid, pred_pose, pred_motion, gt_valid, gt_pose, gt_motion, w_pos: float, w_rot: float, w_spd: float):
    """utils/rewards.py:35-85 for one step -> (out4 f32 [..., 4] = pos, rot, spd, sum; valid u8 [...]). gt_valid None: no imitation terms."""
    n = pred_valid.numel()
    out4 = torch.empty(*pred_valid.shape, 4, dtype=torch.float32, device=pred_pose.device)
    ov = torch.empty(pred_valid.shape, dtype=torch.uint8, device=pred_pose.device)
    has_gt = gt_valid is not None
    _check(load().tbx_diffbar_reward(_cptr(pred_valid, torch.uint8), _cptr(pred_pose, torch.float32), _cptr(pred_motion, torch.float32),
                                     _cptr(gt_valid, torch.uint8) if has_gt else None, _cptr(gt_pose, torch.float32) if has_gt else None,
                                     _cptr(gt_motion, torch.float32) if has_gt else None, n, float(w_pos), float(w_rot), float(w_spd),
                                     _ptr(out4), _ptr(ov), stream_ptr()), "tbx_diffbar_reward")
    return out4, ov


def pose_embed(pose3, freqs_xy, freqs_yaw, pe_dim: int, out=None, col_off: int = 0):
    n = pose3.numel() // 3
    if out is None:
        out = torch.empty(n, pe_dim, dtype=torch.float32, device=pose3.device)
    rc = load().tbx_pose_embed(_cptr(pose3, torch.float32), n, _cptr(freqs_xy), _cptr(freqs_yaw), pe_dim, _ptr(out),
                               out.stride(0), col_off, stream_ptr())
    _check(rc, "tbx_pose_embed")
    return out


def knarpe_attn(qbuf, q_off: int, qt_off: int, rpe_k_bias, n_batch: int, n_src: int, segs: Sequence[Seg], out, row_no_valid,
                freqs_xy=None, freqs_yaw=None, drop=None, fold=None):
    """tbx_knarpe_attn_fwd. drop = None, or (p, seed int64[1] device tensor, call id[, time_batch, time0]): attention-probability
    dropout (training; the last two for time-batched calls, include/tbx_hip.h).
    fold = the tbx_pack_weight_gemv image of linear_rpe's value half (tbx_attn_t.fold_image): `out` is then [rows, >= 128]."""
    assert fold is None or drop is None
    a = _attn_args(qbuf, q_off, qt_off, rpe_k_bias, n_batch, n_src, segs, (freqs_xy, freqs_yaw), drop)
    a.out, a.ldo, a.row_no_valid, a.fold_image = _ptr(out, torch.float32), out.stride(0), _ptr(row_no_valid, torch.uint8), _ptr(fold, torch.float32)
    _check(load().tbx_knarpe_attn_fwd(C.byref(a), stream_ptr()), "tbx_knarpe_attn_fwd")


def knarpe_attn_form(qbuf, q_off: int, qt_off: int, rpe_k_bias, n_batch: int, n_src: int, segs: Sequence[Seg], out, row_no_valid,
                     freqs_xy=None, freqs_yaw=None, drop=None, fold=None) -> int:
    """tbx_knarpe_attn_fwd_form for knarpe_attn's arguments: the ATTN_FORM_* code (form | flags) of the kernel that call would launch,
    or the negative tbx code it would raise on. Nothing is launched and no tensor is read: host tensors of the call's shapes will do
    (no GPU needed)."""
    hip_base._HOST_PTRS = True
    try:
        a = _attn_args(qbuf, q_off, qt_off, rpe_k_bias, n_batch, n_src, segs, (freqs_xy, freqs_yaw), drop)
        a.out, a.ldo, a.row_no_valid, a.fold_image = _ptr(out, torch.float32), out.stride(0), _ptr(row_no_valid, torch.uint8), _ptr(fold, torch.float32)
    finally:
        hip_base._HOST_PTRS = False
    return int(load().tbx_knarpe_attn_fwd_form(C.byref(a)))


def knarpe_attn_mfma(qbuf, q_off: int, qt_off: int, n_batch: int, n_src: int, segs: Sequence[Seg], out, row_no_valid, freqs_xy, freqs_yaw,
                     drop=None):
    """tbx_knarpe_attn_fwd_mfma: the wave-per-row forward on the bf16 matrix cores (bf16 operands, fp32 accumulation / softmax).
    Same `out` [rows, >= 640] / row_no_valid as knarpe_attn; segments in the relative-pose form. drop: as knarpe_attn's (training:
    the same mask as the VALU kernels draw for that key)."""
    a = _attn_args(qbuf, q_off, qt_off, None, n_batch, n_src, segs, (freqs_xy, freqs_yaw), drop)
    a.out, a.ldo, a.row_no_valid = _ptr(out, torch.float32), out.stride(0), _ptr(row_no_valid, torch.uint8)
    _check(load().tbx_knarpe_attn_fwd_mfma(C.byref(a), stream_ptr()), "tbx_knarpe_attn_fwd_mfma")


# ---- deferred launches (round 6: RolloutEngine's one-queue step). While a list is installed, tbx_front / tbx_knarpe_dec_layer calls
# are not launched but appended to it as (entry point name, descriptor, objects the descriptor points into); the engine then pairs the
# lights' list with the agents' and issues tbx_front_pair / tbx_knarpe_dec_layer_pair. Anything else launched meanwhile is an error of the
# schedule (the pairing assumes the two lists ARE the step), so the other wrappers refuse to run while a list is installed.
class defer:
    """with hip.defer() as calls: tbx_front / tbx_knarpe_dec_layer wrappers append (entry point, argument struct, keep-alive) to `calls`
    instead of launching (hip_base.DEFERRED); any other launch inside raises (hip_base.stream_ptr). The rollout engine's one-queue
    step collects the lights' and the agents' halves this way and launches them pairwise (launch_front_pair, launch_dec_layer_pair)."""

    def __enter__(self):
        assert hip_base.DEFERRED is None, "deferred launch lists do not nest"
        self.calls = []
        hip_base.DEFERRED = self.calls
        return self.calls

    def __exit__(self, *exc):
        hip_base.DEFERRED = None


def launch_front_pair(agents, lights) -> None:
    """agents / lights: ("tbx_front", Front, keep) entries of two deferred lists."""
    assert agents[0] == lights[0] == "tbx_front"
    _check(load().tbx_front_pair(C.byref(agents[1]), C.byref(lights[1]), stream_ptr()), "tbx_front_pair")


def launch_dec_layer_pair(a, b) -> None:
    assert a[0] == b[0] == "tbx_knarpe_dec_layer"
    _check(load().tbx_knarpe_dec_layer_pair(C.byref(a[1]), C.byref(b[1]), stream_ptr()), "tbx_knarpe_dec_layer_pair")


def launch_deferred(call) -> None:
    """One deferred entry as its own launch (the unpaired remainder of a list)."""
    _check(getattr(load(), call[0])(C.byref(call[1]), stream_ptr()), call[0])


def knarpe_dec_mid(qkv, q_off: int, qt_off: int, x, self_seg: Seg, cross_segs: Sequence[Seg], bias_self, bias_cross, ln, n_batch: int,
                   n_src: int, fold_self, out_proj, q_img, qfold, fold_cross, out2, flag2, freqs_xy=None, freqs_yaw=None, tail=None):
    """tbx_knarpe_dec_mid: folded self attention -> out-proj into x -> LN -> q -> W_k^T q -> folded cross attention, one launch.
    ln = (weight, bias, eps); the five images are tbx_pack_weight_gemv images (include/tbx_hip.h).
    tail = dict(out_proj2, linear1, linear2 (images), norm2 (w, b, eps), src_invalid, and for all but the last layer next_in_proj,
    next_qfold (images), next_norm (w, b, eps), qkv_out): tbx_knarpe_dec_layer - the rest of the layer in the same launch
    (out2 / flag2 may then be None)."""
    t = DecLayer() if tail is not None else None
    a = t.mid if t is not None else DecMid()
    a.qkv, a.x = _ptr(qkv, torch.float32), _cptr(x, torch.float32)
    a.self_seg = self_seg.c()
    cs = [sg.c() for sg in cross_segs]
    a.cross_seg[0], a.cross_seg[1] = cs[0], cs[-1]
    a.rpe_k_bias_self, a.rpe_k_bias_cross = _ptr(bias_self, torch.float32), _ptr(bias_cross, torch.float32)
    a.freqs_xy, a.freqs_yaw = _cptr(freqs_xy), _cptr(freqs_yaw)
    a.fold_self_image, a.out_proj_image, a.q_image = _ptr(fold_self), _ptr(out_proj), _ptr(q_img)
    a.qfold_image, a.fold_cross_image = _ptr(qfold), _ptr(fold_cross)
    a.ln_weight, a.ln_bias, a.ln_eps = _ptr(ln[0], torch.float32), _ptr(ln[1], torch.float32), float(ln[2])
    a.out2, a.flag2 = _ptr(out2, torch.float32), _ptr(flag2, torch.uint8)
    a.ld_qkv, a.q_off, a.qt_off, a.ld_out2 = qkv.stride(0), q_off, qt_off, (out2.stride(0) if out2 is not None else 0)
    a.n_cross, a.n_batch, a.n_src = len(cross_segs), n_batch, n_src
    if t is None:
        assert hip_base.DEFERRED is None, "tbx_knarpe_dec_mid inside a deferred step"
        _check(load().tbx_knarpe_dec_mid(C.byref(a), stream_ptr()), "tbx_knarpe_dec_mid")
        return
    t.out_proj2_image, t.linear1_image, t.linear2_image = _ptr(tail["out_proj2"]), _ptr(tail["linear1"]), _ptr(tail["linear2"])
    n2 = tail["norm2"]
    t.norm2_weight, t.norm2_bias, t.norm2_eps = _ptr(n2[0], torch.float32), _ptr(n2[1], torch.float32), float(n2[2])
    t.src_invalid = _cptr(tail["src_invalid"], torch.uint8)
    t.tail_mfma32 = int(tail.get("mfma32") or 0)  # (1: three bf16 products per fp32 product; 2: one - Schedule.linear_bf16)
    qo = tail.get("qkv_out")
    if qo is not None:
        n3 = tail["next_norm"]
        t.next_in_proj_image, t.next_qfold_image = _ptr(tail["next_in_proj"]), _ptr(tail["next_qfold"])
        t.next_norm_weight, t.next_norm_bias, t.next_norm_eps = _ptr(n3[0], torch.float32), _ptr(n3[1], torch.float32), float(n3[2])
        t.qkv_out, t.ld_qkv_out = _ptr(qo, torch.float32), qo.stride(0)
        if tail.get("kv16_out") is not None:
            assert tail["kv16_out"].shape[1] == 256 and tail["kv16_out"].is_contiguous()
            t.kv16_out = _ptr(tail["kv16_out"], torch.bfloat16)
    hd, keep = tail.get("heads"), None
    if hd is not None:  # dict(images = 9 gemv images, navi_emb, latent_emb, navi_valid, latent_invalid, type_mask [3, rows] u8, action_out [rows, 2])
        keep = HeadsTail()
        for i, im in enumerate(hd["images"]):
            keep.images[i] = _ptr(im, torch.float32)
        keep.navi_emb, keep.latent_emb = _cptr(hd["navi_emb"], torch.float32), _cptr(hd["latent_emb"], torch.float32)
        keep.navi_valid, keep.latent_invalid = _cptr(hd["navi_valid"], torch.uint8), _cptr(hd["latent_invalid"], torch.uint8)
        keep.type_mask, keep.action_out = _cptr(hd["type_mask"], torch.uint8), _cptr(hd["action_out"], torch.float32)
        keep.mask_stride = hd["type_mask"].shape[1]
        if hd.get("sim_state") is not None:  # the fused step tail: (SimState, parts) + the next step's AgentPrepArgs
            keep.sim_state, keep.sim_parts = C.addressof(hd["sim_state"]), int(hd["sim_parts"])
            keep.next_prep = C.addressof(hd["next_prep"])
        t.heads = C.addressof(keep)
    lt_, keep_l = tail.get("lights"), None
    if lt_ is not None:
        keep_l = tl_tail_struct(lt_, x.shape[0])
        t.lights = C.addressof(keep_l)
    if hip_base.DEFERRED is not None:
        hip_base.DEFERRED.append(("tbx_knarpe_dec_layer", t, (keep, keep_l, tail, cs)))
        return
    _check(load().tbx_knarpe_dec_layer(C.byref(t), stream_ptr()), "tbx_knarpe_dec_layer")


def tl_tail_struct(lt_: dict, rows: int) -> "TlTail":
    """tbx_tl_tail_t from dict(kv_images[4], norms [(w, b, eps)] * 4, kv_out, mlp_images[3], tl_invalid, logits_out, clamp)."""
    keep_l = TlTail()
    for i in range(4):
        keep_l.kv_images[i] = _ptr(lt_["kv_images"][i], torch.float32)
        w_, b_, e_ = lt_["norms"][i]
        keep_l.norm_weight[i], keep_l.norm_bias[i], keep_l.norm_eps[i] = _ptr(w_, torch.float32), _ptr(b_, torch.float32), float(e_)
    for i in range(3):
        keep_l.mlp_images[i] = _ptr(lt_["mlp_images"][i], torch.float32)
    kvo = lt_["kv_out"]
    assert kvo.dim() == 2 and kvo.stride(1) == 1 and kvo.shape[0] == rows
    keep_l.kv_out, keep_l.ld_kv, keep_l.kv_bf16 = kvo.data_ptr(), kvo.stride(0), int(kvo.dtype == torch.bfloat16)
    assert kvo.dtype in (torch.bfloat16, torch.float32)
    lo = lt_["logits_out"]
    assert lo.is_contiguous() and lo.shape[0] == rows
    keep_l.tl_invalid, keep_l.logits_out, keep_l.n_state = _cptr(lt_["tl_invalid"], torch.uint8), _ptr(lo, torch.float32), lo.shape[1]
    keep_l.clamp_lo, keep_l.clamp_hi = (float(v) for v in lt_["clamp"])
    sim = lt_.get("sim")  # dict(state = SimState of the lights, parts, attr, row_invalid): the light's own step behind its logits
    if sim is not None:
        keep_l.sim_state, keep_l.sim_parts = C.addressof(sim["state"]), int(sim["parts"])
        keep_l.prep_attr, keep_l.prep_ld_attr = _ptr(sim["attr"], torch.float32), sim["attr"].stride(0)
        keep_l.prep_row_invalid = _ptr(sim["row_invalid"], torch.uint8)
    return keep_l


def tl_tail_tile(x: torch.Tensor, lights: dict) -> None:
    """tbx_tl_tail_tile (tbx_tl_tail_tile_bf16 under Schedule.linear_bf16) on the finished light tokens x [rows, 128]."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == 128
    st = tl_tail_struct(lights, x.shape[0])
    fn = "tbx_tl_tail_tile_bf16" if tile_products() == 1 else "tbx_tl_tail_tile"
    _check(getattr(load(), fn)(_ptr(x, torch.float32), x.shape[0], C.byref(st), stream_ptr()), fn)


def _layer_tile_args(x, attn=None, ffn=None, proj=None, store_x: bool = True, drop=None, rider=None) -> "LayerTile":
    """tbx_layer_tile on the token rows x [rows, 128] (in place). Each part is None or a dict:
    attn = dict(out [rows, >= 640], row_no_valid u8 [rows], fold, out_proj (mfma32 images));
    ffn = dict(norm2 (w, b, eps), linear1, linear2 (images), src_invalid u8 [rows] | None);
    proj = dict(norm (w, b, eps), image, qfold (images), n = 128 | 384, out [rows, >= 640 | 896], kv16 = bf16 [rows, 256] | None);
    drop = the keyed dropouts of training's stepping pass (see below);
    rider = dict(inp [r, 128] | pose3 [r, 3] + freqs, add, out [r, 128], valid u8 [r], images = 4 mfma32 images): tbx_layer_tile_t's rider_* (a
    first-projection launch only)."""
    a = LayerTile()
    a.x, a.n_rows, a.store_x = _cptr(x, torch.float32), x.shape[0], int(store_x)
    assert x.dim() == 2 and x.shape[1] == 128
    if attn is not None:
        o = attn["out"]
        assert o.dim() == 2 and o.stride(1) == 1 and o.shape[0] == x.shape[0]
        a.attn_out, a.ld_attn, a.row_no_valid = _ptr(o, torch.float32), o.stride(0), _cptr(attn["row_no_valid"], torch.uint8)
        a.fold_image, a.out_proj_image = _ptr(attn["fold"], torch.float32), _ptr(attn["out_proj"], torch.float32)
    if ffn is not None:
        w, b, eps = ffn["norm2"]
        a.norm2_weight, a.norm2_bias, a.norm2_eps = _cptr(w, torch.float32), _cptr(b, torch.float32), float(eps)
        a.linear1_image, a.linear2_image = _ptr(ffn["linear1"], torch.float32), _ptr(ffn["linear2"], torch.float32)
        a.src_invalid = _cptr(ffn.get("src_invalid"), torch.uint8)
    if proj is not None:
        w, b, eps = proj["norm"]
        a.proj_norm_weight, a.proj_norm_bias, a.proj_norm_eps = _cptr(w, torch.float32), _cptr(b, torch.float32), float(eps)
        a.proj_image, a.qfold_image, a.proj_n = _ptr(proj["image"], torch.float32), _ptr(proj["qfold"], torch.float32), int(proj["n"])
        o = proj["out"]
        assert o.dim() == 2 and o.stride(1) == 1 and o.shape[0] == x.shape[0]
        a.proj_out, a.ld_proj = _ptr(o, torch.float32), o.stride(0)
        kv16 = proj.get("kv16")
        if kv16 is not None:
            assert kv16.shape == (x.shape[0], 256) and kv16.is_contiguous()
            a.kv16_out = _ptr(kv16, torch.bfloat16)
    if drop is not None:  # dict(p, seed int64[1] device tensor, step, sites = (attention residual, FFN hidden, FFN output) | None each)
        _fill_drop(a, drop)
    if rider is not None:
        r = rider["out"].shape[0]
        for k in ("add", "out") + (("inp",) if rider.get("pose3") is None else ()):
            assert rider[k].shape == (r, 128) and rider[k].is_contiguous()
        a.rider_add, a.rider_out = _ptr(rider["add"], torch.float32), _ptr(rider["out"], torch.float32)
        if rider.get("pose3") is not None:  # stage 0 on the pose embedding of pose3 [r, 3], built in the kernel (freqs = (xy, yaw) tables)
            assert rider["pose3"].shape == (r, 3)
            a.rider_pose3 = _cptr(rider["pose3"], torch.float32)
            a.rider_freqs_xy, a.rider_freqs_yaw = _cptr(rider["freqs"][0], torch.float32), _cptr(rider["freqs"][1], torch.float32)
        else:
            a.rider_in = _ptr(rider["inp"], torch.float32)
        assert rider["valid"].numel() == r and len(rider["images"]) == 4
        a.rider_valid, a.rider_rows = _cptr(rider["valid"], torch.uint8), r
        for i, im in enumerate(rider["images"]):
            a.rider_images[i] = _ptr(im, torch.float32)
    return a


# products per LINEAR of the tile kernels: 3 (fp32-class) or 1 (the *_bf16 entry points); engine.py points this at the scoped
# Schedule (linear_bf16) - this module knows no schedules
tile_products = lambda: 3


def layer_tile(x, attn=None, ffn=None, proj=None, store_x: bool = True, drop=None, rider=None):
    """tbx_layer_tile (arguments: _layer_tile_args)."""
    a = _layer_tile_args(x, attn, ffn, proj, store_x, drop, rider)
    fn = "tbx_layer_tile_bf16" if (tile_products() == 1 and drop is None) else "tbx_layer_tile"
    _check(getattr(load(), fn)(C.byref(a), stream_ptr()), fn)


def heads_tile(x, hd: dict):
    """tbx_heads_tile: hd = dict(images = 9 mfma32 images, navi_emb, latent_emb [rows, 128], navi_valid, latent_invalid u8 [rows],
    type_mask u8 [3, rows], action_out [rows, 2])."""
    a = HeadsTile()
    a.x, a.n_rows = _cptr(x, torch.float32), x.shape[0]
    raw = hd.get("raw")
    if raw is not None:  # dict(navi_pe, dest_feature [rows, 128], latent_z [rows, >= 16], images = 7 mfma32 images, drop = None | dict(p, seed, step, sites[12]))
        a.raw = 1
        a.navi_pe, a.dest_feature = _cptr(raw["navi_pe"], torch.float32), _cptr(raw["dest_feature"], torch.float32)
        z = raw["latent_z"]
        assert z.dim() == 2 and z.stride(1) == 1 and z.shape[1] >= 16 and z.shape[0] == x.shape[0]
        a.latent_z, a.ld_z = _ptr(z, torch.float32), z.stride(0)
        assert len(raw["images"]) == 7
        for i, im in enumerate(raw["images"]):
            a.raw_images[i] = _ptr(im, torch.float32)
        if raw.get("drop") is not None:
            _fill_drop(a, raw["drop"])
    else:
        a.navi_emb, a.latent_emb = _cptr(hd["navi_emb"], torch.float32), _cptr(hd["latent_emb"], torch.float32)
    a.navi_valid, a.latent_invalid = _cptr(hd["navi_valid"], torch.uint8), _cptr(hd["latent_invalid"], torch.uint8)
    a.type_mask, a.mask_stride, a.action_out = _cptr(hd["type_mask"], torch.uint8), hd["type_mask"].shape[1], _cptr(hd["action_out"], torch.float32)
    assert len(hd["images"]) == 9 and hd["action_out"].shape == (x.shape[0], 2)
    for i, im in enumerate(hd["images"]):
        a.images[i] = _ptr(im, torch.float32)
    fn = "tbx_heads_tile_bf16" if (tile_products() == 1 and a.drop_thresh == 0) else "tbx_heads_tile"
    _check(getattr(load(), fn)(C.byref(a), stream_ptr()), fn)


def _window_tile_args(attr, pe, row_invalid, in_images, pn_images, window: int, out, add_mode: bool = False, drop=None) -> "WindowTile":
    """tbx_window_tile. cat mode: attr [G * window, >= 4 cols], pe [G * window, 64]; add mode: pe = one feature row per window
    [G, 128], the input MLP is 128 wide. row_invalid u8 [G * window] -> out [G, 128]."""
    a = WindowTile()
    assert attr.dim() == 2 and attr.stride(1) == 1 and pe.is_contiguous() and out.shape[1] == 128 and out.is_contiguous()
    assert pe.shape == ((out.shape[0], 128) if add_mode else (attr.shape[0], 64))
    a.attr_cols, a.d_mlp, a.add_mode = min(32, attr.shape[1] // 4 * 4), (128 if add_mode else 64), int(add_mode)
    a.attr, a.ld_attr, a.pe, a.row_invalid = _ptr(attr, torch.float32), attr.stride(0), _ptr(pe, torch.float32), _cptr(row_invalid, torch.uint8)
    for i in range(3):
        a.in_images[i], a.pn_images[i] = _ptr(in_images[i], torch.float32), _ptr(pn_images[i], torch.float32)
    a.out, a.window, a.n_groups = _ptr(out, torch.float32), int(window), out.shape[0]
    assert attr.shape[0] == out.shape[0] * window
    if drop is not None:  # dict(p, seed, step, sites = the three PointNet layers' dropout site ids): training's stepping pass
        _fill_drop(a, drop)
    return a


def window_tile(attr, pe, row_invalid, in_images, pn_images, window: int, out, add_mode: bool = False, drop=None):
    """tbx_window_tile (arguments: _window_tile_args)."""
    a = _window_tile_args(attr, pe, row_invalid, in_images, pn_images, window, out, add_mode, drop)
    fn = "tbx_window_tile_bf16" if (tile_products() == 1 and drop is None) else "tbx_window_tile"
    _check(getattr(load(), fn)(C.byref(a), stream_ptr()), fn)


def front(window: dict, proj: dict, rider=None, jobs=None, pose_embed_job=None):
    """tbx_front: the window PointNet (window = window_tile's arguments as a dict), the first projection of its pooled rows (proj =
    layer_tile's proj dict) + rider, and the K-nearest searches `jobs` (knn_embed_multi's job dicts, relative-pose form) + pose-
    embedding job in ONE launch. -> the searches' [(idx, invalid, rel_pose, None)]."""
    f = Front()
    f.win = _window_tile_args(**window)
    f.layer = _layer_tile_args(window["out"], proj=proj, store_x=False, rider=rider)
    outs, keep = [], []
    if jobs:
        assert all(not q.get("want_emb", True) for q in jobs)
        outs, cj = _knn_jobs(jobs)
        keep.append(cj)
        f.jobs, f.n_jobs, f.pe_dim = C.addressof(cj), len(jobs), 128
        if pose_embed_job is not None:
            pj = _pose_job(pose_embed_job)
            keep.append(pj)
            f.pe = C.addressof(pj)
    if hip_base.DEFERRED is not None:
        hip_base.DEFERRED.append(("tbx_front", f, (keep, window, proj, rider, jobs, outs)))
        return outs
    _check(load().tbx_front(C.byref(f), stream_ptr()), "tbx_front")
    return outs


def agent_prep_args(hist_valid, hist_pose, hist_motion, ag_attr6, ag_type_idx, freqs_xy, freqs_yaw, pe_dim, out, dest=None,
                    mp_tok_pose=None, n_mp=0, mp_batch_div=1) -> AgentPrepArgs:
    """tbx_agent_prep_args_t: what agent_prep launches on, and what the fused step tail of tbx_knarpe_dec_layer takes as next_prep."""
    n, A, W = hist_valid.shape
    a = AgentPrepArgs()
    a.hist_valid, a.hist_pose, a.hist_motion = _cptr(hist_valid, torch.uint8), _cptr(hist_pose, torch.float32), _cptr(hist_motion, torch.float32)
    a.ag_attr6, a.ag_type_idx = _cptr(ag_attr6, torch.float32), _cptr(ag_type_idx, torch.uint8)
    a.freqs_xy, a.freqs_yaw = _cptr(freqs_xy), _cptr(freqs_yaw)
    a.tok_pose, a.tok_invalid, a.attr, a.pe, a.row_invalid = (_ptr(out[k]) for k in ("tok_pose", "tok_invalid", "attr", "pe", "row_invalid"))
    a.type_mask, a.dest, a.mp_tok_pose = _ptr(out.get("type_mask")), _cptr(dest, torch.int64), _cptr(mp_tok_pose, torch.float32)
    a.navi_pose3, a.navi_row = _ptr(out.get("navi_pose3")), _ptr(out.get("navi_row"))
    a.n_tok, a.n_ag, a.window, a.pe_dim, a.n_mp, a.mp_batch_div = n * A, A, W, pe_dim, n_mp, mp_batch_div
    return a


def agent_prep(*args, **kw):
    """tbx_agent_prep (arguments: agent_prep_args)."""
    _check(load().tbx_agent_prep(C.byref(agent_prep_args(*args, **kw)), stream_ptr()), "tbx_agent_prep")


def _tl_rows(tl_invalid, attr, row_invalid) -> TlRows:
    """tbx_tl_rows_t: tl_invalid u8 [n*L], attr f32 [n*L*W, ld], row_invalid u8 [n*L*W]."""
    return TlRows(_cptr(tl_invalid, torch.uint8), _ptr(attr, torch.float32), _ptr(row_invalid, torch.uint8), attr.stride(0), 0)


def tl_prep(hist_tl, tl_invalid, attr, row_invalid):
    n, L, W = hist_tl.shape
    rows = _tl_rows(tl_invalid, attr, row_invalid)
    _check(load().tbx_tl_prep(_cptr(hist_tl, torch.uint8), n, L, W, C.byref(rows), stream_ptr()), "tbx_tl_prep")


def map_prep(mp_valid_u8, mp_type11, mp_pose, attr, pe, row_invalid, tok_pose, tok_invalid):
    n, M, N = mp_valid_u8.shape
    rc = load().tbx_map_prep(_cptr(mp_valid_u8, torch.uint8), _cptr(mp_type11, torch.float32), _cptr(mp_pose, torch.float32),
                             n, M, N, _ptr(attr), _ptr(pe), _ptr(row_invalid), _ptr(tok_pose), _ptr(tok_invalid), stream_ptr())
    _check(rc, "tbx_map_prep")


SIM_AGENTS, SIM_LIGHTS, SIM_ADVANCE, SIM_NO_DISABLE, SIM_NO_APPEND, SIM_APPEND = 1, 2, 4, 8, 16, 32


def sim_step(state: SimState, parts: int = SIM_AGENTS | SIM_LIGHTS | SIM_ADVANCE, tl_prep=None):
    """tl_prep = (tl_invalid u8 [n*L], attr f32 [n*L*W, ld], row_invalid u8 [n*L*W]): the lights' update also writes the tbx_tl_prep
    rows of their new windows (tbx_sim_step's tl_rows)."""
    assert hip_base.DEFERRED is None, "tbx_sim_step inside a deferred step (the one-queue step runs the lights' update in their last layer's tail)"
    rows = _tl_rows(*tl_prep) if tl_prep is not None else None
    _check(load().tbx_sim_step(C.byref(state), parts, rows, stream_ptr()), "tbx_sim_step")




def _flag8(t: Optional[torch.Tensor], shape, what: str, who: str = "loss_shape") -> Optional[torch.Tensor]:
    """A 0/1 byte tensor (u8 or bool storage) of the given shape, on the device, as it lies."""
    if t is None:
        return None
    if t.dtype not in (torch.uint8, torch.bool) or tuple(t.shape) != tuple(shape):
        raise TypeError(f"{who}: {what} must be u8 / bool {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def loss_shape(pred_valid, tf, step_training_start: int, loss_for_teacher_forcing: bool, reward=None, reward_valid=None, relevant=None,
               pick=None, mask_irrelevant: bool = False, w_relevant: float = 0.0, discount: float = -1.0, want_w: bool = False, acc=None,
               partials=None):
    """tbx_loss_shape (include/tbx_hip_loss.h) on [rows, A, T] VIEWS of any strides - the training chain's permuted [n, T, A] log, a buffer's
    [rows, A, T], a time slice of the engine's log: read in place. pred_valid / tf / reward_valid u8 or bool, reward f32; relevant / pick
    [rows, A] u8 or bool, contiguous. -> (any_valid u8 [rows, A], w_agent f32 [rows, A], w f32 [rows, A, T] | None, acc f64 [2] | None):
    acc[0] = the shaped reward sum, acc[1] = #rv, ADDED to `acc` if one is passed (else to zeros); without reward: masks only."""
    rows, A, T = pred_valid.shape
    dev = pred_valid.device
    _flag8(pred_valid, (rows, A, T), "pred_valid"), _flag8(tf, (rows, A, T), "tf"), _flag8(reward_valid, (rows, A, T), "reward_valid")
    _flag8(relevant, (rows, A), "relevant"), _flag8(pick, (rows, A), "pick")
    if reward is not None and (reward.dtype != torch.float32 or tuple(reward.shape) != (rows, A, T)):
        raise TypeError(f"loss_shape: reward must be f32 {(rows, A, T)}")
    a = LossShape()
    a.pred_valid, a.tf, a.reward_valid, a.reward = _ptr(pred_valid), _ptr(tf), _ptr(reward_valid), _ptr(reward, torch.float32)
    a.relevant, a.pick = _cptr(relevant), _cptr(pick)
    any_valid = torch.empty(rows, A, dtype=torch.uint8, device=dev)
    w_agent = torch.empty(rows, A, dtype=torch.float32, device=dev)
    w = torch.empty_like(reward) if (want_w and reward is not None) else None  # (the reward's own layout where that is dense)
    if reward is not None:
        acc = torch.zeros(2, dtype=torch.float64, device=dev) if acc is None else acc
        partials = torch.empty(LOSS_PARTIALS, dtype=torch.float64, device=dev) if partials is None else partials
        if acc.numel() < 2 or partials.numel() < LOSS_PARTIALS:
            raise RuntimeError("loss_shape: acc needs 2, partials LOSS_PARTIALS float64 values")
    else:
        acc = partials = None
    a.any_valid, a.w_agent, a.w = _ptr(any_valid), _ptr(w_agent), _ptr(w)
    a.acc, a.partials = _cptr(acc, torch.float64), _cptr(partials, torch.float64)
    a.rows = rows
    for name, t in (("pred_valid", pred_valid), ("tf", tf), ("reward_valid", reward_valid), ("reward", reward), ("w", w)):
        if t is not None:
            setattr(a, name + "_stride", (C.c_int64 * 3)(*t.stride()))
    a.n_ag, a.n_step, a.step_training_start = A, T, int(step_training_start)
    a.loss_for_teacher_forcing, a.mask_irrelevant = int(bool(loss_for_teacher_forcing)), int(bool(mask_irrelevant))
    a.w_relevant, a.discount = float(w_relevant), float(discount)
    _check(load().tbx_loss_shape(C.byref(a), stream_ptr()), "tbx_loss_shape")
    return any_valid, w_agent, w, acc


def tf_threshold_args(thresholds, step, valid, pose, motion, gt_valid, gt_pose, gt_motion, tf_mask, out_reset=None) -> "TfThreshold":
    """tbx_tf_threshold_t over the caller's tensors, as they lie (all contiguous; 0/1 bytes as u8 or bool): thresholds = (xy [m], yaw
    [deg], spd [m/s]), <= 0 is off; step an int (step_host) or an int32 device tensor whose first word is the 1-based step about to run
    (step_dev: the word tbx_sim_state_t.step points to). The struct holds pointers only: the caller keeps the tensors alive."""
    rows, A, Tg = gt_valid.shape
    for name, t, shape in (("valid", valid, (rows, A)), ("gt_valid", gt_valid, (rows, A, Tg)), ("tf_mask", tf_mask, (rows, A, Tg)),
                           ("out_reset", out_reset, (rows, A))):
        _flag8(t, shape, name, who="tf_threshold")
    for name, t, shape in (("pose", pose, (rows, A, 3)), ("motion", motion, (rows, A, 3)), ("gt_pose", gt_pose, (rows, A, Tg, 3)),
                           ("gt_motion", gt_motion, (rows, A, Tg, 3))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise TypeError(f"tf_threshold: {name} must be f32 {shape}, got {t.dtype} {tuple(t.shape)}")
    a = TfThreshold()
    a.valid, a.pose, a.motion = _cptr(valid), _cptr(pose), _cptr(motion)
    a.gt_valid, a.gt_pose, a.gt_motion = _cptr(gt_valid), _cptr(gt_pose), _cptr(gt_motion)
    a.tf_mask, a.out_reset = _cptr(tf_mask), _cptr(out_reset)
    if torch.is_tensor(step):
        a.step_dev, a.step_host = _cptr(step, torch.int32), 0
    else:
        a.step_dev, a.step_host = None, int(step)
    a.n_rows, a.n_ag, a.n_step_gt = rows, A, Tg
    a.threshold_xy, a.threshold_yaw, a.threshold_spd = (float(t) for t in thresholds)
    return a


def tf_threshold_launch(a: "TfThreshold") -> None:
    """tbx_tf_threshold (include/tbx_hip_tf.h) on the current stream: one step's error-threshold resets ORed into column s of a.tf_mask."""
    _check(load().tbx_tf_threshold(C.byref(a), stream_ptr()), "tbx_tf_threshold")


def tf_threshold(thresholds, step, valid, pose, motion, gt_valid, gt_pose, gt_motion, tf_mask, out_reset=None) -> None:
    """tf_threshold_args + tf_threshold_launch: utils/teacher_forcing.py:131-145 for one step, in place on tf_mask [rows, A, Tg]."""
    tf_threshold_launch(tf_threshold_args(thresholds, step, valid, pose, motion, gt_valid, gt_pose, gt_motion, tf_mask, out_reset))


def grad_norms_args(g, seg_off, seg_len, chunk_seg, chunk_off, chunk_len, chunk_max: int, partial, partial_nf, out, norm_type: int,
                    max_norm: Optional[float]) -> "GradNorms":
    """tbx_grad_norms_t over the caller's tensors (include/tbx_hip_grad.h): g the flat f32 buffer; the segment / chunk tables and the two
    workspaces as FlatGrads.norm_plan() lays them out; `out` f32 [n_seg + 3] = norms | total | coef | nonfinite (the last word read as
    i32). norm_type GRAD_NORM_2 / GRAD_NORM_INF; max_norm None or <= 0: no clipping. The struct holds pointers only: the caller keeps the
    tensors alive."""
    n_seg, n_chunk = seg_off.numel(), chunk_seg.numel()
    if g.dim() != 1 or seg_len.numel() != n_seg or chunk_off.numel() != n_chunk or chunk_len.numel() != n_chunk:
        raise TypeError("grad_norms: g must be flat, seg_off / seg_len and chunk_seg / chunk_off / chunk_len of one length each")
    if out.numel() != n_seg + 3 or partial.numel() < n_chunk or partial_nf.numel() < n_chunk:
        raise RuntimeError("grad_norms: out needs n_seg + 3 values, partial / partial_nf n_chunk each")
    a = GradNorms()
    a.g = _cptr(g, torch.float32)
    a.seg_off, a.seg_len = _cptr(seg_off, torch.int64), _cptr(seg_len, torch.int64)
    a.chunk_seg, a.chunk_off, a.chunk_len = _cptr(chunk_seg, torch.int32), _cptr(chunk_off, torch.int64), _cptr(chunk_len, torch.int32)
    a.partial, a.partial_nf = _cptr(partial, torch.float64), _cptr(partial_nf, torch.int32)
    base = _cptr(out, torch.float32)
    a.norms, a.total, a.coef, a.nonfinite = base, base + 4 * n_seg, base + 4 * (n_seg + 1), base + 4 * (n_seg + 2)
    a.n, a.n_seg, a.n_chunk, a.chunk_max, a.norm_type = g.numel(), n_seg, n_chunk, int(chunk_max), int(norm_type)
    a.max_norm = float(max_norm) if max_norm is not None and max_norm > 0 else 0.0
    return a


def grad_norms_launch(a: "GradNorms") -> None:
    """tbx_grad_norms (include/tbx_hip_grad.h, libtbx_grad.so) on the current stream: two launches, a third when a.max_norm > 0. No host
    read."""
    _check(load_grad().tbx_grad_norms(C.byref(a), stream_ptr()), "tbx_grad_norms")


def _sub_in(t, dtype, shape, what: str, who: str):
    """A dense device input of tbx_hip_sub.h: the given dtype (bool storage passes for u8) and shape -> its pointer (None for no elements)."""
    if t.dtype != dtype and not (dtype == torch.uint8 and t.dtype == torch.bool):
        raise TypeError(f"{who}: {what} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise TypeError(f"{who}: {what} must be {tuple(shape)}, got {tuple(t.shape)}")
    p = _cptr(t)  # (a CPU tensor raises here, an empty one too)
    return p if t.numel() else None


def wosac_joint_scenes(pos_sim, yaw_sim, valid_sim, z_sim, object_id_sim, pos_no_sim, yaw_no_sim, z_no_sim, valid_no_sim, object_id_no_sim,
                       step_current: int, const_vel_z_sim: bool, const_vel_no_sim: bool, out=None):
    """tbx_wosac_joint_scenes (include/tbx_hip_sub.h, libtbx_sub.so) on the current stream. Dense device tensors in the shapes of the
    header's table: pos_sim [n_sc, K, A, T, 2], yaw_sim [n_sc, K, A, T], valid_sim [n_sc, A, Th] u8 / bool, z_sim [n_sc, A, Th],
    object_id_sim [n_sc, A] i64 and the no-sim five [n_sc, N, Th(, 2)] / [n_sc, N].
    -> (traj_sim f32 [n_sc, K, A, T, 4], traj_no_sim f32 [n_sc, N, T, 4], id_sim i64 [n_sc, A], id_no_sim i64 [n_sc, N], count i32 [n_sc, 2]);
    out = such a tuple of a previous call: written in place (every element, whatever it held)."""
    who = "wosac_joint_scenes"
    if pos_sim.dim() != 5 or valid_sim.dim() != 3 or pos_no_sim.dim() != 4:
        raise TypeError(f"{who}: pos_sim [n_sc, K, A, T, 2], valid_sim [n_sc, A, Th], pos_no_sim [n_sc, N, Th, 2]")
    n_sc, K, A, T = pos_sim.shape[:4]
    Th, N = valid_sim.shape[2], pos_no_sim.shape[1]
    f32, u8, i64 = torch.float32, torch.uint8, torch.int64
    a = JointScenes()
    a.pos_sim, a.yaw_sim = _sub_in(pos_sim, f32, (n_sc, K, A, T, 2), "pos_sim", who), _sub_in(yaw_sim, f32, (n_sc, K, A, T), "yaw_sim", who)
    a.valid_sim, a.z_sim = _sub_in(valid_sim, u8, (n_sc, A, Th), "valid_sim", who), _sub_in(z_sim, f32, (n_sc, A, Th), "z_sim", who)
    a.object_id_sim = _sub_in(object_id_sim, i64, (n_sc, A), "object_id_sim", who)
    a.pos_no_sim, a.yaw_no_sim = _sub_in(pos_no_sim, f32, (n_sc, N, Th, 2), "pos_no_sim", who), _sub_in(yaw_no_sim, f32, (n_sc, N, Th), "yaw_no_sim", who)
    a.z_no_sim, a.valid_no_sim = _sub_in(z_no_sim, f32, (n_sc, N, Th), "z_no_sim", who), _sub_in(valid_no_sim, u8, (n_sc, N, Th), "valid_no_sim", who)
    a.object_id_no_sim = _sub_in(object_id_no_sim, i64, (n_sc, N), "object_id_no_sim", who)
    dev = pos_sim.device
    if out is None:
        out = (torch.empty(n_sc, K, A, T, 4, dtype=f32, device=dev), torch.empty(n_sc, N, T, 4, dtype=f32, device=dev),
               torch.empty(n_sc, A, dtype=i64, device=dev), torch.empty(n_sc, N, dtype=i64, device=dev),
               torch.empty(n_sc, 2, dtype=torch.int32, device=dev))
    traj_sim, traj_no_sim, id_sim, id_no_sim, count = out
    a.traj_sim, a.traj_no_sim = _sub_in(traj_sim, f32, (n_sc, K, A, T, 4), "traj_sim", who), _sub_in(traj_no_sim, f32, (n_sc, N, T, 4), "traj_no_sim", who)
    a.id_sim, a.id_no_sim = _sub_in(id_sim, i64, (n_sc, A), "id_sim", who), _sub_in(id_no_sim, i64, (n_sc, N), "id_no_sim", who)
    a.count = _sub_in(count, torch.int32, (n_sc, 2), "count", who)
    a.n_sc, a.n_k, a.n_ag, a.n_no_sim, a.n_step, a.n_hist, a.step_current = n_sc, K, A, N, T, Th, int(step_current)
    a.const_vel_z_sim, a.const_vel_no_sim = int(bool(const_vel_z_sim)), int(bool(const_vel_no_sim))
    _check(load_sub().tbx_wosac_joint_scenes(C.byref(a), stream_ptr()), "tbx_wosac_joint_scenes")
    return out


def womd_predictions(trajs, scores, object_id, mask_pred, scenario_center, scenario_yaw, out=None):
    """tbx_womd_predictions (include/tbx_hip_sub.h, libtbx_sub.so) on the current stream. trajs [n_sc, A, k, n, 3] (the "trajs" of
    WOMDPostProcessing.forward), scores [n_sc, A, k], object_id [n_sc, A] i64, mask_pred [n_sc, A] u8 / bool, scenario_center [n_sc, 2],
    scenario_yaw [n_sc]: dense device tensors -> (pos f32 [n_sc, A, k, n, 2] global frame, scores [n_sc, A, k], object_id i64 [n_sc, A],
    count i32 [n_sc]), the agents with mask_pred first; out = such a tuple of a previous call: written in place."""
    who = "womd_predictions"
    if trajs.dim() != 5:
        raise TypeError(f"{who}: trajs [n_sc, A, k, n, 3]")
    n_sc, A, k, n = trajs.shape[:4]
    f32, u8, i64 = torch.float32, torch.uint8, torch.int64
    a = WomdPred()
    a.trajs, a.scores = _sub_in(trajs, f32, (n_sc, A, k, n, 3), "trajs", who), _sub_in(scores, f32, (n_sc, A, k), "scores", who)
    a.object_id, a.mask_pred = _sub_in(object_id, i64, (n_sc, A), "object_id", who), _sub_in(mask_pred, u8, (n_sc, A), "mask_pred", who)
    a.scenario_center = _sub_in(scenario_center, f32, (n_sc, 2), "scenario_center", who)
    a.scenario_yaw = _sub_in(scenario_yaw, f32, (n_sc,), "scenario_yaw", who)
    dev = trajs.device
    if out is None:
        out = (torch.empty(n_sc, A, k, n, 2, dtype=f32, device=dev), torch.empty(n_sc, A, k, dtype=f32, device=dev),
               torch.empty(n_sc, A, dtype=i64, device=dev), torch.empty(n_sc, dtype=torch.int32, device=dev))
    pos, out_scores, out_id, count = out
    a.out_pos, a.out_scores = _sub_in(pos, f32, (n_sc, A, k, n, 2), "pos", who), _sub_in(out_scores, f32, (n_sc, A, k), "scores (out)", who)
    a.out_object_id, a.out_count = _sub_in(out_id, i64, (n_sc, A), "object_id (out)", who), _sub_in(count, torch.int32, (n_sc,), "count", who)
    a.n_sc, a.n_ag, a.n_mode, a.n_sample = n_sc, A, k, n
    _check(load_sub().tbx_womd_predictions(C.byref(a), stream_ptr()), "tbx_womd_predictions")
    return out
