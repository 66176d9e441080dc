"""The C-ABI mirror: constants and ctypes structures of include/tbx_hip.h and the topical headers it includes (tbx_hip_metrics.h, _reward.h,
_loss.h, _tf.h), and `load()` - dlopen of the in-tree libtbx_hip.so, the one library, with every declared symbol checked and every
prototype set. Nothing here computes; the wrappers that launch kernels are in hip.py (which re-exports this module's names).
tests/test_abi_and_host.py compiles the header with gcc and compares every structure's `sizeof` and every field's `offsetof` with the
classes below. Two headers stand on their own, each with a library and a loader of its own: tbx_hip_grad.h (libtbx_grad.so, `load_grad()`)
and tbx_hip_sub.h (libtbx_sub.so, `load_sub()`); their mirrors are checked by tests/test_grad_norm_host.py and tests/test_sub_records_host.py.
tbx_hip_aggr.h (libtbx_aggr.so, `load_aggr()`) is a third of that kind: tests/test_womd_aggr_host.py; tbx_hip_il.h (libtbx_il.so, `load_il()`:
the imitation terms of the differentiable reward for every criterion / angular type) a fourth: tests/test_il_loss_ref.py."""
import ctypes as C
import os
import re
from pathlib import Path
from typing import List

_lib = None
_grad_lib = None
_sub_lib = None
_aggr_lib = None
_il_lib = None
_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "csrc" / "libtbx_hip.so"
GRAD_LIB_PATH = _PKG / "csrc" / "libtbx_grad.so"  # tbx_grad_norms alone (include/tbx_hip_grad.h): libtbx_hip.so's export list is ABI 7's, closed
SUB_LIB_PATH = _PKG / "csrc" / "libtbx_sub.so"  # tbx_wosac_joint_scenes, tbx_womd_predictions (include/tbx_hip_sub.h), for the same reason
AGGR_LIB_PATH = _PKG / "csrc" / "libtbx_aggr.so"  # tbx_womd_aggr alone (include/tbx_hip_aggr.h), for the same reason
IL_LIB_PATH = _PKG / "csrc" / "libtbx_il.so"  # tbx_il_reward_fwd / _bwd, tbx_train_chain_bwd_state (include/tbx_hip_il.h), for the same reason
HEADER_PATH = _PKG.parent / "include" / "tbx_hip.h"

# ---- constants mirrored from include/tbx_hip.h
OP_LOAD, OP_LINEAR, OP_LAYERNORM, OP_ADD, OP_COPY, OP_ROWMASK, OP_GROUPMAX, OP_POOLMAX, OP_STORE, OP_CLAMP, OP_DROPOUT = range(1, 12)
ACT_NONE, ACT_RELU = 0, 1
F_ACCUM, F_WT, F_ROW_DIV, F_ROW_MOD, F_ROW_IDX, F_ROW_BATCH_MOD, F_WPACK, F_MASK_INV = 1, 2, 4, 8, 16, 32, 64, 128
F_POOL_KEEP = 256
F_WSPLIT = 512
F_ROWSKIP = 1024
F_LOAD2 = 2048
F_WGEMV = 4096
F_OUT_BF16 = 8192
F_MASKED_SUM = 16384
F_ROWZERO = 32768
BUF0, BUF1, AUX, GLOBAL = 0, 1, 2, 3
MAX_STAGES, AUX_LD = 44, 260
# TBX_ATTN_FORM_* (tbx_knarpe_attn_fwd_form): the kernel form in the low bits, flags ORed on
ATTN_FORM_SPLIT4, ATTN_FORM_WAVE, ATTN_FORM_RING, ATTN_FORM_MASK = 1, 2, 3, 0xF
ATTN_FORM_DROP, ATTN_FORM_KV16, ATTN_FORM_FOLD, ATTN_FORM_FOLD_LOOP, ATTN_FORM_BATCH_MAJOR, ATTN_FORM_XCD = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200


class Stage(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("op", "src", "dst", "src_col", "dst_col", "k", "n", "act", "flags", "ld", "div",
                                         "reserved", "ld2", "pad")] + [("f0", C.c_float), ("f1", C.c_float), ("p0", C.c_void_p),
                                                                       ("p1", C.c_void_p), ("p2", C.c_void_p)]


class AttnSeg(C.Structure):
    _fields_ = [("kv", C.c_void_p), ("idx", C.c_void_p), ("invalid", C.c_void_p), ("emb", C.c_void_p), ("rel_pose", C.c_void_p)] + [
        (n, C.c_int32) for n in ("ld_kv", "k_off", "v_off", "n_tgt", "batch_div", "k", "kv_bf16")]


class Attn(C.Structure):
    """tbx_attn_t (include/tbx_hip.h): the arguments of tbx_knarpe_attn_fwd / _fwd_mfma / _bwd."""
    _fields_ = ([(n, C.c_void_p) for n in ("qbuf", "rpe_k_bias", "freqs_xy", "freqs_yaw")] + [("seg", AttnSeg * 2)]
                + [(n, C.c_void_p) for n in ("drop_seed", "out", "row_no_valid", "fold_image", "dout", "dqbuf")]
                + [("dkv", C.c_void_p * 2), ("dbias_k", C.c_void_p), ("inv_ptr", C.c_void_p * 2), ("inv_list", C.c_void_p * 2), ("coef", C.c_void_p)]
                + [(n, C.c_int32) for n in ("ldq", "q_off", "qt_off", "n_batch", "n_src", "n_seg", "ldo")]
                + [("p_drop", C.c_float), ("drop_call", C.c_uint32), ("time_batch", C.c_int32), ("time0", C.c_int32), ("pad_", C.c_int32)])


class Drop(C.Structure):
    """tbx_drop_t (include/tbx_hip.h): an elementwise keyed dropout. Filled by hip_base.drop_struct."""
    _fields_ = [("seed", C.c_void_p), ("p", C.c_float), ("site", C.c_uint32), ("rows_per_scene", C.c_int32), ("time_batch", C.c_int32),
                ("time0", C.c_int32), ("pad_", C.c_int32)]


class Linear(C.Structure):
    """tbx_linear_t (include/tbx_hip.h): the arguments of tbx_tall_linear / _bf16."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "image", "y", "y16")] + [("m", C.c_int64)]
                + [(n, C.c_int32) for n in ("k", "ldx", "n", "has_bias", "relu", "ldy", "ldy16", "pad_")] + [("drop", Drop)])


class KnnJob(C.Structure):
    """tbx_knn_job_t (include/tbx_hip.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("src_pose", "src_invalid", "tgt_pose", "tgt_invalid", "idx", "invalid", "rel_pose", "emb")]
                + [(n, C.c_int32) for n in ("n_batch", "n_src", "n_tgt", "tgt_batch_div", "k")] + [("dist_limit", C.c_float)])


class PoseEmbedJob(C.Structure):
    """tbx_pose_embed_job_t (include/tbx_hip.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("pose3", "freqs_xy", "freqs_yaw", "out")] + [("n", C.c_int64)]
                + [(n, C.c_int32) for n in ("pe_dim", "ld_out", "col_off", "reserved")])


class DecMid(C.Structure):
    """tbx_dec_mid_t (include/tbx_hip.h)."""
    _fields_ = ([("qkv", C.c_void_p), ("x", C.c_void_p), ("self_seg", AttnSeg), ("cross_seg", AttnSeg * 2)]
                + [(n, C.c_void_p) for n in ("rpe_k_bias_self", "rpe_k_bias_cross", "freqs_xy", "freqs_yaw", "fold_self_image",
                                             "out_proj_image", "q_image", "qfold_image", "fold_cross_image", "ln_weight", "ln_bias",
                                             "out2", "flag2")]
                + [("ln_eps", C.c_float)]
                + [(n, C.c_int32) for n in ("ld_qkv", "q_off", "qt_off", "ld_out2", "n_cross", "n_batch", "n_src")])


class HeadsTail(C.Structure):
    """tbx_heads_tail_t (include/tbx_hip.h)."""
    _fields_ = ([("images", C.c_void_p * 9)]
                + [(n, C.c_void_p) for n in ("navi_emb", "latent_emb", "navi_valid", "latent_invalid", "type_mask", "action_out")]
                + [("mask_stride", C.c_int32), ("sim_parts", C.c_int32), ("sim_state", C.c_void_p), ("next_prep", C.c_void_p)])


class AgentPrepArgs(C.Structure):
    """tbx_agent_prep_args_t (include/tbx_hip.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("hist_valid", "hist_pose", "hist_motion", "ag_attr6", "ag_type_idx", "freqs_xy", "freqs_yaw", "tok_pose",
                                           "tok_invalid", "attr", "pe", "row_invalid", "type_mask", "dest", "mp_tok_pose", "navi_pose3", "navi_row")]
                + [(n, C.c_int32) for n in ("n_tok", "n_ag", "window", "pe_dim", "n_mp", "mp_batch_div")])


class TlRows(C.Structure):
    """tbx_tl_rows_t (include/tbx_hip.h)."""
    _fields_ = [("tl_invalid", C.c_void_p), ("attr", C.c_void_p), ("row_invalid", C.c_void_p), ("ld_attr", C.c_int32), ("pad_", C.c_int32)]


class DecLayer(C.Structure):
    """tbx_dec_layer_t (include/tbx_hip.h)."""
    _fields_ = ([("mid", DecMid)]
                + [(n, C.c_void_p) for n in ("out_proj2_image", "linear1_image", "linear2_image", "next_in_proj_image", "next_qfold_image",
                                             "norm2_weight", "norm2_bias", "next_norm_weight", "next_norm_bias", "src_invalid", "qkv_out", "kv16_out", "heads")]
                + [("norm2_eps", C.c_float), ("next_norm_eps", C.c_float), ("ld_qkv_out", C.c_int32), ("tail_mfma32", C.c_int32),
                   ("lights", C.c_void_p)])


class TlTail(C.Structure):
    """tbx_tl_tail_t (include/tbx_hip.h)."""
    _fields_ = [("kv_images", C.c_void_p * 4), ("norm_weight", C.c_void_p * 4), ("norm_bias", C.c_void_p * 4), ("norm_eps", C.c_float * 4),
                ("kv_out", C.c_void_p), ("mlp_images", C.c_void_p * 3), ("tl_invalid", C.c_void_p), ("logits_out", C.c_void_p),
                ("ld_kv", C.c_int32), ("kv_bf16", C.c_int32), ("n_state", C.c_int32), ("pad_", C.c_int32),
                ("clamp_lo", C.c_float), ("clamp_hi", C.c_float), ("sim_parts", C.c_int32), ("prep_ld_attr", C.c_int32),
                ("sim_state", C.c_void_p), ("prep_attr", C.c_void_p), ("prep_row_invalid", C.c_void_p)]


class PackJob(C.Structure):
    """tbx_pack_job_t (include/tbx_hip.h)."""
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("n", C.c_int32), ("k", C.c_int32), ("ld", C.c_int32),
                ("groups", C.c_int32), ("wt", C.c_int32), ("pad_", C.c_int32)]


class LayerTile(C.Structure):
    """tbx_layer_tile_t (include/tbx_hip.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "attn_out", "row_no_valid", "fold_image", "out_proj_image", "norm2_weight", "norm2_bias",
                                           "linear1_image", "linear2_image", "src_invalid", "proj_norm_weight", "proj_norm_bias", "proj_image",
                                           "qfold_image", "proj_out", "kv16_out")]
                + [("norm2_eps", C.c_float), ("proj_norm_eps", C.c_float)]
                + [(n, C.c_int32) for n in ("ld_attn", "ld_proj", "proj_n", "store_x")] + [("n_rows", C.c_int64)]
                + [("drop_seed", C.c_void_p), ("drop_thresh", C.c_uint32), ("drop_scale", C.c_float), ("drop_site", C.c_int32 * 3),
                   ("drop_step", C.c_int32)]
                + [("rider_in", C.c_void_p), ("rider_add", C.c_void_p), ("rider_pose3", C.c_void_p), ("rider_freqs_xy", C.c_void_p),
                   ("rider_freqs_yaw", C.c_void_p), ("rider_images", C.c_void_p * 4), ("rider_valid", C.c_void_p),
                   ("rider_out", C.c_void_p), ("rider_rows", C.c_int64)])


class HeadsTile(C.Structure):
    """tbx_heads_tile_t (include/tbx_hip.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "navi_emb", "latent_emb", "navi_valid", "latent_invalid", "type_mask")]
                + [("images", C.c_void_p * 9), ("action_out", C.c_void_p), ("mask_stride", C.c_int32), ("raw", C.c_int32), ("n_rows", C.c_int64),
                   ("navi_pe", C.c_void_p), ("dest_feature", C.c_void_p), ("latent_z", C.c_void_p), ("raw_images", C.c_void_p * 7),
                   ("drop_seed", C.c_void_p), ("drop_thresh", C.c_uint32), ("drop_scale", C.c_float), ("drop_site", C.c_int32 * 12),
                   ("drop_step", C.c_int32), ("ld_z", C.c_int32)])


class WindowTile(C.Structure):
    """tbx_window_tile_t (include/tbx_hip.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("attr", "pe", "row_invalid")] + [("in_images", C.c_void_p * 3), ("pn_images", C.c_void_p * 3),
                ("out", C.c_void_p), ("window", C.c_int32), ("ld_attr", C.c_int32), ("n_groups", C.c_int64)]
                + [(n, C.c_int32) for n in ("attr_cols", "d_mlp", "add_mode", "pad_")]
                + [("drop_seed", C.c_void_p), ("drop_thresh", C.c_uint32), ("drop_scale", C.c_float), ("drop_site", C.c_int32 * 3),
                   ("drop_step", C.c_int32)])


class Front(C.Structure):
    """tbx_front_t (include/tbx_hip.h)."""
    _fields_ = [("win", WindowTile), ("layer", LayerTile), ("jobs", C.c_void_p), ("pe", C.c_void_p), ("freqs_xy", C.c_void_p),
                ("freqs_yaw", C.c_void_p), ("n_jobs", C.c_int32), ("pe_dim", C.c_int32)]


class SimState(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ("n_batch", "n_ag", "n_tl", "window", "n_step_gt", "n_step_tl_gt", "n_step_out", "n_node")]
        + [(n, C.c_void_p) for n in (
            "step", "ag_valid", "ag_disabled", "ag_pose", "ag_motion", "navi_valid", "outside_map", "dest_reached",
            "tl_state", "hist_valid", "hist_pose", "hist_motion", "hist_tl", "ag_type_idx", "tf_mask", "gt_valid", "gt_pose",
            "gt_motion", "tl_gt", "boundary", "dest_pos", "dest_dir", "dest_invalid", "dest_kind", "dest_thresh",
            "action_mean", "tl_logits", "out_valid", "out_pose", "out_motion", "out_action", "out_tl_state",
            "out_outside_map", "out_dest_reached")]
        + [("max_acc", C.c_float * 3), ("max_yaw_rate", C.c_float * 3), ("dt", C.c_float)]
        + [(n, C.c_void_p) for n in ("out_reward", "out_reward_valid", "out_tf", "out_tl_nll")]
        + [(n, C.c_float) for n in ("w_pos", "w_rot", "w_spd")]
        + [(n, C.c_void_p) for n in ("player_valid", "player_action", "ov_valid", "ov_pose", "ov_motion", "ov_tl_valid",
                                     "ov_tl_state", "now_outside", "now_reached")]
        # sampled actions (act_seed NULL = off)
        + [("act_seed", C.c_void_p), ("act_log_std", (C.c_float * 2) * 3), ("out_act_noise", C.c_void_p), ("out_act_log_prob", C.c_void_p)]
    )


class TrainChainArgs(C.Structure):
    """tbx_train_chain_t (include/tbx_hip.h)."""
    _fields_ = ([(n, C.c_int32) for n in ("n_batch", "n_ag", "n_step", "n_step_gt", "n_node", "window")]
                + [(n, C.c_float) for n in ("dt", "w_pos", "w_rot", "w_spd")]
                + [(n, C.c_void_p) for n in (
                    "gt_valid", "gt_pose", "gt_motion", "tf_mask", "lim", "dest_pos", "dest_dir", "dest_invalid", "dest_thresh",
                    "dest_kind", "boundary", "valid", "disabled", "navi_valid", "outside", "reached", "pose", "motion",
                    "rec_valid", "rec_pose", "rec_motion", "rec_navi_valid", "pred_valid", "tf", "ov", "reward_valid",
                    "pred_pose", "pred_motion", "reward")])


class RuleCtx(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("n_batch", "n_ag", "n_tl", "map_batch_div", "cap")]
                + [(n, C.c_void_p) for n in ("seg", "n_seg", "lane", "n_lane", "ag_size", "ag_type_idx", "tl_valid", "tl_pose")]
                + [("collision_size_scale", C.c_float)]
                + [(n, C.c_void_p) for n in ("seg_start", "seg_grid", "lane_start", "lane_grid")])


class LossShape(C.Structure):
    """tbx_loss_shape_t (include/tbx_hip_loss.h). Filled by hip_train.loss_shape."""
    _fields_ = ([(n, C.c_void_p) for n in ("pred_valid", "tf", "reward_valid", "reward", "relevant", "pick", "any_valid", "w_agent", "w", "acc",
                                           "partials")] + [("rows", C.c_int64)]
                + [(n, C.c_int64 * 3) for n in ("pred_valid_stride", "tf_stride", "reward_valid_stride", "reward_stride", "w_stride")]
                + [(n, C.c_int32) for n in ("n_ag", "n_step", "step_training_start", "loss_for_teacher_forcing", "mask_irrelevant", "pad_")]
                + [("w_relevant", C.c_float), ("discount", C.c_float)])


class TfThreshold(C.Structure):
    """tbx_tf_threshold_t (include/tbx_hip_tf.h). Filled by hip.tf_threshold."""
    _fields_ = ([(n, C.c_void_p) for n in ("step_dev", "valid", "pose", "motion", "gt_valid", "gt_pose", "gt_motion", "tf_mask", "out_reset")]
                + [("n_rows", C.c_int64)] + [(n, C.c_int32) for n in ("n_ag", "n_step_gt", "step_host", "pad_")]
                + [(n, C.c_float) for n in ("threshold_xy", "threshold_yaw", "threshold_spd", "pad2_")])


class GradNorms(C.Structure):
    """tbx_grad_norms_t (include/tbx_hip_grad.h: the one entry point of libtbx_grad.so, `load_grad()`). Filled by hip.grad_norms_args."""
    _fields_ = ([(n, C.c_void_p) for n in ("g", "seg_off", "seg_len", "chunk_seg", "chunk_off", "chunk_len", "partial", "partial_nf", "norms",
                                           "total", "nonfinite", "coef")] + [("n", C.c_int64)]
                + [(n, C.c_int32) for n in ("n_seg", "n_chunk", "chunk_max", "norm_type")] + [("max_norm", C.c_double)])


class JointScenes(C.Structure):
    """tbx_joint_scenes_t (include/tbx_hip_sub.h: libtbx_sub.so, `load_sub()`). Filled by hip.wosac_joint_scenes."""
    _fields_ = ([(n, C.c_void_p) for n in ("pos_sim", "yaw_sim", "valid_sim", "z_sim", "object_id_sim", "pos_no_sim", "yaw_no_sim", "z_no_sim",
                                           "valid_no_sim", "object_id_no_sim", "traj_sim", "traj_no_sim", "id_sim", "id_no_sim", "count")]
                + [(n, C.c_int32) for n in ("n_sc", "n_k", "n_ag", "n_no_sim", "n_step", "n_hist", "step_current", "const_vel_z_sim",
                                            "const_vel_no_sim", "pad_")])


class WomdPred(C.Structure):
    """tbx_womd_pred_t (include/tbx_hip_sub.h). Filled by hip.womd_predictions."""
    _fields_ = ([(n, C.c_void_p) for n in ("trajs", "scores", "object_id", "mask_pred", "scenario_center", "scenario_yaw", "out_pos", "out_scores",
                                           "out_object_id", "out_count")]
                + [(n, C.c_int32) for n in ("n_sc", "n_ag", "n_mode", "n_sample")])


class WomdAggr(C.Structure):
    """tbx_womd_aggr_t (include/tbx_hip_aggr.h: the one entry point of libtbx_aggr.so, `load_aggr()`). Filled by hip.womd_aggr."""
    _fields_ = ([(n, C.c_void_p) for n in ("pred_pose", "log_prob", "ag_type", "out_trajs", "out_scores", "out_idx")]
                + [(n, C.c_int32) for n in ("n_scene", "n_k", "n_ag", "ld_t", "t_start", "n_step", "k_pred", "use_ade", "n_iter_em",
                                            "sample_first", "sample_stride", "sample_end", "has_mpa")]
                + [("aggr_thresh", C.c_float * 3), ("mpa_nms_thresh", C.c_float * 3), ("score_temperature", C.c_float)])


class IlReward(C.Structure):
    """tbx_il_reward_t (include/tbx_hip_il.h: libtbx_il.so, `load_il()`). Filled by hip.il_reward_args."""
    _fields_ = ([(n, C.c_void_p) for n in ("pred_valid", "pred_pose", "pred_motion", "gt_valid", "gt_pose", "gt_motion", "out_pos", "out_rot",
                                           "out_spd", "out_sum", "g", "d_pred_pose", "d_pred_spd")] + [("rows", C.c_int64)]
                + [(n, C.c_int64 * 3) for n in ("valid_stride", "pose_stride", "motion_stride", "out_stride", "g_stride")]
                + [(n, C.c_int32) for n in ("n_k", "n_ag", "n_step", "n_step_gt", "gt_offset", "crit_pos", "crit_rot", "crit_spd", "angular")]
                + [(n, C.c_float) for n in ("w_pos", "w_rot", "w_spd")])


RULE_COLLIDED, RULE_COLLIDED_WOSAC, RULE_RUN_ROAD_EDGE, RULE_RUN_RED_LIGHT, RULE_PASSIVE = 1, 2, 4, 8, 16
COLLISION_MAX_AG, COLLISION_LANES = 512, 4  # TBX_COLLISION_* of include/tbx_hip_reward.h: the collision kernels' agent cap / lanes per agent
METRICS_SLOTS, METRICS_PARTIAL_ROWS = 16, 256  # TBX_METRICS_* of include/tbx_hip_metrics.h: tbx_rollout_metrics' acc vector and workspace rows
LOSS_PARTIALS = 512  # TBX_LOSS_PARTIALS of include/tbx_hip_loss.h: tbx_loss_shape's float64 workspace
GRAD_CHUNK, GRAD_NORM_2, GRAD_NORM_INF = 8192, 2, 0  # TBX_GRAD_* of include/tbx_hip_grad.h: tbx_grad_norms' chunk size and norm types
SUB_MAX_OBJECTS = 1024  # TBX_SUB_MAX_OBJECTS of include/tbx_hip_sub.h: most objects per scene on a compacted axis
AGGR_MAX_K, AGGR_MAX_KEEP, AGGR_MAX_T = 128, 8, 91  # TBX_AGGR_* of include/tbx_hip_aggr.h: tbx_womd_aggr's futures, modes and steps
# TBX_IL_* / TBX_IL_ANG_* of include/tbx_hip_il.h: the criterion of an imitation term and the angular type of the rotation term, by the
# names the reference's configuration uses (torch.nn class names; angular_type null = None)
IL_SMOOTH_L1, IL_MSE, IL_L1, IL_HUBER = 0, 1, 2, 3
IL_ANG_COSINE, IL_ANG_NONE, IL_ANG_CAST, IL_ANG_VECTOR = 0, 1, 2, 3
IL_CRITERIA = {"SmoothL1Loss": IL_SMOOTH_L1, "MSELoss": IL_MSE, "L1Loss": IL_L1, "HuberLoss": IL_HUBER}
IL_ANGULAR = {"cosine": IL_ANG_COSINE, None: IL_ANG_NONE, "cast": IL_ANG_CAST, "vector": IL_ANG_VECTOR}
IL_SYMBOLS = ("tbx_il_reward_fwd", "tbx_il_reward_bwd", "tbx_train_chain_bwd_state")

_DECL = r"^(?:int|int64_t|const char\*)\s+(tbx_\w+)\s*\("


def declared_symbols() -> List[str]:
    """Entry points declared in include/tbx_hip.h and in the topical tbx_*.h headers it includes (the C-ABI contract): everything
    libtbx_hip.so exports."""
    txt = HEADER_PATH.read_text()
    for name in re.findall(r'^#include "(tbx_\w+\.h)"', txt, flags=re.M):
        txt += (HEADER_PATH.parent / name).read_text()
    return sorted(set(re.findall(_DECL, txt, flags=re.M)))


def load():
    """dlopen the in-tree libtbx_hip.so (or the build TBX_HIP_LIB names), check it exports every declared symbol and set every prototype.
    No GPU needed. A missing library is an error: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    lib_path = Path(os.environ.get("TBX_HIP_LIB", LIB_PATH))  # profiling / host-sanitizer builds only (tools/stage_clock.py, tools/sanitize_host.sh)
    if not lib_path.exists():
        raise ImportError(
            f"{lib_path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = C.CDLL(str(lib_path))
    symbols = declared_symbols()
    for s in symbols:
        if not hasattr(lib, s):
            raise ImportError(f"libtbx_hip.so does not export {s}")
    for s in symbols:  # (tbx_version included; the *_size functions below return int64_t)
        getattr(lib, s).restype = C.c_int
    lib.tbx_error_string.restype = C.c_char_p
    i32, i64, f32, vp = C.c_int, C.c_int64, C.c_float, C.c_void_p
    lib.tbx_knn_embed.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.tbx_pose_embed.argtypes = [vp, i64, vp, vp, i32, vp, i32, i32, vp]
    lib.tbx_rel_pose_dense.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.tbx_diffbar_reward.argtypes = [vp, vp, vp, vp, vp, vp, i64, f32, f32, f32, vp, vp, vp]
    lib.tbx_knarpe_attn_fwd.argtypes = [C.POINTER(Attn), vp]
    lib.tbx_knarpe_attn_fwd_form.argtypes = [C.POINTER(Attn)]
    lib.tbx_knarpe_attn_fwd_mfma.argtypes = [C.POINTER(Attn), vp]
    lib.tbx_knarpe_attn_bwd.argtypes = [C.POINTER(Attn), vp]
    lib.tbx_knarpe_dec_mid.argtypes = [C.POINTER(DecMid), vp]
    lib.tbx_knarpe_dec_layer.argtypes = [C.POINTER(DecLayer), vp]
    lib.tbx_knn_embed_multi.argtypes = [C.POINTER(KnnJob), i32, vp, vp, i32, C.POINTER(PoseEmbedJob), vp]
    lib.tbx_keyed_dropout.argtypes = [vp, vp, i64, i32, C.POINTER(Drop), vp]
    lib.tbx_linear_wgrad_splits.argtypes = [i64, i32, i32]
    lib.tbx_linear_wgrad.argtypes = [vp, i32, vp, i32, i64, i32, i32, vp, vp, vp, i32, vp]
    lib.tbx_linear_wgrad_bf16.argtypes = lib.tbx_linear_wgrad.argtypes
    lib.tbx_residual_drop_fwd.argtypes = [vp, vp, vp, vp, i64, i32, C.POINTER(Drop), vp, vp]
    lib.tbx_residual_drop_bwd.argtypes = [vp, vp, vp, i64, i32, C.POINTER(Drop), vp, vp, vp]
    lib.tbx_relu_drop_fwd.argtypes = [vp, i64, i32, C.POINTER(Drop), vp, vp]
    lib.tbx_relu_drop_bwd.argtypes = [vp, vp, i64, i32, C.c_float, vp, vp]
    lib.tbx_pair_bias_relu.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, vp]
    lib.tbx_pointnet_tail_fwd.argtypes = [vp, vp, i64, i32, i32, C.POINTER(Drop), vp, vp]
    lib.tbx_pointnet_tail_bwd.argtypes = [vp, vp, vp, i64, i32, i32, C.c_float, vp, vp]
    lib.tbx_masked_maxpool_fwd.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    lib.tbx_masked_maxpool_bwd.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    lib.tbx_layernorm_fwd.argtypes = [vp, vp, vp, C.c_float, i64, i32, vp, vp, vp, vp]
    lib.tbx_layernorm_bwd_partials.argtypes = [i64]
    lib.tbx_layernorm_bwd.argtypes = [vp, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp]
    lib.tbx_layernorm_bwd_add.argtypes = [vp, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp]
    lib.tbx_train_chain_fwd.argtypes = [C.POINTER(TrainChainArgs), vp, i64, i64, i32, i32, vp]
    lib.tbx_train_chain_fwd_windows.argtypes = [C.POINTER(TrainChainArgs), vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.tbx_train_chain_bwd.argtypes = [C.POINTER(TrainChainArgs), vp, i64, i64, vp, vp, vp]
    lib.tbx_knn_inverse.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.tbx_pack_weight_size.argtypes = [i32, i32, i32]
    lib.tbx_pack_weight_size.restype = C.c_int64
    lib.tbx_pack_weight.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.tbx_pack_weight_split.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.tbx_pack_weight_gemv_size.argtypes = [i32, i32, i32]
    lib.tbx_pack_weight_gemv_size.restype = C.c_int64
    lib.tbx_pack_weight_gemv.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.tbx_layer_tile.argtypes = [C.POINTER(LayerTile), vp]
    lib.tbx_heads_tile.argtypes = [C.POINTER(HeadsTile), vp]
    lib.tbx_window_tile.argtypes = [C.POINTER(WindowTile), vp]
    lib.tbx_layer_tile_bf16.argtypes = [C.POINTER(LayerTile), vp]
    lib.tbx_heads_tile_bf16.argtypes = [C.POINTER(HeadsTile), vp]
    lib.tbx_window_tile_bf16.argtypes = [C.POINTER(WindowTile), vp]
    lib.tbx_front.argtypes = [C.POINTER(Front), vp]
    lib.tbx_front_pair.argtypes = [C.POINTER(Front), C.POINTER(Front), vp]
    lib.tbx_knarpe_dec_layer_pair.argtypes = [C.POINTER(DecLayer), C.POINTER(DecLayer), vp]
    lib.tbx_tall_linear.argtypes = [C.POINTER(Linear), vp]
    lib.tbx_tall_linear_bf16.argtypes = [C.POINTER(Linear), vp]
    lib.tbx_tl_tail_tile.argtypes = [vp, i64, C.POINTER(TlTail), vp]
    lib.tbx_tl_tail_tile_bf16.argtypes = lib.tbx_tl_tail_tile.argtypes
    lib.tbx_pack_weight_mfma32_size.argtypes = [i32, i32, i32]
    lib.tbx_pack_weight_mfma32_size.restype = C.c_int64
    lib.tbx_pack_weight_mfma32.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.tbx_pack_weight_mfma32_multi.argtypes = [C.POINTER(PackJob), i32, vp]
    lib.tbx_rowchain_live.argtypes = [C.POINTER(Stage), i32, i64, i32, i32, i32, i32, vp]
    lib.tbx_rowchain.argtypes = [C.POINTER(Stage), i32, i64, i32, i32, i32, vp]
    lib.tbx_rowchain_ex.argtypes = [C.POINTER(Stage), i32, i64, i32, i32, i32, i32, i32, vp]
    lib.tbx_agent_prep.argtypes = [C.POINTER(AgentPrepArgs), vp]
    lib.tbx_tl_prep.argtypes = [vp, i32, i32, i32, C.POINTER(TlRows), vp]
    lib.tbx_map_prep.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.tbx_sim_step.argtypes = [C.POINTER(SimState), i32, C.POINTER(TlRows), vp]
    lib.tbx_rule_tables.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.tbx_rule_grid.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.tbx_rule_grid_cells.argtypes = []
    lib.tbx_rule_check.argtypes = [C.POINTER(RuleCtx), vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.tbx_rule_accumulate.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.tbx_filter_futures.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, f32, i32, vp, vp, vp, vp, vp]
    lib.tbx_womd_modes.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), f32, i32, i32, i32,
                                   vp, vp, vp, vp]
    lib.tbx_pose_to_global.argtypes = [vp, i32, vp, i32, vp, vp, i32, i64, i32, i32, vp, vp, vp]
    lib.tbx_attn_fold_fwd.argtypes = [vp] * 14
    lib.tbx_attn_fold_bwd.argtypes = [vp] * 19
    lib.tbx_rule_navi_check.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.tbx_rollout_metrics.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.tbx_collision_reward_fwd.argtypes = [vp, vp, i64, i32, i32, i32, i64, i64, i64, i64, i64, i64, vp, i32, vp, i64, i64, i64, vp, vp]
    lib.tbx_collision_reward_bwd.argtypes = [vp, vp, i64, i32, i32, i32, i64, i64, i64, i64, i64, i64, vp, i32, vp, i64, i64, i64, vp, vp, vp]
    lib.tbx_train_chain_bwd_pose.argtypes = [C.POINTER(TrainChainArgs), vp, i64, i64, vp, vp, vp, vp]
    lib.tbx_loss_shape.argtypes = [C.POINTER(LossShape), vp]
    lib.tbx_tf_threshold.argtypes = [C.POINTER(TfThreshold), vp]
    if lib.tbx_version() != 7:
        raise ImportError("libtbx_hip.so ABI version mismatch")
    # (an entry point without argtypes would get 64-bit handles - stream pointers under graph capture - as C ints)
    untyped = [s for s in symbols if getattr(lib, s).argtypes is None and s not in ("tbx_error_string", "tbx_version")]
    if untyped:
        raise ImportError(f"abi.load(): no argtypes for {untyped}")
    _lib = lib
    return lib


def load_grad():
    """dlopen the in-tree libtbx_grad.so (built by the same Makefile) and set the prototype of its one entry point, tbx_grad_norms
    (include/tbx_hip_grad.h). No GPU needed. A missing library is an error: there is no fallback path."""
    global _grad_lib
    if _grad_lib is not None:
        return _grad_lib
    if not GRAD_LIB_PATH.exists():
        raise ImportError(f"{GRAD_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = C.CDLL(str(GRAD_LIB_PATH))
    if not hasattr(lib, "tbx_grad_norms"):
        raise ImportError("libtbx_grad.so does not export tbx_grad_norms")
    lib.tbx_grad_norms.restype = C.c_int
    lib.tbx_grad_norms.argtypes = [C.POINTER(GradNorms), C.c_void_p]
    _grad_lib = lib
    return lib


def load_sub():
    """dlopen the in-tree libtbx_sub.so (built by the same Makefile) and set the prototypes of its two entry points, tbx_wosac_joint_scenes
    and tbx_womd_predictions (include/tbx_hip_sub.h). No GPU needed. A missing library is an error: there is no fallback path."""
    global _sub_lib
    if _sub_lib is not None:
        return _sub_lib
    if not SUB_LIB_PATH.exists():
        raise ImportError(f"{SUB_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = C.CDLL(str(SUB_LIB_PATH))
    for name, struct in (("tbx_wosac_joint_scenes", JointScenes), ("tbx_womd_predictions", WomdPred)):
        if not hasattr(lib, name):
            raise ImportError(f"libtbx_sub.so does not export {name}")
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.POINTER(struct), C.c_void_p]
    _sub_lib = lib
    return lib


def load_aggr():
    """dlopen the in-tree libtbx_aggr.so (built by the same Makefile) and set the prototype of its one entry point, tbx_womd_aggr
    (include/tbx_hip_aggr.h). No GPU needed. A missing library is an error: there is no fallback path."""
    global _aggr_lib
    if _aggr_lib is not None:
        return _aggr_lib
    if not AGGR_LIB_PATH.exists():
        raise ImportError(f"{AGGR_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = C.CDLL(str(AGGR_LIB_PATH))
    if not hasattr(lib, "tbx_womd_aggr"):
        raise ImportError("libtbx_aggr.so does not export tbx_womd_aggr")
    lib.tbx_womd_aggr.restype = C.c_int
    lib.tbx_womd_aggr.argtypes = [C.POINTER(WomdAggr), C.c_void_p]
    _aggr_lib = lib
    return lib


def load_il():
    """dlopen the in-tree libtbx_il.so (built by the same Makefile) and set the prototypes of its three entry points, tbx_il_reward_fwd,
    tbx_il_reward_bwd and tbx_train_chain_bwd_state (include/tbx_hip_il.h). No GPU needed. A missing library is an error: there is no
    fallback path."""
    global _il_lib
    if _il_lib is not None:
        return _il_lib
    if not IL_LIB_PATH.exists():
        raise ImportError(f"{IL_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = C.CDLL(str(IL_LIB_PATH))
    for name in IL_SYMBOLS:
        if not hasattr(lib, name):
            raise ImportError(f"libtbx_il.so does not export {name}")
        getattr(lib, name).restype = C.c_int
    lib.tbx_il_reward_fwd.argtypes = [C.POINTER(IlReward), C.c_void_p]
    lib.tbx_il_reward_bwd.argtypes = [C.POINTER(IlReward), C.c_void_p]
    lib.tbx_train_chain_bwd_state.argtypes = [C.POINTER(TrainChainArgs), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
    _il_lib = lib
    return lib
