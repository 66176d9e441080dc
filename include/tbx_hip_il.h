/*
 * The imitation terms of the differentiable reward with the criteria and angular types of the reference's configuration
 * (configs/model/sim_agent.yaml: l_pos / l_rot / l_spd `criterion`, l_rot `angular_type`; utils/rewards.py:25-33,58-74,
 * models/metrics/loss.py:9-36): THREE entry points, exported by a library of its own, libtbx_il.so (source: csrc/il_reward.hip). Like
 * tbx_hip_grad.h, tbx_hip_sub.h and tbx_hip_aggr.h this is not a section of include/tbx_hip.h and that header does not include this one:
 * the entry points of libtbx_hip.so are the closed list of ABI 7. The contract is the same - device pointers to caller-owned buffers,
 * nothing allocated or retained, ONE kernel enqueued on `stream` (a hipStream_t, passed as void* so that the header compiles as plain C),
 * the TBX_* return codes of tbx_hip.h before any launch; tbx_error_string of libtbx_hip.so names them. No atomics: two calls on the same
 * input leave the same bytes, and EVERY output element is written by every call. The host reads nothing back: the calls can be captured
 * into a graph.
 *
 * The reward never feeds back into the simulated state, so - like the collision term (tbx_hip_reward.h) - the terms are one kernel pair
 * over a FINISHED log: tbx_sim_step and tbx_train_chain_fwd keep the default terms written into them, and a caller with another
 * configuration overwrites the reward with tbx_il_reward_fwd (and, in training, runs the chain with zero weights, tbx_il_reward_bwd and
 * tbx_train_chain_bwd_state).
 */
#ifndef TBX_HIP_IL_H
#define TBX_HIP_IL_H

#include <stdint.h>

#include "tbx_hip.h" /* TBX_ERR_* codes, tbx_train_chain_t */

#ifdef __cplusplus
extern "C" {
#endif

/* criterion of a term (torch.nn.<name>(reduction="none") of the reference), on d = gt - pred:
 *   SMOOTH_L1, HUBER   |d| < 1 ? 0.5 d^2 : |d| - 0.5        derivative clamp(d, -1, 1)
 *                      (torch.nn.HuberLoss() at delta = 1 IS torch.nn.SmoothL1Loss() at beta = 1, value and gradient: two names, one definition)
 *   MSE                d^2                                   derivative 2 d
 *   L1                 |d|                                   derivative sign(d), sign(0) = 0 */
#define TBX_IL_SMOOTH_L1 0
#define TBX_IL_MSE 1
#define TBX_IL_L1 2
#define TBX_IL_HUBER 3

/* angular type of the rotation term, on the yaws gw (ground truth) and pw (prediction):
 *   COSINE   0.5 (1 - cos(gw - pw)); the rotation criterion is not read
 *   NONE     crit(gw - pw), not wrapped
 *   CAST     crit(wrap(gw - pw)), wrap(a) in float32: r = fmodf(a + pi, 2 pi); if (r != 0 && r < 0) r += 2 pi; r - pi  (slope 1)
 *   VECTOR   crit(cos gw - cos pw) + crit(sin gw - sin pw) */
#define TBX_IL_ANG_COSINE 0
#define TBX_IL_ANG_NONE 1
#define TBX_IL_ANG_CAST 2
#define TBX_IL_ANG_VECTOR 3

/* ------------------------------------------------------------------------------------------------------------------
 * tbx_il_reward_t: a log of `rows` rollouts x n_step slots x n_ag agents, every tensor a VIEW [rows, n_step, n_ag(, 3)] addressed
 * through the element strides {row, step, agent} (the x / y / yaw and speed / acc / yaw-rate triples contiguous) - the rollout engine's
 * agent-major log [rows, n_ag, n_step, ..] and the training chain's time-major log [rows, n_step, n_ag, ..] are read where they lie -
 * and the ground truth [rows / n_k, n_ag, n_step_gt(, 3)], dense, shared by the n_k consecutive rows of a scene. Slot t is compared
 * with ground-truth index t + gt_offset (1 for both logs: slot t holds step t + 1; 0 for one step against one step).
 *
 * With d = gt - pred per component:
 *   e_pos = crit_pos(gx - px) + crit_pos(gy - py),  e_spd = crit_spd(g_spd - p_spd),  e_rot by `angular` (above)
 *   r_pos = -w_pos e_pos, r_rot = -w_rot e_rot, r_spd = -w_spd e_spd, each 0 where !(pred_valid && gt_valid) and at every slot with
 *   t + gt_offset >= n_step_gt;  sum = (r_pos + r_rot) + r_spd.
 * All codes 0 = the terms tbx_sim_step / tbx_train_chain_fwd / tbx_diffbar_reward compute (an all-zero struct is that configuration).
 * Arithmetic: float32, no contraction into fused multiply-adds.
 */
typedef struct tbx_il_reward_t {
  const uint8_t* pred_valid; /* view [rows, n_step, n_ag] 0 / 1, valid_stride */
  const float* pred_pose;    /* view [rows, n_step, n_ag, 3] x, y, yaw, pose_stride */
  const float* pred_motion;  /* view [rows, n_step, n_ag, 3] speed first, motion_stride */
  const uint8_t* gt_valid;   /* [rows / n_k, n_ag, n_step_gt] */
  const float* gt_pose;      /* [rows / n_k, n_ag, n_step_gt, 3] */
  const float* gt_motion;    /* [rows / n_k, n_ag, n_step_gt, 3] */
  /* forward: planes [rows, n_step, n_ag], all four through out_stride (the four columns of a [.., 4] tensor are four such planes).
   * out_sum is required; out_pos / out_rot / out_spd are all given or all NULL (then only the sum is written). */
  float* out_pos;
  float* out_rot;
  float* out_spd;
  float* out_sum;
  /* backward */
  const float* g;     /* view [rows, n_step, n_ag], g_stride: dL/d(sum) */
  float* d_pred_pose; /* [rows, n_step, n_ag, 3] dense out: dL/d(x, y, yaw of the prediction), 0 wherever the forward masked */
  float* d_pred_spd;  /* [rows, n_step, n_ag] dense out: dL/d(predicted speed), 0 wherever the forward masked */
  int64_t rows;
  int64_t valid_stride[3], pose_stride[3], motion_stride[3], out_stride[3], g_stride[3]; /* elements: {row, step, agent} */
  int32_t n_k, n_ag, n_step, n_step_gt, gt_offset;
  int32_t crit_pos, crit_rot, crit_spd; /* TBX_IL_* */
  int32_t angular;                      /* TBX_IL_ANG_* */
  float w_pos, w_rot, w_spd;
} tbx_il_reward_t;

/* Forward: writes the planes. Reads neither g nor d_pred_*.
 * TBX_ERR_ARG: NULL struct, a NULL pred_* / gt_* / out_sum, only some of out_pos / out_rot / out_spd, rows / n_k / n_ag / n_step /
 * n_step_gt < 1, rows % n_k != 0, gt_offset < 0, a negative stride; TBX_ERR_UNSUPPORTED: a criterion or angular code that is none of the
 * above. Nothing is launched then. */
int tbx_il_reward_fwd(const tbx_il_reward_t* args /* host */, void* stream);

/* Backward, gradients with respect to the prediction: with c'_x the derivative of the term's criterion,
 *   d_px = g w_pos c'_pos(gx - px), d_py likewise, d_spd = g w_spd c'_spd(g_spd - p_spd), d_pw = -g w_rot d(e_rot)/d(pw):
 *   COSINE  d_pw = g 0.5 w_rot sin(gw - pw);   NONE / CAST  d(e_rot)/d(pw) = -c'_rot(gw - pw | wrap(gw - pw));
 *   VECTOR  d(e_rot)/d(pw) = c'_rot(cos gw - cos pw) sin pw - c'_rot(sin gw - sin pw) cos pw.
 * Reads no out_* plane. Same refusals, with g / d_pred_pose / d_pred_spd in place of the out planes. */
int tbx_il_reward_bwd(const tbx_il_reward_t* args /* host */, void* stream);

/* The training chain's reverse walk (tbx_train_chain_bwd of tbx_hip.h: same kernel source, csrc/train_chain_core.h) with adjoints of
 * the prediction from outside the chain: d_pred_pose [n, T, A, 3] is added to the adjoint of (x', y', yaw') as tbx_train_chain_bwd_pose
 * adds it, d_pred_spd [n, T, A] to the adjoint of the predicted speed at the same place. Either may be NULL; with both NULL the result is
 * tbx_train_chain_bwd's bit for bit. */
int tbx_train_chain_bwd_state(const tbx_train_chain_t* c /* host */, const float* mean, int64_t mean_stride_n, int64_t mean_stride_t,
                              const float* d_reward, const float* d_pred_pose, const float* d_pred_spd, float* d_mean, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TBX_HIP_IL_H */
