/*
 * The reward section of the C ABI of include/tbx_hip.h, exported by libtbx_hip.so like every other entry point (tbx_hip.h includes this
 * header; its contract - device pointers to caller-owned buffers, nothing allocated or retained, kernels only enqueued on `stream`,
 * TBX_* return codes - holds here too). Sources: csrc/collision.hip and csrc/train_chain.hip. The entry points are the reward term that
 * couples the agents of a scene (differentiable_reward.w_collision > 0) and the training chain's reverse walk with an adjoint of the
 * predicted pose as a further input.
 */
#ifndef TBX_HIP_REWARD_H
#define TBX_HIP_REWARD_H

#include <stdint.h>

#include "tbx_hip.h" /* tbx_train_chain_t, TBX_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * Relaxed five-circle overlap of utils/rewards.py:87-154 (DifferentiableReward._get_r_traffic_rule_approx) for every (row, step)
 * of a pose log, UNWEIGHTED (the caller multiplies by -w_collision): c [n_rows, n_t, n_ag] in [0, 1]. Replaces ~120 elementwise
 * launches per step on a dense [n_sc, A, A, 5, 5] tensor by one launch for the whole log. float32, in the reference's order:
 *   w = min(size0, size1), l = max(size0, size1), d = (l - w) / 4; centroid k = xy + ((k - 2) (cos yaw, sin yaw)) d, k = 0..4;
 *   eps = FLT_EPSILON, r = w / 2 + eps; pair distance sqrt(dx^2 + dy^2) + eps, minimum over the 25 circle pairs;
 *   c_ij = max(1 - dmin / (r_i + r_j), 0), forced to 0 for i == j or when either agent is invalid at the step;
 *   reduce_with_max != 0: c_i = max_j c_ij;  else: c_i = sum_j min(c_ij, 1) / n_valid, n_valid = the step's count of valid agents
 *   (summed in ascending j within TBX_COLLISION_LANES contiguous j-ranges whose partial sums are added in ascending order).
 * DEVIATION: a (row, step) without a valid agent gives c = 0 and zero gradient in sum mode (the reference: 0 / 0 = NaN).
 *   pose f32, valid u8 0/1: element (row, agent a, step t, component k) is pose[row * pose_stride_row + a * pose_stride_ag +
 *   t * pose_stride_t + k] and valid[row * valid_stride_row + a * valid_stride_ag + t * valid_stride_t] - strides in ELEMENTS, the
 *   three pose components contiguous. Both the training chain's [n, T, A, 3] log (strides T*A*3, 3, A*3) and a time slice of the
 *   rollout engine's [rows, A, ld_t, 3] log (strides A*ld_t*3, ld_t*3, 3; the pointer addresses the first step read) are read in
 *   place. c (and g below) are addressed the same way through c_stride_* (g_stride_*).
 *   ag_size [n_rows / n_k, n_ag, 3] (length, width, height) of the row's scene (row / n_k).
 *   arg: NULL, or int32 [n_rows, n_t, n_ag] (dense, overwritten) - what tbx_collision_reward_bwd needs of a max-mode forward: the
 *   partner j that gave c_i (the lowest such j), -1 where c_i == 0. Not touched in sum mode.
 * tbx_collision_reward_bwd: d_pose [n_rows, n_t, n_ag, 3] (dense; x, y, yaw; OVERWRITTEN, not accumulated) from g = dL/dc. Agent a
 * receives its own row's contribution and that of every row i whose term reads the pair (i, a). No atomics: the
 * TBX_COLLISION_LANES lanes of agent a walk contiguous ranges of i in index order and their sums are added in lane order - two calls
 * give bit-equal results. Conventions (torch's on the CPU): coincident centres (distance 0 before eps) pass no gradient; the minimum
 * over the 25 circle pairs sends the gradient to the FIRST minimum (own circle major, partner's circle minor); the clamp at 0
 * passes gradient where 1 - dmin / r_sum >= 0; the max over j sends it to the lowest j on ties (torch splits among ties: ties at 0
 * carry no gradient either way). ag_size gets no gradient. arg: the forward's, required in max mode (NULL: TBX_ERR_ARG), ignored in
 * sum mode.
 * One workgroup per (row, step); centroids, radii and validity of the n_ag agents are staged in LDS.
 * A NULL pointer (arg aside), n_rows / n_ag / n_t / n_k < 1, n_rows % n_k != 0, a pose stride < 3 or another stride < 1 along an
 * axis longer than 1: TBX_ERR_ARG. n_ag > TBX_COLLISION_MAX_AG or n_rows * n_t >= 2^31: TBX_ERR_UNSUPPORTED. Both before any launch.
 * One launch each, nothing allocated: both run inside a captured graph. */
#define TBX_COLLISION_MAX_AG 512
#define TBX_COLLISION_LANES 4
int tbx_collision_reward_fwd(const float* pose, const uint8_t* valid, int64_t n_rows, int n_k, int n_ag, int n_t, int64_t pose_stride_row,
                             int64_t pose_stride_ag, int64_t pose_stride_t, int64_t valid_stride_row, int64_t valid_stride_ag,
                             int64_t valid_stride_t, const float* ag_size, int reduce_with_max, float* c, int64_t c_stride_row,
                             int64_t c_stride_ag, int64_t c_stride_t, int32_t* arg, void* stream);
int tbx_collision_reward_bwd(const float* pose, const uint8_t* valid, int64_t n_rows, int n_k, int n_ag, int n_t, int64_t pose_stride_row,
                             int64_t pose_stride_ag, int64_t pose_stride_t, int64_t valid_stride_row, int64_t valid_stride_ag,
                             int64_t valid_stride_t, const float* ag_size, int reduce_with_max, const float* g, int64_t g_stride_row,
                             int64_t g_stride_ag, int64_t g_stride_t, const int32_t* arg, float* d_pose, void* stream);

/* tbx_train_chain_bwd (include/tbx_hip.h) with one more, nullable input: d_pred_pose [n, T, A, 3], an adjoint of the step's
 * PREDICTION (pred_pose: x, y, yaw) from a term outside the chain - the collision term above. It is added to the prediction's
 * adjoint whether or not the step was overridden by teacher forcing (the term reads the prediction, as the imitation terms do).
 * d_pred_pose == NULL is tbx_train_chain_bwd, bit for bit (both launch the one reverse-walk kernel of csrc/train_chain.hip; that entry
 * point is this one's NULL case). */
int tbx_train_chain_bwd_pose(const tbx_train_chain_t* c /* host */, const float* mean, int64_t mean_stride_n, int64_t mean_stride_t,
                             const float* d_reward, const float* d_pred_pose, float* d_mean, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TBX_HIP_REWARD_H */
