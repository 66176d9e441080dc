/*
 * Trajectory aggregation of the WOMD post-processing on the device: ONE entry point, exported by a library of its own, libtbx_aggr.so
 * (source: csrc/womd_aggr.hip). Like tbx_hip_grad.h and tbx_hip_sub.h this is not a section of include/tbx_hip.h and that header does not
 * include this one: the entry points of libtbx_hip.so are the closed list of ABI 7. The contract is the same - device pointers to
 * caller-owned buffers, nothing allocated or retained, ONE kernel enqueued on `stream` (a hipStream_t, passed as void* so that the header
 * compiles as plain C), the TBX_* return codes of tbx_hip.h before any launch; tbx_error_string of libtbx_hip.so names them. No atomics:
 * two calls on the same input leave the same bytes, and EVERY output element is written by every call. The host reads nothing back: the
 * call can be captured into a graph.
 */
#ifndef TBX_HIP_AGGR_H
#define TBX_HIP_AGGR_H

#include <stdint.h>

#include "tbx_hip.h" /* TBX_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

#define TBX_AGGR_MAX_K 128   /* most joint futures per agent */
#define TBX_AGGR_MAX_KEEP 8  /* most modes kept */
#define TBX_AGGR_MAX_T 91    /* most future steps */

/* ------------------------------------------------------------------------------------------------------------------
 * tbx_womd_aggr: WOMDPostProcessing.forward with a non-empty aggr_thresh (data_modules/womd_post_processing.py:37-72 and traj_aggr
 * :178-278 of the reference) for n_k > k_pred, one workgroup per (scene, agent), on the rollout log in place - addressed as
 * tbx_womd_modes addresses it: pred_pose[(s * n_k + j), a, t_start + t, :] for t < n_step, rows of ld_t steps.
 *
 * Per (scene, agent), with s[j] the softmax of the log-probabilities (float64; zeros when log_prob is NULL), thr the float32 sum
 * ((0 + ty0 a0) + ty1 a1) + ty2 a2 of the agent's type bytes and aggr_thresh (0 for an agent without a type: nothing is within it) and
 * d(a, b) the mean over the n_step steps of the xy distance (use_ade) or the last step's (float32, summed in step order):
 *   seeds    k_pred times: p = the FIRST maximum of work (work = s at the start); work[j] *= 0.1f where d(p, j) < thr (p itself included
 *            when thr > 0); work[p] -= 1. out_idx holds the picks in pick order.
 *   centres  start as the (x, y, yaw) rows of the picks, their scores as s[picks].
 *   EM       n_iter_em times: every future joins its nearest centre (d on xy; ties: the FIRST minimum); empty clusters are repaired in
 *            ascending cluster index, one after the other, counts re-taken after each: the largest cluster (FIRST maximum) gives its
 *            first count / 2 members in ascending future index to the empty one; each centre becomes the arithmetic mean of its members'
 *            rows (float32 sum in ascending future index, divided by the count; yaw is not wrapped), its score the mean of their s.
 *   after    scores divided by their sum; then, as tbx_womd_modes: mpa_nms on the centres (has_mpa), the temperature (> 0), and
 *            out_trajs = the centres at the steps sample_first, sample_first + sample_stride, .. < sample_end.
 * n_iter_em = 0 returns the picks' rows bit for bit.
 *
 * Returns TBX_ERR_ARG for a NULL struct, a NULL pred_pose / ag_type / out_trajs / out_scores, a non-positive n_scene, n_k, n_ag, ld_t,
 * n_step or k_pred, t_start < 0, t_start + n_step > ld_t, n_iter_em < 0, sample_first < 0, sample_stride < 1, sample_end > n_step, or
 * n_k <= k_pred (nothing to aggregate: that is tbx_womd_modes' case); TBX_ERR_UNSUPPORTED for n_k > TBX_AGGR_MAX_K, k_pred >
 * TBX_AGGR_MAX_KEEP, n_step > TBX_AGGR_MAX_T or n_scene * n_ag >= 2^31.
 */
typedef struct tbx_womd_aggr_t {
  const float* pred_pose;   /* [n_scene * n_k, n_ag, ld_t, 3] x, y, yaw */
  const float* log_prob;    /* [n_scene * n_k, n_ag] or NULL (zeros) */
  const uint8_t* ag_type;   /* [n_scene, n_ag, 3] 0 / 1: veh, ped, cyc */
  float* out_trajs;         /* [n_scene, n_ag, k_pred, n_out, 3] out, n_out = the number of sampled steps */
  float* out_scores;        /* [n_scene, n_ag, k_pred] out */
  int32_t* out_idx;         /* [n_scene, n_ag, k_pred] out: the seeds, or NULL */
  int32_t n_scene, n_k, n_ag, ld_t, t_start, n_step, k_pred, use_ade, n_iter_em, sample_first, sample_stride, sample_end, has_mpa;
  float aggr_thresh[3];     /* metres: veh, ped, cyc */
  float mpa_nms_thresh[3];  /* read if has_mpa */
  float score_temperature;  /* > 0: on */
} tbx_womd_aggr_t;

int tbx_womd_aggr(const tbx_womd_aggr_t* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TBX_HIP_AGGR_H */
