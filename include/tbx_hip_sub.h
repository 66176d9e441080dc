/*
 * Submission records of the test loop on the device: TWO entry points, exported by a library of their own, libtbx_sub.so (source:
 * csrc/sub_records.hip). Like tbx_hip_grad.h this is not a section of include/tbx_hip.h and that header does not include this one: the
 * entry points of libtbx_hip.so are the closed list of ABI 7. The contract is the same - device pointers to caller-owned buffers,
 * nothing allocated or retained, ONE kernel enqueued on `stream` (a hipStream_t, passed as void* so that the header compiles as plain
 * C), the TBX_* return codes of tbx_hip.h before any launch; tbx_error_string of libtbx_hip.so names them. No atomics: two calls on
 * the same input leave the same bytes, and EVERY output element is written by every call - the result does not depend on what the
 * buffers held before.
 *
 * What they replace are the host loops over scenes x rollouts x objects behind the reference's challenge writers, up to - not including -
 * the protobuf messages: per-scene compaction by a validity mask, constant-velocity extrapolation, the global-frame transform.
 */
#ifndef TBX_HIP_SUB_H
#define TBX_HIP_SUB_H

#include <stdint.h>

#include "tbx_hip.h" /* TBX_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

#define TBX_SUB_MAX_OBJECTS 1024 /* most objects per scene on a compacted axis (n_ag, n_no_sim): the data has 64 - 128 and 256 */

/* ------------------------------------------------------------------------------------------------------------------
 * tbx_wosac_joint_scenes: the joint scenes of WOSACPostProcessing.get_scenario_rollouts (data_modules/wosac_post_processing.py:142-202
 * of the reference: _get_sim_joint_scene, _get_no_sim_joint_scene) from the `wosac_data` arrays its forward returns.
 *
 * Compaction: an object is kept iff it is valid at step_current. Kept objects come in index order (the reference's np.where), packed to
 *   the front of their axis; count[s] = (kept sim objects, kept no-sim objects). Rows from the count on are zeros, their ids -1.
 * Sim objects: traj_sim[s, k, j, t] = (x, y, z, heading) with x, y, heading bit copies of pos_sim / yaw_sim[s, k, a_j, t] and
 *   z = fmaf(v_z, (float)(t + 1), z_sim[s, a_j, c]), c = step_current, v_z = z[c] - z[c-1] (float32) if const_vel_z_sim and the object is
 *   valid at c and c-1, else 0.
 * No-sim objects: traj_no_sim[s, j, t] = the same rule for x, y and z with const_vel_no_sim, heading yaw_no_sim[s, a_j, c] at every step.
 *   Stored ONCE per scene (the reference puts a copy into each of the n_k joint scenes): the writer repeats it.
 * The fmaf is one rounding of z + v (t + 1): the correctly rounded float32 of what the reference computes in float64; with v = 0 it is
 *   the value at c exactly.
 *
 * Returns TBX_ERR_ARG for a NULL struct, a NULL array with a non-zero extent, n_sc < 1, n_k < 1, n_step < 1, n_ag < 0, n_no_sim < 0,
 * step_current < 1 (the reference would wrap to index -1) or step_current >= n_hist; TBX_ERR_UNSUPPORTED for n_ag or n_no_sim above
 * TBX_SUB_MAX_OBJECTS; TBX_ERR_ALIGN for a traj_sim / traj_no_sim that is not 16-byte or a pos_sim that is not 8-byte aligned.
 * n_ag == 0 and n_no_sim == 0 are legal (count is still written).
 */
typedef struct tbx_joint_scenes_t {
  const float* pos_sim;            /* [n_sc, n_k, n_ag, n_step, 2] global frame */
  const float* yaw_sim;            /* [n_sc, n_k, n_ag, n_step] */
  const uint8_t* valid_sim;        /* [n_sc, n_ag, n_hist] 0 / 1 */
  const float* z_sim;              /* [n_sc, n_ag, n_hist] */
  const int64_t* object_id_sim;    /* [n_sc, n_ag] */
  const float* pos_no_sim;         /* [n_sc, n_no_sim, n_hist, 2] global frame */
  const float* yaw_no_sim;         /* [n_sc, n_no_sim, n_hist] */
  const float* z_no_sim;           /* [n_sc, n_no_sim, n_hist] */
  const uint8_t* valid_no_sim;     /* [n_sc, n_no_sim, n_hist] 0 / 1 */
  const int64_t* object_id_no_sim; /* [n_sc, n_no_sim] */
  float* traj_sim;                 /* [n_sc, n_k, n_ag, n_step, 4] out: center_x, center_y, center_z, heading */
  float* traj_no_sim;              /* [n_sc, n_no_sim, n_step, 4] out */
  int64_t* id_sim;                 /* [n_sc, n_ag] out */
  int64_t* id_no_sim;              /* [n_sc, n_no_sim] out */
  int32_t* count;                  /* [n_sc, 2] out: kept sim, kept no-sim objects */
  int32_t n_sc, n_k, n_ag, n_no_sim;
  int32_t n_step;       /* future steps T = step_gt - step_current */
  int32_t n_hist;       /* history steps */
  int32_t step_current; /* 1 .. n_hist - 1 */
  int32_t const_vel_z_sim, const_vel_no_sim, pad_;
} tbx_joint_scenes_t;

int tbx_wosac_joint_scenes(const tbx_joint_scenes_t* args /* host */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * tbx_womd_predictions: the prediction records of SubWOMD (utils/submission.py:54-62 of the reference: the xy of the scored modes moved
 * to the global frame; :94-96: the agents with mask_pred selected per scene).
 *
 * out_pos[s, j, m, i] = R(scenario_yaw[s]) trajs[s, a_j, m, i, :2] + scenario_center[s] - the transform tbx_pose_to_global computes, bit
 * for bit (one device function, csrc/pose_global_core.h) -, out_scores[s, j] = scores[s, a_j], out_object_id[s, j] = object_id[s, a_j]
 * for the agents a_0 < a_1 < .. with mask_pred, out_count[s] their number. Rows from the count on are zeros, their ids -1.
 *
 * Returns TBX_ERR_ARG for a NULL struct or array, n_sc < 1, n_ag < 1, n_mode < 1, n_sample < 1; TBX_ERR_UNSUPPORTED for n_ag above
 * TBX_SUB_MAX_OBJECTS; TBX_ERR_ALIGN for an out_pos that is not 8-byte aligned.
 */
typedef struct tbx_womd_pred_t {
  const float* trajs;           /* [n_sc, n_ag, n_mode, n_sample, 3] scenario frame: x, y, yaw */
  const float* scores;          /* [n_sc, n_ag, n_mode] */
  const int64_t* object_id;     /* [n_sc, n_ag] */
  const uint8_t* mask_pred;     /* [n_sc, n_ag] 0 / 1 */
  const float* scenario_center; /* [n_sc, 2] */
  const float* scenario_yaw;    /* [n_sc] */
  float* out_pos;               /* [n_sc, n_ag, n_mode, n_sample, 2] out */
  float* out_scores;            /* [n_sc, n_ag, n_mode] out */
  int64_t* out_object_id;       /* [n_sc, n_ag] out */
  int32_t* out_count;           /* [n_sc] out */
  int32_t n_sc, n_ag, n_mode, n_sample;
} tbx_womd_pred_t;

int tbx_womd_predictions(const tbx_womd_pred_t* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TBX_HIP_SUB_H */
