/*
 * The teacher-forcing section of the C ABI of include/tbx_hip.h, exported by libtbx_hip.so like every other entry point (tbx_hip.h
 * includes this header; its contract - device pointers to caller-owned buffers, nothing allocated or retained, kernels only enqueued on
 * `stream`, TBX_* return codes before any launch - holds here too). Source: csrc/tf_threshold.hip. It is the error-threshold form of
 * teacher forcing (utils/teacher_forcing.py:128-151: threshold_xy, threshold_yaw, threshold_spd): an agent whose simulated state has
 * drifted from the logged one by more than a threshold is put back on the ground truth at the next step.
 */
#ifndef TBX_HIP_TF_H
#define TBX_HIP_TF_H

#include <stdint.h>

#include "tbx_hip.h" /* TBX_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * tbx_tf_threshold: the resets of ONE step s, ORed into column s of the teacher-forcing table BEFORE the step reads it. The reference
 * does the same in place on ag_teacher_forcing[:, :, step] (teacher_forcing.py:129-145); every step kernel (tbx_sim_step, the fused tail
 * of tbx_knarpe_dec_layer(_pair), tbx_train_chain_fwd) already indexes the table by the step and logs what it read, so none of them
 * changes. s = *step_dev when step_dev != NULL (the word tbx_sim_state_t.step points to: one captured graph serves every step), else
 * step_host. For 0 < s < n_step_gt, per (row, agent), in float32 and in the reference's operation order, no product fused into a sum:
 *   inv   = !(valid && gt_valid[s-1])
 *   e_xy  = inv ? 0 : pose.xy - gt_pose[s-1].xy;   e_yaw = inv ? 0 : pose.yaw - gt_pose[s-1].yaw;   e_spd = inv ? 0 : motion[0] - gt_motion[s-1][0]
 *   reset = (threshold_xy  > 0 && sqrt(e_x^2 + e_y^2)                   > threshold_xy)
 *        || (threshold_yaw > 0 && |rad2deg(cast_rad(e_yaw))|            > threshold_yaw)      degrees; cast_rad(a) = (a + pi) mod 2 pi - pi,
 *        || (threshold_spd > 0 && |e_spd|                               > threshold_spd)      the modulo with the divisor's sign
 *   tf_mask[row, agent, s] |= reset;   out_reset[row, agent] = reset   (when given)
 * The comparisons are strict. (valid, pose, motion) is the state at ENTRY of step s - after step s-1's override and disabling -, what the
 * reference hands to TeacherForcing.get (waymo_motion.py:234-236). Any other s returns without a write (out_reset included).
 * Two properties of the reference are kept:
 *   1. a reset does not ask for gt_valid[s]: an agent whose track ends at s-1 is overridden with whatever gt_pose[:, :, s] holds and becomes
 *      valid; the step's own override applies ~disabled afterwards as for any forced agent;
 *   2. the resets are part of the table, hence of the logged flag (out_tf / tf): RolloutBuffer.mask_teacher_forcing,
 *      loss_for_teacher_forcing = False and tbx_loss_shape all see them.
 * One thread per (row, agent); a thread reads and writes its own byte of column s only (ordinary byte stores, no atomics, no LDS): two
 * calls on the same input leave the same bytes. Makes no host read, so it is graph-capturable. Thresholds <= 0 are off; with all three
 * off the call is an error (a caller launches nothing then).
 * Returns TBX_ERR_ARG for a NULL struct / required pointer, sizes <= 0 (n_rows == 0 is TBX_OK without a launch) or no threshold on;
 * TBX_ERR_UNSUPPORTED for n_rows * n_ag >= 2^31. A step_host outside (0, n_step_gt) is TBX_OK without a launch.
 */
typedef struct tbx_tf_threshold_t {
  const int32_t* step_dev; /* device step counter (1-based step about to run), or NULL: step_host */
  const uint8_t* valid;    /* [n_rows, n_ag]     state at entry of the step */
  const float* pose;       /* [n_rows, n_ag, 3]  (x, y, yaw) */
  const float* motion;     /* [n_rows, n_ag, 3]  (spd, acc, yaw_rate) */
  const uint8_t* gt_valid; /* [n_rows, n_ag, n_step_gt] */
  const float* gt_pose;    /* [n_rows, n_ag, n_step_gt, 3] */
  const float* gt_motion;  /* [n_rows, n_ag, n_step_gt, 3] */
  uint8_t* tf_mask;        /* [n_rows, n_ag, n_step_gt]  0 / 1, column s is ORed into */
  uint8_t* out_reset;      /* [n_rows, n_ag] this step's new bits, or NULL */
  int64_t n_rows;
  int32_t n_ag, n_step_gt, step_host, pad_;
  float threshold_xy, threshold_yaw, threshold_spd, pad2_;
} tbx_tf_threshold_t;

int tbx_tf_threshold(const tbx_tf_threshold_t* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TBX_HIP_TF_H */
