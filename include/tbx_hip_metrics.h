/*
 * The metrics section of the C ABI of include/tbx_hip.h, exported by libtbx_hip.so like every other entry point (tbx_hip.h includes this
 * header; its contract - device pointers to caller-owned buffers, nothing allocated or retained, kernels only enqueued on `stream`,
 * TBX_* return codes - holds here too). Source: csrc/metrics.hip. It is the reduction of a device-resident rollout log to the
 * validation epoch's numbers.
 */
#ifndef TBX_HIP_METRICS_H
#define TBX_HIP_METRICS_H

#include <stdint.h>

#include "tbx_hip.h" /* TBX_RULE_* bits, TBX_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * Epoch metrics of a rollout log. Replaces ErrorMetrics.update and TrafficRuleMetrics.update (models/metrics/logging.py:19-49,
 * 79-107; ~40 elementwise / reduction launches per update) with one reduction of the log where the engine wrote it. The 13 sums
 * of the two classes are ADDED to acc[TBX_METRICS_SLOTS] (float64, caller-owned, zeroed by the caller at the start of an epoch):
 *   acc[0] err_counter   = #{(row, agent, step): pred_valid & gt_valid}                  and over those steps
 *   acc[1] err_pos_meter = sum |pred_xy - gt_xy|_2     acc[2] err_rot_deg = sum |rad2deg(cast_rad(pred_yaw - gt_yaw))|,
 *          cast_rad(a) = (a + pi) mod 2 pi - pi with the floored modulo         acc[3] err_spd_m_per_s = sum |pred_spd - gt_spd|
 *   acc[4] counter_agent = #{(row, agent): pred_valid at any step}    acc[5] counter_veh = those with ag_type[.., 0]
 *   acc[6] outside_map, [7] collided, [8] run_road_edge, [9] run_red_light, [10] passive, [11] goal_reached, [12] dest_reached
 *          = #{(row, agent): the flag is set at any step at which pred_valid is}         acc[13..15] are not touched.
 * Rows are n_rows = n_scene * n_k rollouts; ground truth and types are per scene (row / n_k).
 *   pred_valid [n_rows, n_ag, ld_t] u8 0/1, pred_pose / pred_motion [n_rows, n_ag, ld_t, 3]: the pointers address step 0 of row 0's
 *   log, steps [t0, t0 + n_t) are read (a time slice of a dense log is read in place). pred_pose / pred_motion may be NULL
 *   without the error half.
 *   Error half (gt_valid non-NULL; then all three, pred_pose and pred_motion are needed): gt_valid [n_scene, n_ag, n_step_gt] u8,
 *   gt_pose / gt_motion [n_scene, n_ag, n_step_gt, 3]; read step t0 + i of the log is compared with ground-truth step gt_t0 + i
 *   (gt_t0 = RolloutBuffer.step_start for t0 = 0). Defined for n_k == 1 only (the reference squeezes that axis): TBX_ERR_UNSUPPORTED.
 *   Rule half (flags non-NULL; then outside_map, dest_reached and ag_type are needed): flags [n_rows, n_ag, ld_flags] u8 TBX_RULE_*
 *   bits whose step 0 is the FIRST step read (tbx_rule_accumulate's out_acc, or a packed copy); outside_map / dest_reached /
 *   goal_reached [n_rows, n_ag, ld_t] u8 0/1 logs laid out and sliced like pred_valid, goal_reached NULL = all false (navi_mode
 *   "dest"); ag_type [n_scene, n_ag, 3] u8.
 * A pointer of a half that is off must be NULL; both halves off, a missing pointer, n_rows % n_k != 0, ld_t < t0 + n_t,
 * n_step_gt < gt_t0 + n_t or ld_flags < n_t: TBX_ERR_ARG before any launch. n_rows * n_ag >= 2^31: TBX_ERR_UNSUPPORTED.
 *   partials [TBX_METRICS_PARTIAL_ROWS, TBX_METRICS_SLOTS] float64: workspace, overwritten.
 * Deterministic: no atomics. One wave per (row, agent) reduces over time, a workgroup's four waves are added in wave order into one
 * row of `partials`, and a second, one-workgroup launch adds the rows to acc in row order - two calls on the same input give
 * bit-equal sums. The per-step errors are float64 expressions of the float32 logs and every sum is float64 (the reference's
 * float32 counters stop counting at 2^24). Two launches, no host synchronisation. */
#define TBX_METRICS_SLOTS 16
#define TBX_METRICS_PARTIAL_ROWS 256
int tbx_rollout_metrics(const uint8_t* pred_valid, const float* pred_pose, const float* pred_motion, int64_t n_rows, int n_k, int n_ag,
                        int ld_t, int t0, int n_t, const uint8_t* gt_valid, const float* gt_pose, const float* gt_motion,
                        int n_step_gt, int gt_t0, const uint8_t* flags, int ld_flags, const uint8_t* outside_map,
                        const uint8_t* dest_reached, const uint8_t* goal_reached, const uint8_t* ag_type, double* acc, double* partials,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TBX_HIP_METRICS_H */
