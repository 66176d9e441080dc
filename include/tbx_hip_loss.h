/*
 * The loss section of the C ABI of include/tbx_hip.h, exported by libtbx_hip.so like every other entry point (tbx_hip.h includes this
 * header; its contract - device pointers to caller-owned buffers, nothing allocated or retained, kernels only enqueued on `stream`,
 * TBX_* return codes before any launch - holds here too). Source: csrc/loss_shape.hip. It is the loss shaping of the training
 * objective (models/metrics/training.py:90-138: temporal_discount, p_loss_for_irrelevant, w_relevant_agent), a pure function of a
 * finished rollout log.
 */
#ifndef TBX_HIP_LOSS_H
#define TBX_HIP_LOSS_H

#include <stdint.h>

#include "tbx_hip.h" /* TBX_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * tbx_loss_shape: the loss masks, the agent weight and the discounted, weighted reward sum of a log with axes (row, agent, step).
 * Per (row, agent), steps t = 0 .. n_step - 1 in order:
 *   keep  = !mask_irrelevant || relevant || (pick != NULL && pick)                         (training.py:92-96)
 *   lv_t  = pred_valid_t && keep && t >= step_training_start && (loss_for_teacher_forcing || !tf_t)   (:97-102)
 *   any_valid = OR_t lv_t
 *   w_agent   = w_relevant > 0 ? (float)any_valid + (relevant ? w_relevant : 0) : (float)any_valid   (:104-107; float32)
 *   m_0 = 1;  m_t = tf_t ? 1 : m_{t-1} * discount  (float32 products: the reference's chain, bit for bit)   (:130-135);  discount <= 0: m = 1
 *   rv_t = lv_t && reward_valid_t;   w_t = rv_t ? w_agent * m_t : 0   (float32; rv_t implies any_valid, so w_agent is known at step t)
 *   acc[0] += sum (double)reward_t * (double)w_t over rv_t;   acc[1] += #rv_t          (ADDED to acc: the caller zeroes it)
 * DEVIATION: the reference multiplies the reward by w_mask_rel.unsqueeze(1) ([n_sc, 1, n_ag] against [n_sc, n_ag, n_step], :128), which
 * broadcasts only for n_ag == 1 or n_ag == n_step; here the weight is per (row, agent) over all of its steps - the evident intent, and
 * what the reference computes where it runs and means the same thing (n_ag == 1).
 *   pred_valid, tf, reward_valid u8 0/1, reward / w f32: element (row, agent a, step t) of log X is X[row * X_stride[0] + a * X_stride[1] +
 *   t * X_stride[2]] - strides in ELEMENTS. The training chain's [n, T, A] log (strides T*A, 1, A), a buffer's [rows, A, T] (A*T, T, 1) and
 *   a time slice of the rollout engine's [rows, A, ld_t] log (A*ld_t, ld_t, 1; the pointer addresses the first step read) are read in place.
 *   reward and reward_valid may BOTH be NULL (masks only: any_valid and w_agent are written, one launch, acc / partials / w not touched).
 *   relevant [rows, n_ag] u8 (ag_role.any(-1)): NULL only when mask_irrelevant == 0 and w_relevant <= 0.  pick [rows, n_ag] u8 or NULL: the
 *   Bernoulli(p_loss_for_irrelevant) draw per (row, agent), read only with mask_irrelevant.
 *   any_valid [rows, n_ag] u8, w_agent [rows, n_ag] f32: dense, overwritten.  w: NULL or the combined weight per element (overwritten),
 *   addressed through w_stride.  acc: float64 [2].  partials: float64 [TBX_LOSS_PARTIALS] workspace.
 * A lane owns one (row, agent) and walks its steps in order (consecutive lanes: consecutive agents, so the [n, T, A] layout coalesces);
 * lane sums are float64, added across the wave by a butterfly, across the waves of a workgroup in wave order into one row of partials;
 * a second one-workgroup launch adds the rows to acc in row order. No atomics: two calls on the same input give bit-equal acc, w, w_agent
 * and any_valid. Rows are independent; no cap on n_ag.
 * TBX_ERR_ARG: NULL args, pred_valid, tf, any_valid or w_agent; reward given without acc or partials; rows < 0, n_ag <= 0, n_step <= 0,
 * step_training_start < 0; mask_irrelevant or w_relevant > 0 without relevant; exactly one of reward / reward_valid; w without reward.
 * rows == 0: TBX_OK, nothing launched. rows * n_ag >= 2^31: TBX_ERR_UNSUPPORTED. All before any launch. Nothing allocated: runs inside a
 * captured graph. */
#define TBX_LOSS_PARTIAL_ROWS 256
#define TBX_LOSS_PARTIALS (2 * TBX_LOSS_PARTIAL_ROWS)

typedef struct {
  const uint8_t* pred_valid;
  const uint8_t* tf;
  const uint8_t* reward_valid; /* nullable, with reward */
  const float* reward;         /* nullable, with reward_valid */
  const uint8_t* relevant;     /* [rows, n_ag]; nullable when neither relevance switch is on */
  const uint8_t* pick;         /* [rows, n_ag]; nullable */
  uint8_t* any_valid;          /* out [rows, n_ag] */
  float* w_agent;              /* out [rows, n_ag] */
  float* w;                    /* out, nullable */
  double* acc;                 /* in/out [2] */
  double* partials;            /* workspace [TBX_LOSS_PARTIALS] */
  int64_t rows;
  int64_t pred_valid_stride[3]; /* (row, agent, step), in elements */
  int64_t tf_stride[3];
  int64_t reward_valid_stride[3];
  int64_t reward_stride[3];
  int64_t w_stride[3];
  int32_t n_ag, n_step, step_training_start;
  int32_t loss_for_teacher_forcing; /* != 0: forced steps keep their loss */
  int32_t mask_irrelevant;          /* != 0: p_loss_for_irrelevant < 1 */
  int32_t pad_;
  float w_relevant; /* <= 0: off */
  float discount;   /* <= 0: off */
} tbx_loss_shape_t;

int tbx_loss_shape(const tbx_loss_shape_t* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TBX_HIP_LOSS_H */
