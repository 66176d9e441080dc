// The ONE definition of the training chain's reverse walk and of its argument check, shared by the two translation units that launch it:
// train_chain.hip (tbx_train_chain_bwd / _bwd_pose, libtbx_hip.so) and il_reward.hip (tbx_train_chain_bwd_state, libtbx_il.so).
// Everything here has internal linkage (an anonymous namespace per translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbx_hip.h"

namespace {

__device__ __forceinline__ float sl1(float d) {  // F.smooth_l1_loss, beta = 1
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}
__device__ __forceinline__ float sl1_grad(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f); }

// d(mean) from d(reward), all steps, in reverse, for the agent (b, a). Reads what the forward over [0, T) left behind: the records of the
// state before every step (slot window - 1 + t holds the state before step t + 1), the override flags and the predictions.
// kSpd: an adjoint of the predicted speed from outside the chain exists (d_pred_spd, may still be NULL); false: the pointer is not read.
template <bool kSpd>
__device__ __forceinline__ void train_chain_bwd_walk(const tbx_train_chain_t& c, const float* __restrict__ mean, int64_t sn, int64_t st,
                                                     const float* __restrict__ d_reward, const float* __restrict__ d_pred_pose,
                                                     const float* __restrict__ d_pred_spd, float* __restrict__ d_mean, int b, int a) {
#pragma clang fp contract(off)
  const int A = c.n_ag, T = c.n_step, Tg = c.n_step_gt;
  const int64_t ia = (int64_t)b * A + a;
  const float lim0 = c.lim[ia * 2], lim1 = c.lim[ia * 2 + 1], dt = c.dt;
  const int rec_T = T + c.window;
  float ax = 0.f, ay = 0.f, aw = 0.f, av = 0.f;  // adjoint of the state after step s (x, y, yaw, speed)
  for (int t = T - 1; t >= 0; --t) {
    const int s = t + 1;
    const int64_t it = ((int64_t)b * T + t) * A + a;
    const int64_t ir = ((int64_t)b * rec_T + (c.window - 1 + t)) * A + a;
    const bool valid = c.rec_valid[ir] != 0;
    float dm0 = 0.f, dm1 = 0.f;
    if (!valid) {  // the prediction is the constant 0: nothing flows to the state before or to the action
      ax = ay = aw = av = 0.f;
    } else {
      float dx = 0.f, dy = 0.f, dw = 0.f, dv = 0.f;  // adjoint of the prediction (x', y', yaw', speed')
      if (!c.ov[it]) dx = ax, dy = ay, dw = aw, dv = av;
      if (s < Tg && c.reward_valid[it]) {
        const int64_t ig = ((int64_t)b * A + a) * Tg + s;
        const float g = d_reward[it];
        const float nx = c.pred_pose[it * 3], ny = c.pred_pose[it * 3 + 1], nw = c.pred_pose[it * 3 + 2], nv = c.pred_motion[it * 3];
        dx += g * c.w_pos * sl1_grad(c.gt_pose[ig * 3] - nx);
        dy += g * c.w_pos * sl1_grad(c.gt_pose[ig * 3 + 1] - ny);
        dw += g * 0.5f * c.w_rot * sinf(c.gt_pose[ig * 3 + 2] - nw);
        dv += g * c.w_spd * sl1_grad(c.gt_motion[ig * 3] - nv);
      }
      // adjoints of the prediction from outside the chain (tbx_train_chain_bwd_pose: the collision term reads pred_pose;
      // tbx_train_chain_bwd_state: the imitation terms of tbx_il_reward_bwd read pred_pose and the predicted speed)
      if (d_pred_pose != nullptr) dx += d_pred_pose[it * 3], dy += d_pred_pose[it * 3 + 1], dw += d_pred_pose[it * 3 + 2];
      if (kSpd) {
        if (d_pred_spd != nullptr) dv += d_pred_spd[it];
      }
      const float pw = c.rec_pose[ir * 3 + 2], mv = c.rec_motion[ir * 3];
      const float u0 = tanhf(mean[b * sn + t * st + a * 2]), u1 = tanhf(mean[b * sn + t * st + a * 2 + 1]);
      const float acc = u0 * lim0, yr = u1 * lim1;
      const float v_t = mv + 0.5f * dt * acc, th_t = pw + 0.5f * dt * yr;
      const float cs = cosf(th_t), sn_ = sinf(th_t);
      const float d_vt = dt * (dx * cs + dy * sn_);
      const float d_th = dt * v_t * (dy * cs - dx * sn_);
      const float d_yr = dt * dw + 0.5f * dt * d_th;
      const float d_acc = dt * dv + 0.5f * dt * d_vt;
      ax = dx, ay = dy, aw = dw + d_th, av = dv + d_vt;
      dm0 = d_acc * lim0 * (1.f - u0 * u0);
      dm1 = d_yr * lim1 * (1.f - u1 * u1);
    }
    d_mean[it * 2] = dm0;
    d_mean[it * 2 + 1] = dm1;
  }
}

template <bool kSpd>
__global__ __launch_bounds__(64) void train_chain_bwd_kernel(const tbx_train_chain_t c, const float* __restrict__ mean, int64_t sn,
                                                             int64_t st, const float* __restrict__ d_reward,
                                                             const float* __restrict__ d_pred_pose, const float* __restrict__ d_pred_spd,
                                                             float* __restrict__ d_mean) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (a >= c.n_ag) return;
  train_chain_bwd_walk<kSpd>(c, mean, sn, st, d_reward, d_pred_pose, d_pred_spd, d_mean, b, a);
}

int train_chain_check(const tbx_train_chain_t* c) {
  if (!c) return TBX_ERR_ARG;
  if (c->n_batch <= 0 || c->n_ag <= 0 || c->n_step <= 0 || c->n_step_gt <= 0 || c->n_node < 0 || c->window < 1) return TBX_ERR_ARG;
  const void* ptrs[] = {c->gt_valid, c->gt_pose, c->gt_motion, c->tf_mask, c->lim, c->dest_thresh, c->dest_kind, c->boundary, c->valid,
                        c->disabled, c->navi_valid, c->outside, c->reached, c->pose, c->motion, c->rec_valid, c->rec_pose, c->rec_motion,
                        c->rec_navi_valid, c->pred_valid, c->tf, c->ov, c->reward_valid, c->pred_pose, c->pred_motion, c->reward};
  for (const void* p : ptrs)
    if (!p) return TBX_ERR_ARG;
  if (c->n_node > 0 && (!c->dest_pos || !c->dest_dir || !c->dest_invalid)) return TBX_ERR_ARG;
  return TBX_OK;
}

// The reverse walk's launch (every entry point that runs it: tbx_train_chain_bwd, _bwd_pose, _bwd_state).
template <bool kSpd>
int train_chain_launch_bwd(const tbx_train_chain_t* c, const float* mean, int64_t mean_stride_n, int64_t mean_stride_t, const float* d_reward,
                           const float* d_pred_pose, const float* d_pred_spd, float* d_mean, void* stream) {
  const int rc = train_chain_check(c);
  if (rc != TBX_OK) return rc;
  if (!mean || !d_reward || !d_mean) return TBX_ERR_ARG;
  hipLaunchKernelGGL(train_chain_bwd_kernel<kSpd>, dim3((c->n_ag + 63) / 64, c->n_batch), dim3(64), 0, (hipStream_t)stream, *c, mean,
                     mean_stride_n, mean_stride_t, d_reward, d_pred_pose, d_pred_spd, d_mean);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}

}  // namespace
