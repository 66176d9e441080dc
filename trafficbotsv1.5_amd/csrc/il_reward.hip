// The imitation terms of the differentiable reward for every criterion / angular type of the reference's configuration
// (tbx_il_reward_fwd / _bwd, include/tbx_hip_il.h; utils/rewards.py:25-33,58-74, models/metrics/loss.py:9-36 of the reference), and the
// training chain's reverse walk with the adjoints they produce (tbx_train_chain_bwd_state). The reward never feeds back into the state,
// so - as for the collision term (collision.hip) - this is one elementwise launch over a finished log, not a part of every step:
// one thread per (row, slot, agent), the threads running along whichever of the agent / step axes of the pose view has the smaller
// stride (the engine's log is agent-major, the chain's time-major), a grid-stride loop, no LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbx_hip_il.h"
#include "train_chain_core.h"  // sl1 / sl1_grad and the chain's reverse walk: one definition, shared with train_chain.hip

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;

__device__ __forceinline__ float crit(int code, float d) {
  if (code == TBX_IL_MSE) return d * d;
  if (code == TBX_IL_L1) return fabsf(d);
  return sl1(d);  // TBX_IL_SMOOTH_L1, TBX_IL_HUBER
}

__device__ __forceinline__ float crit_grad(int code, float d) {
  if (code == TBX_IL_MSE) return 2.f * d;
  if (code == TBX_IL_L1) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  return sl1_grad(d);
}

// cast_rad (utils/transform_utils.py:9-11) as torch evaluates it on float32: (a + pi) % (2 pi) - pi with the floor-mod of `%`
__device__ __forceinline__ float wrap_rad(float a) {
  const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
  float r = fmodf(a + pi, two_pi);
  if (r != 0.f && r < 0.f) r += two_pi;
  return r - pi;
}

struct Elem {  // one (row, slot, agent)
  int64_t row;
  int t, a;
};

// Element i of rows x n_step x n_ag with the fast axis along the agents (agent_fast) or along the steps.
__device__ __forceinline__ Elem elem_of(int64_t i, int n_step, int n_ag, bool agent_fast) {
  Elem e;
  if (agent_fast) {
    e.a = (int)(i % n_ag);
    const int64_t q = i / n_ag;
    e.t = (int)(q % n_step), e.row = q / n_step;
  } else {
    e.t = (int)(i % n_step);
    const int64_t q = i / n_step;
    e.a = (int)(q % n_ag), e.row = q / n_ag;
  }
  return e;
}

__device__ __forceinline__ int64_t at(const int64_t* s, const Elem& e) { return e.row * s[0] + e.t * s[1] + e.a * s[2]; }

// The pair (prediction, ground truth) of an element; false: the element is masked (every term 0, no gradient).
struct Pair {
  float px, py, pw, pv, gx, gy, gw, gv;
};

__device__ __forceinline__ bool load_pair(const tbx_il_reward_t& k, const Elem& e, Pair& p) {
  const int s = e.t + k.gt_offset;
  if (s >= k.n_step_gt) return false;
  if (k.pred_valid[at(k.valid_stride, e)] == 0) return false;
  const int64_t ig = ((e.row / k.n_k) * k.n_ag + e.a) * k.n_step_gt + s;
  if (k.gt_valid[ig] == 0) return false;
  const float* pp = k.pred_pose + at(k.pose_stride, e);
  p.px = pp[0], p.py = pp[1], p.pw = pp[2];
  p.pv = k.pred_motion[at(k.motion_stride, e)];
  p.gx = k.gt_pose[ig * 3], p.gy = k.gt_pose[ig * 3 + 1], p.gw = k.gt_pose[ig * 3 + 2];
  p.gv = k.gt_motion[ig * 3];
  return true;
}

__global__ __launch_bounds__(kThreads) void il_reward_fwd_kernel(const tbx_il_reward_t k, int64_t total, int agent_fast) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const Elem e = elem_of(i, k.n_step, k.n_ag, agent_fast != 0);
    float r_pos = 0.f, r_rot = 0.f, r_spd = 0.f;
    Pair p;
    if (load_pair(k, e, p)) {
      const float e_pos = crit(k.crit_pos, p.gx - p.px) + crit(k.crit_pos, p.gy - p.py);
      const float e_spd = crit(k.crit_spd, p.gv - p.pv);
      float e_rot;
      if (k.angular == TBX_IL_ANG_COSINE) e_rot = 0.5f * (1.f - cosf(p.gw - p.pw));
      else if (k.angular == TBX_IL_ANG_NONE) e_rot = crit(k.crit_rot, p.gw - p.pw);
      else if (k.angular == TBX_IL_ANG_CAST) e_rot = crit(k.crit_rot, wrap_rad(p.gw - p.pw));
      else e_rot = crit(k.crit_rot, cosf(p.gw) - cosf(p.pw)) + crit(k.crit_rot, sinf(p.gw) - sinf(p.pw));
      r_pos = -k.w_pos * e_pos, r_rot = -k.w_rot * e_rot, r_spd = -k.w_spd * e_spd;
    }
    const int64_t o = at(k.out_stride, e);
    if (k.out_pos != nullptr) k.out_pos[o] = r_pos, k.out_rot[o] = r_rot, k.out_spd[o] = r_spd;
    k.out_sum[o] = (r_pos + r_rot) + r_spd;
  }
}

__global__ __launch_bounds__(kThreads) void il_reward_bwd_kernel(const tbx_il_reward_t k, int64_t total, int agent_fast) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const Elem e = elem_of(i, k.n_step, k.n_ag, agent_fast != 0);
    float dx = 0.f, dy = 0.f, dw = 0.f, dv = 0.f;
    Pair p;
    if (load_pair(k, e, p)) {
      const float g = k.g[at(k.g_stride, e)];
      dx = g * k.w_pos * crit_grad(k.crit_pos, p.gx - p.px);
      dy = g * k.w_pos * crit_grad(k.crit_pos, p.gy - p.py);
      dv = g * k.w_spd * crit_grad(k.crit_spd, p.gv - p.pv);
      if (k.angular == TBX_IL_ANG_COSINE) {
        dw = g * 0.5f * k.w_rot * sinf(p.gw - p.pw);  // (the form of the chain's own reverse walk)
      } else {
        float de;  // d(e_rot) / d(pw)
        if (k.angular == TBX_IL_ANG_NONE) de = -crit_grad(k.crit_rot, p.gw - p.pw);
        else if (k.angular == TBX_IL_ANG_CAST) de = -crit_grad(k.crit_rot, wrap_rad(p.gw - p.pw));
        else {
          const float sp = sinf(p.pw), cp = cosf(p.pw);
          de = crit_grad(k.crit_rot, cosf(p.gw) - cp) * sp - crit_grad(k.crit_rot, sinf(p.gw) - sp) * cp;
        }
        dw = -(g * k.w_rot) * de;
      }
    }
    const int64_t o = (e.row * k.n_step + e.t) * k.n_ag + e.a;  // dense [rows, n_step, n_ag]
    k.d_pred_pose[o * 3] = dx, k.d_pred_pose[o * 3 + 1] = dy, k.d_pred_pose[o * 3 + 2] = dw;
    k.d_pred_spd[o] = dv;
  }
}

bool known_crit(int c) { return c == TBX_IL_SMOOTH_L1 || c == TBX_IL_MSE || c == TBX_IL_L1 || c == TBX_IL_HUBER; }

int check(const tbx_il_reward_t* k, bool bwd) {
  if (!k) return TBX_ERR_ARG;
  if (!k->pred_valid || !k->pred_pose || !k->pred_motion || !k->gt_valid || !k->gt_pose || !k->gt_motion) return TBX_ERR_ARG;
  if (k->rows < 1 || k->n_k < 1 || k->n_ag < 1 || k->n_step < 1 || k->n_step_gt < 1 || k->gt_offset < 0) return TBX_ERR_ARG;
  if (k->rows % k->n_k != 0) return TBX_ERR_ARG;
  const int64_t* strides[4] = {k->valid_stride, k->pose_stride, k->motion_stride, bwd ? k->g_stride : k->out_stride};
  for (const int64_t* s : strides)
    if (s[0] < 0 || s[1] < 0 || s[2] < 0) return TBX_ERR_ARG;
  if (bwd) {
    if (!k->g || !k->d_pred_pose || !k->d_pred_spd) return TBX_ERR_ARG;
  } else {
    if (!k->out_sum) return TBX_ERR_ARG;
    const int n_planes = (k->out_pos != nullptr) + (k->out_rot != nullptr) + (k->out_spd != nullptr);
    if (n_planes != 0 && n_planes != 3) return TBX_ERR_ARG;
  }
  if (!known_crit(k->crit_pos) || !known_crit(k->crit_rot) || !known_crit(k->crit_spd)) return TBX_ERR_UNSUPPORTED;
  if (k->angular < TBX_IL_ANG_COSINE || k->angular > TBX_IL_ANG_VECTOR) return TBX_ERR_UNSUPPORTED;
  return TBX_OK;
}

int launch(const tbx_il_reward_t* k, bool bwd, void* stream) {
  const int rc = check(k, bwd);
  if (rc != TBX_OK) return rc;
  const int64_t total = k->rows * k->n_step * k->n_ag;
  const int64_t want = (total + kThreads - 1) / kThreads;
  const unsigned blocks = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
  const int agent_fast = k->pose_stride[2] <= k->pose_stride[1] || k->n_step == 1;
  if (bwd) hipLaunchKernelGGL(il_reward_bwd_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, *k, total, agent_fast);
  else hipLaunchKernelGGL(il_reward_fwd_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, *k, total, agent_fast);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}

}  // namespace

extern "C" int tbx_il_reward_fwd(const tbx_il_reward_t* args, void* stream) { return launch(args, false, stream); }

extern "C" int tbx_il_reward_bwd(const tbx_il_reward_t* args, void* stream) { return launch(args, true, stream); }

extern "C" int tbx_train_chain_bwd_state(const tbx_train_chain_t* c, const float* mean, int64_t mean_stride_n, int64_t mean_stride_t,
                                         const float* d_reward, const float* d_pred_pose, const float* d_pred_spd, float* d_mean,
                                         void* stream) {
  return train_chain_launch_bwd<true>(c, mean, mean_stride_n, mean_stride_t, d_reward, d_pred_pose, d_pred_spd, d_mean, stream);
}
