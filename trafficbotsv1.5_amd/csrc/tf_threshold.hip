// Error-threshold teacher forcing: one step's resets into the teacher-forcing table (include/tbx_hip_tf.h: tbx_tf_threshold).
#include "../../include/tbx_hip.h"
#include "tbx_common.h"

namespace {

// utils/teacher_forcing.py:128-151 for ONE step, before the step kernel reads the table's column.
//   * a thread owns one (row, agent) pair: consecutive lanes take consecutive agents, so the state ([n, A(,3)]) is read coalesced; the
//     ground truth and the table are strided by n_step_gt (one byte / three floats per pair and call - 12 KB at 64 agents x 2 rows).
//   * the step index is read from the device (step_dev) when given: the same launch, captured once, serves every step of a rollout.
//   * float32 in the reference's order; products are rounded before they are added (__fmul_rn / __fadd_rn: no fused multiply-add), so an
//     offset of (3, 4) has the distance 5 exactly.
//   * the only writes are the pair's own byte of column s and its out_reset byte: ordinary vector byte stores.
constexpr int TF_THREADS = 256;

struct TfArgs {
  const int32_t* step_dev;
  const uint8_t* valid;
  const float* pose;
  const float* motion;
  const uint8_t* gt_valid;
  const float* gt_pose;
  const float* gt_motion;
  uint8_t* tf_mask;
  uint8_t* out_reset;  // or null
  int64_t n_pairs;     // rows * A
  int Tg, step_host;
  float thr_xy, thr_yaw, thr_spd;
};

// transform_utils.py:9-11: (a + pi) % (2 pi) - pi with python's modulo (the result takes the divisor's sign), float32 constants
__device__ __forceinline__ float cast_rad(float a) {
  const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
  float r = fmodf(__fadd_rn(a, pi), two_pi);
  if (r < 0.f) r = __fadd_rn(r, two_pi);
  return __fadd_rn(r, -pi);
}

__global__ __launch_bounds__(TF_THREADS) void tf_threshold_kernel(const TfArgs p) {
  const int s = p.step_dev != nullptr ? p.step_dev[0] : p.step_host;
  if (s <= 0 || s >= p.Tg) return;  // (uniform over the grid) the empty override: nothing is written
  const int64_t pair = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
  if (pair >= p.n_pairs) return;
  const int64_t g = pair * p.Tg + (s - 1);  // this pair's ground truth at s - 1
  const bool ok = p.valid[pair] != 0 && p.gt_valid[g] != 0;
  bool reset = false;
  if (ok) {  // (an invalid pair's errors are 0: no threshold > 0 is exceeded)
    if (p.thr_xy > 0.f || p.thr_yaw > 0.f) {
      const float* ps = p.pose + pair * 3;
      const float* gp = p.gt_pose + g * 3;
      if (p.thr_xy > 0.f) {
        const float ex = __fadd_rn(ps[0], -gp[0]), ey = __fadd_rn(ps[1], -gp[1]);
        reset |= __fsqrt_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey))) > p.thr_xy;
      }
      if (p.thr_yaw > 0.f) {
        const float deg = __fmul_rn(cast_rad(__fadd_rn(ps[2], -gp[2])), 57.29577951308232f);
        reset |= fabsf(deg) > p.thr_yaw;
      }
    }
    if (p.thr_spd > 0.f) reset |= fabsf(__fadd_rn(p.motion[pair * 3], -p.gt_motion[g * 3])) > p.thr_spd;
  }
  uint8_t* cell = p.tf_mask + pair * p.Tg + s;
  if (reset) *cell = 1;  // |= on a 0 / 1 table
  if (p.out_reset != nullptr) p.out_reset[pair] = reset ? 1 : 0;
}

}  // namespace

extern "C" int tbx_tf_threshold(const tbx_tf_threshold_t* args, void* stream) {
  if (!args) return TBX_ERR_ARG;
  const tbx_tf_threshold_t& a = *args;
  if (!a.valid || !a.pose || !a.motion || !a.gt_valid || !a.gt_pose || !a.gt_motion || !a.tf_mask) return TBX_ERR_ARG;
  if (a.n_rows < 0 || a.n_ag <= 0 || a.n_step_gt <= 0) return TBX_ERR_ARG;
  if (!(a.threshold_xy > 0.f || a.threshold_yaw > 0.f || a.threshold_spd > 0.f)) return TBX_ERR_ARG;
  if (a.n_rows == 0) return TBX_OK;
  if (a.n_rows >= ((int64_t)1 << 31) / a.n_ag + (((int64_t)1 << 31) % a.n_ag != 0)) return TBX_ERR_UNSUPPORTED;  // rows * n_ag >= 2^31
  if (!a.step_dev && (a.step_host <= 0 || a.step_host >= a.n_step_gt)) return TBX_OK;  // (the kernel would return at once)
  TfArgs p;
  p.step_dev = a.step_dev, p.valid = a.valid, p.pose = a.pose, p.motion = a.motion;
  p.gt_valid = a.gt_valid, p.gt_pose = a.gt_pose, p.gt_motion = a.gt_motion, p.tf_mask = a.tf_mask, p.out_reset = a.out_reset;
  p.n_pairs = a.n_rows * a.n_ag;
  p.Tg = a.n_step_gt, p.step_host = a.step_host;
  p.thr_xy = a.threshold_xy, p.thr_yaw = a.threshold_yaw, p.thr_spd = a.threshold_spd;
  const int64_t n_blocks = (p.n_pairs + TF_THREADS - 1) / TF_THREADS;
  hipLaunchKernelGGL(tf_threshold_kernel, dim3((unsigned)n_blocks), dim3(TF_THREADS), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
