// Scenario frame -> global frame, the ONE definition: tbx_pose_to_global (womd.hip, libtbx_hip.so) and tbx_womd_predictions
// (sub_records.hip, libtbx_sub.so) inline these, so that a point gets the same bits from either.
// utils/transform_utils.py:160-171 torch_pos2global (pos @ R(yaw)^T + center) and :216-226 torch_rad2global (cast_rad(yaw + scenario_yaw),
// :9-11: (a + pi) % (2 pi) - pi with the sign of the divisor).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace tbx {

// (sn, cs) = sincosf(scenario_yaw)
__device__ __forceinline__ void pos_to_global(const float x, const float y, const float sn, const float cs, const float cx, const float cy,
                                              float* __restrict__ ox, float* __restrict__ oy) {
  *ox = (x * cs + y * -sn) + cx;
  *oy = (x * sn + y * cs) + cy;
}

__device__ __forceinline__ float yaw_to_global(const float yaw, const float th) {
  const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
  float r = fmodf((yaw + th) + pi, two_pi);
  if (r < 0.f) r += two_pi;
  return r - pi;
}

}  // namespace tbx
