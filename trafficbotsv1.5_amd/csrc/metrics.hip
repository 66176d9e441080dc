// Epoch metrics of a device-resident rollout log (include/tbx_hip_metrics.h: tbx_rollout_metrics).
#include "../../include/tbx_hip.h"
#include "tbx_common.h"

namespace {

// ErrorMetrics.update / TrafficRuleMetrics.update (models/metrics/logging.py:19-49, 79-107) as ONE reduction over the log.
//   * one wave64 per (row, agent): the lanes stride the time axis (the logs are contiguous in time, so a wave's loads coalesce), the
//     any-over-time of every flag is a ballot, the three error sums a wave butterfly. A wave walks pairs wave, wave + n_waves, ...: which
//     wave sees which pair depends on the shapes alone.
//   * 4 waves per workgroup; wave sums -> LDS -> threads 0..15 add the four waves in wave order -> one partial row per workgroup,
//     written with ordinary stores. metrics_final_kernel (one workgroup) adds the partial rows to acc in row order.
//   No atomics anywhere: two calls on the same input give bit-equal results.
// Arithmetic: the per-step errors are float64 expressions of the float32 logs (the differences are then exact, one rounding each for
// the norm, the wrap and the degree conversion) and all sums are float64 - the reference's float32 counters saturate at 2^24.
constexpr int MET_WAVES = 4, MET_THREADS = 64 * MET_WAVES, MET_SLOTS = TBX_METRICS_SLOTS, MET_MAX_BLOCKS = TBX_METRICS_PARTIAL_ROWS;
constexpr int MET_USED = 13;  // slots written; the rest of a row is zero

struct MetArgs {
  const uint8_t* valid;     // [R, A, ld_t]
  const float* pose;        // [R, A, ld_t, 3]
  const float* motion;      // [R, A, ld_t, 3]
  const uint8_t* gt_valid;  // [n, A, Tg]      (null: no error half)
  const float* gt_pose;     // [n, A, Tg, 3]
  const float* gt_motion;   // [n, A, Tg, 3]
  const uint8_t* flags;     // [R, A, ld_f]    (null: no rule half) TBX_RULE_* bits, step 0 = the first step read
  const uint8_t* outside;   // [R, A, ld_t]
  const uint8_t* dest;      // [R, A, ld_t]
  const uint8_t* goal;      // [R, A, ld_t] or null (all false)
  const uint8_t* ag_type;   // [n, A, 3]
  double* partials;         // [gridDim.x, MET_SLOTS]
  int64_t n_pairs;          // R * A
  int K, A, ld_t, t0, T, Tg, gt_t0, ld_f;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(MET_THREADS) void metrics_partial_kernel(const MetArgs p) {
  __shared__ double part[MET_WAVES][MET_SLOTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool has_err = p.gt_valid != nullptr, has_rule = p.flags != nullptr;
  const double PI = 3.141592653589793, TWO_PI = 6.283185307179586, DEG = 180.0 / 3.141592653589793;
  double e_pos = 0.0, e_rot = 0.0, e_spd = 0.0;                      // per lane
  unsigned long long c_err = 0;                                        // wave-uniform from here on
  unsigned c_agent = 0, c_veh = 0, c_out = 0, c_col = 0, c_edge = 0, c_red = 0, c_pas = 0, c_goal = 0, c_dest = 0;
  const int64_t stride = (int64_t)gridDim.x * MET_WAVES;
  for (int64_t pair = (int64_t)blockIdx.x * MET_WAVES + wave; pair < p.n_pairs; pair += stride) {
    const int64_t row = pair / p.A;
    const int a = (int)(pair - row * p.A);
    const int64_t sa = (row / p.K) * p.A + a;                         // (scene, agent) of the ground truth / the type
    const int64_t log0 = pair * p.ld_t + p.t0, gt0 = sa * p.Tg + p.gt_t0, f0 = pair * p.ld_f;
    unsigned any_v = 0, any_out = 0, any_dest = 0, any_goal = 0, bits = 0;  // per lane: OR over its steps
    for (int t = lane; t < p.T; t += 64) {
      const bool v = p.valid[log0 + t] != 0;
      if (has_err) {
        const bool ev = v && p.gt_valid[gt0 + t] != 0;
        const float* pp = p.pose + (log0 + t) * 3;
        const float* gp = p.gt_pose + (gt0 + t) * 3;
        const double dx = (double)pp[0] - (double)gp[0], dy = (double)pp[1] - (double)gp[1], dyaw = (double)pp[2] - (double)gp[2];
        const double dspd = (double)p.motion[(log0 + t) * 3] - (double)p.gt_motion[(gt0 + t) * 3];
        const double w = dyaw + PI;
        const double rot = fabs((w - TWO_PI * floor(w / TWO_PI) - PI) * DEG);  // |rad2deg(cast_rad(dyaw))|, floored modulo
        e_pos += ev ? sqrt(dx * dx + dy * dy) : 0.0;
        e_rot += ev ? rot : 0.0;
        e_spd += ev ? fabs(dspd) : 0.0;
        c_err += __popcll(__ballot(ev));
      }
      if (has_rule) {
        any_v |= v;
        if (v) {
          bits |= p.flags[f0 + t];
          any_out |= p.outside[log0 + t] != 0;
          any_dest |= p.dest[log0 + t] != 0;
          if (p.goal) any_goal |= p.goal[log0 + t] != 0;
        }
      }
    }
    if (has_rule) {
      const bool va = __ballot(any_v) != 0;
      c_agent += va;
      c_veh += va && p.ag_type[sa * 3] != 0;
      c_out += __ballot(any_out) != 0;
      c_dest += __ballot(any_dest) != 0;
      c_goal += __ballot(any_goal) != 0;
      c_col += __ballot(bits & TBX_RULE_COLLIDED) != 0;
      c_edge += __ballot(bits & TBX_RULE_RUN_ROAD_EDGE) != 0;
      c_red += __ballot(bits & TBX_RULE_RUN_RED_LIGHT) != 0;
      c_pas += __ballot(bits & TBX_RULE_PASSIVE) != 0;
    }
  }
  e_pos = wave_sum_f64(e_pos);
  e_rot = wave_sum_f64(e_rot);
  e_spd = wave_sum_f64(e_spd);
  if (lane == 0) {
    double* o = part[wave];
    o[0] = (double)c_err, o[1] = e_pos, o[2] = e_rot, o[3] = e_spd;
    o[4] = c_agent, o[5] = c_veh, o[6] = c_out, o[7] = c_col, o[8] = c_edge, o[9] = c_red, o[10] = c_pas, o[11] = c_goal, o[12] = c_dest;
    o[13] = o[14] = o[15] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < MET_SLOTS) {
    double s = part[0][threadIdx.x];
    for (int w = 1; w < MET_WAVES; ++w) s += part[w][threadIdx.x];
    p.partials[(int64_t)blockIdx.x * MET_SLOTS + threadIdx.x] = s;
  }
}

// acc[c] += partials[0][c] + partials[1][c] + ... in row order. One workgroup: the rows are staged in LDS by all threads, then thread c
// walks its column.
__global__ __launch_bounds__(MET_THREADS) void metrics_final_kernel(const double* __restrict__ partials, int n_rows, double* __restrict__ acc) {
  __shared__ double rows[MET_MAX_BLOCKS * MET_SLOTS];
  for (int i = threadIdx.x; i < n_rows * MET_SLOTS; i += MET_THREADS) rows[i] = partials[i];
  __syncthreads();
  if (threadIdx.x < MET_USED) {
    double s = rows[threadIdx.x];
    for (int r = 1; r < n_rows; ++r) s += rows[r * MET_SLOTS + threadIdx.x];
    acc[threadIdx.x] += s;
  }
}

}  // namespace

extern "C" int tbx_rollout_metrics(const uint8_t* pred_valid, const float* pred_pose, const float* pred_motion, int64_t n_rows, int n_k,
                                   int n_ag, int ld_t, int t0, int n_t, const uint8_t* gt_valid, const float* gt_pose,
                                   const float* gt_motion, int n_step_gt, int gt_t0, const uint8_t* flags, int ld_flags,
                                   const uint8_t* outside_map, const uint8_t* dest_reached, const uint8_t* goal_reached,
                                   const uint8_t* ag_type, double* acc, double* partials, void* stream) {
  if (!pred_valid || !acc || !partials) return TBX_ERR_ARG;
  if (n_rows <= 0 || n_k <= 0 || n_ag <= 0 || n_t <= 0 || t0 < 0 || ld_t < t0 + n_t || n_rows % n_k != 0) return TBX_ERR_ARG;
  const bool has_err = gt_valid != nullptr, has_rule = flags != nullptr;
  if (!has_err && !has_rule) return TBX_ERR_ARG;
  if (has_err) {
    if (!gt_pose || !gt_motion || !pred_pose || !pred_motion) return TBX_ERR_ARG;
    if (gt_t0 < 0 || n_step_gt < gt_t0 + n_t) return TBX_ERR_ARG;
    if (n_k != 1) return TBX_ERR_UNSUPPORTED;  // the reference squeezes the joint-future axis (logging.py:40)
  } else if (gt_pose || gt_motion) {
    return TBX_ERR_ARG;
  }
  if (has_rule) {
    if (!outside_map || !dest_reached || !ag_type || ld_flags < n_t) return TBX_ERR_ARG;
  } else if (outside_map || dest_reached || goal_reached || ag_type) {
    return TBX_ERR_ARG;
  }
  if (n_rows > 0x7fffffff / n_ag) return TBX_ERR_UNSUPPORTED;  // (row, agent) pairs are counted in 32-bit counters per workgroup
  MetArgs p;
  p.valid = pred_valid, p.pose = pred_pose, p.motion = pred_motion;
  p.gt_valid = gt_valid, p.gt_pose = gt_pose, p.gt_motion = gt_motion;
  p.flags = flags, p.outside = outside_map, p.dest = dest_reached, p.goal = goal_reached, p.ag_type = ag_type;
  p.partials = partials;
  p.n_pairs = n_rows * n_ag;
  p.K = n_k, p.A = n_ag, p.ld_t = ld_t, p.t0 = t0, p.T = n_t, p.Tg = n_step_gt, p.gt_t0 = gt_t0, p.ld_f = ld_flags;
  const int64_t want = (p.n_pairs + MET_WAVES - 1) / MET_WAVES;
  const int n_blocks = (int)(want < MET_MAX_BLOCKS ? want : MET_MAX_BLOCKS);
  hipLaunchKernelGGL(metrics_partial_kernel, dim3((unsigned)n_blocks), dim3(MET_THREADS), 0, (hipStream_t)stream, p);
  if (hipGetLastError() != hipSuccess) return TBX_ERR_LAUNCH;
  hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(MET_THREADS), 0, (hipStream_t)stream, (const double*)partials, n_blocks, acc);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
