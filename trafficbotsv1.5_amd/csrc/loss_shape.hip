// Loss shaping of the training objective over a finished rollout log (include/tbx_hip_loss.h: tbx_loss_shape).
#include "../../include/tbx_hip.h"
#include "tbx_common.h"

namespace {

// models/metrics/training.py:90-138 (p_loss_for_irrelevant, w_relevant_agent, temporal_discount) as ONE pass over the log.
//   * a lane owns one (row, agent) pair and walks its steps in order: the discount m_t = tf_t ? 1 : m_{t-1} * discount is a recurrence in
//     time. Consecutive lanes take consecutive agents, so the training chain's [n, T, A] log is read coalesced. A lane walks pairs
//     lane, lane + n_lanes, ...: which lane sees which pair depends on the shapes alone.
//   * rv_t implies any_valid, so the agent weight a valid summand carries (1 + relevant * w_relevant) is known when step t is read: no
//     second walk for w.
//   * lane sums (float64 products of the float32 reward and weight) -> wave butterfly -> LDS -> thread 0/1 adds the waves in wave order ->
//     one partial row per workgroup, ordinary stores. loss_final_kernel (one workgroup) adds the rows to acc in row order.
//   No atomics anywhere: two calls on the same input give bit-equal results.
constexpr int LS_WAVES = 4, LS_THREADS = 64 * LS_WAVES, LS_MAX_BLOCKS = TBX_LOSS_PARTIAL_ROWS;

struct Log3 {
  int64_t s_row, s_ag, s_t;
};

struct LsArgs {
  const uint8_t* pred_valid;
  const uint8_t* tf;
  const uint8_t* reward_valid;  // null with reward: masks only
  const float* reward;
  const uint8_t* relevant;  // [n_pairs] or null
  const uint8_t* pick;      // [n_pairs] or null
  uint8_t* any_valid;       // [n_pairs]
  float* w_agent;           // [n_pairs]
  float* w;                 // or null
  double* partials;         // [gridDim.x, 2] (null with reward)
  Log3 l_pv, l_tf, l_rv, l_r, l_w;
  int64_t n_pairs;  // rows * A
  int A, T, t_start;
  bool tf_loss, mask_irrelevant;
  float w_relevant, discount;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(LS_THREADS) void loss_shape_kernel(const LsArgs p) {
  __shared__ double part[LS_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool has_reward = p.reward != nullptr;
  double sum = 0.0, count = 0.0;  // per lane
  const int64_t stride = (int64_t)gridDim.x * LS_THREADS;
  for (int64_t pair = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x; pair < p.n_pairs; pair += stride) {
    const int64_t row = pair / p.A;
    const int64_t a = pair - row * p.A;
    const bool rel = p.relevant != nullptr && p.relevant[pair] != 0;
    const bool keep = !p.mask_irrelevant || rel || (p.pick != nullptr && p.pick[pair] != 0);
    const float w_rel = (p.w_relevant > 0.f && rel) ? p.w_relevant : 0.f;
    const float w_valid = 1.f + w_rel;  // w_agent of an agent with any_valid
    const uint8_t* pv = p.pred_valid + row * p.l_pv.s_row + a * p.l_pv.s_ag;
    const uint8_t* tf = p.tf + row * p.l_tf.s_row + a * p.l_tf.s_ag;
    const uint8_t* rv = has_reward ? p.reward_valid + row * p.l_rv.s_row + a * p.l_rv.s_ag : nullptr;
    const float* r = has_reward ? p.reward + row * p.l_r.s_row + a * p.l_r.s_ag : nullptr;
    float* w = p.w != nullptr ? p.w + row * p.l_w.s_row + a * p.l_w.s_ag : nullptr;
    bool any = false;
    float m = 1.f;
    for (int t = 0; t < p.T; ++t) {
      const bool forced = tf[t * p.l_tf.s_t] != 0;
      const bool lv = keep && t >= p.t_start && (p.tf_loss || !forced) && pv[t * p.l_pv.s_t] != 0;
      any |= lv;
      if (has_reward) {
        if (p.discount > 0.f && t > 0) m = forced ? 1.f : m * p.discount;
        const bool v = lv && rv[t * p.l_rv.s_t] != 0;
        const float wt = v ? w_valid * m : 0.f;
        if (v) {
          sum += (double)r[t * p.l_r.s_t] * (double)wt;
          count += 1.0;
        }
        if (w != nullptr) w[t * p.l_w.s_t] = wt;
      }
    }
    p.any_valid[pair] = any ? 1 : 0;
    p.w_agent[pair] = (any ? 1.f : 0.f) + w_rel;
  }
  if (!has_reward) return;  // (uniform over the grid)
  sum = wave_sum_f64(sum);
  count = wave_sum_f64(count);
  if (lane == 0) part[wave][0] = sum, part[wave][1] = count;
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = part[0][threadIdx.x];
    for (int w = 1; w < LS_WAVES; ++w) s += part[w][threadIdx.x];
    p.partials[(int64_t)blockIdx.x * 2 + threadIdx.x] = s;
  }
}

// acc[c] += partials[0][c] + partials[1][c] + ... in row order. One workgroup: the rows are staged in LDS by all threads, then thread c
// walks its column.
__global__ __launch_bounds__(LS_THREADS) void loss_final_kernel(const double* __restrict__ partials, int n_rows, double* __restrict__ acc) {
  __shared__ double rows[LS_MAX_BLOCKS * 2];
  for (int i = threadIdx.x; i < n_rows * 2; i += LS_THREADS) rows[i] = partials[i];
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = rows[threadIdx.x];
    for (int r = 1; r < n_rows; ++r) s += rows[r * 2 + threadIdx.x];
    acc[threadIdx.x] += s;
  }
}

Log3 log3(const int64_t* s) { return Log3{s[0], s[1], s[2]}; }

}  // namespace

extern "C" int tbx_loss_shape(const tbx_loss_shape_t* args, void* stream) {
  if (!args) return TBX_ERR_ARG;
  const tbx_loss_shape_t& a = *args;
  if (!a.pred_valid || !a.tf || !a.any_valid || !a.w_agent) return TBX_ERR_ARG;
  if (a.rows < 0 || a.n_ag <= 0 || a.n_step <= 0 || a.step_training_start < 0) return TBX_ERR_ARG;
  if ((a.mask_irrelevant != 0 || a.w_relevant > 0.f) && !a.relevant) return TBX_ERR_ARG;
  if ((a.reward != nullptr) != (a.reward_valid != nullptr)) return TBX_ERR_ARG;
  if (a.w && !a.reward) return TBX_ERR_ARG;
  if (a.reward && (!a.acc || !a.partials)) return TBX_ERR_ARG;
  if (a.rows == 0) return TBX_OK;
  if (a.rows >= ((int64_t)1 << 31) / a.n_ag + (((int64_t)1 << 31) % a.n_ag != 0)) return TBX_ERR_UNSUPPORTED;  // rows * n_ag >= 2^31
  LsArgs p;
  p.pred_valid = a.pred_valid, p.tf = a.tf, p.reward_valid = a.reward_valid, p.reward = a.reward;
  p.relevant = a.relevant, p.pick = a.mask_irrelevant != 0 ? a.pick : nullptr;
  p.any_valid = a.any_valid, p.w_agent = a.w_agent, p.w = a.w, p.partials = a.partials;
  p.l_pv = log3(a.pred_valid_stride), p.l_tf = log3(a.tf_stride), p.l_rv = log3(a.reward_valid_stride), p.l_r = log3(a.reward_stride);
  p.l_w = log3(a.w_stride);
  p.n_pairs = a.rows * a.n_ag;
  p.A = a.n_ag, p.T = a.n_step, p.t_start = a.step_training_start;
  p.tf_loss = a.loss_for_teacher_forcing != 0, p.mask_irrelevant = a.mask_irrelevant != 0;
  p.w_relevant = a.w_relevant, p.discount = a.discount;
  const int64_t want = (p.n_pairs + LS_THREADS - 1) / LS_THREADS;
  const int n_blocks = (int)(want < LS_MAX_BLOCKS ? want : LS_MAX_BLOCKS);
  hipLaunchKernelGGL(loss_shape_kernel, dim3((unsigned)n_blocks), dim3(LS_THREADS), 0, (hipStream_t)stream, p);
  if (hipGetLastError() != hipSuccess) return TBX_ERR_LAUNCH;
  if (!a.reward) return TBX_OK;
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(LS_THREADS), 0, (hipStream_t)stream, (const double*)a.partials, n_blocks, a.acc);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
