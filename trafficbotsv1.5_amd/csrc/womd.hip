// Post-processing of the joint futures on the device-resident rollout log (include/tbx_hip.h: tbx_womd_modes, tbx_pose_to_global).
#include "../../include/tbx_hip.h"
#include "pose_global_core.h"
#include "tbx_common.h"

namespace {

// ---------------------------------------------------------------------------------------------- WOMD modes
// WOMDPostProcessing.forward (data_modules/womd_post_processing.py:37-182) for ONE (scene, agent) per workgroup:
//   softmax over the K futures -> reduction to k = min(K, k_pred) modes (traj_topk :159-176 or mtr_nms :110-157) -> mpa_nms (:74-108)
//   -> temperature (:69-70) -> the 2 Hz samples of the kept futures (:72).
// Phases (256 threads, __syncthreads between them):
//   1. wave 0: softmax of the K log-probabilities into LDS.
//   2. selection. top-k: every future ranks itself by (score desc, index asc) against the K scores in LDS. mtr_nms: the xy rows of all K
//      futures are staged in LDS first (t-major, odd pitch: the staging writes and the per-future reads are both conflict-free); each
//      of the k greedy picks then needs ONE row of the K x K distance matrix, thread j sums the T distances pick <-> j in step order.
//   3. the k x k distances of the kept modes (from the staged rows; the top-k path stages only the k kept rows), one thread per pair.
//   4. thread 0: the order-dependent mpa_nms loop, renormalisation, temperature - k <= 8 values.
//   5. all threads: gather of the sampled steps from the log.
// Score arithmetic is double: the check against the reference is bounded by the reference's own float32 - float64 difference, the
// values are K <= 128 per workgroup, and float64 keeps this side of the comparison at the exact end. Distances are float32 sums in
// step order, compared with the float32 threshold as the reference does.
constexpr int WOMD_MAX_K = 128, WOMD_MAX_KEEP = 8, WOMD_MAX_T = 91, WOMD_THREADS = 256;

struct WomdArgs {
  const float* pose;      // [n_scene * K, A, ld_t, 3]
  const float* log_prob;  // [n_scene * K, A] or null (zeros)
  const uint8_t* ag_type; // [n_scene, A, 3]
  float* out_trajs;       // [n_scene, A, k, n_out, 3]
  float* out_scores;      // [n_scene, A, k]
  int32_t* out_idx;       // [n_scene, A, k] or null
  int K, A, ld_t, t_start, T, k_pred, use_ade, has_mtr, has_mpa, s_first, s_stride, n_out;
  float mtr[3], mpa[3], temperature;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

// mean (use_ade) or last-step (n_t == 1) xy distance of the staged columns ca and cb
__device__ __forceinline__ float staged_dist(const float* xs, const float* ys, int pitch, int n_t, int ca, int cb) {
  float acc = 0.f;
  for (int t = 0; t < n_t; ++t) {
    const float dx = xs[t * pitch + ca] - xs[t * pitch + cb], dy = ys[t * pitch + ca] - ys[t * pitch + cb];
    acc += sqrtf(dx * dx + dy * dy);
  }
  return acc / (float)n_t;
}

__global__ __launch_bounds__(WOMD_THREADS) void womd_modes_kernel(const WomdArgs p) {
  extern __shared__ __align__(16) float staged[];  // xs [n_t, pitch] | ys [n_t, pitch]
  __shared__ double sc[WOMD_MAX_K];                // softmax scores
  __shared__ double work[WOMD_MAX_K];              // mtr_nms: the suppressed clone
  __shared__ double kept[WOMD_MAX_KEEP];
  __shared__ int sel[WOMD_MAX_KEEP], pick;
  __shared__ uint8_t within[WOMD_MAX_KEEP * WOMD_MAX_KEEP];

  const int tid = threadIdx.x, lane = tid & 63;
  const int s = blockIdx.x / p.A, a = blockIdx.x % p.A;
  const int K = p.K, k = K < p.k_pred ? K : p.k_pred;
  const bool reduce = K > p.k_pred, mtr = reduce && p.has_mtr;
  const int n_t = p.use_ade ? p.T : 1, t_lo = p.T - n_t;
  const int n_col = mtr ? K : k, pitch = n_col | 1;
  float* xs = staged;
  float* ys = staged + n_t * pitch;
  const uint8_t* ty = p.ag_type + ((int64_t)s * p.A + a) * 3;
  // threshold = sum_i type_i * thresh_i in float32 (womd_post_processing.py:88-90, :127-129); 0 for an agent without a type
  const float thr_mtr = ((0.f + (ty[0] ? p.mtr[0] : 0.f)) + (ty[1] ? p.mtr[1] : 0.f)) + (ty[2] ? p.mtr[2] : 0.f);
  const float thr_mpa = ((0.f + (ty[0] ? p.mpa[0] : 0.f)) + (ty[1] ? p.mpa[1] : 0.f)) + (ty[2] ? p.mpa[2] : 0.f);
  auto row = [&](int j) { return p.pose + ((((int64_t)s * K + j) * p.A + a) * p.ld_t + p.t_start) * 3; };
  auto stage = [&](bool by_sel) {
    for (int i = tid; i < n_col * n_t; i += WOMD_THREADS) {
      const int c = i / n_t, t = i % n_t;
      const float* r = row(by_sel ? sel[c] : c) + (t_lo + t) * 3;
      xs[t * pitch + c] = r[0];
      ys[t * pitch + c] = r[1];
    }
  };

  // ---- 1. softmax (:55)
  if (tid < 64) {
    double v[2], m = -INFINITY;
    for (int h = 0; h < 2; ++h) {
      const int j = lane + 64 * h;
      v[h] = j < K ? (p.log_prob ? (double)p.log_prob[((int64_t)s * K + j) * p.A + a] : 0.0) : -INFINITY;
      m = fmax(m, v[h]);
    }
    m = wave_max_f64(m);
    double e[2], sum = 0.0;
    for (int h = 0; h < 2; ++h) {
      e[h] = lane + 64 * h < K ? exp(v[h] - m) : 0.0;
      sum += e[h];
    }
    sum = wave_sum_f64(sum);
    for (int h = 0; h < 2; ++h)
      if (lane + 64 * h < K) sc[lane + 64 * h] = e[h] / sum;
  }
  if (tid < WOMD_MAX_KEEP) sel[tid] = tid < K ? tid : 0;  // K <= k_pred: the futures pass through; every entry stays a valid index
  __syncthreads();

  // ---- 2. K -> k
  if (mtr) {
    stage(false);
    if (tid < K) work[tid] = sc[tid];
    for (int it = 0; it < k; ++it) {
      if (tid == 0) pick = 0;
      __syncthreads();
      if (tid < K) {  // first maximum (:140)
        const double v = work[tid];
        bool best = true;
        for (int j = 0; j < K; ++j) best = best && !(work[j] > v || (work[j] == v && j < tid));
        if (best) pick = tid;
      }
      __syncthreads();
      const int pk = pick;
      if (tid < K) {  // :142-145 (the pick itself is within its own threshold, then marked taken)
        const bool near = staged_dist(xs, ys, pitch, n_t, pk, tid) < thr_mtr;
        work[tid] = tid == pk ? -1.0 : work[tid] * (double)(near ? 0.01f : 1.0f);
      }
      if (tid == 0) sel[it] = pk;
      __syncthreads();
    }
  } else if (reduce) {
    if (tid < K) {  // descending score, ties to the lower future index
      const double v = sc[tid];
      int rank = 0;
      for (int j = 0; j < K; ++j) rank += (sc[j] > v || (sc[j] == v && j < tid)) ? 1 : 0;
      if (rank < k) sel[rank] = tid;
    }
    __syncthreads();
  }
  if (!mtr) {
    stage(true);
    __syncthreads();
  }

  // ---- 3. which kept modes lie within the mpa_nms threshold of each other (:92-96)
  if (p.has_mpa && tid < k * k) {
    const int m1 = tid / k, m2 = tid % k;
    within[tid] = staged_dist(xs, ys, pitch, n_t, mtr ? sel[m1] : m1, mtr ? sel[m2] : m2) < thr_mpa;
  }
  __syncthreads();

  // ---- 4. the serial part on k <= 8 values
  if (tid == 0) {
    double v[WOMD_MAX_KEEP], sum = 0.0;
    for (int m = 0; m < k; ++m) sum += (v[m] = sc[sel[m]]);
    if (reduce)
      for (int m = 0; m < k; ++m) v[m] /= sum;  // :155, :175
    if (p.has_mpa) {
      // visited in descending order of the INCOMING scores (ties: lower mode first); the comparison reads the CURRENT ones (:98-104)
      int order[WOMD_MAX_KEEP];
      for (int m = 0; m < k; ++m) {
        int r = 0;
        for (int j = 0; j < k; ++j) r += (v[j] > v[m] || (v[j] == v[m] && j < m)) ? 1 : 0;
        order[r] = m;
      }
      for (int o = 0; o < k; ++o) {
        const int m = order[o];
        bool hit = false;
        for (int j = 0; j < k; ++j) hit = hit || (within[m * k + j] && v[j] > v[m]);
        if (hit) v[m] = (double)1e-3f;
      }
      sum = 0.0;
      for (int m = 0; m < k; ++m) sum += v[m];
      for (int m = 0; m < k; ++m) v[m] /= sum;
    }
    if (p.temperature > 0.f) {  // :69-70
      double mx = -INFINITY;
      for (int m = 0; m < k; ++m) mx = fmax(mx, v[m] = log(v[m]) / (double)p.temperature);
      sum = 0.0;
      for (int m = 0; m < k; ++m) sum += (v[m] = exp(v[m] - mx));
      for (int m = 0; m < k; ++m) v[m] /= sum;
    }
    for (int m = 0; m < k; ++m) kept[m] = v[m];
  }
  __syncthreads();

  // ---- 5. outputs
  const int64_t o = ((int64_t)s * p.A + a) * k;
  if (tid < k) {
    p.out_scores[o + tid] = (float)kept[tid];
    if (p.out_idx) p.out_idx[o + tid] = sel[tid];
  }
  for (int i = tid; i < k * p.n_out * 3; i += WOMD_THREADS) {
    const int m = i / (p.n_out * 3), r = i % (p.n_out * 3);
    p.out_trajs[o * p.n_out * 3 + i] = row(sel[m])[(p.s_first + (r / 3) * p.s_stride) * 3 + r % 3];
  }
}

// ---------------------------------------------------------------------------------------------- scenario frame -> global frame
// torch_pos2global / torch_rad2global as pose_global_core.h states them (shared with tbx_womd_predictions of libtbx_sub.so). One thread per
// point; points are rows of n_t steps with ld_t steps per row.
__global__ void pose_to_global_kernel(const float* __restrict__ xy, int ld_xy, const float* __restrict__ yaw, int ld_yaw,
                                      const float* __restrict__ center, const float* __restrict__ scen_yaw, int64_t per_scene, int n_t,
                                      int ld_t, int64_t total, float* __restrict__ out_pos, float* __restrict__ out_yaw) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t sc = i / per_scene, src = (i / n_t) * ld_t + i % n_t;
  const float th = scen_yaw[sc];
  float sn, cs;
  sincosf(th, &sn, &cs);
  tbx::pos_to_global(xy[src * ld_xy], xy[src * ld_xy + 1], sn, cs, center[sc * 2], center[sc * 2 + 1], out_pos + i * 2, out_pos + i * 2 + 1);
  out_yaw[i] = tbx::yaw_to_global(yaw[src * ld_yaw], th);
}

}  // namespace

extern "C" int tbx_womd_modes(const float* pred_pose, const float* log_prob, const uint8_t* ag_type, int n_scene, int n_k, int n_ag,
                              int ld_t, int t_start, int n_step, int k_pred, int use_ade, const float* mtr_nms_thresh,
                              const float* mpa_nms_thresh, float score_temperature, int sample_first, int sample_stride, int sample_end,
                              float* out_trajs, float* out_scores, int32_t* out_idx, void* stream) {
  if (!pred_pose || !ag_type || !out_trajs || !out_scores) return TBX_ERR_ARG;
  if (n_scene <= 0 || n_k <= 0 || n_ag <= 0 || ld_t <= 0 || t_start < 0 || n_step <= 0 || t_start + n_step > ld_t || k_pred <= 0)
    return TBX_ERR_ARG;
  if (sample_first < 0 || sample_stride <= 0 || sample_end > n_step) return TBX_ERR_ARG;
  if (n_k > WOMD_MAX_K || k_pred > WOMD_MAX_KEEP || n_step > WOMD_MAX_T) return TBX_ERR_UNSUPPORTED;
  if ((int64_t)n_scene * n_ag > 0x7fffffff) return TBX_ERR_UNSUPPORTED;
  WomdArgs p;
  p.pose = pred_pose, p.log_prob = log_prob, p.ag_type = ag_type;
  p.out_trajs = out_trajs, p.out_scores = out_scores, p.out_idx = out_idx;
  p.K = n_k, p.A = n_ag, p.ld_t = ld_t, p.t_start = t_start, p.T = n_step, p.k_pred = k_pred, p.use_ade = use_ade ? 1 : 0;
  p.has_mtr = mtr_nms_thresh != nullptr, p.has_mpa = mpa_nms_thresh != nullptr;
  p.s_first = sample_first, p.s_stride = sample_stride;
  p.n_out = sample_end > sample_first ? (sample_end - sample_first + sample_stride - 1) / sample_stride : 0;
  for (int i = 0; i < 3; ++i) p.mtr[i] = p.has_mtr ? mtr_nms_thresh[i] : 0.f, p.mpa[i] = p.has_mpa ? mpa_nms_thresh[i] : 0.f;
  p.temperature = score_temperature;
  const int k = n_k < k_pred ? n_k : k_pred;
  const int n_col = (n_k > k_pred && p.has_mtr) ? n_k : k, n_t = p.use_ade ? n_step : 1;
  const size_t lds = (size_t)2 * n_t * (n_col | 1) * sizeof(float);  // <= 2 * 91 * 129 * 4 = 93 912 B of the CU's 160 KiB
  static tbx::PerDeviceOnce lds_attr;
  if (!lds_attr([&] {
        return hipFuncSetAttribute((const void*)womd_modes_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   2 * WOMD_MAX_T * (WOMD_MAX_K | 1) * (int)sizeof(float)) == hipSuccess;
      }))
    return TBX_ERR_LAUNCH;
  hipLaunchKernelGGL(womd_modes_kernel, dim3((unsigned)(n_scene * n_ag)), dim3(WOMD_THREADS), lds, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}

extern "C" int tbx_pose_to_global(const float* xy, int ld_xy, const float* yaw, int ld_yaw, const float* scenario_center,
                                  const float* scenario_yaw, int n_scene, int64_t rows_per_scene, int n_t, int ld_t, float* out_pos,
                                  float* out_yaw, void* stream) {
  if (!xy || !yaw || !scenario_center || !scenario_yaw || !out_pos || !out_yaw) return TBX_ERR_ARG;
  if (n_scene <= 0 || rows_per_scene <= 0 || n_t <= 0 || ld_t < n_t || ld_xy < 2 || ld_yaw < 1) return TBX_ERR_ARG;
  const int64_t per_scene = rows_per_scene * n_t, total = per_scene * n_scene;
  if ((total + 255) / 256 > 0x7fffffff) return TBX_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pose_to_global_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xy, ld_xy, yaw,
                     ld_yaw, scenario_center, scenario_yaw, per_scene, n_t, ld_t, total, out_pos, out_yaw);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
