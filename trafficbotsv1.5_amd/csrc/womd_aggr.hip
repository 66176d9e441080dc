// Trajectory aggregation of the WOMD post-processing on the device-resident rollout log (include/tbx_hip_aggr.h: tbx_womd_aggr).
#include "../../include/tbx_hip_aggr.h"
#include "tbx_common.h"

namespace {

// WOMDPostProcessing.forward with aggr_thresh set (data_modules/womd_post_processing.py:37-72, traj_aggr :178-278) for ONE (scene, agent)
// per workgroup: softmax over the K futures -> k_pred greedy seeds with suppression (:220-232) -> n_iter_em rounds of k-means over whole
// trajectories (:242-275) -> renormalisation (:277) -> mpa_nms on the centres -> temperature -> the 2 Hz samples of the centres.
// Phases (256 threads, __syncthreads between them):
//   1. wave 0: softmax of the K log-probabilities into LDS; all threads: the xy rows of the K futures into LDS (t-major, odd pitch, as
//      womd.hip stages them: the staging writes and the per-future reads are conflict-free).
//   2. seeds: per pick ONE row of the K x K distance matrix, thread j sums the T distances pick <-> j in step order.
//   3. per EM round: E - the K x k (future, centre) distances spread over the threads (future fastest: the staged reads are consecutive,
//      the centre reads broadcast), then thread j takes the first minimum of its row; k threads count the members; repair - only when a
//      cluster is empty: thread 0, in the reference's order, on K <= 128 bytes and k <= 8 counts; every future finds its place in its
//      cluster's member list (ascending future index); M - one thread per (step, cluster) sums its members' xy in list order.
//   4. the k x k distances of the centres; thread 0: the order-dependent mpa_nms loop, renormalisation, temperature.
//   5. all threads: the centres at the sampled steps, (x, y, yaw) summed from the log over the members in ascending future index - for
//      x, y the operations of the M-step on the same values, hence the LDS centres' bits; yaw is needed nowhere else.
// Score arithmetic is double, distances and thresholds float32, for the reason womd.hip gives (its lines 20-22).
constexpr int AGGR_THREADS = 256, AGGR_CPITCH = TBX_AGGR_MAX_KEEP + 1;

struct AggrArgs {
  const float* pose;
  const float* log_prob;
  const uint8_t* ag_type;
  float* out_trajs;
  float* out_scores;
  int32_t* out_idx;
  int K, A, ld_t, t_start, T, k, use_ade, n_iter, has_mpa, s_first, s_stride, n_out;
  float aggr[3], mpa[3], temperature;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

// mean (use_ade) or last-step (n_t == 1) xy distance of column ca of (ax, ay) and column cb of (bx, by)
__device__ __forceinline__ float col_dist(const float* ax, const float* ay, int pa, int ca, const float* bx, const float* by, int pb, int cb,
                                          int n_t) {
  float acc = 0.f;
  for (int t = 0; t < n_t; ++t) {
    const float dx = ax[t * pa + ca] - bx[t * pb + cb], dy = ay[t * pa + ca] - by[t * pb + cb];
    acc += sqrtf(dx * dx + dy * dy);
  }
  return acc / (float)n_t;
}

__global__ __launch_bounds__(AGGR_THREADS) void womd_aggr_kernel(const AggrArgs p) {
  extern __shared__ __align__(16) float staged[];  // xs [n_t, pitch] | ys [n_t, pitch] | cx [n_t, 9] | cy [n_t, 9]
  __shared__ double sc[TBX_AGGR_MAX_K];            // softmax scores
  __shared__ double work[TBX_AGGR_MAX_K];          // the suppressed clone
  __shared__ double csc[TBX_AGGR_MAX_KEEP];        // centre scores, then the final ones
  __shared__ float dist[TBX_AGGR_MAX_KEEP * TBX_AGGR_MAX_K];
  __shared__ int sel[TBX_AGGR_MAX_KEEP], cnt[TBX_AGGR_MAX_KEEP], first[TBX_AGGR_MAX_KEEP], pick;
  __shared__ uint8_t assign[TBX_AGGR_MAX_K];   // the cluster of every future
  __shared__ uint8_t members[TBX_AGGR_MAX_K];  // the futures sorted by (cluster, index): cluster m owns [first[m], first[m] + cnt[m])
  __shared__ uint8_t within[TBX_AGGR_MAX_KEEP * TBX_AGGR_MAX_KEEP];
  __shared__ uint8_t was_empty[TBX_AGGR_MAX_KEEP];  // per round: the clusters without a member before the repair

  const int tid = threadIdx.x, lane = tid & 63;
  const int s = blockIdx.x / p.A, a = blockIdx.x % p.A;
  const int K = p.K, k = p.k;
  const int n_t = p.use_ade ? p.T : 1, t_lo = p.T - n_t;
  const int pitch = K | 1;
  float* xs = staged;
  float* ys = xs + n_t * pitch;
  float* cx = ys + n_t * pitch;
  float* cy = cx + n_t * AGGR_CPITCH;
  const uint8_t* ty = p.ag_type + ((int64_t)s * p.A + a) * 3;
  // threshold = sum_i type_i * thresh_i in float32 (womd_post_processing.py:88-90, :124-126); 0 for an agent without a type
  const float thr_aggr = ((0.f + (ty[0] ? p.aggr[0] : 0.f)) + (ty[1] ? p.aggr[1] : 0.f)) + (ty[2] ? p.aggr[2] : 0.f);
  const float thr_mpa = ((0.f + (ty[0] ? p.mpa[0] : 0.f)) + (ty[1] ? p.mpa[1] : 0.f)) + (ty[2] ? p.mpa[2] : 0.f);
  auto row = [&](int j) { return p.pose + ((((int64_t)s * K + j) * p.A + a) * p.ld_t + p.t_start) * 3; };

  // ---- 1. softmax (:53), staging
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
      if (lane + 64 * h < K) sc[lane + 64 * h] = work[lane + 64 * h] = e[h] / sum;
  }
  for (int i = tid; i < K * n_t; i += AGGR_THREADS) {
    const int c = i / n_t, t = i % n_t;
    const float* r = row(c) + (t_lo + t) * 3;
    xs[t * pitch + c] = r[0];
    ys[t * pitch + c] = r[1];
  }
  __syncthreads();

  // ---- 2. seeds (:220-232)
  for (int it = 0; it < k; ++it) {
    if (tid == 0) pick = 0;
    __syncthreads();
    if (tid < K) {  // first maximum (:223)
      const double v = work[tid];
      bool best = true;
      for (int j = 0; j < K; ++j) best = best && !(work[j] > v || (work[j] == v && j < tid));
      if (best) pick = tid;
    }
    __syncthreads();
    const int pk = pick;
    if (tid < K) {  // :225-230 (the pick itself is within its own threshold, suppressed like the others, then 1 is taken off)
      const bool near = col_dist(xs, ys, pitch, pk, xs, ys, pitch, tid, n_t) < thr_aggr;
      const double w = work[tid] * (double)(near ? 0.1f : 1.0f);
      work[tid] = tid == pk ? w - 1.0 : w;
    }
    if (tid == 0) sel[it] = pk;
    __syncthreads();
  }
  // the centres start as the picks (:237-238)
  for (int i = tid; i < k * n_t; i += AGGR_THREADS) {
    const int m = i % k, t = i / k;
    cx[t * AGGR_CPITCH + m] = xs[t * pitch + sel[m]];
    cy[t * AGGR_CPITCH + m] = ys[t * pitch + sel[m]];
  }
  if (tid < k) csc[tid] = sc[sel[tid]];
  __syncthreads();

  // ---- 3. EM (:242-275)
  for (int it = 0; it < p.n_iter; ++it) {
    for (int i = tid; i < K * k; i += AGGR_THREADS) {
      const int j = i % K, m = i / K;
      dist[m * K + j] = col_dist(cx, cy, AGGR_CPITCH, m, xs, ys, pitch, j, n_t);
    }
    __syncthreads();
    if (tid < K) {  // first minimum (:251)
      int best = 0;
      float bd = dist[tid];
      for (int m = 1; m < k; ++m) {
        const float d = dist[m * K + tid];
        if (d < bd) bd = d, best = m;
      }
      assign[tid] = (uint8_t)best;
    }
    __syncthreads();
    if (tid < k) {
      int n = 0;
      for (int j = 0; j < K; ++j) n += assign[j] == tid ? 1 : 0;
      cnt[tid] = n;
      was_empty[tid] = n == 0;
    }
    __syncthreads();
    // the list of empty clusters is taken once, before the first repair. Read from was_empty, which the repair does not write (it
    // moves cnt and assign): every thread forms the same mask whenever it reads, so the barrier inside the branch is uniform
    unsigned empty = 0;
    for (int m = 0; m < k; ++m) empty |= was_empty[m] ? 1u << m : 0u;
    if (empty) {
      if (tid == 0) {  // :254-268
        for (int m = 0; m < k; ++m) {
          if (!((empty >> m) & 1u)) continue;
          int big = 0;
          for (int c = 1; c < k; ++c)
            if (cnt[c] > cnt[big]) big = c;
          int move = cnt[big] / 2;
          for (int j = 0; j < K && move > 0; ++j)
            if (assign[j] == big) assign[j] = (uint8_t)m, --move, --cnt[big], ++cnt[m];
        }
      }
      __syncthreads();
    }
    if (tid < K) {  // the clusters' member lists, each in ascending future index
      const int m = assign[tid];
      int pos = 0;
      for (int c = 0; c < m; ++c) pos += cnt[c];
      for (int j = 0; j < tid; ++j) pos += assign[j] == m ? 1 : 0;
      members[pos] = (uint8_t)tid;
    }
    if (tid < k) {
      int f = 0;
      for (int c = 0; c < tid; ++c) f += cnt[c];
      first[tid] = f;
    }
    __syncthreads();
    for (int i = tid; i < k * n_t; i += AGGR_THREADS) {  // :272-273
      const int m = i % k, t = i / k, f = first[m], n = cnt[m];
      float ax = 0.f, ay = 0.f;
      for (int q = f; q < f + n; ++q) {
        const int j = members[q];
        ax += xs[t * pitch + j], ay += ys[t * pitch + j];
      }
      cx[t * AGGR_CPITCH + m] = ax / (float)n;
      cy[t * AGGR_CPITCH + m] = ay / (float)n;
    }
    if (tid < k) {  // :275
      const int f = first[tid], n = cnt[tid];
      double acc = 0.0;
      for (int q = f; q < f + n; ++q) acc += sc[members[q]];
      csc[tid] = acc / (double)n;
    }
    __syncthreads();
  }

  // ---- 4. which centres lie within the mpa_nms threshold of each other (:92-96), then the serial part on k <= 8 values
  if (p.has_mpa && tid < k * k) {
    const int m1 = tid / k, m2 = tid % k;
    within[tid] = col_dist(cx, cy, AGGR_CPITCH, m1, cx, cy, AGGR_CPITCH, m2, n_t) < thr_mpa;
  }
  __syncthreads();
  if (tid == 0) {
    double v[TBX_AGGR_MAX_KEEP], sum = 0.0;
    for (int m = 0; m < k; ++m) sum += (v[m] = csc[m]);
    for (int m = 0; m < k; ++m) v[m] /= sum;  // :277
    if (p.has_mpa) {
      // visited in descending order of the INCOMING scores (ties: lower mode first); the comparison reads the CURRENT ones (:98-104)
      int order[TBX_AGGR_MAX_KEEP];
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
    for (int m = 0; m < k; ++m) csc[m] = v[m];
  }
  __syncthreads();

  // ---- 5. outputs
  const int64_t o = ((int64_t)s * p.A + a) * k;
  if (tid < k) {
    p.out_scores[o + tid] = (float)csc[tid];
    if (p.out_idx) p.out_idx[o + tid] = sel[tid];
  }
  for (int i = tid; i < k * p.n_out * 3; i += AGGR_THREADS) {
    const int m = i / (p.n_out * 3), r = i % (p.n_out * 3);
    const int off = (p.s_first + (r / 3) * p.s_stride) * 3 + r % 3;
    float v;
    if (p.n_iter == 0) {
      v = row(sel[m])[off];
    } else {
      const int f = first[m], n = cnt[m];
      float acc = 0.f;
      for (int q = f; q < f + n; ++q) acc += row(members[q])[off];
      v = acc / (float)n;
    }
    p.out_trajs[o * p.n_out * 3 + i] = v;
  }
}

constexpr int AGGR_MAX_LDS = 2 * TBX_AGGR_MAX_T * ((TBX_AGGR_MAX_K | 1) + AGGR_CPITCH) * (int)sizeof(float);  // 100 464 B of the CU's 160 KiB

}  // namespace

extern "C" int tbx_womd_aggr(const tbx_womd_aggr_t* a, void* stream) {
  if (!a || !a->pred_pose || !a->ag_type || !a->out_trajs || !a->out_scores) return TBX_ERR_ARG;
  if (a->n_scene <= 0 || a->n_k <= 0 || a->n_ag <= 0 || a->ld_t <= 0 || a->t_start < 0 || a->n_step <= 0 ||
      (int64_t)a->t_start + a->n_step > a->ld_t || a->k_pred <= 0 || a->n_iter_em < 0)
    return TBX_ERR_ARG;
  if (a->sample_first < 0 || a->sample_stride <= 0 || a->sample_end > a->n_step) return TBX_ERR_ARG;
  if (a->n_k > TBX_AGGR_MAX_K || a->k_pred > TBX_AGGR_MAX_KEEP || a->n_step > TBX_AGGR_MAX_T) return TBX_ERR_UNSUPPORTED;
  if (a->n_k <= a->k_pred) return TBX_ERR_ARG;  // nothing to aggregate: tbx_womd_modes' case
  if ((int64_t)a->n_scene * a->n_ag > 0x7fffffff) return TBX_ERR_UNSUPPORTED;
  AggrArgs p;
  p.pose = a->pred_pose, p.log_prob = a->log_prob, p.ag_type = a->ag_type;
  p.out_trajs = a->out_trajs, p.out_scores = a->out_scores, p.out_idx = a->out_idx;
  p.K = a->n_k, p.A = a->n_ag, p.ld_t = a->ld_t, p.t_start = a->t_start, p.T = a->n_step, p.k = a->k_pred, p.use_ade = a->use_ade ? 1 : 0;
  p.n_iter = a->n_iter_em, p.has_mpa = a->has_mpa ? 1 : 0;
  p.s_first = a->sample_first, p.s_stride = a->sample_stride;
  p.n_out = a->sample_end > a->sample_first ? (a->sample_end - a->sample_first + a->sample_stride - 1) / a->sample_stride : 0;
  for (int i = 0; i < 3; ++i) p.aggr[i] = a->aggr_thresh[i], p.mpa[i] = p.has_mpa ? a->mpa_nms_thresh[i] : 0.f;
  p.temperature = a->score_temperature;
  const int n_t = p.use_ade ? p.T : 1;
  const size_t lds = (size_t)2 * n_t * ((p.K | 1) + AGGR_CPITCH) * sizeof(float);
  static tbx::PerDeviceOnce lds_attr;
  if (!lds_attr([&] {
        return hipFuncSetAttribute((const void*)womd_aggr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AGGR_MAX_LDS) == hipSuccess;
      }))
    return TBX_ERR_LAUNCH;
  hipLaunchKernelGGL(womd_aggr_kernel, dim3((unsigned)(a->n_scene * a->n_ag)), dim3(AGGR_THREADS), lds, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
