// The reward term that couples the agents of a scene (tbx_collision_reward_fwd / _bwd, include/tbx_hip_reward.h): the relaxed
// five-circle overlap of utils/rewards.py:87-154 for every (row, step) of a finished pose log, and its gradient with respect to
// the poses. The term never feeds back into the state (the policy inputs are detached, the reward is only logged), so it is one
// launch over the whole log instead of a part of every step. One workgroup per (row, step): the A agents' circle centres, radii,
// headings and validity are staged in LDS once, then TBX_COLLISION_LANES lanes per agent share the loop over the partners
// (contiguous ranges, combined in lane order: no atomics, bit-equal between calls).
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbx_hip.h"
#include "tbx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kCap = TBX_COLLISION_MAX_AG;
constexpr int kLanes = TBX_COLLISION_LANES;
constexpr int kThreads = 256;
constexpr int kGroups = kThreads / kLanes;  // agents per pass
constexpr float kEps = FLT_EPSILON;
static_assert(kLanes == 4 && 64 % kLanes == 0, "an agent's lanes are neighbours inside one wave");

struct Log {  // a [row, agent, step] log addressed through element strides
  int64_t s_row, s_ag, s_t;
  __host__ __device__ int64_t at(int64_t row, int a, int t) const { return row * s_row + a * s_ag + t * s_t; }
};

struct Args {
  const float* pose;
  const uint8_t* valid;
  const float* ag_size;
  Log lp, lv, lc;
  int n_k, n_ag, n_t, reduce_max;
};

// LDS image of one (row, step): per agent the five circle centres, the radius, d = (l - w) / 4, the heading and the validity.
// (forward: the first 11 arrays + valid; backward: all, and the upstream weight / arg-max partner of every row)
struct Stage {
  float* cx;  // [5][A]
  float* cy;  // [5][A]
  float* r;   // [A]
  float* d;   // [A]
  float* hx;  // [A]
  float* hy;  // [A]
  float* g;   // [A]
  int* arg;   // [A]
  int* valid; // [A]
  int* wsum;  // [kThreads / 64]
};
constexpr int kWordsFwd = 12, kWordsBwd = 17;  // per agent

__device__ __forceinline__ Stage carve(float* smem, int A, bool bwd) {
  Stage s;
  s.cx = smem, s.cy = smem + 5 * A, s.r = smem + 10 * A;
  s.valid = reinterpret_cast<int*>(smem + 11 * A);
  float* p = smem + 12 * A;
  s.d = s.hx = s.hy = s.g = nullptr, s.arg = nullptr;
  if (bwd) s.d = p, s.hx = p + A, s.hy = p + 2 * A, s.g = p + 3 * A, p += 4 * A;
  s.wsum = reinterpret_cast<int*>(p);
  if (bwd) s.arg = reinterpret_cast<int*>(p) + kThreads / 64;
  return s;
}

// Stages the step and returns the step's count of valid agents (to every thread).
__device__ __forceinline__ int stage_step(const Args& k, const Stage& s, int64_t row, int t, bool bwd) {
  const int A = k.n_ag;
  const int64_t scene = row / k.n_k;
  int cnt = 0;
  for (int a = threadIdx.x; a < A; a += kThreads) {
    const float* p = k.pose + k.lp.at(row, a, t);
    const float x = p[0], y = p[1], yaw = p[2];
    const float s0 = k.ag_size[(scene * A + a) * 3], s1 = k.ag_size[(scene * A + a) * 3 + 1];
    const float w = fminf(s0, s1), l = fmaxf(s0, s1);
    const float d = (l - w) / 4.0f;
    const float hx = cosf(yaw), hy = sinf(yaw);
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const float m = (float)(c - 2);
      s.cx[c * A + a] = x + (m * hx) * d;
      s.cy[c * A + a] = y + (m * hy) * d;
    }
    s.r[a] = w / 2.0f + kEps;
    const int v = k.valid[k.lv.at(row, a, t)] != 0;
    s.valid[a] = v;
    cnt += v;
    if (bwd) s.d[a] = d, s.hx[a] = hx, s.hy[a] = hy;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) s.wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  int n_valid = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) n_valid += s.wsum[w];
  return n_valid;
}

struct Circles {
  float x[5], y[5];
};

__device__ __forceinline__ Circles load_circles(const Stage& s, int A, int a) {
  Circles c;
#pragma unroll
  for (int q = 0; q < 5; ++q) c.x[q] = s.cx[q * A + a], c.y[q] = s.cy[q * A + a];
  return c;
}

// The first minimum of the 25 squared centre distances, p's circle major, q's minor (sqrt is monotone: the minimum of the distances
// is the distance of the minimum; two squared distances that differ round to one distance only within an ulp of a tie).
__device__ __forceinline__ void min_pair(const Circles& p, const Circles& q, float& d2m, float& dxm, float& dym, int& im, int& jm) {
  d2m = INFINITY, dxm = dym = 0.f, im = jm = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const float dx = p.x[i] - q.x[j], dy = p.y[i] - q.y[j];
      const float d2 = dx * dx + dy * dy;
      if (d2 < d2m) d2m = d2, dxm = dx, dym = dy, im = i, jm = j;
    }
}

__device__ __forceinline__ float pair_term(const Circles& p, const Circles& q, float r_sum) {
  float d2, dx, dy;
  int i, j;
  min_pair(p, q, d2, dx, dy, i, j);
  return fmaxf(1.0f - (sqrtf(d2) + kEps) / r_sum, 0.0f);
}

__global__ __launch_bounds__(kThreads) void collision_fwd_kernel(const Args k, float* __restrict__ c_out, int32_t* __restrict__ arg_out) {
  extern __shared__ float smem[];
  const int A = k.n_ag;
  const int64_t row = blockIdx.x / k.n_t;
  const int t = blockIdx.x % k.n_t;
  const Stage s = carve(smem, A, false);
  const int n_valid = stage_step(k, s, row, t, false);
  const int lane = threadIdx.x % kLanes, base = (threadIdx.x & 63) - lane;
  const int chunk = (A + kLanes - 1) / kLanes;
  const int j0 = lane * chunk, j1 = min(A, j0 + chunk);
  for (int i0 = 0; i0 < A; i0 += kGroups) {  // (uniform trip count: the combine below shuffles across the whole wave)
    const int i = i0 + threadIdx.x / kLanes;
    const bool live = i < A && s.valid[i];
    float best = 0.f, sum = 0.f;
    int bj = -1;
    if (live) {
      const Circles ci = load_circles(s, A, i);
      const float ri = s.r[i];
      for (int j = j0; j < j1; ++j) {
        if (j == i || !s.valid[j]) continue;
        const float c = pair_term(ci, load_circles(s, A, j), s.r[j] + ri);
        if (c > best) best = c, bj = j;
        sum += fminf(c, 1.0f);
      }
    }
    // lane order = ascending j: a later lane wins the max only when strictly larger
    float best_all = 0.f, sum_all = 0.f;
    int bj_all = -1;
#pragma unroll
    for (int q = 0; q < kLanes; ++q) {
      const float b = __shfl(best, base + q, 64), sm = __shfl(sum, base + q, 64);
      const int bq = __shfl(bj, base + q, 64);
      if (b > best_all) best_all = b, bj_all = bq;
      sum_all = q == 0 ? sm : sum_all + sm;
    }
    if (i < A && lane == 0) {
      float c = 0.f;
      if (live) c = k.reduce_max ? best_all : (n_valid > 0 ? sum_all / (float)n_valid : 0.f);
      c_out[k.lc.at(row, i, t)] = c;
      if (k.reduce_max && arg_out) arg_out[((int64_t)blockIdx.x) * A + i] = live ? bj_all : -1;
    }
  }
}

struct Grad3 {
  float x, y, w;
};

// d(c_pq)/d(pose of `self`) times `weight` added to acc, for the pair (first agent p, second agent q); self_first: the pose is p's.
__device__ __forceinline__ void pair_grad(const Stage& s, int A, int p, int q, bool self_first, float weight, Grad3& acc) {
  float d2, dx, dy;
  int i, j;
  min_pair(load_circles(s, A, p), load_circles(s, A, q), d2, dx, dy, i, j);
  const float dist = sqrtf(d2), r_sum = s.r[q] + s.r[p];
  if (!(1.0f - (dist + kEps) / r_sum >= 0.0f) || dist == 0.0f) return;  // clamped away / coincident centres: no gradient
  const float coef = -weight / r_sum;                                      // dL/d(dist)
  float gx = coef * (dx / dist), gy = coef * (dy / dist);                  // dL/d(centre i of p) = -dL/d(centre j of q)
  const int self = self_first ? p : q;
  const float m = (float)((self_first ? i : j) - 2);
  if (!self_first) gx = -gx, gy = -gy;
  acc.x += gx, acc.y += gy;
  acc.w += m * s.d[self] * (gy * s.hx[self] - gx * s.hy[self]);
}

__global__ __launch_bounds__(kThreads) void collision_bwd_kernel(const Args k, const float* __restrict__ g, const int32_t* __restrict__ arg,
                                                                 float* __restrict__ d_pose) {
  extern __shared__ float smem[];
  const int A = k.n_ag;
  const int64_t row = blockIdx.x / k.n_t;
  const int t = blockIdx.x % k.n_t;
  const Stage s = carve(smem, A, true);
  for (int a = threadIdx.x; a < A; a += kThreads) {
    s.g[a] = g[k.lc.at(row, a, t)];
    s.arg[a] = k.reduce_max ? arg[(int64_t)blockIdx.x * A + a] : -1;
  }
  const int n_valid = stage_step(k, s, row, t, true);  // (its barrier covers g / arg too)
  const int lane = threadIdx.x % kLanes, base = (threadIdx.x & 63) - lane;
  const int chunk = (A + kLanes - 1) / kLanes;
  const int i0 = lane * chunk, i1 = min(A, i0 + chunk);
  for (int a0 = 0; a0 < A; a0 += kGroups) {
    const int a = a0 + threadIdx.x / kLanes;
    Grad3 acc = {0.f, 0.f, 0.f};
    if (a < A && s.valid[a]) {
      for (int i = i0; i < i1; ++i) {
        if (!s.valid[i]) continue;
        if (k.reduce_max) {
          if (i == a) {  // the own row reads the pair (a, arg[a])
            const int j = s.arg[a];
            if (j >= 0 && j < A && j != a && s.valid[j]) pair_grad(s, A, a, j, true, s.g[a], acc);
          } else if (s.arg[i] == a) {  // row i reads the pair (i, a)
            pair_grad(s, A, i, a, false, s.g[i], acc);
          }
        } else if (i != a) {  // the own row's pair (a, i), then row i's pair (i, a); n_valid >= 1: a is valid
          pair_grad(s, A, a, i, true, s.g[a] / (float)n_valid, acc);
          pair_grad(s, A, i, a, false, s.g[i] / (float)n_valid, acc);
        }
      }
    }
    Grad3 all = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < kLanes; ++q) {
      const float x = __shfl(acc.x, base + q, 64), y = __shfl(acc.y, base + q, 64), w = __shfl(acc.w, base + q, 64);
      if (q == 0) all.x = x, all.y = y, all.w = w;
      else all.x += x, all.y += y, all.w += w;
    }
    if (a < A && lane == 0) {
      float* o = d_pose + ((int64_t)blockIdx.x * A + a) * 3;
      o[0] = all.x, o[1] = all.y, o[2] = all.w;
    }
  }
}

int check(const float* pose, const uint8_t* valid, int64_t n_rows, int n_k, int n_ag, int n_t, const Log& lp, const Log& lv, const float* ag_size,
          const float* c, const Log& lc) {
  if (!pose || !valid || !ag_size || !c) return TBX_ERR_ARG;
  if (n_rows < 1 || n_k < 1 || n_ag < 1 || n_t < 1 || n_rows % n_k != 0) return TBX_ERR_ARG;
  const Log* logs[3] = {&lp, &lv, &lc};
  for (int q = 0; q < 3; ++q) {
    const int64_t least = q == 0 ? 3 : 1;
    if ((n_rows > 1 && logs[q]->s_row < least) || (n_ag > 1 && logs[q]->s_ag < least) || (n_t > 1 && logs[q]->s_t < least)) return TBX_ERR_ARG;
  }
  if (n_ag > kCap || n_rows * (int64_t)n_t >= (int64_t)1 << 31) return TBX_ERR_UNSUPPORTED;
  return TBX_OK;
}

size_t lds_bytes(int n_ag, bool bwd) { return ((size_t)(bwd ? kWordsBwd : kWordsFwd) * n_ag + kThreads / 64) * sizeof(float); }

}  // namespace

extern "C" int tbx_collision_reward_fwd(const float* pose, const uint8_t* valid, int64_t n_rows, int n_k, int n_ag, int n_t,
                                        int64_t pose_stride_row, int64_t pose_stride_ag, int64_t pose_stride_t, int64_t valid_stride_row,
                                        int64_t valid_stride_ag, int64_t valid_stride_t, const float* ag_size, int reduce_with_max, float* c,
                                        int64_t c_stride_row, int64_t c_stride_ag, int64_t c_stride_t, int32_t* arg, void* stream) {
  const Log lp = {pose_stride_row, pose_stride_ag, pose_stride_t}, lv = {valid_stride_row, valid_stride_ag, valid_stride_t};
  const Log lc = {c_stride_row, c_stride_ag, c_stride_t};
  const int rc = check(pose, valid, n_rows, n_k, n_ag, n_t, lp, lv, ag_size, c, lc);
  if (rc != TBX_OK) return rc;
  const Args k = {pose, valid, ag_size, lp, lv, lc, n_k, n_ag, n_t, reduce_with_max != 0};
  hipLaunchKernelGGL(collision_fwd_kernel, dim3((unsigned)(n_rows * n_t)), dim3(kThreads), lds_bytes(n_ag, false), (hipStream_t)stream, k, c, arg);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}

extern "C" int tbx_collision_reward_bwd(const float* pose, const uint8_t* valid, int64_t n_rows, int n_k, int n_ag, int n_t,
                                        int64_t pose_stride_row, int64_t pose_stride_ag, int64_t pose_stride_t, int64_t valid_stride_row,
                                        int64_t valid_stride_ag, int64_t valid_stride_t, const float* ag_size, int reduce_with_max,
                                        const float* g, int64_t g_stride_row, int64_t g_stride_ag, int64_t g_stride_t, const int32_t* arg,
                                        float* d_pose, void* stream) {
  const Log lp = {pose_stride_row, pose_stride_ag, pose_stride_t}, lv = {valid_stride_row, valid_stride_ag, valid_stride_t};
  const Log lg = {g_stride_row, g_stride_ag, g_stride_t};
  const int rc = check(pose, valid, n_rows, n_k, n_ag, n_t, lp, lv, ag_size, g, lg);
  if (rc != TBX_OK) return rc;
  if (!d_pose || (reduce_with_max && !arg)) return TBX_ERR_ARG;
  const Args k = {pose, valid, ag_size, lp, lv, lg, n_k, n_ag, n_t, reduce_with_max != 0};
  hipLaunchKernelGGL(collision_bwd_kernel, dim3((unsigned)(n_rows * n_t)), dim3(kThreads), lds_bytes(n_ag, true), (hipStream_t)stream, k, g, arg,
                     d_pose);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
