// Submission records of the test loop (include/tbx_hip_sub.h: tbx_wosac_joint_scenes, tbx_womd_predictions; libtbx_sub.so).
#include "../../include/tbx_hip_sub.h"
#include "pose_global_core.h"
#include "tbx_common.h"

namespace {

// Both kernels are a per-scene stream compaction followed by a row writer, in ONE launch and without atomics:
//   * a scene's output is cut into contiguous shares of vectors (float4 / float2), one workgroup per share; blockIdx.x = scene * shares + share.
//   * every workgroup first builds the compaction of ITS scene from the validity bytes (scene_compact: 256 objects per pass - a wave
//     ballot, the popcount of the lower lanes, the four wave totals exchanged through LDS - so that slot j knows its object a_j, in
//     index order) and the per-slot constants of the rows it will write. That is A + N strided bytes and a few values per kept object,
//     out of L2 for all but the first workgroup of a scene; a workgroup whose share holds no no-sim row skips that table.
//   * it then writes its share: thread i of the share owns vector i, i + 256, ... - a wave stores 1 KiB contiguous per instruction
//     whatever the row length (a row of T steps is T float4s; rows follow each other without a gap, so T % 64 needs no special case) -,
//     zeros from the scene's count on. The reads of a kept row are contiguous too (T float2s + T floats).
// The kernels are memory-bound: 16 B out for 12 B in per sim step.
constexpr int SUB_THREADS = 256, SUB_WAVES = SUB_THREADS / 64, SUB_MAX = TBX_SUB_MAX_OBJECTS;
constexpr int SUB_VEC_PER_BLOCK = 4 * SUB_THREADS;  // vectors of one share, at least (16 KiB of float4s)
constexpr int SUB_MAX_BLOCKS = 8192;

// Compaction of n <= SUB_MAX objects by the bytes valid[a * stride], a = 0 .. n-1: src[j] = the j-th object with a non-zero byte.
// All SUB_THREADS threads call it; -> the count (the same in every thread). `wtot` = SUB_WAVES ints of LDS. Ends with a barrier.
__device__ __forceinline__ int scene_compact(const uint8_t* __restrict__ valid, const int64_t stride, const int n, uint16_t* __restrict__ src,
                                             int* __restrict__ wtot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int base = 0; base < n; base += SUB_THREADS) {  // (n is uniform: every thread runs every pass and meets every barrier)
    const int a = base + tid;
    const bool v = a < n && valid[a * stride] != 0;
    const unsigned long long bal = __ballot(v);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int off = running, all = 0;
    for (int w = 0; w < SUB_WAVES; ++w) {
      const int c = wtot[w];
      off += w < wave ? c : 0;
      all += c;
    }
    if (v) src[off + below] = (uint16_t)a;  // off + below < count <= n <= SUB_MAX
    running += all;
    __syncthreads();  // wtot is rewritten by the next pass; src is read after the last one
  }
  return running;
}

// ---------------------------------------------------------------------------------------------- WOSAC joint scenes
struct JsArgs {
  tbx_joint_scenes_t a;
  int shares;           // workgroups per scene
  int64_t vec_sim, vec; // float4s of a scene's sim rows (K * A * T) and of all its rows (+ N * T)
  int64_t per_share;
};

__global__ __launch_bounds__(SUB_THREADS) void wosac_joint_scenes_kernel(const JsArgs p) {
  // per-slot tables, sized by the launch (js_lds_bytes: 10 B per sim, 30 B per no-sim object - 8 KiB at 64 + 256, 40 KiB at the maximum)
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ int wtot[SUB_WAVES];

  const tbx_joint_scenes_t& q = p.a;
  const int tid = threadIdx.x;
  const int s = blockIdx.x / p.shares, share = blockIdx.x % p.shares;
  const int A = q.n_ag, N = q.n_no_sim, T = q.n_step, Th = q.n_hist, c = q.step_current;
  float(*ns_at)[4] = reinterpret_cast<float(*)[4]>(lds);          // [N] (x, y, z, yaw) at step_current
  float(*ns_vel)[3] = reinterpret_cast<float(*)[3]>(ns_at + N);   // [N] (v_x, v_y, v_z)
  float* zc_sim = reinterpret_cast<float*>(ns_vel + N);           // [A]
  float* vz_sim = zc_sim + A;                                     // [A]
  uint16_t* src_sim = reinterpret_cast<uint16_t*>(vz_sim + A);    // [A]
  uint16_t* src_ns = src_sim + A;                                 // [N]
  const int64_t lo = share * p.per_share, hi = lo + p.per_share < p.vec ? lo + p.per_share : p.vec;
  const bool first = share == 0, need_sim = first || lo < p.vec_sim, need_ns = first || hi > p.vec_sim;  // (uniform in the workgroup)

  int n_sim = 0, n_ns = 0;
  if (need_sim) {
    const uint8_t* valid = q.valid_sim + (int64_t)s * A * Th;
    n_sim = scene_compact(valid + c, Th, A, src_sim, wtot);
    for (int j = tid; j < n_sim; j += SUB_THREADS) {
      const int64_t r = ((int64_t)s * A + src_sim[j]) * Th + c;
      const float z = q.z_sim[r];
      zc_sim[j] = z;
      vz_sim[j] = (q.const_vel_z_sim && q.valid_sim[r - 1]) ? z - q.z_sim[r - 1] : 0.f;
    }
  }
  if (need_ns) {
    const uint8_t* valid = q.valid_no_sim + (int64_t)s * N * Th;
    n_ns = scene_compact(valid + c, Th, N, src_ns, wtot);
    for (int j = tid; j < n_ns; j += SUB_THREADS) {
      const int64_t r = ((int64_t)s * N + src_ns[j]) * Th + c;
      const float x = q.pos_no_sim[r * 2], y = q.pos_no_sim[r * 2 + 1], z = q.z_no_sim[r];
      const bool vel = q.const_vel_no_sim && q.valid_no_sim[r - 1];
      ns_at[j][0] = x, ns_at[j][1] = y, ns_at[j][2] = z, ns_at[j][3] = q.yaw_no_sim[r];
      ns_vel[j][0] = vel ? x - q.pos_no_sim[(r - 1) * 2] : 0.f;
      ns_vel[j][1] = vel ? y - q.pos_no_sim[(r - 1) * 2 + 1] : 0.f;
      ns_vel[j][2] = vel ? z - q.z_no_sim[r - 1] : 0.f;
    }
  }
  __syncthreads();

  if (first) {  // ids and counts: the scene's first workgroup (it built both compactions)
    for (int j = tid; j < A; j += SUB_THREADS) q.id_sim[(int64_t)s * A + j] = j < n_sim ? q.object_id_sim[(int64_t)s * A + src_sim[j]] : -1;
    for (int j = tid; j < N; j += SUB_THREADS)
      q.id_no_sim[(int64_t)s * N + j] = j < n_ns ? q.object_id_no_sim[(int64_t)s * N + src_ns[j]] : -1;
    if (tid == 0) q.count[s * 2] = n_sim, q.count[s * 2 + 1] = n_ns;
  }

  float4* out_sim = reinterpret_cast<float4*>(q.traj_sim) + (int64_t)s * p.vec_sim;
  float4* out_ns = reinterpret_cast<float4*>(q.traj_no_sim) + (int64_t)s * (p.vec - p.vec_sim);
  const float2* pos_sim = reinterpret_cast<const float2*>(q.pos_sim);
  const int64_t AT = (int64_t)A * T;
  for (int64_t e = lo + tid; e < hi; e += SUB_THREADS) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < p.vec_sim) {  // e = (k * A + j) * T + t
      const int64_t k = e / AT;
      const int r = (int)(e - k * AT), j = r / T, t = r - j * T;
      if (j < n_sim) {
        const int64_t i = (((int64_t)s * q.n_k + k) * A + src_sim[j]) * T + t;
        const float2 xy = pos_sim[i];
        o = make_float4(xy.x, xy.y, fmaf(vz_sim[j], (float)(t + 1), zc_sim[j]), q.yaw_sim[i]);
      }
      out_sim[e] = o;
    } else {  // e - vec_sim = j * T + t
      const int r = (int)(e - p.vec_sim), j = r / T, t = r - j * T;
      if (j < n_ns) {
        const float ft = (float)(t + 1);
        o = make_float4(fmaf(ns_vel[j][0], ft, ns_at[j][0]), fmaf(ns_vel[j][1], ft, ns_at[j][1]), fmaf(ns_vel[j][2], ft, ns_at[j][2]), ns_at[j][3]);
      }
      out_ns[r] = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------- WOMD prediction records
struct WpArgs {
  tbx_womd_pred_t a;
  int shares;
  int64_t vec, per_share;  // float2s of a scene's out_pos (A * k * n)
};

__global__ __launch_bounds__(SUB_THREADS) void womd_predictions_kernel(const WpArgs p) {
  __shared__ uint16_t src[SUB_MAX];
  __shared__ int wtot[SUB_WAVES];

  const tbx_womd_pred_t& q = p.a;
  const int tid = threadIdx.x;
  const int s = blockIdx.x / p.shares, share = blockIdx.x % p.shares;
  const int A = q.n_ag, km = q.n_mode, per_ag = q.n_mode * q.n_sample;
  const int64_t lo = share * p.per_share, hi = lo + p.per_share < p.vec ? lo + p.per_share : p.vec;
  const int n_pred = scene_compact(q.mask_pred + (int64_t)s * A, 1, A, src, wtot);

  if (share == 0) {
    for (int j = tid; j < A; j += SUB_THREADS) q.out_object_id[(int64_t)s * A + j] = j < n_pred ? q.object_id[(int64_t)s * A + src[j]] : -1;
    for (int i = tid; i < A * km; i += SUB_THREADS) {
      const int j = i / km, m = i - j * km;
      q.out_scores[(int64_t)s * A * km + i] = j < n_pred ? q.scores[((int64_t)s * A + src[j]) * km + m] : 0.f;
    }
    if (tid == 0) q.out_count[s] = n_pred;
  }

  const float th = q.scenario_yaw[s], cx = q.scenario_center[s * 2], cy = q.scenario_center[s * 2 + 1];
  float sn, cs;
  sincosf(th, &sn, &cs);
  float2* out = reinterpret_cast<float2*>(q.out_pos) + (int64_t)s * p.vec;
  for (int64_t e = lo + tid; e < hi; e += SUB_THREADS) {  // e = j * (k * n) + point
    const int j = (int)(e / per_ag), r = (int)(e - (int64_t)j * per_ag);
    float2 o = make_float2(0.f, 0.f);
    if (j < n_pred) {
      const float* pt = q.trajs + (((int64_t)s * A + src[j]) * per_ag + r) * 3;
      tbx::pos_to_global(pt[0], pt[1], sn, cs, cx, cy, &o.x, &o.y);
    }
    out[e] = o;
  }
}

inline size_t js_lds_bytes(const int n_ag, const int n_no_sim) { return (size_t)n_no_sim * 30 + (size_t)n_ag * 10; }

// shares per scene for `vec` vectors per scene: SUB_VEC_PER_BLOCK each, at least one, the grid capped at SUB_MAX_BLOCKS
inline int scene_shares(const int64_t vec, const int n_sc, int64_t* per_share) {
  int64_t shares = (vec + SUB_VEC_PER_BLOCK - 1) / SUB_VEC_PER_BLOCK;
  const int64_t cap = SUB_MAX_BLOCKS / n_sc > 1 ? SUB_MAX_BLOCKS / n_sc : 1;
  shares = shares < 1 ? 1 : (shares > cap ? cap : shares);
  *per_share = (vec + shares - 1) / shares;
  return (int)shares;
}

}  // namespace

extern "C" int tbx_wosac_joint_scenes(const tbx_joint_scenes_t* a, void* stream) {
  if (!a) return TBX_ERR_ARG;
  if (a->n_sc < 1 || a->n_k < 1 || a->n_step < 1 || a->n_ag < 0 || a->n_no_sim < 0 || a->n_hist < 1) return TBX_ERR_ARG;
  if (a->step_current < 1 || a->step_current >= a->n_hist) return TBX_ERR_ARG;
  if (a->n_ag > TBX_SUB_MAX_OBJECTS || a->n_no_sim > TBX_SUB_MAX_OBJECTS) return TBX_ERR_UNSUPPORTED;
  if (!a->count) return TBX_ERR_ARG;
  if (a->n_ag > 0 && (!a->pos_sim || !a->yaw_sim || !a->valid_sim || !a->z_sim || !a->object_id_sim || !a->traj_sim || !a->id_sim))
    return TBX_ERR_ARG;
  if (a->n_no_sim > 0 &&
      (!a->pos_no_sim || !a->yaw_no_sim || !a->z_no_sim || !a->valid_no_sim || !a->object_id_no_sim || !a->traj_no_sim || !a->id_no_sim))
    return TBX_ERR_ARG;
  if (((uintptr_t)a->traj_sim & 15) || ((uintptr_t)a->traj_no_sim & 15) || ((uintptr_t)a->pos_sim & 7)) return TBX_ERR_ALIGN;
  if ((int64_t)a->n_sc > SUB_MAX_BLOCKS) return TBX_ERR_UNSUPPORTED;
  JsArgs p;
  p.a = *a;
  p.vec_sim = (int64_t)a->n_k * a->n_ag * a->n_step;
  p.vec = p.vec_sim + (int64_t)a->n_no_sim * a->n_step;
  if ((int64_t)a->n_ag * a->n_step > 0x7fffffff || (int64_t)a->n_no_sim * a->n_step > 0x7fffffff) return TBX_ERR_UNSUPPORTED;
  p.shares = scene_shares(p.vec, a->n_sc, &p.per_share);
  hipLaunchKernelGGL(wosac_joint_scenes_kernel, dim3((unsigned)(a->n_sc * p.shares)), dim3(SUB_THREADS), js_lds_bytes(a->n_ag, a->n_no_sim),
                     (hipStream_t)stream, p);  // (<= 40 KiB of dynamic LDS: inside the 64 KiB a kernel gets without an attribute)
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}

extern "C" int tbx_womd_predictions(const tbx_womd_pred_t* a, void* stream) {
  if (!a) return TBX_ERR_ARG;
  if (!a->trajs || !a->scores || !a->object_id || !a->mask_pred || !a->scenario_center || !a->scenario_yaw || !a->out_pos || !a->out_scores ||
      !a->out_object_id || !a->out_count)
    return TBX_ERR_ARG;
  if (a->n_sc < 1 || a->n_ag < 1 || a->n_mode < 1 || a->n_sample < 1) return TBX_ERR_ARG;
  if (a->n_ag > TBX_SUB_MAX_OBJECTS || (int64_t)a->n_sc > SUB_MAX_BLOCKS) return TBX_ERR_UNSUPPORTED;
  if ((int64_t)a->n_ag * a->n_mode * a->n_sample > 0x7fffffff) return TBX_ERR_UNSUPPORTED;
  if ((uintptr_t)a->out_pos & 7) return TBX_ERR_ALIGN;
  WpArgs p;
  p.a = *a;
  p.vec = (int64_t)a->n_ag * a->n_mode * a->n_sample;
  p.shares = scene_shares(p.vec, a->n_sc, &p.per_share);
  hipLaunchKernelGGL(womd_predictions_kernel, dim3((unsigned)(a->n_sc * p.shares)), dim3(SUB_THREADS), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
