// tbx_front: everything between tbx_agent_prep / tbx_tl_prep and a block's first decoder layer as ONE launch, for the closed loop at a
// few scenes (launches of <= 1024 windows). It replaced three dependent launches on the critical path of every step - the window
// PointNet (tbx_window_tile: 8 us), the K-nearest searches (tbx_knn_embed_multi: 13 us) and the block's first projection
// (tbx_layer_tile + rider: 7 us) - whose work is independent or per-window:
//   window workgroups (2 windows each, csrc/window_core.h): the temporal PointNet, then - the two pooled rows never leave the CU -
//     LayerNorm + q | k | v = in_proj(norm x) + qt = W_rpe_k^T q of the first layer (transformer_rpe.py:207-211, attention_rpe.py:92-98,147)
//     on single-row B operands (tile_core.h row1), weights as per-wave register units;
//   rider workgroups (16 rows each): tbx_layer_tile_t's rider (the heads' navigation embedding);
//   search workgroups (one source row each, 256 of the 512 threads, csrc/knn_core.h): the K-nearest searches + pose-embedding job.
// The launch takes as long as its longest part (the searches) instead of the sum.
#include <string.h>

#ifdef TBX_STAGE_CLOCK
// profiling build (`make clk`, tools/front_clock.py): thread 0 of four workgroups of the paired launch - the lights' first window
// workgroup, the agents' first window workgroup, one search workgroup (a job with n_tgt = 1024 if there is one) and the first rider
// workgroup - stamps the shader clock at the stage boundaries. Stamps: 0 entry, 1 inputs in LDS, 2-4 input MLP, 5-7 PointNet,
// 8 LayerNorm, 9 q, 10 k | v, 11 W_k^T q (end); 16 search entry, 17 candidates loaded, 18 bisection done, 19 outputs written;
// 20 rider entry, 21 inputs in LDS, 22-24 its first three stages, 25 end.
#include <hip/hip_runtime.h>
__device__ unsigned long long g_front_clk[4 * 32];
__device__ int g_front_clk_blk[4];
__shared__ int g_front_clk_slot;
#define TBX_FRONT_CLK(i)                                                                 \
  do {                                                                                   \
    if (threadIdx.x == 0 && g_front_clk_slot >= 0) g_front_clk[g_front_clk_slot * 32 + (i)] = clock64(); \
  } while (0)
#define TBX_FRONT_CLK_LOADS() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")  // (the stamp behind it means "candidates loaded")
#endif

#include "knn_core.h"
#include "tile_core.h"
#include "window_core.h"

using namespace tbx_tile;

namespace {

typedef Planes<16, 4> RPL;  // the rider's planes (K = 128)
constexpr int XLD = 132;
constexpr size_t WIN_BYTES = tbx_window::LDS_BYTES;                   // the window body's ping / pong planes
constexpr size_t POOL_OFF = WIN_BYTES;                                // float pooled[2][128]
constexpr size_t ROWP_OFF = POOL_OFF + 2 * D * sizeof(float);         // row planes: Ph[2], Pq[2] of 512 B
constexpr size_t WIN_TOTAL = ROWP_OFF + 4 * 512;
constexpr size_t RIDER_TOTAL = 16 * XLD * sizeof(float) + 4 * RPL::PLANE;
constexpr size_t LDS_BYTES = WIN_TOTAL > RIDER_TOTAL ? WIN_TOTAL : RIDER_TOTAL;

// ---- kernel arguments. What the dispatch needs leads the block (FrontHead: 64 bytes, one scalar load); behind it every body has a
// compact group of its own - pointers and sizes contiguous - that it reads at constant offsets: the half, the block kind and the search
// job are resolved ONCE from the head, and the kernel then branches into one inlined body (window + projection in the "cat" or the
// "add" form, rider, one search job at the candidates-per-lane form its n_tgt needs, pose embedding).
struct WinArgs {  // tbx_window_tile_t's members that window_body<., ., false> reads
  const float *attr, *pe;
  const uint8_t* row_invalid;
  float* out;
  const float* in_images[3];
  const float* pn_images[3];
  int64_t n_groups;
  int32_t window, ld_attr, attr_cols, pad_;
};
struct ProjArgs {  // the first projection's members of tbx_layer_tile_t
  const float *proj_norm_weight, *proj_norm_bias, *proj_image, *qfold_image;
  float* proj_out;
  void* kv16_out;
  int64_t n_rows;
  int32_t ld_proj;
  float proj_norm_eps;
};
struct RiderArgs {  // tbx_layer_tile_t's rider_* members
  const float *rider_in, *rider_add, *rider_pose3, *rider_freqs_xy, *rider_freqs_yaw;
  const uint8_t* rider_valid;
  float* rider_out;
  const float* rider_images[4];
  int64_t rider_rows;
};
struct HalfArgs {
  WinArgs win;
  ProjArgs proj;
  RiderArgs rider;
  tbx_knn::KnnArgs job[tbx_knn::KNN_MAX_JOBS];
  tbx_knn::PoseEmbedArgs pe;  // pe.n == 0: none
};
// half 0 = the grid's first n0 workgroups, half 1 = the rest (a single launch has half 0 only). Per half: window, rider workgroups and
// the first search / embedding workgroup of job 1, 2, 3 and of the pose embedding (job 0's is 0; a job that is not there starts where
// the pose embedding does, tbx_knn::knn_multi_fill)
struct FrontHead {
  int32_t n0;
  int32_t n_win[2], n_rider[2];
  int32_t fb[2][tbx_knn::KNN_MAX_JOBS];
  int32_t pad_[3];
};
static_assert(sizeof(FrontHead) == 64, "the head is one 64-byte scalar load");

// the first projection of the workgroup's two pooled rows (global rows 2 * block, 2 * block + 1); lg, lb = row1::ln_params' values,
// requested by the caller at entry
__device__ __forceinline__ void proj_rows(const ProjArgs& t, const int block, const float* pooled, char* rowp, const float (&lg)[2],
                                          const float (&lb)[2]) {
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g4 = lane >> 4;
  const bool col0 = (lane & 15) == 0;
  const int c_out = 16 * wave + 4 * g4;
  constexpr int LO = 256;
  char* Ph = rowp;          // [2][512]: LayerNorm(x) planes
  char* Pq = rowp + 1024;   // [2][512]: q planes
  W wb[2];
  load_unit(wb[0], t.proj_image, wave, lane);
  load_unit(wb[1], t.proj_image, 8 + wave, lane);
  if (wave < 2) row1::ln_planes(pooled + wave * D, Ph + wave * 512, lane, t.proj_norm_eps, lg, lb);
  __syncthreads();
  TBX_FRONT_CLK(8);
  const int64_t row0 = (int64_t)block * 2;
  const int nv = (t.n_rows - row0) < 2 ? (int)(t.n_rows - row0) : 2;
  const bool kv16 = t.kv16_out != nullptr;
#pragma unroll
  for (int r = 0; r < 2; ++r) {  // q
    const f32x4 q = row1::gemv4(wb[0], Ph + r * 512, LO, 0, g4) + wb[0].bias;
    if (col0) {
      row1::put4(Pq + r * 512, LO, c_out, q);
      if (r < nv) gst4(t.proj_out + (row0 + r) * (int64_t)t.ld_proj + c_out, q);
    }
  }
  TBX_FRONT_CLK(9);
  load_unit(wb[0], t.proj_image, 16 + wave, lane);
#pragma unroll
  for (int kv = 0; kv < 2; ++kv) {  // k (wb[1]), v (wb[0])
    const W& w = wb[1 - kv];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const f32x4 y = row1::gemv4(w, Ph + r * 512, LO, 0, g4) + w.bias;
      if (col0 && r < nv) {
        gst4(t.proj_out + (row0 + r) * (int64_t)t.ld_proj + (1 + kv) * D + c_out, y);
        if (kv16) {
          const bf16x4 h16 = __builtin_convertvector(y, bf16x4);
          *(TBX_GLOBAL u32x2*)((uint16_t*)t.kv16_out + (row0 + r) * (2 * D) + kv * D + c_out) = __builtin_bit_cast(u32x2, h16);
        }
      }
    }
    if (kv == 0) load_unit(wb[1], t.qfold_image, wave, lane);
  }
  __syncthreads();  // q's planes complete
  TBX_FRONT_CLK(10);
  {  // qt_h = W_rpe_k,h^T q_h: wave w = head w / 2, 4 of its 8 tiles of 16 channels, K = 32 (the head's own step)
    const W& w = wb[1];
    const int h = wave >> 1;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        Acc acc;
        acc.zero();
        row1::step(acc, w.hi[st], w.lo[st], Pq + r * 512, LO, h, g4);
        if (col0 && r < nv) gst4(t.proj_out + (row0 + r) * (int64_t)t.ld_proj + 3 * D + h * D + ((wave & 1) * 4 + st) * 16 + 4 * g4, acc.sum());
      }
  }
  TBX_FRONT_CLK(11);
}

// workgroup b of a half: n_win window workgroups, n_rider rider workgroups, then the searches (job j's from f[j], f0 = 0) and the pose
// embedding (from f4). BIG: a job of the launch has n_tgt > 1024 (the 32-candidates-per-lane search body is compiled in).
template <int DM, bool ADD, bool BIG>
__device__ __forceinline__ void front_half(const HalfArgs& a, int b, const int n_win, const int n_rider, const int f1, const int f2, const int f3,
                                           const int f4, char* lds_c) {
  if (b < n_win) {
    float lg[2], lb[2];
    row1::ln_params(a.proj.proj_norm_weight, a.proj.proj_norm_bias, (int)threadIdx.x & 63, lg, lb);
    float* pooled = (float*)(lds_c + POOL_OFF);
    tbx_window::window_body<DM, ADD, false>(a.win, b, lds_c, pooled);
    __syncthreads();
    TBX_FRONT_CLK(7);
    proj_rows(a.proj, b, pooled, lds_c + ROWP_OFF, lg, lb);
    return;
  }
  b -= n_win;
  if (b < n_rider) {
    float* X = (float*)lds_c;
    char* Pa = (char*)(X + 16 * XLD);
    rider_tile<RPL, XLD>(a.rider, b, X, Pa, Pa + 2 * RPL::PLANE);
    return;
  }
  b -= n_rider;
  if (threadIdx.x >= 256) return;
  if (b >= f4) tbx_knn::pose_embed_block(a.pe, b - f4);
  else if (b < f1) tbx_knn::knn_job_block<BIG, false>(a.job[0], b);
  else if (b < f2) tbx_knn::knn_job_block<BIG, false>(a.job[1], b - f1);
  else if (b < f3) tbx_knn::knn_job_block<BIG, false>(a.job[2], b - f2);
  else tbx_knn::knn_job_block<BIG, false>(a.job[3], b - f3);
}

struct FrontArgs {
  FrontHead h;
  HalfArgs a;
};
template <int DM, bool ADD, bool BIG>
__global__ __launch_bounds__(NT) void front_kernel(const FrontArgs p) {
  extern __shared__ __attribute__((aligned(16))) char lds_c[];
#ifdef TBX_STAGE_CLOCK
  if (threadIdx.x == 0) g_front_clk_slot = -1;  // (only the paired launch is stamped)
#endif
  const FrontHead h = p.h;
  front_half<DM, ADD, BIG>(p.a, (int)blockIdx.x, h.n_win[0], h.n_rider[0], h.fb[0][0], h.fb[0][1], h.fb[0][2], h.fb[0][3], lds_c);
}

// The agents' front ("cat" input encoder, d_mlp 64) and the lights' ("add", d_mlp 128) of one closed-loop step as ONE launch (round 6,
// with tbx_knarpe_dec_layer_pair: the step on one queue): blocks [0, n0) run the lights' half, the rest the agents' - the two read nothing of
// each other's (the lights run one step ahead).
// Block order: the lights' blocks (all window blocks, the launch's longest) first, then the agents' (windows, rider, and last their
// K-nearest searches - the short ones): at configs[1] the grid is 64 + 228 = 292 workgroups on 256 CUs with one workgroup per CU (LDS),
// so the last 36 to start must be short ones (agents first, the lights' last 36 window blocks waited for a CU: the launch 13 -> 20 us).
struct FrontPair {
  FrontHead h;
  HalfArgs m[2];  // [0] the lights' (the grid's first half), [1] the agents'
};
template <bool BIG>
__global__ __launch_bounds__(NT) void front_pair_kernel(const FrontPair p) {
  extern __shared__ __attribute__((aligned(16))) char lds_c[];
#ifdef TBX_STAGE_CLOCK
  if (threadIdx.x == 0) {
    int slot = -1;
    for (int q = 0; q < 4; ++q)
      if (g_front_clk_blk[q] == (int)blockIdx.x) slot = q;
    g_front_clk_slot = slot;  // (read by thread 0 only)
  }
#endif
  const FrontHead h = p.h;
  const int b = (int)blockIdx.x;
  if (b < h.n0) front_half<128, true, BIG>(p.m[0], b, h.n_win[0], h.n_rider[0], h.fb[0][0], h.fb[0][1], h.fb[0][2], h.fb[0][3], lds_c);
  else front_half<64, false, BIG>(p.m[1], b - h.n0, h.n_win[1], h.n_rider[1], h.fb[1][0], h.fb[1][1], h.fb[1][2], h.fb[1][3], lds_c);
}

// tbx_front's checks + half `half` of the launch descriptor; blocks = its workgroups, big |= a job with n_tgt > 1024
static int front_fill(const tbx_front_t* args, FrontHead& h, const int half, HalfArgs& a, int& blocks, bool& big) {
  if (args == nullptr) return TBX_ERR_ARG;
  const tbx_window_tile_t& w = args->win;
  const tbx_layer_tile_t& t = args->layer;
  // the window part: tbx_window_tile's checks
  if (w.n_groups <= 0 || w.attr == nullptr || w.pe == nullptr || w.row_invalid == nullptr || w.out == nullptr) return TBX_ERR_ARG;
  for (int i = 0; i < 3; ++i)
    if (w.in_images[i] == nullptr || w.pn_images[i] == nullptr) return TBX_ERR_ARG;
  if (w.window <= 0 || w.window > 16 || w.ld_attr % 4 != 0 || w.attr_cols <= 0 || w.attr_cols > 32 || w.attr_cols % 4 != 0 || w.attr_cols > w.ld_attr)
    return TBX_ERR_UNSUPPORTED;
  if (!((w.d_mlp == 64 && w.add_mode == 0) || (w.d_mlp == 128 && w.add_mode == 1))) return TBX_ERR_UNSUPPORTED;
  if (w.drop_thresh != 0u) return TBX_ERR_UNSUPPORTED;  // inference only
  if ((((uintptr_t)w.attr) | ((uintptr_t)w.pe) | ((uintptr_t)w.out)) & 15) return TBX_ERR_ALIGN;
  // the projection part: a first-projection tbx_layer_tile_t on the windows' pooled rows
  if (t.x != w.out || t.n_rows != w.n_groups || t.attn_out != nullptr || t.linear1_image != nullptr || t.proj_n != 3 * D) return TBX_ERR_ARG;
  if (t.proj_image == nullptr || t.qfold_image == nullptr || t.proj_norm_weight == nullptr || t.proj_norm_bias == nullptr || t.proj_out == nullptr ||
      t.ld_proj < 7 * D || t.ld_proj % 4 != 0 || t.drop_thresh != 0u)
    return TBX_ERR_ARG;
  if (((uintptr_t)t.proj_out) & 15) return TBX_ERR_ALIGN;
  if (t.rider_rows < 0) return TBX_ERR_ARG;
  if (t.rider_rows > 0) {
    if ((t.rider_in == nullptr && t.rider_pose3 == nullptr) || t.rider_add == nullptr || t.rider_valid == nullptr || t.rider_out == nullptr)
      return TBX_ERR_ARG;
    if (t.rider_pose3 != nullptr && (t.rider_freqs_xy == nullptr || t.rider_freqs_yaw == nullptr)) return TBX_ERR_ARG;
    for (int i = 0; i < 4; ++i)
      if (t.rider_images[i] == nullptr) return TBX_ERR_ARG;
    if ((((uintptr_t)t.rider_in) | ((uintptr_t)t.rider_add) | ((uintptr_t)t.rider_out)) & 15) return TBX_ERR_ALIGN;
  }
  a.win = WinArgs{w.attr, w.pe, w.row_invalid, w.out, {w.in_images[0], w.in_images[1], w.in_images[2]}, {w.pn_images[0], w.pn_images[1], w.pn_images[2]},
                  w.n_groups, w.window, w.ld_attr, w.attr_cols, 0};
  a.proj = ProjArgs{t.proj_norm_weight, t.proj_norm_bias, t.proj_image, t.qfold_image, t.proj_out, t.kv16_out, t.n_rows, t.ld_proj, t.proj_norm_eps};
  a.rider = RiderArgs{t.rider_in, t.rider_add, t.rider_pose3, t.rider_freqs_xy, t.rider_freqs_yaw, t.rider_valid, t.rider_out,
                      {t.rider_images[0], t.rider_images[1], t.rider_images[2], t.rider_images[3]}, t.rider_rows};
  h.n_win[half] = (int)((w.n_groups + tbx_window::RT - 1) / tbx_window::RT);
  h.n_rider[half] = (int)((t.rider_rows + 15) / 16);
  int n_knn_blocks = 0;
  tbx_knn::KnnMulti m;
  memset(&m, 0, sizeof(m));
  if (args->n_jobs > 0) {
    const int rc = tbx_knn::knn_multi_fill(args->jobs, args->n_jobs, args->freqs_xy, args->freqs_yaw, args->pe_dim, args->pe, m, n_knn_blocks);
    if (rc != TBX_OK) return rc;
    for (int j = 0; j < args->n_jobs; ++j) {
      if (args->jobs[j].emb != nullptr) return TBX_ERR_UNSUPPORTED;  // (the relative-pose form only: no embedding phase behind a barrier)
      // (INVARIANT: the <BIG = false> kernels run the 16-candidate body for every n_tgt > 128 - tbx_knn::knn_job_block - so `big` must be
      // OR-ed over EVERY job of EVERY half before the kernel is picked; tbx_front_pair passes the same flag through both fills)
      big = big || args->jobs[j].n_tgt > 1024;
    }
  } else if (args->pe != nullptr) {
    return TBX_ERR_ARG;
  }
  for (int j = 0; j < tbx_knn::KNN_MAX_JOBS; ++j) a.job[j] = m.job[j], h.fb[half][j] = m.first_block[j + 1];
  a.pe = m.pe;
  blocks = h.n_win[half] + h.n_rider[half] + n_knn_blocks;
  return TBX_OK;
}

static bool front_lds_attr() {
  static tbx::PerDeviceOnce lds_attr;  // (per device, thread-safe: tbx_common.h)
  return lds_attr([&] {
    const void* ks[] = {(const void*)front_kernel<64, false, false>, (const void*)front_kernel<64, false, true>, (const void*)front_kernel<128, true, false>,
                        (const void*)front_kernel<128, true, true>, (const void*)front_pair_kernel<false>, (const void*)front_pair_kernel<true>};
    for (const void* k : ks)
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES) != hipSuccess) return false;
    return true;
  });
}

}  // namespace

// (the kernel without the 32-candidate search body where no job needs it, as dec_mid.hip's entry points pick the tail kind)
#define TBX_FRONT_LAUNCH(K, GRID, ARGS)                                                                             \
  do {                                                                                                              \
    if (big) hipLaunchKernelGGL((K<true>), GRID, dim3(NT), LDS_BYTES, (hipStream_t)stream, ARGS);                   \
    else hipLaunchKernelGGL((K<false>), GRID, dim3(NT), LDS_BYTES, (hipStream_t)stream, ARGS);                      \
  } while (0)
template <bool BIG>
static constexpr auto front_cat_kernel = front_kernel<64, false, BIG>;
template <bool BIG>
static constexpr auto front_add_kernel = front_kernel<128, true, BIG>;

extern "C" int tbx_front(const tbx_front_t* args, void* stream) {
  FrontArgs p;
  memset(&p.h, 0, sizeof(p.h));
  int blocks = 0;
  bool big = false;
  const int rc = front_fill(args, p.h, 0, p.a, blocks, big);
  if (rc != TBX_OK) return rc;
  if (!front_lds_attr()) return TBX_ERR_LAUNCH;
  p.h.n0 = blocks;
  const dim3 grid((unsigned)blocks);
  if (args->win.d_mlp == 64) TBX_FRONT_LAUNCH(front_cat_kernel, grid, p);
  else TBX_FRONT_LAUNCH(front_add_kernel, grid, p);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}

extern "C" int tbx_front_pair(const tbx_front_t* agents, const tbx_front_t* lights, void* stream) {
  FrontPair p;
  memset(&p.h, 0, sizeof(p.h));
  int na = 0, nb = 0;
  bool big = false;
  int rc = front_fill(agents, p.h, 1, p.m[1], na, big);
  if (rc != TBX_OK) return rc;
  rc = front_fill(lights, p.h, 0, p.m[0], nb, big);
  if (rc != TBX_OK) return rc;
  if (agents->win.d_mlp != 64 || lights->win.d_mlp != 128) return TBX_ERR_UNSUPPORTED;  // ("cat" agents first, "add" lights second)
  if (!front_lds_attr()) return TBX_ERR_LAUNCH;
  p.h.n0 = nb;
#ifdef TBX_STAGE_CLOCK
  {
    int sj = 0;
    for (int j = 0; j < agents->n_jobs; ++j)
      if (p.m[1].job[j].n_tgt == 1024) sj = j;
    const int base = nb + p.h.n_win[1] + p.h.n_rider[1];
    const int blk[4] = {0, nb, agents->n_jobs > 0 ? base + (sj > 0 ? p.h.fb[1][sj - 1] : 0) : -1, p.h.n_rider[1] > 0 ? nb + p.h.n_win[1] : -1};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_front_clk_blk), blk, sizeof(blk)) != hipSuccess) return TBX_ERR_LAUNCH;
  }
#endif
  TBX_FRONT_LAUNCH(front_pair_kernel, dim3((unsigned)(na + nb)), p);
  return hipGetLastError() == hipSuccess ? TBX_OK : TBX_ERR_LAUNCH;
}
#undef TBX_FRONT_LAUNCH

#ifdef TBX_STAGE_CLOCK
extern "C" int tbx_debug_front_dump(unsigned long long* host_out) {  // the last paired launch's stamps [4][32]; zeroes them
  static const unsigned long long z[4 * 32] = {};
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_front_clk), sizeof(z)) != hipSuccess) return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_front_clk), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
