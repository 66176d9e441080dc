// Per-parameter gradient norms, their total and clip_grad_norm_'s scale on the flat gradient buffer (include/tbx_hip_grad.h: tbx_grad_norms).
#include "../../include/tbx_hip_grad.h"
#include "tbx_common.h"

namespace {

// A segmented reduction over a static layout, in three launches (the header has the contract):
//   * grad_partial_kernel, a workgroup per chunk (<= TBX_GRAD_CHUNK elements of ONE segment): a thread walks the chunk's float4s
//     t, t + 256, ... and keeps one float64 accumulator per float4 component; (a0 + a1) + (a2 + a3), then the wave butterfly, then the
//     waves in wave order. Which element meets which accumulator depends on the chunk's address and length alone.
//   * grad_final_kernel, one workgroup: a thread per segment finds the segment's first chunk (chunk_seg is ascending: a binary search)
//     and adds its partials in chunk order.
//   * grad_scale_kernel, a workgroup per chunk: the same walk, x * coef.
// The 16-byte path starts at the first 16-byte-aligned ADDRESS of a chunk: a packed layout (FlatGrads(align=1)) puts most chunk starts
// off that grid; up to three elements before and after go through single loads. Every write is an ordinary vector store. No atomics.
constexpr int GN_WAVES = 4, GN_THREADS = 64 * GN_WAVES;

struct GnArgs {
  float* g;
  const int64_t* seg_off;
  const int64_t* seg_len;
  const int32_t* chunk_seg;
  const int64_t* chunk_off;
  const int32_t* chunk_len;
  double* partial;
  int32_t* partial_nf;
  float* norms;
  float* total;
  int32_t* nonfinite;
  float* coef;
  int64_t n;
  int n_seg, n_chunk;
  double max_norm;
};

// chunk c as (first element, head, float4s, tail): head / tail = the single elements before / after the 16-byte-aligned middle. The
// entry is cut to its segment and to [0, n): a table that disagrees with the layout reads and writes nothing outside the segments.
struct Span {
  float* x;
  int head, nvec, tail;
};

__device__ __forceinline__ Span chunk_span(const GnArgs& p, const int c) {
  Span sp{p.g, 0, 0, 0};
  const int s = p.chunk_seg[c];
  if (s < 0 || s >= p.n_seg) return sp;
  int64_t lo = p.seg_off[s], hi = lo + p.seg_len[s];
  lo = lo < 0 ? 0 : lo;
  hi = hi > p.n ? p.n : hi;
  const int64_t off = p.chunk_off[c];
  int64_t len = p.chunk_len[c];
  len = len > TBX_GRAD_CHUNK ? TBX_GRAD_CHUNK : len;
  const int64_t b = off < lo ? lo : off;
  int64_t e = off + len;
  e = e > hi ? hi : e;
  if (len <= 0 || e <= b) return sp;
  const int n = (int)(e - b);
  sp.x = p.g + b;
  const int to_grid = (int)(((16 - ((uintptr_t)sp.x & 15)) & 15) >> 2);  // (g is 4-byte aligned: checked by the host)
  sp.head = to_grid < n ? to_grid : n;
  sp.nvec = (n - sp.head) >> 2;
  sp.tail = n - sp.head - 4 * sp.nvec;
  return sp;
}

// max with a NaN winning, as torch's norm(inf)
__device__ __forceinline__ double nan_max(const double a, const double b) { return (a != a || a >= b) ? a : b; }

template <bool INF>
__device__ __forceinline__ double join(const double a, const double b) {
  return INF ? nan_max(a, b) : a + b;
}

template <bool INF>
__device__ __forceinline__ void take(double& acc, int& nf, const float x) {
  nf += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;  // exponent all ones: NaN or +-Inf
  const double d = (double)x;
  acc = INF ? nan_max(acc, fabs(d)) : fma(d, d, acc);  // (d * d is exact in float64: the fused form rounds once, as the plain one)
}

// lanes -> wave butterfly -> LDS -> thread 0 joins the waves in wave order. Returns the workgroup's value in thread 0.
template <bool INF>
__device__ __forceinline__ void block_join(double& v, int& nf) {
  __shared__ double part[GN_WAVES];
  __shared__ int part_nf[GN_WAVES];
  for (int m = 32; m >= 1; m >>= 1) {
    v = join<INF>(v, __shfl_xor(v, m));
    nf += __shfl_xor(nf, m);
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v, part_nf[threadIdx.x >> 6] = nf;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = part[0], nf = part_nf[0];
    for (int w = 1; w < GN_WAVES; ++w) v = join<INF>(v, part[w]), nf += part_nf[w];
  }
}

template <bool INF>
__global__ __launch_bounds__(GN_THREADS) void grad_partial_kernel(const GnArgs p) {
  const int c = blockIdx.x, t = threadIdx.x;
  const Span sp = chunk_span(p, c);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int nf = 0;
  if (t < sp.head) take<INF>(a0, nf, sp.x[t]);
  const float4* xv = reinterpret_cast<const float4*>(sp.x + sp.head);
#pragma unroll 4
  for (int i = t; i < sp.nvec; i += GN_THREADS) {
    const float4 v = xv[i];
    take<INF>(a0, nf, v.x), take<INF>(a1, nf, v.y), take<INF>(a2, nf, v.z), take<INF>(a3, nf, v.w);
  }
  if (t < sp.tail) take<INF>(a0, nf, sp.x[sp.head + 4 * sp.nvec + t]);
  double a = join<INF>(join<INF>(a0, a1), join<INF>(a2, a3));
  block_join<INF>(a, nf);
  if (t == 0) p.partial[c] = a, p.partial_nf[c] = nf;
}

template <bool INF>
__global__ __launch_bounds__(GN_THREADS) void grad_final_kernel(const GnArgs p) {
  const int t = threadIdx.x;
  double tot = 0.0;
  int nf = 0;
  for (int s = t; s < p.n_seg; s += GN_THREADS) {
    int lo = 0, hi = p.n_chunk;  // the first chunk of a segment >= s
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.chunk_seg[mid] < s) lo = mid + 1; else hi = mid;
    }
    double a = 0.0;
    for (int c = lo; c < p.n_chunk && p.chunk_seg[c] == s; ++c) a = join<INF>(a, p.partial[c]), nf += p.partial_nf[c];
    p.norms[s] = (float)(INF ? a : sqrt(a));
    tot = join<INF>(tot, a);
  }
  block_join<INF>(tot, nf);
  if (t == 0) {
    const float total = (float)(INF ? tot : sqrt(tot));
    float coef = 1.f;
    if (p.max_norm > 0.0) {
      const double k = p.max_norm / ((double)total + 1e-6);
      coef = (float)((k != k || k < 1.0) ? k : 1.0);  // clamp(max = 1) keeps a NaN
    }
    p.total[0] = total, p.nonfinite[0] = nf, p.coef[0] = coef;
  }
}

__global__ __launch_bounds__(GN_THREADS) void grad_scale_kernel(const GnArgs p) {
  const float k = p.coef[0];
  if (k == 1.0f) return;  // (uniform over the grid)
  const int t = threadIdx.x;
  const Span sp = chunk_span(p, blockIdx.x);
  if (t < sp.head) sp.x[t] *= k;
  float4* xv = reinterpret_cast<float4*>(sp.x + sp.head);
#pragma unroll 4
  for (int i = t; i < sp.nvec; i += GN_THREADS) {
    float4 v = xv[i];
    v.x *= k, v.y *= k, v.z *= k, v.w *= k;
    xv[i] = v;
  }
  if (t < sp.tail) sp.x[sp.head + 4 * sp.nvec + t] *= k;
}

}  // namespace

extern "C" int tbx_grad_norms(const tbx_grad_norms_t* args, void* stream) {
  if (!args) return TBX_ERR_ARG;
  const tbx_grad_norms_t& a = *args;
  if (!a.g || !a.seg_off || !a.seg_len || !a.norms || !a.total || !a.nonfinite || !a.coef) return TBX_ERR_ARG;
  if (a.n <= 0 || a.n_seg <= 0 || a.n_chunk < 0) return TBX_ERR_ARG;
  if (a.n_chunk > 0 && (!a.chunk_seg || !a.chunk_off || !a.chunk_len || !a.partial || !a.partial_nf)) return TBX_ERR_ARG;
  if (a.n_chunk > 0 && (a.chunk_max <= 0 || a.chunk_max > TBX_GRAD_CHUNK)) return TBX_ERR_ARG;
  if (a.norm_type != TBX_GRAD_NORM_2 && a.norm_type != TBX_GRAD_NORM_INF) return TBX_ERR_ARG;
  if (((uintptr_t)a.g & 3) != 0) return TBX_ERR_ALIGN;
  GnArgs p;
  p.g = a.g, p.seg_off = a.seg_off, p.seg_len = a.seg_len;
  p.chunk_seg = a.chunk_seg, p.chunk_off = a.chunk_off, p.chunk_len = a.chunk_len;
  p.partial = a.partial, p.partial_nf = a.partial_nf;
  p.norms = a.norms, p.total = a.total, p.nonfinite = a.nonfinite, p.coef = a.coef;
  p.n = a.n, p.n_seg = a.n_seg, p.n_chunk = a.n_chunk, p.max_norm = a.max_norm;
  const bool inf = a.norm_type == TBX_GRAD_NORM_INF;
  hipStream_t st = (hipStream_t)stream;
  if (p.n_chunk > 0) {
    if (inf) hipLaunchKernelGGL(grad_partial_kernel<true>, dim3((unsigned)p.n_chunk), dim3(GN_THREADS), 0, st, p);
    else hipLaunchKernelGGL(grad_partial_kernel<false>, dim3((unsigned)p.n_chunk), dim3(GN_THREADS), 0, st, p);
    if (hipGetLastError() != hipSuccess) return TBX_ERR_LAUNCH;
  }
  if (inf) hipLaunchKernelGGL(grad_final_kernel<true>, dim3(1), dim3(GN_THREADS), 0, st, p);
  else hipLaunchKernelGGL(grad_final_kernel<false>, dim3(1), dim3(GN_THREADS), 0, st, p);
  if (hipGetLastError() != hipSuccess) return TBX_ERR_LAUNCH;
  if (p.n_chunk > 0 && a.max_norm > 0.0) {
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)p.n_chunk), dim3(GN_THREADS), 0, st, p);
    if (hipGetLastError() != hipSuccess) return TBX_ERR_LAUNCH;
  }
  return TBX_OK;
}
