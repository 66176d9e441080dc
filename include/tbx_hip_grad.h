/*
 * Gradient norms on the flat gradient buffer: ONE entry point, exported by a library of its own, libtbx_grad.so (source:
 * csrc/grad_norm.hip). It is not a section of include/tbx_hip.h and that header does not include this one: the entry points of
 * libtbx_hip.so are the closed list of ABI 7, and a host bound to it needs nothing from here. The contract is the same - device pointers
 * to caller-owned buffers, nothing allocated or retained, kernels only enqueued on `stream`, the TBX_* return codes of tbx_hip.h before
 * any launch; tbx_error_string of libtbx_hip.so names them. It is what Lightning's
 * `track_grad_norm` + `gradient_clip_val` do around an optimizer step (one norm per parameter, their total, clip_grad_norm_'s in-place
 * scale) for gradients that live in ONE flat float32 buffer with a static layout (pl_modules/data_parallel.py: FlatGrads).
 */
#ifndef TBX_HIP_GRAD_H
#define TBX_HIP_GRAD_H

#include <stdint.h>

#include "tbx_hip.h" /* TBX_ERR_* codes */

#ifdef __cplusplus
extern "C" {
#endif

#define TBX_GRAD_CHUNK 8192 /* most elements of one chunk: one workgroup's share of launch 1 and launch 3 */
#define TBX_GRAD_NORM_2 2   /* norm_type: sqrt(sum x^2) */
#define TBX_GRAD_NORM_INF 0 /* norm_type: max |x| */

/* ------------------------------------------------------------------------------------------------------------------
 * tbx_grad_norms: per-segment norms of a flat buffer, their total, the non-finite count, clip_grad_norm_'s coefficient and (max_norm > 0)
 * the in-place scale, as three launches on `stream` without a host read.
 *
 * Layout, built once by the host (it is static):
 *   segments  s = 0 .. n_seg-1: g[seg_off[s] .. seg_off[s] + seg_len[s]), disjoint and ascending. Elements between segments (the gaps of
 *             an aligned layout) belong to no segment: they are neither read nor written.
 *   chunks    c = 0 .. n_chunk-1: g[chunk_off[c] .. chunk_off[c] + chunk_len[c]) inside segment chunk_seg[c] (chunk_off is an offset
 *             into g, not into the segment). The chunks of a segment are consecutive in the table, tile the segment exactly once in
 *             ascending order, and none is longer than TBX_GRAD_CHUNK; chunk_seg is therefore ascending. A segment of length 0 has no
 *             chunk (its norm is 0). chunk_max = the longest chunk_len of the table, as the host that built it knows it.
 *
 * Launch 1, one workgroup per chunk: every element once, through 16-byte loads from the first 16-byte-aligned address of the chunk on
 *   and single loads for the (up to three) elements before and after. 2-norm: x^2 accumulated in float64 (the square of a float32 is
 *   exact there; nothing under- or overflows between 1e-154 and 1e154). Inf-norm: the maximum |x|, a NaN winning. Lanes -> wave
 *   butterfly -> LDS -> the waves in wave order -> partial[c], partial_nf[c] (the count of NaN / +-Inf elements), ordinary stores.
 * Launch 2, one workgroup: a thread per segment adds the segment's partials in chunk order; norms[s] = (float)sqrt(sum) (inf: the
 *   maximum). total = (float)sqrt(sum over ALL segments' float64 sums) - the 2-norm of the segment norms without their float32 rounding
 *   in between - (inf: the maximum), added over threads, waves and segments in an order the shapes alone fix. nonfinite = the sum of
 *   the chunk counts. coef = (float)min(1, max_norm / ((double)total + 1e-6)) with max_norm > 0, else 1; a NaN total gives a NaN coef.
 * Launch 3, only with max_norm > 0, one workgroup per chunk: g[i] = g[i] * coef (float32) over the chunks; a workgroup that reads
 *   coef == 1.0f returns without a store (x * 1.0f is x bit for bit).
 * Non-finite values propagate as in torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False). No atomics: two calls on the same input
 * leave the same bytes. A chunk entry that does not lie inside its segment and inside [0, n) is cut to the part that does.
 *
 * Returns TBX_ERR_ARG for a NULL struct / pointer (partial and partial_nf may be NULL only with n_chunk == 0), n <= 0, n_seg <= 0,
 * n_chunk < 0, chunk_max outside [1, TBX_GRAD_CHUNK] (n_chunk > 0) or an unknown norm_type; TBX_ERR_ALIGN for a g that is not 4-byte
 * aligned.
 */
typedef struct tbx_grad_norms_t {
  float* g;                 /* [n] the flat buffer; scaled in place when max_norm > 0 */
  const int64_t* seg_off;   /* [n_seg] */
  const int64_t* seg_len;   /* [n_seg] */
  const int32_t* chunk_seg; /* [n_chunk] ascending */
  const int64_t* chunk_off; /* [n_chunk] first element, an index into g */
  const int32_t* chunk_len; /* [n_chunk] 1 .. TBX_GRAD_CHUNK */
  double* partial;          /* [n_chunk] workspace: sum of squares (inf: maximum) per chunk */
  int32_t* partial_nf;      /* [n_chunk] workspace: non-finite elements per chunk */
  float* norms;             /* [n_seg] out */
  float* total;             /* [1] out */
  int32_t* nonfinite;       /* [1] out */
  float* coef;              /* [1] out */
  int64_t n;
  int32_t n_seg, n_chunk, chunk_max, norm_type; /* TBX_GRAD_NORM_2 | TBX_GRAD_NORM_INF */
  double max_norm;                              /* <= 0: no clipping (coef = 1, g is only read) */
} tbx_grad_norms_t;

int tbx_grad_norms(const tbx_grad_norms_t* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TBX_HIP_GRAD_H */
