// Host half of the KNARPE attention ABI (include/tbx_hip.h, tbx_attn_t), shared by attn.hip and attn_mfma.hip: the argument checks
// with the fields both kernel families take, and the dropout set-up. Training may run its forward on one file's kernels and its
// backward on the other's, and the backward regenerates the forward's mask from (threshold, scale): they are computed HERE only.
#pragma once
#include <math.h>

#include "attn_core.h"

namespace tbx_attn {

// Checks of the query side and the segments of `t`, in the order (= the precedence of the return codes) callers have always seen,
// and the fields every kernel's argument struct A (AttnArgs, MArgs) has. ldo: the width to hold against the 640-wide row. mfma: the
// matrix-core forward's rules - no rpe_k_bias but `out` in the alignment step, relative-pose segments only, K/V columns in 8-element
// steps, 32-bit byte offsets inside a batch entry's table (they sit between the shared checks, where their codes always ranked).
template <class A>
inline int fill_common(A& a, const tbx_attn_t& t, int ldo, bool mfma) {
  if (!t.qbuf || (!mfma && !t.rpe_k_bias) || t.n_batch <= 0 || t.n_src <= 0) return TBX_ERR_ARG;
  if (t.n_seg < 1 || t.n_seg > 2 || ldo < D + NH * DR) return TBX_ERR_UNSUPPORTED;
  if ((t.ldq % 4) || (t.q_off % 4) || (t.qt_off % 4) || (ldo % 4) || (((uintptr_t)t.qbuf) & 15) ||
      (((uintptr_t)(mfma ? (const void*)t.out : (const void*)t.rpe_k_bias)) & 15))
    return TBX_ERR_ALIGN;
  const int kv_step = mfma ? 8 : 4;
  int ktot = 0;
  for (int i = 0; i < t.n_seg; ++i) {
    const tbx_attn_seg_t& s = t.seg[i];
    if (!s.kv || !s.idx || !s.invalid || (mfma ? !s.rel_pose : (!s.emb && !s.rel_pose)) || s.k <= 0 || s.n_tgt <= 0 || s.batch_div <= 0)
      return TBX_ERR_ARG;
    if (!s.emb && (!t.freqs_xy || !t.freqs_yaw)) return TBX_ERR_ARG;
    if (mfma && s.emb != nullptr) return TBX_ERR_UNSUPPORTED;  // relative-pose form only
    if ((s.ld_kv % kv_step) || (s.k_off % kv_step) || (s.v_off % kv_step) || (((uintptr_t)s.kv) & 15) || (s.emb && (((uintptr_t)s.emb) & 15)))
      return TBX_ERR_ALIGN;
    if ((s.kv_bf16 != 0) != (t.seg[0].kv_bf16 != 0)) return TBX_ERR_UNSUPPORTED;  // one element type per call
    if (mfma && (int64_t)s.n_tgt * s.ld_kv * 4 >= (1ll << 32)) return TBX_ERR_UNSUPPORTED;
    ktot += s.k;
    a.seg[i] = s;
  }
  if (t.n_seg == 1) a.seg[1] = a.seg[0];
  if (ktot > KMAX) return TBX_ERR_UNSUPPORTED;
  a.qbuf = t.qbuf;
  a.fxy = t.freqs_xy;
  a.fyaw = t.freqs_yaw;
  a.ldq = t.ldq;
  a.q_off = t.q_off;
  a.qt_off = t.qt_off;
  a.ldo = ldo;
  a.n_rows = t.n_batch * t.n_src;
  a.n_src = t.n_src;
  a.n_seg = t.n_seg;
  a.scale2 = 1.4426950408889634f / sqrtf((float)DH);
  return TBX_OK;
}

// The dropout fields of A from t's (drop_key.h: make_key). drop_thresh != 0 exactly when p_drop > 0.
template <class A>
inline int set_dropout(A& a, const tbx_attn_t& t) {
  a.drop_seed = t.drop_seed;
  a.drop_call = t.drop_call;
  a.drop_time_batch = t.time_batch;
  a.drop_time0 = t.time0;
  a.drop_thresh = 0u;
  a.drop_scale = 1.f;
  // (time_batch and time0 are held to their ranges without dropout too; the rows are n_batch whole scenes of n_src > 0 rows, which
  // fill_common has checked by now, so of the key's arguments only the seed can still be wrong)
  if (t.p_drop < 0.f || t.p_drop >= 1.f || t.time_batch < 1 || t.time0 < 0) return TBX_ERR_ARG;
  const tbx_drop_t d{t.drop_seed, t.p_drop, t.drop_call, t.n_src, t.time_batch, t.time0, 0};
  tbx_drop::Key key;
  if (const int rc = tbx_drop::make_key(&d, (int64_t)t.n_batch * t.n_src, &key)) return rc;
  a.drop_thresh = key.thresh;
  a.drop_scale = key.scale;
  return TBX_OK;
}

}  // namespace tbx_attn
