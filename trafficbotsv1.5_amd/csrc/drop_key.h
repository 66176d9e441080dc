// Keyed dropout: the ONE definition of the mask (include/tbx_hip.h at tbx_drop_t).
//   keep(element) = drop_mix(counter, stream_key(seed, site, step)) >= thresh,   survivors scaled by `scale`
// * stream key: (seed, site, step) -> (lo, hi); step and the scene row come from row_key(row, rows_per_scene, time_batch, time0):
//   batch entry b = row / rows_per_scene is closed-loop step time0 + b % time_batch of scene b / time_batch.
// * counter: the owner's layout - elementwise sites scene_row * cols + column, attention (scene_row * 128 + target slot) * 4 + head.
// * (thresh, scale) from the float p: drop_rate, host only; a launch's whole key from its tbx_drop_t: make_key, host only.
// Every kernel and every host set-up of the library goes through here, so a backward kernel in one file regenerates the mask a
// forward kernel in another drew. Compiles under hipcc (device + host) and under a plain C++ compiler without HIP headers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/tbx_hip.h"  // (plain C: tbx_drop_t, the return codes)

#ifdef __HIP__
#define TBX_DROP_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define TBX_DROP_FN inline
#endif

namespace tbx_drop {

// lowbias32-style finaliser over the counter, keyed by the stream's (lo, hi)
TBX_DROP_FN uint32_t drop_mix(uint32_t x, uint32_t lo, uint32_t hi) {
  x ^= lo;
  x *= 0x9E3779B1u;
  x ^= hi;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

struct StreamKey {
  uint32_t lo, hi;
};
TBX_DROP_FN StreamKey stream_key(uint64_t seed, uint32_t site, uint32_t step) {
  return {(uint32_t)seed ^ (site * 0x85EBCA6Bu) ^ (step * 0x27D4EB2Fu), (uint32_t)(seed >> 32) + site * 0xC2B2AE35u + step * 0x165667B1u};
}

struct RowKey {
  uint32_t step, scene_row;
};
// I: the integer type the caller's row arithmetic runs in (int64_t for the streaming kernels, 32-bit where the divisions sit in a
// loop with no issue slots to spare) - the divisions are done in exactly that type. The second form is for a caller that holds the
// row's batch entry b = row / rows_per_scene already (written out rather than called by the first: the nested call cost the
// streaming kernels a scalar register).
template <class I>
TBX_DROP_FN RowKey row_key(I row, int rows_per_scene, int time_batch, int time0) {
  const I rps = (I)rows_per_scene, tb = (I)time_batch;
  const I b = row / rps;
  const I sc = b / tb;
  return {(uint32_t)time0 + (uint32_t)(b - sc * tb), (uint32_t)(sc * rps + (row - b * rps))};
}
template <class I>
TBX_DROP_FN RowKey row_key(I row, I b, int rows_per_scene, int time_batch, int time0) {
  const I rps = (I)rows_per_scene, tb = (I)time_batch;
  const I sc = b / tb;
  return {(uint32_t)time0 + (uint32_t)(b - sc * tb), (uint32_t)(sc * rps + (row - b * rps))};
}

// ---- action noise: the ONE definition of the standard-normal pair the closed-loop step adds to an agent's action mean (tbx_sim_state_t
// act_seed; Python restatement: hip_base.action_noise_bits / action_noise).
//   (h1, h2) = drop_mix(scene_row * 2 [+ 1], stream_key(seed, ACTION_NOISE_SITE, step))   step: the 1-based device step counter
//   u1 = (h1 + 1) * 2^-32 in (0, 1],  theta = 2 pi * h2 * 2^-32,  eps = sqrt(-2 ln u1) * (cos theta, sin theta)   (Box-Muller)
// so ln u1 is finite and |eps| <= sqrt(64 ln 2) = 6.66. The site id is none of the dropout sites' (those count up from 1 per module
// of a step's pass, attention calls likewise): the ASCII of "ACTN".
constexpr uint32_t ACTION_NOISE_SITE = 0x4143544Eu;

struct NoiseBits {
  uint32_t h1, h2;
};
TBX_DROP_FN NoiseBits action_noise_bits(uint64_t seed, uint32_t step, uint32_t scene_row) {
  const StreamKey k = stream_key(seed, ACTION_NOISE_SITE, step);
  return {drop_mix(scene_row * 2u, k.lo, k.hi), drop_mix(scene_row * 2u + 1u, k.lo, k.hi)};
}

struct Noise2 {
  float e0, e1;
};
// The float part, with the accurate library functions (the hardware approximations miss the 1e-5 the restatement is held to).
// ln u1 in the upper half of the range goes through log1pf of the exact integer distance to 1: (float)(h1 + 1) rounds to 24 bits, and
// next to u1 = 1 that rounding is as large as 1 - u1 itself (r = sqrt(-2 ln u1) would be off by up to 2e-4).
TBX_DROP_FN Noise2 action_noise(NoiseBits b) {
  const float two_m32 = 2.3283064365386963e-10f;  // 2^-32
  const float ln_u1 = b.h1 >= 0x80000000u ? log1pf(-((float)(0xFFFFFFFFu - b.h1) * two_m32)) : logf(((float)b.h1 + 1.0f) * two_m32);
  const float r = sqrtf(-2.0f * ln_u1);
  const float theta = (float)b.h2 * 1.4629180792671596e-9f;  // 2 pi * 2^-32
  float sn, cs;
  sincosf(theta, &sn, &cs);
  return {r * cs, r * sn};
}
TBX_DROP_FN Noise2 action_noise(uint64_t seed, uint32_t step, uint32_t scene_row) { return action_noise(action_noise_bits(seed, step, scene_row)); }

// What a kernel holds of an elementwise site's key (by value, inside its argument struct). thresh == 0: no dropout - the neutral key
// {NULL, 0, 0, 1.0f, 1, 1, 0}, whose seed is never read.
struct Key {
  const uint64_t* seed;  // device memory
  uint32_t site, thresh;
  float scale;
  int rows_per_scene, time_batch, time0;
};

// ---- host side ----
struct Rate {
  uint32_t thresh;  // drop when the hash < thresh; 0 exactly when p <= 0: no dropout
  float scale;      // 1 / (1 - p)
};
inline Rate drop_rate(float p) {  // p < 1: make_key's check
  if (!(p > 0.f)) return {0u, 1.0f};
  const double th = (double)p * 4294967296.0;
  return {th < 1.0 ? 1u : (uint32_t)th, 1.0f / (1.0f - p)};
}
// the key's arguments of a launch that drops (p > 0) over `rows` rows
inline bool key_args_ok(const uint64_t* seed, int64_t rows, int rows_per_scene, int time_batch, int time0) {
  return seed != nullptr && rows_per_scene > 0 && time_batch >= 1 && time0 >= 0 && rows % rows_per_scene == 0;
}

// 1 / (1 - p) alone: a backward that reads the mask off the forward's output (tbx_relu_drop_bwd, tbx_pointnet_tail_bwd)
inline float keep_scale(float p) { return drop_rate(p).scale; }

// The key of a launch over `rows` rows from the caller's tbx_drop_t: the ONE host set-up. Return codes, in this order:
//   1. d == NULL, or d->p is not > 0   -> TBX_OK, the neutral key; no other field of d is looked at
//   2. d->p >= 1, or !key_args_ok(..)  -> TBX_ERR_ARG
//   3. otherwise                       -> TBX_OK, (thresh, scale) = drop_rate(d->p)
// Where that sits in each caller (the first check that fails decides; this is the only place the order is written down):
//   tbx_tall_linear(_bf16)                   args == NULL or p < 0 -> ARG; x / image / y == NULL or m <= 0 -> ARG; k, n not multiples of
//                                            64 in 64 .. 1024 -> UNSUPPORTED; ldx < k, ldy < n, ldx or ldy % 4 -> ARG; x / y / image not
//                                            16-byte aligned -> ALIGN; y16 with ldy16 < n, ldy16 % 4 or not 8-byte aligned -> ALIGN;
//                                            p > 0 without relu -> ARG; p > 0 with y16 -> UNSUPPORTED (no caller, the kernel path is
//                                            untested); the key; p > 0 and m > 0x7fffffff -> UNSUPPORTED (its row arithmetic is 32-bit)
//   tbx_residual_drop_*, tbx_relu_drop_fwd   pointers -> ARG; alignment -> ALIGN; rows < 0, cols <= 0 or cols % 4 -> UNSUPPORTED;
//                                            rows == 0 -> OK; p < 0 -> ARG; the key
//   tbx_keyed_dropout                        pointers, rows < 0, cols <= 0, d == NULL or p not > 0 -> ARG (this call IS the dropout);
//                                            the key; rows == 0 -> OK
//   tbx_pointnet_tail_fwd                    pointers -> ARG; the shape -> UNSUPPORTED; the key (p < 0 is "none", as it always was)
//   tbx_knarpe_attn_* (tbx_attn_t)           after fill_common: p < 0, p >= 1, time_batch < 1, time0 < 0 -> ARG with or without
//                                            dropout; the key
inline int make_key(const tbx_drop_t* d, int64_t rows, Key* out) {
  *out = Key{nullptr, 0u, 0u, 1.0f, 1, 1, 0};
  if (d == nullptr || !(d->p > 0.f)) return TBX_OK;
  if (d->p >= 1.f || !key_args_ok(d->seed, rows, d->rows_per_scene, d->time_batch, d->time0)) return TBX_ERR_ARG;
  const Rate r = drop_rate(d->p);
  *out = Key{d->seed, d->site, r.thresh, r.scale, d->rows_per_scene, d->time_batch, d->time0};
  return TBX_OK;
}

}  // namespace tbx_drop
