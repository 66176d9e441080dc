// Keyed dropout: the ONE definition of the mask (include/tbx_hip.h at tbx_keyed_dropout).
//   keep(element) = drop_mix(counter, stream_key(seed, site, step)) >= thresh,   survivors scaled by `scale`
// * stream key: (seed, site, step) -> (lo, hi); step and the scene row come from row_key(row, rows_per_scene, time_batch, time0):
//   batch entry b = row / rows_per_scene is closed-loop step time0 + b % time_batch of scene b / time_batch.
// * counter: the owner's layout - elementwise sites scene_row * cols + column, attention (scene_row * 128 + target slot) * 4 + head.
// * (thresh, scale) from the float p: drop_rate, host only.
// Every kernel and every host set-up of the library goes through here, so a backward kernel in one file regenerates the mask a
// forward kernel in another drew. Compiles under hipcc (device + host) and under a plain C++ compiler without HIP headers.
#pragma once
#include <stdint.h>

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

// ---- host side ----
struct Rate {
  uint32_t thresh;  // drop when the hash < thresh; 0 exactly when p <= 0: no dropout
  float scale;      // 1 / (1 - p)
};
inline Rate drop_rate(float p) {  // p < 1: the caller's check
  if (!(p > 0.f)) return {0u, 1.0f};
  const double th = (double)p * 4294967296.0;
  return {th < 1.0 ? 1u : (uint32_t)th, 1.0f / (1.0f - p)};
}
// the key's arguments of a launch that drops (p > 0) over `rows` rows
inline bool key_args_ok(const uint64_t* seed, int64_t rows, int rows_per_scene, int time_batch, int time0) {
  return seed != nullptr && rows_per_scene > 0 && time_batch >= 1 && time0 >= 0 && rows % rows_per_scene == 0;
}

}  // namespace tbx_drop
