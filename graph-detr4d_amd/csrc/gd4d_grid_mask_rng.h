// The device-resident draws of GridMask (models/utils/grid_mask.py:84-95, 118): which step applies the mask, the grid period d, the
// band width l, the two starts, and - with `offset` - one value in [-1, 1) per pixel.
//
// The reference draws them on the host with np.random (rand(), randint(2, h), randint(d), randint(d), rand(h, w)).  The device route
// (gd4d_grid_mask_draw, gd4d_grid_mask_fwd's generated offset) draws each of them as a function of (seed, step, index) only, so
// nothing is uploaded, a replayed hipGraph draws a new mask whenever the step counter has advanced, and tests restate the draws on
// the host (tests/grid_mask_ref.py).  THIS FILE IS THE CONTRACT:
//
//   fmix(x)                      = murmur3's 32-bit finaliser
//   hash(seed, step, i)          = fmix((i ^ seed_lo) * 0x9E3779B1 + fmix((step + 0x9E3779B9) ^ seed_hi))        (all mod 2^32)
//   draw k of a step             = hash(seed, step, 0xFFFFFFFF - k): k = 0 gate, 1 d, 2 st_h, 3 st_w
//   pixel (y, x) of an H x W map = hash(seed, step, y W + x); H W < 2^31, so a pixel never meets a draw
//   apply  <=>  draw0 < thresh, thresh = round(prob 2^32) clamped to 2^32 - 1, which itself means "always" (prob >= 1)
//   d      = 2 + ((H - 2) draw1 >> 32)                                in [2, H)            randint(2, h)
//   l      = min(max(int(d ratio + 0.5), 1), d - 1), in double        in [1, d - 1]        grid_mask.py:92
//   st_h   = d draw2 >> 32,  st_w = d draw3 >> 32                     in [0, d)            randint(d)
//   offset = (hash >> 8) 2^-23 - 1, exact in fp32                     in [-1, 1)           2 (rand - 0.5)
#pragma once
#include <cstdint>

namespace gd4d {

__host__ __device__ __forceinline__ uint32_t gm_fmix(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// the part of the hash that is the same for every index of a step
__host__ __device__ __forceinline__ uint32_t gm_step_key(uint32_t seed_hi, uint32_t step) { return gm_fmix((step + 0x9E3779B9u) ^ seed_hi); }

__host__ __device__ __forceinline__ uint32_t gm_hash_keyed(uint32_t seed_lo, uint32_t key, uint32_t i) {
  return gm_fmix((i ^ seed_lo) * 0x9E3779B1u + key);
}

__host__ __device__ __forceinline__ uint32_t gm_hash(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t i) {
  return gm_hash_keyed(seed_lo, gm_step_key(seed_hi, step), i);
}

__host__ __device__ __forceinline__ uint32_t gm_bounded(uint32_t range, uint32_t h) { return (uint32_t)(((uint64_t)range * h) >> 32); }

__host__ __device__ __forceinline__ float gm_offset_value(uint32_t h) { return (float)(h >> 8) * 1.1920928955078125e-07f - 1.0f; }

struct GmDraw {
  int32_t apply, d, l, st_h, st_w;
};

// one step's draws; H >= 3
__host__ __device__ __forceinline__ GmDraw gm_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t thresh, int H, double ratio) {
  const uint32_t key = gm_step_key(seed_hi, step);
  GmDraw r;
  r.apply = (thresh == 0xFFFFFFFFu || gm_hash_keyed(seed_lo, key, 0xFFFFFFFFu) < thresh) ? 1 : 0;
  r.d = 2 + (int32_t)gm_bounded((uint32_t)(H - 2), gm_hash_keyed(seed_lo, key, 0xFFFFFFFEu));
  int32_t l = (int32_t)((double)r.d * ratio + 0.5);
  l = l < 1 ? 1 : l;
  r.l = l > r.d - 1 ? r.d - 1 : l;
  r.st_h = (int32_t)gm_bounded((uint32_t)r.d, gm_hash_keyed(seed_lo, key, 0xFFFFFFFDu));
  r.st_w = (int32_t)gm_bounded((uint32_t)r.d, gm_hash_keyed(seed_lo, key, 0xFFFFFFFCu));
  return r;
}

}  // namespace gd4d
