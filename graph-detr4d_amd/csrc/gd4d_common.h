// Shared helpers for libgd4d.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

#include "gd4d.h"

#define GD4D_WAVE 64

namespace gd4d {

void set_last_hip_error(hipError_t e);

// Record and translate a launch failure (never synchronises).
inline int check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_hip_error(e);
    return GD4D_ELAUNCH;
  }
  return GD4D_OK;
}

// Allow `bytes` of dynamic LDS for `kern` on the CURRENT device.  hipFuncAttributeMaxDynamicSharedMemorySize is a
// per-device attribute, so what has been granted is remembered per (kernel, device id) - a process driving several GPUs
// configures each of them (a process-wide "configured" flag would leave every device but the first at 64 KB).
inline bool allow_dynamic_lds(const void* kern, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> granted;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> guard(mu);
  int& have = granted[std::make_pair(kern, dev)];
  if (have >= bytes) return true;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
  have = bytes;
  return true;
}

// The metre range of the reference points, as every kernel that de-normalises one reads it: rng_scale =
// float(double(hi) - double(lo)), rng_lo = float(lo), for as many axes as the struct keeps (pc_range = lo xyz, hi xyz).
// Written once: the kernels that project a query must agree on these two roundings bit for bit.
template <class P>
inline void fill_metre_range(P& p, const double* pc_range) {
  constexpr int axes = sizeof(p.rng_scale) / sizeof(p.rng_scale[0]);
  static_assert(axes <= 3 && sizeof(p.rng_lo) == sizeof(p.rng_scale), "rng_scale / rng_lo: one float per axis");
  for (int k = 0; k < axes; ++k) {
    p.rng_scale[k] = static_cast<float>(pc_range[k + 3] - pc_range[k]);
    p.rng_lo[k] = static_cast<float>(pc_range[k]);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ float bf16_to_f32(uint16_t v) {
  return __uint_as_float(static_cast<uint32_t>(v) << 16);
}

// round-to-nearest-even f32 -> bf16 bits (NaN kept quiet)
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

// the sum over the 32 lanes of a wave's half, by an xor butterfly: every lane of the half gets the same bits
__device__ __forceinline__ float half_wave_sum(float s) {
#pragma unroll
  for (int m = 1; m < 32; m <<= 1) s += __shfl_xor(s, m);
  return s;
}

// the sum over the WIDTH lanes of an aligned lane group, widest exchange first: every lane of the group gets the same bits
// (T: float, double or int)
template <int WIDTH, class T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return group_sum<GD4D_WAVE>(v); }

// ---- the fixed-order workgroup sum --------------------------------------------------------------------------------------------
// THE order of every sum over a workgroup (one value per thread) that promises equal bits from run to run: wave_sum in each wave,
// lane 0 of wave w stores to s_red[w], a barrier, then ((s_red[0] + s_red[1]) + s_red[2]) + ... in wave order.  The first wave's
// value starts the sum, no 0 is added: a site whose waves may all hold -0 and that wants +0 writes `0.f +` at its call.
//   block_sum_put  the part before the barrier.  s_red: LDS, blockDim.x / 64 elements (blockDim.x a multiple of 64).
//   block_sum_get  the part after it, for any thread that wants the sum: each gets the same bits.  WAVES: the wave count where it
//                  is a constant of the kernel (the loop unrolls), 0 = blockDim.x / 64.
//   block_sum      put, __syncthreads(), get: EVERY thread holds the sum.
// The barrier between put and get is the caller's when it has several values (put them all, ONE barrier, get them) or a
// __syncthreads_or to share.  Nothing here ENDS with a barrier: s_red is free for its next writer only after a barrier that
// follows the last get - the caller's, where it reuses the array.
template <class T>
__device__ __forceinline__ void block_sum_put(T v, T* s_red) {
  v = wave_sum(v);
  if ((threadIdx.x & (GD4D_WAVE - 1)) == 0) s_red[threadIdx.x / GD4D_WAVE] = v;
}
template <int WAVES = 0, class T>
__device__ __forceinline__ T block_sum_get(const T* s_red) {
  T s = s_red[0];
  if constexpr (WAVES > 0) {
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += s_red[w];
  } else {
    for (int w = 1; w < (int)(blockDim.x / GD4D_WAVE); ++w) s += s_red[w];
  }
  return s;
}
template <int WAVES = 0, class T>
__device__ __forceinline__ T block_sum(T v, T* s_red) {
  block_sum_put(v, s_red);
  __syncthreads();
  return block_sum_get<WAVES>(s_red);
}

// inverse_sigmoid of the reference (deform3d_cross_attn.py:16-31), eps = 1e-5
__device__ __forceinline__ float inv_sigmoid(float x) {
  x = fminf(fmaxf(x, 0.f), 1.f);
  const float a = fminf(fmaxf(x, 1e-5f), 1.f), b = fminf(fmaxf(1.f - x, 1e-5f), 1.f);
  return logf(a / b);
}

// inv_sigmoid on the transcendental unit: log(a / b) = (log2 a - log2 b) ln 2 with v_log_f32 (~1 ulp), |error| <~ 2e-6 on
// results of up to 11.5; the clamps are inv_sigmoid's
__device__ __forceinline__ float inv_sigmoid_fast(float x) {
  x = fminf(fmaxf(x, 0.f), 1.f);
  const float a = fminf(fmaxf(x, 1e-5f), 1.f), b = fminf(fmaxf(1.f - x, 1e-5f), 1.f);
  return (__builtin_amdgcn_logf(a) - __builtin_amdgcn_logf(b)) * 0.69314718055994530942f;
}

// ---- dev tracing (gd4d_trace_enable): block 0 of a kernel stamps s_memrealtime (100 MHz) at entry / exit -----------
// buffer: [0] entries written, [1] capacity (entries), then {id, time} pairs.  One device-global pointer per translation
// unit (no relocatable device code); nullptr = off: one scalar load per kernel.
#define GD4D_TRACE_UNIT(tag)                                                                          \
  __device__ unsigned long long* g_trace_##tag = nullptr;                                              \
  void trace_set_##tag(unsigned long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_trace_##tag), &p, sizeof(p)); }
__device__ __forceinline__ void trace_mark_if(unsigned long long* t, unsigned long long id, bool stamping_block) {
  if (t && stamping_block && threadIdx.x == 0) {
    const unsigned long long slot = atomicAdd(t, 1ull);
    if (slot < t[1]) { t[2 + 2 * slot] = id; t[3 + 2 * slot] = __builtin_amdgcn_s_memrealtime(); }
  }
}
__device__ __forceinline__ void trace_mark(unsigned long long* t, unsigned long long id) {
  trace_mark_if(t, id, blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0);
}

}  // namespace gd4d
