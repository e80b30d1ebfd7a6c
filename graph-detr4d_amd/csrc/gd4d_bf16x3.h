// The split-bf16 ("bf16x3") arithmetic of every bf16 MFMA GEMM in the library, defined once.
//
// An fp32 value is split x ~= hi + lo, both bf16: hi is x rounded to bf16 (cvt_pk_bf16, to nearest even), lo is
// x - hi rounded to bf16.  Because hi is a rounding of x, x - hi is exact in fp32; only lo's own rounding is lost, so hi + lo
// holds x to ~2^-16 relative.  A product a b is taken as three bf16 MFMAs accumulated in fp32, a_lo b_hi + a_hi b_lo + a_hi b_hi
// (a_lo b_lo dropped): ~2^-16 relative per product.  split8x3 cuts the residual once more (x = hi + mid + lo to ~2^-24) for the
// six-product arithmetic of GD4D_CHAIN_EXACT (gd4d_rowchain.hip).
//
// 8 bf16 are 16 bytes: u32x4 is how a piece is split, stored and loaded, bf16x8 (frag) is what the MFMA builtins take.
#pragma once
#include <hip/hip_runtime.h>

namespace gd4d {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// bf16 of lo_elem in bits 0-15, bf16 of hi_elem in bits 16-31
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo_elem, float hi_elem) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo_elem), "v"(hi_elem));
  return r;
}

// 8 consecutive floats -> 16 bytes of bf16 hi halves and 16 bytes of bf16 lo halves
__device__ __forceinline__ void split8(const float* v, u32x4& h, u32x4& l) {
  unsigned hh[4], ll[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    hh[i] = cvt_pk_bf16(v[2 * i], v[2 * i + 1]);
    ll[i] = cvt_pk_bf16(v[2 * i] - __uint_as_float(hh[i] << 16), v[2 * i + 1] - __uint_as_float(hh[i] & 0xffff0000u));
  }
  h = u32x4{hh[0], hh[1], hh[2], hh[3]};
  l = u32x4{ll[0], ll[1], ll[2], ll[3]};
}

// 8 consecutive floats -> three bf16 pieces, x = hi + mid + lo
__device__ __forceinline__ void split8x3(const float* v, u32x4& h, u32x4& m, u32x4& l) {
  unsigned hh[4], mm[4], ll[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    hh[i] = cvt_pk_bf16(v[2 * i], v[2 * i + 1]);
    const float r0 = v[2 * i] - __uint_as_float(hh[i] << 16), r1 = v[2 * i + 1] - __uint_as_float(hh[i] & 0xffff0000u);
    mm[i] = cvt_pk_bf16(r0, r1);
    ll[i] = cvt_pk_bf16(r0 - __uint_as_float(mm[i] << 16), r1 - __uint_as_float(mm[i] & 0xffff0000u));
  }
  h = u32x4{hh[0], hh[1], hh[2], hh[3]};
  m = u32x4{mm[0], mm[1], mm[2], mm[3]};
  l = u32x4{ll[0], ll[1], ll[2], ll[3]};
}

__device__ __forceinline__ bf16x8 frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

// acc + a b from split operands, in the order a_lo b_hi, a_hi b_lo, a_hi b_hi (smallest terms first).  Sites that sum the
// products in another order write them out and say so: a different order is a different fp32 result.
__device__ __forceinline__ f32x16 mfma_32x32x16_x3(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl,
                                                  f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(al), frag(bh), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(ah), frag(bl), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(ah), frag(bh), acc, 0, 0, 0);
  return acc;
}
// C/D of 32x32x16: a lane holds column lane & 31 and, with kg = lane >> 5, accumulator register r (0 .. 15) is row
// 4 kg + (r & 3) + 8 (r >> 2) of the tile.  row0 = the tile's first row: added first, so that the register's constant stays the last
// term of the sum and folds into the store's address as when the sum is written out (added to a finished row it costs an
// instruction per store, and registers in dcn_bwd_data_kernel).
__host__ __device__ __forceinline__ constexpr int mfma32_row(int kg, int r, int row0 = 0) { return row0 + 4 * kg + (r & 3) + 8 * (r >> 2); }

__device__ __forceinline__ f32x4 mfma_16x16x32_x3(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl,
                                                 f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(al), frag(bh), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(ah), frag(bl), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(ah), frag(bh), acc, 0, 0, 0);
  return acc;
}

}  // namespace gd4d
