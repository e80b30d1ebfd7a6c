// What the channel-sliced kernels share: the layout of the plan (gd4d_cross_attn_sliced.hip writes it; the gather, the
// training backward in gd4d_cross_attn_sliced_bwd.hip and the pyramid-gradient kernels read it), and the pieces the forward
// gathers and the backward gather-dot are built from: the walk, the pass, the corner-slot reduction, the host-side argument
// check and the dispatcher from (heads, value type, levels) to an instantiation.
#pragma once
#include <type_traits>

#include "gd4d_common.h"
#include "gd4d_cross_attn_shared.h"

namespace gd4d {

constexpr int kSlice = 32;                       // channels per slice: 128 bytes fp32 = one L2 line
constexpr int kSlices = kChannels / kSlice;      // 8
constexpr int kPlanHdr = 16;                     // ints per query in the plan header: item count per head

// How the pyramid the gather reads is addressed: offset of (camera row, level l, pixel) inside level l's base pointer
// = row * cam_stride[l] + pixel * pix_stride  (the plan stores these byte offsets).
struct PyramidGeom {
  unsigned cam_stride[4];       // bytes between camera rows of level l
  int lvl_w[4], lvl_h[4];
  unsigned pix_stride;          // bytes between pixels
};

// plan = [header: kPlanHdr ints per position, padded to 256 B][pairs: (position, head, pass < cap_t, 64) uint2]
// GD4D_CA_PLAN_ITEMS: [the same header][items: (position, head, item < cap_i) x {u, v, camera row, M}{level weight 0..3}];
// cap_i * 32 <= cap_t * 512, so gd4d_cross_attn_plan_bytes covers both forms
static inline int plan_cap_t(int N, int P) { return (N * P + 3) / 4; }      // passes of 4 items a head can need
static inline int plan_cap_items(int N, int P) { return (N * P + 15) & ~15; }  // GD4D_CA_PLAN_ITEMS: 32-byte records a head can need
static inline size_t plan_hdr_bytes(int B, int Q) { return (((size_t)B * Q * kPlanHdr * sizeof(int)) + 255) & ~(size_t)255; }

// What a launch of the gather (gd4d_cross_attn_sliced.hip) or of the gather-dot (gd4d_cross_attn_sliced_bwd.hip) walks.
struct SlicedParams {
  const char* lvl_base[4];      // level l: address of (camera row 0, pixel 0, slice 0, channel 0)
  long long slice_stride;       // bytes between slices
  const int* hdr;
  const uint2* pair;
  const int32_t* order;
  float* agg;                   // (BQ, HH, 256): the gather's sums; the gather-dot READS dL/d agg here
  int BQ, per_xcd, cap_t;
  int slice_lo, slice_n;        // slices [slice_lo, slice_lo + slice_n) in this launch
  int blk;                      // queries per block of the walk: within an XCD, block-major, then slice, then query
};

// (the walk: which (position, phase) workgroup `block` is; false: none.  A phase is one of the launch's slice_n slices - in
//  gd4d_cross_attn_agg_items_coarse_fwd one of its 8 / NS groups of NS consecutive slices, then the projected rows' phase.  Host
//  and device: gd4d_gather_walk runs it without a GPU)
__host__ __device__ __forceinline__ bool sliced_walk(const SlicedParams& p, int block, int& pos, int& sl) {
  const int xcd = block & 7, jb = block >> 3;
  const int per_blk = p.blk * p.slice_n;                   // workgroups of one block of queries
  const int kb = jb / per_blk, rb = jb - kb * per_blk;
  sl = rb / p.blk;
  const int qi = kb * p.blk + (rb - sl * p.blk);
  pos = xcd * p.per_xcd + qi;
  return qi < p.per_xcd && pos < p.BQ;
}

// The wave's LDS patch: [passes of a round][8 corner slots][GP bytes], pair j of slot g at byte 8 j
constexpr int kPatchGP = 80;                     // LDS bytes per corner slot: 64 B of pairs + 16 B pad (conflict-free b128)
constexpr int kPatchPass = 8 * kPatchGP;
constexpr int kPairsCH = 6;                      // pairs form: passes staged per round (30 KB per workgroup of 8 waves: 4 per CU)

typedef float f2v __attribute__((ext_vector_type(2)));

#ifndef GD4D_GATHER_NOLOAD
#define GD4D_GATHER_NOLOAD 0     // 1 (dev builds, timing only - results are wrong): no feature load, a value made of its offset instead
#endif

// One pass of a forward gather: four 16-byte reads of the wave's patch (the 8 lanes of a corner slot read one address: broadcast;
// pairs j = 2 i, 2 i + 1: {off, w, off, w}), up to eight loads of 8 corners x 128 B, then per load two packed FMAs into the lane's
// four channels.  rd = the pass's row of this lane's corner slot; load j = pair j of the slot = (item pair j / LAP, level slot
// j % LAP) of the pass (LAP = 4: 4 items x 4 level slots; 2: 8 items x 2), of which LA level slots are gathered; left = items the
// pass still holds (wave-uniform): load j's pair exists while 2 (j / LAP) < left.  WIDE: the parked offsets are in units of 16 bytes.
template <int LA, int LAP, typename VT, bool WIDE>
__device__ __forceinline__ void gather_pass(const char* rd, const char* const (&base)[LA], const unsigned lane_off, const int left,
                                            f2v& acc0, f2v& acc1) {
  const uint4* row = reinterpret_cast<const uint4*>(rd);
  uint4 pr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) pr[i] = row[i];
  float4 val[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if ((j % LAP) >= LA) continue;
    if (2 * (j / LAP) >= left) break;
    const unsigned raw = (j & 1) ? pr[j >> 1].z : pr[j >> 1].x;
    const unsigned o = raw + lane_off;
    const VT* ap = WIDE ? reinterpret_cast<const VT*>(base[j % LAP] + (((size_t)raw << 4) + lane_off))
                        : reinterpret_cast<const VT*>(base[j % LAP] + o);
#if GD4D_GATHER_NOLOAD
    val[j] = make_float4(__uint_as_float(o), 1.f, 2.f, 3.f); (void)ap;
#else
    val[j] = Quad<VT>::load(ap);
#endif
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if ((j % LAP) >= LA) continue;
    if (2 * (j / LAP) >= left) break;
    const float w = __uint_as_float((j & 1) ? pr[j >> 1].w : pr[j >> 1].y);
    const f2v ww = {w, w};
    acc0 = __builtin_elementwise_fma(ww, f2v{val[j].x, val[j].y}, acc0);
    acc1 = __builtin_elementwise_fma(ww, f2v{val[j].z, val[j].w}, acc1);
  }
}

// the 8 corner slots meet in a fixed order (deterministic): every lane ends with the sums of its four channels
__device__ __forceinline__ float4 sum_corner_slots(const f2v acc0, const f2v acc1) {
  float4 acc = make_float4(acc0.x, acc0.y, acc1.x, acc1.y);
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    acc.x += __shfl_xor(acc.x, o); acc.y += __shfl_xor(acc.y, o);
    acc.z += __shfl_xor(acc.z, o); acc.w += __shfl_xor(acc.w, o);
  }
  return acc;
}

// Host: the arguments every sliced launch takes, checked and filled in.  `io` is the (BQ, HH, 256) array of the call: agg, or
// dL/d agg of the gather-dot (dot = true), where P only sizes the plan (4 or 8, whatever the head count) and the workspace
// (dot_ws_ok) is judged between the strides and the level pointers.
static inline int fill_sliced_params(SlicedParams& p, const void* const* level_ptrs, int64_t slice_stride_bytes, const void* plan,
                                     float* io, int B, int N, int Q, int Hh, int C, int L, int P, int feats_dtype,
                                     const int32_t* query_order, int slice_lo, int slice_n, bool dot = false, bool dot_ws_ok = true) {
  if (!level_ptrs || !plan || !io) return GD4D_EINVAL;
  if (B <= 0 || N <= 0 || Q <= 0 || Hh <= 0 || L <= 0) return GD4D_EINVAL;
  const bool p_ok = dot ? (P == kPoints || P == 8) : ((P == 1 || P == 2 || P == 4 || P == 8) && (P == kPoints || Hh == 8));
  if (C != kChannels || !p_ok || L > 4 || N > 64 || B > 16) return GD4D_EUNSUPPORTED;
  if (feats_dtype != GD4D_F32 && feats_dtype != GD4D_BF16) return GD4D_EUNSUPPORTED;
  if (Hh != 4 && Hh != 8 && Hh != 16) return GD4D_EUNSUPPORTED;
  if (slice_lo < 0 || slice_n <= 0 || slice_lo + slice_n > kSlices) return GD4D_EINVAL;
  if (!aligned16(io) || !aligned16(plan)) return GD4D_EALIGN;
  const int es = feats_dtype == GD4D_BF16 ? 2 : 4;
  if (slice_stride_bytes % (4 * es)) return GD4D_EALIGN;
  if (!dot_ws_ok) return GD4D_EWORKSPACE;
  for (int l = 0; l < L; ++l) {
    if (!level_ptrs[l]) return GD4D_EINVAL;
    if (reinterpret_cast<uintptr_t>(level_ptrs[l]) % (4 * es)) return GD4D_EALIGN;
    p.lvl_base[l] = static_cast<const char*>(level_ptrs[l]);
  }
  for (int l = L; l < 4; ++l) p.lvl_base[l] = p.lvl_base[0];
  p.slice_stride = slice_stride_bytes;
  p.hdr = static_cast<const int*>(plan);
  p.pair = reinterpret_cast<const uint2*>(static_cast<const char*>(plan) + plan_hdr_bytes(B, Q));
  p.order = query_order; p.agg = io;
  p.BQ = B * Q; p.per_xcd = (B * Q + 7) / 8; p.cap_t = plan_cap_t(N, P);
  p.slice_lo = slice_lo; p.slice_n = slice_n;
  p.blk = p.per_xcd;                                // one block = the XCD's whole sector: plain slice-major
  return GD4D_OK;
}

// Host: (Hh in {4, 8, 16}, value type, L in 1 .. 4) of a checked call as compile-time constants:
// f(std::integral_constant<int, HH>, VT{}, std::integral_constant<int, LT>) -> int
template <typename F>
static inline int dispatch_sliced(int Hh, bool bf16, int L, F&& f) {
  auto with_l = [&](auto hh, auto vt) -> int {
    switch (L) {
      case 1: return f(hh, vt, std::integral_constant<int, 1>{});
      case 2: return f(hh, vt, std::integral_constant<int, 2>{});
      case 3: return f(hh, vt, std::integral_constant<int, 3>{});
      default: return f(hh, vt, std::integral_constant<int, 4>{});
    }
  };
  auto with_vt = [&](auto hh) -> int { return bf16 ? with_l(hh, uint16_t{}) : with_l(hh, float{}); };
  switch (Hh) {
    case 4: return with_vt(std::integral_constant<int, 4>{});
    case 8: return with_vt(std::integral_constant<int, 8>{});
    default: return with_vt(std::integral_constant<int, 16>{});
  }
}

}  // namespace gd4d
