// gd4d_mha_core_fwd: softmax(q k^T / sqrt(d) [+ mask]) v for the decoder self-attention, gfx950.
//
// Reference: third-party mmcv MultiheadAttention -> nn.MultiheadAttention (config call site
// projects/configs/detr4d/detr4d_res50_deform_pe_testaug_320_fullset_ceph.py:74-78); H-DETR passes a
// boolean self-attention mask (h_detr3d_transformer.py:149-157).  The packed in-projection and the
// out-projection are gd4d_linear_fwd launches; this kernel is the part in between and never
// materialises the (heads, Q, Q) score tensor the reference writes and re-reads.
//
// Which kernel runs: without dropout the split-bf16 body of gd4d_mha_body.h (inference, and training in eval mode: it writes the
// log-sum-exp when asked), on fp32 K / V rows or on pre-split planes; with dropout on fp32 rows the fp32 kernel below, on planes
// the body again (it carries DROP there).  GD4D_MHA_FP32=1 runs the fp32 kernel without dropout too.
//
// The fp32 kernel: everything on v_mfma_f32_16x16x4_f32 (exact fp32 products).  One workgroup = 8 waves =
// one (batch, head, 16-query tile); the waves split the keys 8 ways (flash-decoding style) and merge
// their (max, sum, O) triples through LDS (gd4d_attn_pieces.h).
//
// Layout trick: the scores are computed TRANSPOSED, S^T = K Q^T (MFMA rows = keys, cols = queries),
// with MFMA row rho of a 16-key tile holding key (rho>>2) + 4*(rho&3).  The C/D layout then leaves
// lane (query i = lane&15, g = lane>>4), register r with key g + 4r - which is exactly the
// B-operand layout (k = g + 4s at step s) of the second product O^T = V^T P^T.  The probabilities
// never move between lanes; the softmax reductions are 4 in-lane values + two xor-shuffles.
#include <stdlib.h>

#include <type_traits>

#include "gd4d_common.h"
#include "gd4d_mha_dropout.h"
#include "gd4d_mha_body.h"

namespace gd4d {


GD4D_TRACE_UNIT(mha)

// DROP: each probability is kept with chance 1 - p and scaled by 1 / (1 - p) before it multiplies v, as F.dropout on the
// softmax output inside nn.MultiheadAttention; the normaliser (and the saved log-sum-exp) are those of the full softmax.
// MASK: 0 none, 1 bool, 2 additive float (compile-time: the unmasked kernel of the decoder carries neither the registers nor
// the branches).  A tile's four mask entries are requested with its K rows and V columns - read where they are used, per
// score, each was a branch with its own load and wait (28.7 us per layer with H-DETR's mask against 20.8 without).
template <bool DROP, int MASK>
__global__ __launch_bounds__(64 * MHA_WAVES) void mha_core_kernel(const MhaParams p) {
  trace_mark(g_trace_mha, 2ull);
  __shared__ MhaShared sh;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int qi = lane & 15;            // query column of this lane
  const int g = lane >> 4;             // lane group
  const int q0 = blockIdx.x * 16;
  const int h = blockIdx.y, b = blockIdx.z;
  const float NEG_INF = -__builtin_inff();
  const float qscale = p.scale * ATTN_LOG2E;     // base-2 softmax (softmax_step); an additive mask is scaled like the scores

  // Q^T as B operand: lane (col = query qi, g) holds q[qi][8g + s] at k-step s (any k<->dim map works
  // as long as A uses the same one).  Rows beyond Lq are clamped (their outputs are never written).
  float qf[8];
  {
    const int qrow = min(q0 + qi, p.Lq - 1);
    const float* src = p.q + ((size_t)qrow * p.B + b) * p.ldq + h * MHA_D + 8 * g;
    const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
    qf[0] = a.x * qscale; qf[1] = a.y * qscale; qf[2] = a.z * qscale; qf[3] = a.w * qscale;
    qf[4] = c.x * qscale; qf[5] = c.y * qscale; qf[6] = c.z * qscale; qf[7] = c.w * qscale;
  }
  const int krho = (qi >> 2) + 4 * (qi & 3);     // key (within a tile) held by MFMA row rho = lane&15

  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};    // O^T rows d = 4g + r, and 16 + 4g + r
  float m = NEG_INF, l = 0.f;                                     // running max (per query), partial sum (per lane)

  const int ntiles = (p.Lk + 15) / 16;
  const size_t hoff = (size_t)h * MHA_D;
  uint32_t seed_lo = 0, seed_hi = 0, drop_row = 0;
  if (DROP) {
    seed_lo = p.seed[0]; seed_hi = p.seed[1];
    drop_row = mha_drop_row(b, h, min(q0 + qi, p.Lq - 1), p.H, p.Lq, p.Lk);
  }
  const size_t mask_row = (size_t)min(q0 + qi, p.Lq - 1) * p.Lk;
  // A wave takes its tiles of 16 keys one at a time, a tile's mask entries, K rows and V columns requested together and nothing
  // ahead of the tile: q / k / v arrive cold from another XCD (~2 us per round trip), but at 65 - 81 registers (the table of
  // docs/measurements_r41.md) three workgroups share a compute unit and hide that better than a deeper request queue in this one did (the sweep: docs/measurements_r41.md).
  for (int kt = wave; kt < ntiles; kt += MHA_WAVES) {
    const int kbase = kt * 16;
    float4 ka, kc;
    float vv[8], mk[4];
    if (MASK) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t mi = mask_row + min(kbase + g + 4 * r, p.Lk - 1);
        if (MASK == 1) mk[r] = static_cast<const uint8_t*>(p.mask)[mi] ? 1.f : 0.f;
        else mk[r] = static_cast<const float*>(p.mask)[mi];
      }
    }
    {
      const int krow = min(kbase + krho, p.Lk - 1);
      const float* src = p.k + ((size_t)krow * p.B + b) * p.ldk + hoff + 8 * g;
      ka = *reinterpret_cast<const float4*>(src);
      kc = *reinterpret_cast<const float4*>(src + 4);
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int vrow = min(kbase + g + 4 * st, p.Lk - 1);      // out-of-range keys get probability 0
      const float* vs = p.v + ((size_t)vrow * p.B + b) * p.ldv + hoff + qi;
      vv[2 * st] = vs[0];
      vv[2 * st + 1] = vs[16];
    }
    // ---- S^T = K Q^T ----
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.x, qf[0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.y, qf[1], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.z, qf[2], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.w, qf[3], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(kc.x, qf[4], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(kc.y, qf[5], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(kc.z, qf[6], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(kc.w, qf[7], s, 0, 0, 0);
    float pr[4];                                                 // lane (qi, g) reg r  <->  key kbase + g + 4r: its score, then its probability
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kbase + g + 4 * r;
      float val = s[r];
      if (key >= p.Lk) {
        val = NEG_INF;
      } else if (MASK == 1) {
        if (mk[r] != 0.f) val = NEG_INF;
      } else if (MASK == 2) {
        val += mk[r] * ATTN_LOG2E;
      }
      pr[r] = val;
    }
    const float corr = softmax_step(pr, m, l);
    if (DROP) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        pr[r] = mha_drop_keep(seed_lo, seed_hi, drop_row + (uint32_t)(kbase + g + 4 * r), p.drop_thresh) ? pr[r] * p.inv_keep : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { o0[r] *= corr; o1[r] *= corr; }
    // ---- O^T += V^T P^T : A = V^T[d = lane&15 (+16)][key = kbase + g + 4s], B = P^T = pr[s] ----
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[2 * st], pr[st], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[2 * st + 1], pr[st], o1, 0, 0, 0);
    }
  }
  mha_merge_and_store(p, sh, q0, h, b, m, l, o0, o1);
  trace_mark(g_trace_mha, 0x82ull);
}


// The split-bf16 form on fp32 K / V rows (no dropout): gd4d_mha_body.h
template <int MASK>
__global__ __launch_bounds__(64 * MHA_WAVES) void mha_core_bf16x3_kernel(const MhaParams p) {
  trace_mark(g_trace_mha, 2ull);
  __shared__ MhaShared sh;
  mha_core_bf16x3_body<MASK>(p, blockIdx.x, blockIdx.y, blockIdx.z, sh);
  trace_mark(g_trace_mha, 0x82ull);
}

// ... with K and V as pre-split bf16 planes (written by the in-projection: GD4D_CHAIN_SPLIT_KV); batch 1
template <int MASK, bool DROP>
__global__ __launch_bounds__(64 * MHA_WAVES) void mha_core_presplit_kernel(const MhaParams p) {
  trace_mark(g_trace_mha, 2ull);
  __shared__ MhaShared sh;
  mha_core_bf16x3_body<MASK, true, DROP>(p, blockIdx.x, blockIdx.y, 0, sh);
  trace_mark(g_trace_mha, 0x82ull);
}

// launch(MASK, DROP) with the two run-time choices as compile-time constants (std::integral_constant)
template <class Launch>
static void mha_dispatch(const int mask_kind, const bool drop, Launch launch) {
  auto with_drop = [&](auto mask) {
    if (drop) launch(mask, std::true_type{});
    else launch(mask, std::false_type{});
  };
  if (mask_kind == 0) with_drop(std::integral_constant<int, 0>{});
  else if (mask_kind == 1) with_drop(std::integral_constant<int, 1>{});
  else with_drop(std::integral_constant<int, 2>{});
}

// What both entry points refuse first, in this order; `present`: their own pointers and sizes, `elements`: B H Lq Lk
static int mha_check_args(const bool present, const float drop_p, const void* seed, const double elements, const int D,
                          const int mask_kind, const void* mask) {
  if (!present) return GD4D_EINVAL;
  const int rc = attn_check_drop(drop_p, seed, elements);
  if (rc != GD4D_OK) return rc;
  if (D != MHA_D || mask_kind < 0 || mask_kind > 2 || (mask_kind && !mask)) return GD4D_EUNSUPPORTED;
  return GD4D_OK;
}

}  // namespace gd4d

extern "C" void gd4d_trace_set_mha(unsigned long long* p) { gd4d::trace_set_mha(p); }

extern "C" int gd4d_mha_core_fwd(const float* q, const float* k, const float* v, const void* mask,
                                 float* out, int Lq, int Lk, int B, int H, int D, int ldq, int ldk,
                                 int ldv, int ldo, int mask_kind, float scale, float* lse, float drop_p, const void* seed,
                                 void* stream) {
  using namespace gd4d;
  const int rc = mha_check_args(q && k && v && out && Lq > 0 && Lk > 0 && B > 0 && H > 0, drop_p, seed, (double)B * H * Lq * Lk, D,
                                mask_kind, mask);
  if (rc != GD4D_OK) return rc;
  if (ldq < H * D || ldk < H * D || ldv < H * D || ldo < H * D) return GD4D_EINVAL;
  if (!aligned16(q) || !aligned16(k) || (ldq % 4) || (ldk % 4)) return GD4D_EALIGN;
  MhaParams p{q, k, v, mask, out, lse, Lq, Lk, B, H, ldq, ldk, ldv, ldo, mask_kind, scale,
              static_cast<const uint32_t*>(seed), mha_drop_thresh(drop_p), 1.f / (1.f - drop_p)};
  const dim3 grid((Lq + 15) / 16, H, B), block(64 * MHA_WAVES);
  hipStream_t st = static_cast<hipStream_t>(stream);
  static const bool fp32_only = [] { const char* e = getenv("GD4D_MHA_FP32"); return e && e[0] == '1'; }();
  mha_dispatch(mask_kind, drop_p > 0.f, [&](auto mask_c, auto drop_c) {
    constexpr int MASK = decltype(mask_c)::value;
    constexpr bool DROP = decltype(drop_c)::value;
    if (!DROP && !fp32_only) hipLaunchKernelGGL((mha_core_bf16x3_kernel<MASK>), grid, block, 0, st, p);      // split-bf16 x3 products
    else hipLaunchKernelGGL((mha_core_kernel<DROP, MASK>), grid, block, 0, st, p);
  });
  return check_launch();
}

extern "C" int gd4d_mha_core_presplit_fwd(const float* q, const void* k_planes, const void* v_planes, float* out, int L, int H, int D,
                                          int ldq, int ldo, long long k_plane_stride, long long v_plane_stride, const void* mask,
                                          int mask_kind, float scale, float* lse, float drop_p, const void* seed, void* stream) {
  using namespace gd4d;
  const int rc = mha_check_args(q && k_planes && v_planes && out && L > 0 && H > 0, drop_p, seed, (double)H * L * L, D, mask_kind, mask);
  if (rc != GD4D_OK) return rc;
  const long long tiles = (L + 15) / 16, steps = (L + 31) / 32;
  if (ldq < H * D || ldo < H * D || k_plane_stride < H * tiles * 512 || v_plane_stride < H * steps * 1024 ||
      (k_plane_stride & 7) || (v_plane_stride & 7))
    return GD4D_EINVAL;
  if (!aligned16(q) || (ldq % 4) || !aligned16(k_planes) || !aligned16(v_planes)) return GD4D_EALIGN;
  MhaParams p{q, nullptr, nullptr, mask, out, lse, L, L, 1, H, ldq, 0, 0, ldo, mask_kind, scale,
              static_cast<const uint32_t*>(seed), mha_drop_thresh(drop_p), 1.f / (1.f - drop_p),
              static_cast<const unsigned short*>(k_planes), static_cast<const unsigned short*>(v_planes), k_plane_stride, v_plane_stride};
  const dim3 grid((L + 15) / 16, H, 1), block(64 * MHA_WAVES);
  hipStream_t st = static_cast<hipStream_t>(stream);
  mha_dispatch(mask_kind, drop_p > 0.f, [&](auto mask_c, auto drop_c) {
    hipLaunchKernelGGL((mha_core_presplit_kernel<decltype(mask_c)::value, decltype(drop_c)::value>), grid, block, 0, st, p);
  });
  return check_launch();
}
