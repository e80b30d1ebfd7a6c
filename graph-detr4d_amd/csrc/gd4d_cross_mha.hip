// Dense cross-attention over a long key axis with a key-padding mask: PETR's global cross-attention, where each of ~900 queries
// attends to every pixel of every camera (6 000 - 48 000 keys).
// Reference: projects/mmdet3d_plugin/models/utils/petr_transformer.py (PETRMultiheadAttention.forward -> nn.MultiheadAttention with
// key_padding_mask); the arithmetic is the split-bf16 core's (gd4d_mha_body.h: S^T = K Q^T, base-2 online softmax, O^T += V^T P^T),
// with the scores on six products instead of three (products6, gd4d_attn_pieces.h).
//
// What differs from gd4d_mha_core_fwd, which is shaped for 900 x 900 self-attention:
//   - K (hi, mid, lo) and V (hi, lo) arrive as split-bf16 planes in the MFMA fragment layout, with a batch dimension and any Lk (gd4d_cross_mha_pack_kv writes
//     them once per layer, pad keys of the last step included); a fragment load is 1 KB contiguous per wave.
//   - a workgroup owns NQ 16-query tiles (64 queries by default): every K / V fragment a wave loads feeds NQ tiles, the Q operands of all
//     of them stay in registers.  Its four waves take the key steps of the workgroup's key split round-robin and merge (m, l, O) in LDS.
//   - the keys are split across workgroups as well (15 x 8 workgroups do not fill 256 compute units); a split writes un-normalised
//     (m, l, O) partials and a small merge kernel combines them.  gd4d_cross_mha_plan is the split on the host.
//   - the mask is (B, Lk) bytes, read as 32 bits per key step (KeyStepMask); a step whose bits are all set is skipped.
//   - a row whose every key is masked: out = NaN (0 / 0, as ATen), lse = -inf (the guarded merge of gd4d_attn_pieces.h).
//   - training (gd4d_cross_mha_train_fwd): the TRAIN instantiations take P V on six products as well (P and V as hi + mid + lo; the
//     training pack writes a third V plane) - `out` feeds the out-projection's weight gradient and Dq of the backward, and on three
//     products those were 5 - 7 times as far from the reference as the fp32 torch-op route's - and drop probabilities as
//     gd4d_mha_core_fwd does (gd4d_mha_dropout.h: a function of the seed and the element's index); l and the lse stay those of the
//     full softmax.
// The packs (fp32 rows -> planes) of inference and training are in gd4d_cross_mha_train.hip.
#include "gd4d_cross_mha.h"
#include "gd4d_mha_dropout.h"

namespace gd4d {

struct CrossMhaParams {
  const float* q;
  const unsigned short* kp;       // [plane hi, mid, lo][b][h][step][tile t][lane = 16 (c / 8) + key % 16][8 channels], key = 32 step + 16 t + key % 16
  const unsigned short* vp;       // [plane hi, lo (TRAIN: hi, mid, lo)][b][h][step][half = d / 16][lane = 16 g + d % 16][j] <-> key 32 step + 16 (j >> 2) + 4 g + (j & 3)
  long long plane;                // elements from one plane to the next
  const uint8_t* mask;            // (B, Lk), nonzero = ignore the key; or null
  float* out; float* lse; float* ws;
  int Lq, Lk, B, H, ldq, ldo, steps, splits;
  float qscale;                   // scale * log2(e): base-2 softmax
  const uint32_t* seed;           // TRAIN: two words in device memory, the threshold round(p 2^32) and 1 / (1 - p)
  uint32_t drop_thresh;
  float inv_keep;
};

// partials of the key splits: O (splits, B, H, Lq, 32), then m and l (splits, B, H, Lq) each; row (s, b, h, q) of all three
__device__ __forceinline__ size_t xm_ws_row(const CrossMhaParams& p, int s, int b, int h, int q) {
  return (((size_t)s * p.B + b) * p.H + h) * p.Lq + q;
}

// grid (query blocks of 16 NQ, H * splits, B), 4 waves
template <int NQ, bool TRAIN>
__global__ __launch_bounds__(64 * XM_WAVES, 2) void cross_mha_kernel(const CrossMhaParams p) {
  __shared__ KeySliceShared<XM_WAVES, NQ * 16> sh;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int qi = lane & 15;            // query column of this lane in a score / output tile
  const int g = lane >> 4;
  const int q0 = blockIdx.x * (16 * NQ);
  const int h = blockIdx.y % p.H, split = blockIdx.y / p.H;
  const int b = blockIdx.z;
  const float NEG_INF = -__builtin_inff();

  Planes3 qp[NQ];                      // Q^T as B operand: lane (query qi, g) holds q[qi][8 g .. 8 g + 7] of each tile, in three pieces
#pragma unroll
  for (int t = 0; t < NQ; ++t) {
    const int qrow = min(q0 + 16 * t + qi, p.Lq - 1);
    const float* src = p.q + ((size_t)qrow * p.B + b) * p.ldq + h * XM_D + 8 * g;
    const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
    const float qf[8] = {a.x * p.qscale, a.y * p.qscale, a.z * p.qscale, a.w * p.qscale,
                         c.x * p.qscale, c.y * p.qscale, c.z * p.qscale, c.w * p.qscale};
    qp[t] = split_planes3(qf);
  }
  uint32_t seed_lo = 0, seed_hi = 0, drow[NQ];
  const bool drop = TRAIN && p.drop_thresh != 0u;
  if constexpr (TRAIN) {
    if (drop) { seed_lo = p.seed[0]; seed_hi = p.seed[1]; }
#pragma unroll
    for (int t = 0; t < NQ; ++t) drow[t] = mha_drop_row(b, h, q0 + 16 * t + qi, p.H, p.Lq, p.Lk);
  }
  f32x4 o0[NQ], o1[NQ];                // O^T rows d = 4 g + r, and 16 + 4 g + r
  float m[NQ], l[NQ];
#pragma unroll
  for (int t = 0; t < NQ; ++t) {
    o0[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    o1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[t] = NEG_INF;
    l[t] = 0.f;
  }

  struct StepData { Planes3 k[2], v[2]; KeyStepMask mask; };
  auto fetch = [&](const int step, StepData& d) {                   // step in [s_first, s_last): every fragment of it was written
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const size_t e = xm_frag(p.H, p.steps, b, h, step, t, lane);
      d.k[t] = load_planes(p.kp, p.plane, e);
      d.v[t] = load_planes<TRAIN ? 3 : 2>(p.vp, p.plane, e);
    }
    d.mask.fetch(p.mask, b, p.Lk, step, lane);
  };
  auto compute = [&](const int step, const StepData& d) {
    const unsigned bits = d.mask.bits();
    if (bits == 0xffffffffu) return;                                  // nothing to see in this step: (m, l, O) stay as they are
    const unsigned mb = KeyStepMask::of_lane(bits, g);
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
      // ---- S^T = K Q^T, two tiles of 16 keys: lane (qi, g) register r <-> key 16 kt + 4 g + r of the step ----
      float pr[8];                                                     // the scores, then their probabilities
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const f32x4 st = products6(d.k[kt], qp[t]);                    // (the probabilities below 1 and P V in inference do not need six)
#pragma unroll
        for (int r = 0; r < 4; ++r) pr[4 * kt + r] = st[r];
      }
      if (bits != 0u) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if ((mb >> (16 * (j >> 2) + (j & 3))) & 1u) pr[j] = NEG_INF;
      }
      const float corr = softmax_step<8, false>(pr, m[t], l[t]);       // no guard: the step has an unmasked key, m_new is finite
      if (drop) {                                                      // (after l: the lse is the full softmax's)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t key = (uint32_t)(32 * step + 16 * (j >> 2) + 4 * g + (j & 3));
          pr[j] = mha_drop_keep(seed_lo, seed_hi, drow[t] + key, p.drop_thresh) ? pr[j] * p.inv_keep : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) { o0[t][r] *= corr; o1[t][r] *= corr; }
      // ---- O^T += V^T P^T: A = V^T[d = lane & 15 (+ 16)][k = 8 g + j], B = P^T = this lane's own eight probabilities ----
      if constexpr (TRAIN) {
        const Planes3 pp = split_planes3(pr);
        o0[t] = xm_x6(d.v[0], pp, o0[t]);
        o1[t] = xm_x6(d.v[1], pp, o1[t]);
      } else {
        u32x4 ph, pl;                                                  // d.v[].m was not loaded (load_planes<2>): h and l only here
        split8(pr, ph, pl);
        o0[t] = mfma_16x16x32_x3(d.v[0].h, d.v[0].l, ph, pl, o0[t]);
        o1[t] = mfma_16x16x32_x3(d.v[1].h, d.v[1].l, ph, pl, o1[t]);
      }
    }
  };
  walk_steps<XM_WAVES, StepData>(xm_split_first(p.steps, p.splits, split), xm_split_first(p.steps, p.splits, split + 1), wave, fetch, compute);

  // ---- merge the waves' key slices (guarded: a wave that saw no unmasked key holds (-inf, 0, 0)); one split writes out / lse,
  //      several write their un-normalised (mm, den, num) for cross_mha_merge_kernel ----
#pragma unroll
  for (int t = 0; t < NQ; ++t) publish_key_slice(sh, wave, 16 * t + qi, g, m[t], l[t], o0[t], o1[t]);
  merge_key_slices<true>(sh, tid, p.Lq - q0, [&](int i, int d, float mm, float num, float den) {
    if (p.splits == 1) {
      store_attn(p.out, p.lse, (size_t)(q0 + i) * p.B + b, p.ldo, p.H, h, d, mm, num, den);
    } else {
      const size_t row = xm_ws_row(p, split, b, h, q0 + i), rows = (size_t)p.splits * p.B * p.H * p.Lq;
      p.ws[row * XM_D + d] = num;
      if (d == 0) {
        p.ws[rows * XM_D + row] = mm;
        p.ws[rows * (XM_D + 1) + row] = den;
      }
    }
  });
}

// the key splits' partials -> out, lse: one thread per (query, batch, head, channel)
__global__ __launch_bounds__(256) void cross_mha_merge_kernel(const CrossMhaParams p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)p.Lq * p.B * p.H * XM_D) return;
  const int d = (int)(e % XM_D);
  const int h = (int)(e / XM_D % p.H);
  const int b = (int)(e / XM_D / p.H % p.B);
  const int q = (int)(e / XM_D / p.H / p.B);
  const size_t rows = (size_t)p.splits * p.B * p.H * p.Lq;
  const float* ms = p.ws + rows * XM_D;
  const float* ls = ms + rows;
  float mm, num, den;
  combine_key_slices<true>(p.splits, [&](int s) { return ms[xm_ws_row(p, s, b, h, q)]; }, [&](int s) { return ls[xm_ws_row(p, s, b, h, q)]; },
                           [&](int s) { return p.ws[xm_ws_row(p, s, b, h, q) * XM_D + d]; }, mm, num, den);
  store_attn(p.out, p.lse, (size_t)q * p.B + b, p.ldo, p.H, h, d, mm, num, den);
}

}  // namespace gd4d

extern "C" int gd4d_cross_mha_plan(int Lq, int Lk, int B, int H, int q_tile, int splits, int32_t* plan) {
  using namespace gd4d;
  int qt, s;
  if (!plan) return GD4D_EINVAL;
  const int rc = xm_plan(Lq, Lk, B, H, q_tile, splits, &qt, &s);
  if (rc != GD4D_OK) return rc;
  const int steps = (Lk + 31) / 32;
  plan[0] = qt; plan[1] = s; plan[2] = steps;
  plan[3] = (Lq + qt - 1) / qt; plan[4] = H * s; plan[5] = B;
  for (int i = 0; i <= s; ++i) plan[6 + i] = xm_split_first(steps, s, i);
  return GD4D_OK;
}

extern "C" size_t gd4d_cross_mha_plane_elems(int Lk, int B, int H) {
  if (Lk <= 0 || B <= 0 || H <= 0) return 0;
  return (size_t)B * H * ((Lk + 31) / 32) * 2 * 64 * 8;
}

extern "C" size_t gd4d_cross_mha_workspace_bytes(int Lq, int Lk, int B, int H, int q_tile, int splits) {
  int qt, s;
  if (gd4d::xm_plan(Lq, Lk, B, H, q_tile, splits, &qt, &s) != GD4D_OK || s == 1) return 0;
  return (size_t)s * B * H * Lq * (gd4d::XM_D + 2) * sizeof(float);
}

namespace gd4d {

static int cross_mha_launch(const float* q, const void* k_planes, const void* v_planes, long long plane_stride,
                            const void* key_padding_mask, float* out, float* lse, void* workspace, size_t workspace_bytes,
                            int Lq, int Lk, int B, int H, int D, int ldq, int ldo, float scale, int q_tile, int splits,
                            bool train, float drop_p, const void* seed, void* stream) {
  if (!q || !k_planes || !v_planes || !out || Lq <= 0 || Lk <= 0 || B <= 0 || H <= 0) return GD4D_EINVAL;
  int rc = attn_check_drop(drop_p, seed, (double)B * H * Lq * Lk);      // (the inference entry point passes drop_p = 0)
  if (rc != GD4D_OK) return rc;
  if (D != XM_D || H != 8) return GD4D_EUNSUPPORTED;
  if (train) {                                        // six products for P V and a third V plane: the 64-query tile would spill
    if (q_tile == 64) return GD4D_EUNSUPPORTED;
    if (q_tile == 0) q_tile = 32;
  }
  int qt, s;
  rc = xm_plan(Lq, Lk, B, H, q_tile, splits, &qt, &s);
  if (rc != GD4D_OK) return rc;
  rc = xm_check_layout(ldq < ldo ? ldq : ldo, plane_stride, Lk, B, H, aligned16(q) && !(ldq % 4) && aligned16(k_planes) && aligned16(v_planes));
  if (rc != GD4D_OK) return rc;
  const size_t need = gd4d_cross_mha_workspace_bytes(Lq, Lk, B, H, qt, s);
  if (need && (!workspace || workspace_bytes < need)) return GD4D_EWORKSPACE;
  CrossMhaParams p{q, static_cast<const unsigned short*>(k_planes), static_cast<const unsigned short*>(v_planes), plane_stride,
                   static_cast<const uint8_t*>(key_padding_mask), out, lse, static_cast<float*>(workspace),
                   Lq, Lk, B, H, ldq, ldo, (Lk + 31) / 32, s, scale * ATTN_LOG2E,
                   static_cast<const uint32_t*>(seed), mha_drop_thresh(drop_p), 1.f / (1.f - drop_p)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((Lq + qt - 1) / qt, H * s, B), block(64 * XM_WAVES);
  if (train) {
    hipLaunchKernelGGL((cross_mha_kernel<2, true>), grid, block, 0, st, p);
  } else {
    if (qt == 64) hipLaunchKernelGGL((cross_mha_kernel<4, false>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((cross_mha_kernel<2, false>), grid, block, 0, st, p);
  }
  if (s > 1) {
    const size_t n = (size_t)Lq * B * H * XM_D;
    hipLaunchKernelGGL(cross_mha_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  }
  return check_launch();
}

}  // namespace gd4d

extern "C" int gd4d_cross_mha_fwd(const float* q, const void* k_planes, const void* v_planes, long long plane_stride,
                                  const void* key_padding_mask, float* out, float* lse, void* workspace, size_t workspace_bytes,
                                  int Lq, int Lk, int B, int H, int D, int ldq, int ldo, float scale, int q_tile, int splits,
                                  void* stream) {
  return gd4d::cross_mha_launch(q, k_planes, v_planes, plane_stride, key_padding_mask, out, lse, workspace, workspace_bytes, Lq, Lk, B,
                                H, D, ldq, ldo, scale, q_tile, splits, false, 0.f, nullptr, stream);
}

extern "C" int gd4d_cross_mha_train_fwd(const float* q, const void* k_planes, const void* v_planes, long long plane_stride,
                                        const void* key_padding_mask, float* out, float* lse, void* workspace,
                                        size_t workspace_bytes, int Lq, int Lk, int B, int H, int D, int ldq, int ldo, float scale,
                                        int q_tile, int splits, float drop_p, const void* seed, void* stream) {
  return gd4d::cross_mha_launch(q, k_planes, v_planes, plane_stride, key_padding_mask, out, lse, workspace, workspace_bytes, Lq, Lk, B,
                                H, D, ldq, ldo, scale, q_tile, splits, true, drop_p, seed, stream);
}
