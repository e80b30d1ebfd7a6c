// Dense cross-attention over a long key axis with a key-padding mask: PETR's global cross-attention, where each of ~900 queries
// attends to every pixel of every camera (6 000 - 48 000 keys).
// Reference: projects/mmdet3d_plugin/models/utils/petr_transformer.py (PETRMultiheadAttention.forward -> nn.MultiheadAttention with
// key_padding_mask); the arithmetic is the split-bf16 core's (gd4d_mha_body.h: S^T = K Q^T, base-2 online softmax, O^T += V^T P^T),
// with the scores on six products instead of three (see the step).
//
// What differs from gd4d_mha_core_fwd, which is shaped for 900 x 900 self-attention:
//   - K (hi, mid, lo) and V (hi, lo) arrive as split-bf16 planes in the MFMA fragment layout, with a batch dimension and any Lk (gd4d_cross_mha_pack_kv writes
//     them once per layer, pad keys of the last step included); a fragment load is 1 KB contiguous per wave.
//   - a workgroup owns NQ 16-query tiles (64 queries by default): every K / V fragment a wave loads feeds NQ tiles, the Q operands of all
//     of them stay in registers.  Its four waves take the key steps of the workgroup's key split round-robin and merge (m, l, O) in LDS.
//   - the keys are split across workgroups as well (15 x 8 workgroups do not fill 256 compute units); a split writes un-normalised
//     (m, l, O) partials and a small merge kernel combines them.  gd4d_cross_mha_plan is the split on the host.
//   - the mask is (B, Lk) bytes: 32 lanes read one byte each per key step, a ballot turns them into the step's 32 mask bits (keys past
//     Lk are folded in as masked), a step whose bits are all set is skipped.
//   - training (gd4d_cross_mha_train_fwd): the TRAIN instantiations take P V on six products as well (P and V as hi + mid + lo; the
//     training pack writes a third V plane) - `out` feeds the out-projection's weight gradient and Dq of the backward, and on three
//     products those were 5 - 7 times as far from the reference as the fp32 torch-op route's - and drop probabilities as
//     gd4d_mha_core_fwd does (gd4d_mha_dropout.h: a function of the seed and the element's index); l and the lse stay those of the
//     full softmax.
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

// partials of the key splits: O (splits, B, H, Lq, 32), then m and l (splits, B, H, Lq) each
__host__ __device__ inline size_t xm_ws_o(const int B, const int H, const int Lq, int s, int b, int h) {
  return (((size_t)s * B + b) * H + h) * Lq * XM_D;
}

template <int NQ>
struct XmShared {
  float m[XM_WAVES][NQ * 16];
  float l[XM_WAVES][NQ * 16];
  float o[XM_WAVES][NQ * 16][XM_D + 1];
};

// grid (query blocks of 16 NQ, H * splits, B), 4 waves
template <int NQ, bool TRAIN>
__global__ __launch_bounds__(64 * XM_WAVES, 2) void cross_mha_kernel(const CrossMhaParams p) {
  __shared__ XmShared<NQ> sh;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int qi = lane & 15;            // query column of this lane in a score / output tile
  const int g = lane >> 4;
  const int q0 = blockIdx.x * (16 * NQ);
  const int h = blockIdx.y % p.H, split = blockIdx.y / p.H;
  const int b = blockIdx.z;
  const float NEG_INF = -__builtin_inff();
  constexpr float LN2 = 0.6931471805599453f;

  u32x4 qh[NQ], qm[NQ], ql[NQ];        // Q^T as B operand: lane (query qi, g) holds q[qi][8 g .. 8 g + 7] of each tile, in three pieces
#pragma unroll
  for (int t = 0; t < NQ; ++t) {
    const int qrow = min(q0 + 16 * t + qi, p.Lq - 1);
    const float* src = p.q + ((size_t)qrow * p.B + b) * p.ldq + h * XM_D + 8 * g;
    const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
    const float qf[8] = {a.x * p.qscale, a.y * p.qscale, a.z * p.qscale, a.w * p.qscale,
                         c.x * p.qscale, c.y * p.qscale, c.z * p.qscale, c.w * p.qscale};
    split8x3(qf, qh[t], qm[t], ql[t]);
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

  const int s_first = xm_split_first(p.steps, p.splits, split), s_last = xm_split_first(p.steps, p.splits, split + 1);
  const size_t frag0 = ((size_t)b * p.H + h) * p.steps * 2;          // in fragments of 64 lanes x 8 bf16
  struct StepData { u32x4 kh[2], km[2], kl[2], vh[2], vm[2], vl[2]; unsigned mk; int step; };
  auto fetch = [&](const int step, StepData& d) {                   // step in [s_first, s_last): every fragment of it was written
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const size_t e = ((frag0 + (size_t)step * 2 + t) * 64 + lane) * 8;
      d.kh[t] = *reinterpret_cast<const u32x4*>(p.kp + e);
      d.km[t] = *reinterpret_cast<const u32x4*>(p.kp + p.plane + e);
      d.kl[t] = *reinterpret_cast<const u32x4*>(p.kp + 2 * p.plane + e);
      d.vh[t] = *reinterpret_cast<const u32x4*>(p.vp + e);
      if constexpr (TRAIN) {
        d.vm[t] = *reinterpret_cast<const u32x4*>(p.vp + p.plane + e);
        d.vl[t] = *reinterpret_cast<const u32x4*>(p.vp + 2 * p.plane + e);
      } else {
        d.vl[t] = *reinterpret_cast<const u32x4*>(p.vp + p.plane + e);
      }
    }
    const int key = step * 32 + (lane & 31);                          // one mask byte per key; a key past Lk counts as masked
    d.mk = key >= p.Lk ? 1u : (p.mask ? (unsigned)p.mask[(size_t)b * p.Lk + key] : 0u);
    d.step = step;
  };
  auto compute = [&](const StepData& d) {
    const unsigned bits = (unsigned)__ballot(d.mk != 0);              // wave-uniform: bit i <-> key 32 step + i
    if (bits == 0xffffffffu) return;                                  // nothing to see in this step: (m, l, O) stay as they are
    const unsigned mb = bits >> (4 * g);                              // bit 16 t + r <-> this lane's score register r of key tile t
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
      // ---- S^T = K Q^T, two tiles of 16 keys: lane (qi, g) register r <-> key 16 kt + 4 g + r of the step ----
      float sc[8];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        // six products, smallest terms first (x = hi + mid + lo holds fp32 to ~2^-24: the arithmetic of GD4D_CHAIN_EXACT).  Three
        // products hold a score to ~2^-17 of the sum of its terms' magnitudes - 1.6e-4 on a score of 57, which is the log-sum-exp
        // of a row one key dominates; the probabilities below 1 and the second product do not need it.
        f32x4 st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(d.km[kt]), frag(qm[t]), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(d.kl[kt]), frag(qh[t]), st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(d.kh[kt]), frag(ql[t]), st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(d.km[kt]), frag(qh[t]), st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(d.kh[kt]), frag(qm[t]), st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(d.kh[kt]), frag(qh[t]), st, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[4 * kt + r] = st[r];
      }
      if (bits != 0u) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if ((mb >> (16 * (j >> 2) + (j & 3))) & 1u) sc[j] = NEG_INF;
      }
      float tmax = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), fmaxf(fmaxf(sc[4], sc[5]), fmaxf(sc[6], sc[7])));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float m_new = fmaxf(m[t], tmax);                           // finite: the step has an unmasked key
      const float corr = __builtin_amdgcn_exp2f(m[t] - m_new);         // m = -inf -> 0
      float pr[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pr[j] = __builtin_amdgcn_exp2f(sc[j] - m_new);
      l[t] = l[t] * corr + (((pr[0] + pr[1]) + (pr[2] + pr[3])) + ((pr[4] + pr[5]) + (pr[6] + pr[7])));
      m[t] = m_new;
      if (drop) {                                                      // (after l: the lse is the full softmax's)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t key = (uint32_t)(32 * d.step + 16 * (j >> 2) + 4 * g + (j & 3));
          pr[j] = mha_drop_keep(seed_lo, seed_hi, drow[t] + key, p.drop_thresh) ? pr[j] * p.inv_keep : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) { o0[t][r] *= corr; o1[t][r] *= corr; }
      // ---- O^T += V^T P^T: A = V^T[d = lane & 15 (+ 16)][k = 8 g + j], B = P^T = this lane's own eight probabilities ----
      if constexpr (TRAIN) {
        u32x4 ph, pm, pl;
        split8x3(pr, ph, pm, pl);
        o0[t] = xm_x6(d.vh[0], d.vm[0], d.vl[0], ph, pm, pl, o0[t]);
        o1[t] = xm_x6(d.vh[1], d.vm[1], d.vl[1], ph, pm, pl, o1[t]);
      } else {
        u32x4 ph, pl;
        split8(pr, ph, pl);
        o0[t] = mfma_16x16x32_x3(d.vh[0], d.vl[0], ph, pl, o0[t]);
        o1[t] = mfma_16x16x32_x3(d.vh[1], d.vl[1], ph, pl, o1[t]);
      }
    }
  };
  {
    StepData cur, nxt;                                                // one step of look-ahead, as the self-attention core
    if (s_first + wave < s_last) fetch(s_first + wave, cur);
    for (int step = s_first + wave; step < s_last; step += XM_WAVES) {
      if (step + XM_WAVES < s_last) fetch(step + XM_WAVES, nxt);
      compute(cur);
      cur = nxt;
    }
  }

  // ---- merge the waves' key slices.  A wave that saw no unmasked key holds (m = -inf, l = 0, O = 0): its factor must be 0, and
  //      exp2(-inf - -inf) is NaN, so the common maximum is replaced by 0 when it is -inf itself ----
#pragma unroll
  for (int t = 0; t < NQ; ++t) {
    float lt = l[t];
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    if (g == 0) { sh.m[wave][16 * t + qi] = m[t]; sh.l[wave][16 * t + qi] = lt; }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sh.o[wave][16 * t + qi][4 * g + r] = o0[t][r];
      sh.o[wave][16 * t + qi][16 + 4 * g + r] = o1[t][r];
    }
  }
  __syncthreads();
  for (int e = tid; e < NQ * 16 * XM_D; e += 64 * XM_WAVES) {
    const int i = e / XM_D, d = e % XM_D;
    if (q0 + i >= p.Lq) continue;
    float mm = sh.m[0][i];
#pragma unroll
    for (int w = 1; w < XM_WAVES; ++w) mm = fmaxf(mm, sh.m[w][i]);
    const float m_use = (mm == NEG_INF) ? 0.f : mm;
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < XM_WAVES; ++w) {
      const float f = __builtin_amdgcn_exp2f(sh.m[w][i] - m_use);
      num += sh.o[w][i][d] * f;
      den += sh.l[w][i] * f;
    }
    if (p.splits == 1) {
      p.out[((size_t)(q0 + i) * p.B + b) * p.ldo + h * XM_D + d] = num / den;       // every key masked: 0 / 0 = NaN, as ATen
      if (p.lse && d == 0) p.lse[((size_t)(q0 + i) * p.B + b) * p.H + h] = mm * LN2 + logf(den);
    } else {
      const size_t row = xm_ws_o(p.B, p.H, p.Lq, split, b, h) / XM_D + (q0 + i);
      p.ws[row * XM_D + d] = num;
      if (d == 0) {
        float* ml = p.ws + (size_t)p.splits * p.B * p.H * p.Lq * XM_D;
        ml[row] = mm;
        ml[(size_t)p.splits * p.B * p.H * p.Lq + row] = den;
      }
    }
  }
}

// the key splits' partials -> out, lse: one thread per (query, batch, head, channel)
__global__ __launch_bounds__(256) void cross_mha_merge_kernel(const CrossMhaParams p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)p.Lq * p.B * p.H * XM_D) return;
  const int d = (int)(e % XM_D);
  const int h = (int)(e / XM_D % p.H);
  const int b = (int)(e / XM_D / p.H % p.B);
  const int q = (int)(e / XM_D / p.H / p.B);
  const float NEG_INF = -__builtin_inff();
  constexpr float LN2 = 0.6931471805599453f;
  const size_t rows = (size_t)p.splits * p.B * p.H * p.Lq;
  const float* ms = p.ws + rows * XM_D;
  const float* ls = ms + rows;
  float mm = NEG_INF;
  for (int s = 0; s < p.splits; ++s) mm = fmaxf(mm, ms[xm_ws_o(p.B, p.H, p.Lq, s, b, h) / XM_D + q]);
  const float m_use = (mm == NEG_INF) ? 0.f : mm;                      // (as in the kernel above)
  float num = 0.f, den = 0.f;
  for (int s = 0; s < p.splits; ++s) {
    const size_t row = xm_ws_o(p.B, p.H, p.Lq, s, b, h) / XM_D + q;
    const float f = __builtin_amdgcn_exp2f(ms[row] - m_use);
    num += p.ws[row * XM_D + d] * f;
    den += ls[row] * f;
  }
  p.out[((size_t)q * p.B + b) * p.ldo + h * XM_D + d] = num / den;     // every key of the row masked: NaN
  if (p.lse && d == 0) p.lse[((size_t)q * p.B + b) * p.H + h] = mm * LN2 + logf(den);
}

// fp32 K rows and V rows -> the planes.  grid (steps, 2 = K | V, B), 4 waves: a wave writes whole fragments (1 KB contiguous per
// plane); a K fragment reads 16 rows x 128 contiguous bytes, a V fragment 32 rows x 64.  Keys past Lk are written as zeros.
struct CrossPackParams {
  const float* k; const float* v;
  unsigned short* kp; unsigned short* vp;
  long long plane;
  int Lk, B, H, ldk, ldv, steps;
};

__global__ __launch_bounds__(64 * XM_WAVES) void cross_mha_pack_kernel(const CrossPackParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int step = blockIdx.x, b = blockIdx.z;
  const int lo = lane & 15, g = lane >> 4;
  for (int f = wave; f < 2 * p.H; f += XM_WAVES) {
    const int h = f >> 1, t = f & 1;
    float x[8];
    if (blockIdx.y == 0) {                                             // K: lane (key lo of tile t, g) <- channels 8 g .. 8 g + 7
      const int key = 32 * step + 16 * t + lo;
      if (key < p.Lk) {
        const float* src = p.k + ((size_t)key * p.B + b) * p.ldk + h * XM_D + 8 * g;
        const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = c.x; x[5] = c.y; x[6] = c.z; x[7] = c.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = 0.f;
      }
    } else {                                                           // V: lane (channel 16 t + lo, g) <- keys 16 (j >> 2) + 4 g + (j & 3)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = 32 * step + 16 * (j >> 2) + 4 * g + (j & 3);
        x[j] = key < p.Lk ? p.v[((size_t)key * p.B + b) * p.ldv + h * XM_D + 16 * t + lo] : 0.f;
      }
    }
    const size_t e = (((((size_t)b * p.H + h) * p.steps + step) * 2 + t) * 64 + lane) * 8;
    if (blockIdx.y == 0) {                                             // K: hi, mid, lo (the scores take six products)
      u32x4 hi, md, lw;
      split8x3(x, hi, md, lw);
      *reinterpret_cast<u32x4*>(p.kp + e) = hi;
      *reinterpret_cast<u32x4*>(p.kp + p.plane + e) = md;
      *reinterpret_cast<u32x4*>(p.kp + 2 * p.plane + e) = lw;
    } else {
      u32x4 hi, lw;
      split8(x, hi, lw);
      *reinterpret_cast<u32x4*>(p.vp + e) = hi;
      *reinterpret_cast<u32x4*>(p.vp + p.plane + e) = lw;
    }
  }
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

extern "C" int gd4d_cross_mha_pack_kv(const float* k, const float* v, int ldk, int ldv, void* k_planes, void* v_planes,
                                      long long plane_stride, int Lk, int B, int H, int D, void* stream) {
  using namespace gd4d;
  if (!k || !v || !k_planes || !v_planes || Lk <= 0 || B <= 0 || H <= 0) return GD4D_EINVAL;
  if (D != XM_D || H != 8 || B > 65535) return GD4D_EUNSUPPORTED;
  if (ldk < H * D || ldv < H * D || plane_stride < (long long)gd4d_cross_mha_plane_elems(Lk, B, H) || (plane_stride & 7)) return GD4D_EINVAL;
  if (!aligned16(k) || (ldk % 4) || !aligned16(k_planes) || !aligned16(v_planes)) return GD4D_EALIGN;
  const int steps = (Lk + 31) / 32;
  CrossPackParams p{k, v, static_cast<unsigned short*>(k_planes), static_cast<unsigned short*>(v_planes), plane_stride, Lk, B, H, ldk, ldv, steps};
  hipLaunchKernelGGL(cross_mha_pack_kernel, dim3(steps, 2, B), dim3(64 * XM_WAVES), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

namespace gd4d {

static int cross_mha_launch(const float* q, const void* k_planes, const void* v_planes, long long plane_stride,
                            const void* key_padding_mask, float* out, float* lse, void* workspace, size_t workspace_bytes,
                            int Lq, int Lk, int B, int H, int D, int ldq, int ldo, float scale, int q_tile, int splits,
                            bool train, float drop_p, const void* seed, void* stream) {
  if (!q || !k_planes || !v_planes || !out || Lq <= 0 || Lk <= 0 || B <= 0 || H <= 0) return GD4D_EINVAL;
  if (train && (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && !seed))) return GD4D_EINVAL;
  if (D != XM_D || H != 8) return GD4D_EUNSUPPORTED;
  if (drop_p > 0.f && (double)B * H * Lq * Lk >= 4294967296.0) return GD4D_EUNSUPPORTED;   // element ids are 32 bits
  if (train) {                                        // six products for P V and a third V plane: the 64-query tile would spill
    if (q_tile == 64) return GD4D_EUNSUPPORTED;
    if (q_tile == 0) q_tile = 32;
  }
  int qt, s;
  const int rc = xm_plan(Lq, Lk, B, H, q_tile, splits, &qt, &s);
  if (rc != GD4D_OK) return rc;
  if (ldq < H * D || ldo < H * D || plane_stride < (long long)gd4d_cross_mha_plane_elems(Lk, B, H) || (plane_stride & 7)) return GD4D_EINVAL;
  if (!aligned16(q) || (ldq % 4) || !aligned16(k_planes) || !aligned16(v_planes)) return GD4D_EALIGN;
  const size_t need = gd4d_cross_mha_workspace_bytes(Lq, Lk, B, H, qt, s);
  if (need && (!workspace || workspace_bytes < need)) return GD4D_EWORKSPACE;
  CrossMhaParams p{q, static_cast<const unsigned short*>(k_planes), static_cast<const unsigned short*>(v_planes), plane_stride,
                   static_cast<const uint8_t*>(key_padding_mask), out, lse, static_cast<float*>(workspace),
                   Lq, Lk, B, H, ldq, ldo, (Lk + 31) / 32, s, scale * 1.4426950408889634f,
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
