// The packs (fp32 rows -> split-bf16 planes) of gd4d_cross_mha_fwd / gd4d_cross_mha_train_fwd, inference and training, and the
// backward: PETR's global cross-attention trained on a long key axis.
// Reference: projects/mmdet3d_plugin/models/utils/petr_transformer.py (PETRMultiheadAttention.forward -> nn.MultiheadAttention with
// key_padding_mask and attn_drop, under autograd).
//
// With M = keep / (1 - p), P = exp(scale q k^T + mask - lse), Dq = sum_d dout o out and dS = P o (M o (dout v^T) - Dq):
//   dq = scale dS k,   dk = scale dS^T q,   dv = (P o M)^T dout.
// Nothing of size Lq x Lk is stored: both compute kernels rebuild P from the saved lse, with the scores on the forward's six bf16
// products of the same hi / mid / lo pieces of q and k.  The other four products - dout v^T, dS k, dS^T q, (P o M)^T dout - take six
// as well, both operands as hi + mid + lo, as the training forward's P V does.  They began on three (hi / lo operands, 2^-17 of the
// terms' magnitudes) and the bounds of the tests decided: in a row that one key dominates (P = 1) dS = P (dout v^T - Dq) is the
// difference of two nearly equal numbers, Dq = dout . out carrying the forward's v, and the spiked-key case had dq off by 2.2e-4
// (bound 1e-4); with dout v^T alone on more pieces it was still off by 1.2e-4 on values up to 13, and the two-layer transformer's
// input gradients were 5 - 6 times as far from the reference as the fp32 torch-op route's (now 1.2 times).
// All accumulate in fp32.
// No atomics: every sum has one owner and a fixed order.
//
//   cross_pack_kernel         fp32 rows -> split-bf16 planes in both fragment layouts (gd4d_cross_mha.h).  One body, three uses: the
//                             inference K|V pack (K rows x3, V columns x2: gd4d_cross_mha_pack_kv), its training form (K rows x3 and V
//                             columns x3 as the training forward reads them, V rows x3 and K columns x3 for the backward), and the
//                             query-side pack of a backward call (q scaled by scale log2(e): rows x3, columns x3; dout: rows x3,
//                             columns x3) which also leaves Dq and lse log2(e) per (batch, head, query).
//   cross_bwd_query_kernel    a workgroup owns 32 queries of one (batch, head) and one key split, as the forward: its waves take the
//                             split's 32-key steps round-robin, S^T = K Q^T and dP^T = V dout^T come out in one register layout,
//                             dS^T in that layout is the B operand of dq^T += K^T dS^T.  Waves merge in LDS in wave order, splits
//                             through the workspace in split order (cross_bwd_merge_kernel).
//   cross_bwd_key_kernel      the mirror image: a workgroup owns 64 keys of one (batch, head), their K and V fragments stay in
//                             registers (wave w: key half w & 1), the waves of a half take the 32-query steps alternately:
//                             S = Q K^T, dP = dout V^T, and P o M and dS as they stand are the B operands of dv^T += dout^T (P o M)
//                             and dk^T += Q^T dS.  The two waves of a half are summed in LDS in wave order; masked keys are written
//                             as exact zeros, keys past Lk not at all.
#include "gd4d_cross_mha.h"
#include "gd4d_mha_dropout.h"

namespace gd4d {

constexpr int XB_KEYS = 64;       // keys per workgroup of the key-side kernel
constexpr int XB_QPLANES = 12;    // planes of the query-side pack

// ---------------------------------------------------------------- pack ----------------------------------------------------------------
struct CrossPackGroup {
  const float* src;               // rows (l B + b) at stride ld
  unsigned short* dst;            // `planes` planes, `plane` elements apart
  int ld, columns;                // columns: 0 = row fragments, 1 = column fragments
  float scale;
  int planes;                     // 3: hi, mid, lo (split8x3); 2: hi, lo (split8: what the inference forward's P V reads of V)
};

struct CrossPackParams {
  CrossPackGroup g[4];
  long long plane;
  int groups, L, B, H, steps;
  // the query-side pack only (null otherwise): Dq = sum_d dout out and lse log2(e), (B, H, steps * 32); rows past L: 0 and +inf
  const float* dout; const float* out; const float* lse;
  float* dsum; float* lse2;
  int ld_dout, ld_out;
};

// grid (steps, groups [+ 1 with dsum], B), 4 waves; a wave writes whole fragments (1 KB contiguous per plane)
__global__ __launch_bounds__(64 * XM_WAVES) void cross_pack_kernel(const CrossPackParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int step = blockIdx.x, b = blockIdx.z;
  const int lo = lane & 15, g = lane >> 4;
  if ((int)blockIdx.y == p.groups) {                                   // one thread per (row of the step, head)
    const int r = threadIdx.x & 31, h = threadIdx.x >> 5;
    const int row = 32 * step + r;
    float s = 0.f, l2 = __builtin_inff();
    if (row < p.L) {
      const float* a = p.dout + ((size_t)row * p.B + b) * p.ld_dout + h * XM_D;
      const float* o = p.out + ((size_t)row * p.B + b) * p.ld_out + h * XM_D;
#pragma unroll
      for (int d = 0; d < XM_D; d += 4) {
        const float4 x = *reinterpret_cast<const float4*>(a + d), y = *reinterpret_cast<const float4*>(o + d);
        s += x.x * y.x; s += x.y * y.y; s += x.z * y.z; s += x.w * y.w;
      }
      l2 = p.lse[((size_t)row * p.B + b) * p.H + h] * ATTN_LOG2E;
    }
    const size_t e = (((size_t)b * p.H + h) * p.steps + step) * 32 + r;
    p.dsum[e] = s;
    p.lse2[e] = l2;
    return;
  }
  const CrossPackGroup& G = p.g[blockIdx.y];
  for (int f = wave; f < 2 * p.H; f += XM_WAVES) {
    const int h = f >> 1, t = f & 1;
    float x[8];
    if (!G.columns) {                                                  // lane (row lo of tile t, g) <- channels 8 g .. 8 g + 7
      const int row = 32 * step + 16 * t + lo;
      if (row < p.L) {
        const float* src = G.src + ((size_t)row * p.B + b) * G.ld + h * XM_D + 8 * g;
        const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = c.x; x[5] = c.y; x[6] = c.z; x[7] = c.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = 0.f;
      }
    } else {                                                           // lane (channel 16 t + lo, g) <- rows 16 (j >> 2) + 4 g + (j & 3)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = 32 * step + 16 * (j >> 2) + 4 * g + (j & 3);
        x[j] = row < p.L ? G.src[((size_t)row * p.B + b) * G.ld + h * XM_D + 16 * t + lo] : 0.f;
      }
    }
    if (G.scale != 1.f) {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] *= G.scale;
    }
    const size_t e = xm_frag(p.H, p.steps, b, h, step, t, lane);
    u32x4 hi, md, lw;
    if (G.planes == 3) {
      split8x3(x, hi, md, lw);
      *reinterpret_cast<u32x4*>(G.dst + p.plane + e) = md;
    } else {
      split8(x, hi, lw);
    }
    *reinterpret_cast<u32x4*>(G.dst + e) = hi;
    *reinterpret_cast<u32x4*>(G.dst + (G.planes - 1) * p.plane + e) = lw;
  }
}

// ---------------------------------------------------------------- backward ----------------------------------------------------------------
struct CrossBwdParams {
  const unsigned short* kk;       // K rows, hi / mid / lo
  const unsigned short* vk;       // V rows, hi / mid / lo
  const unsigned short* kv;       // K columns, hi / mid / lo
  long long kplane;
  const unsigned short* qk;       // q scale log2(e) rows, hi / mid / lo
  const unsigned short* dok;      // dout rows, hi / mid / lo
  const unsigned short* qv;       // q scale log2(e) columns, hi / mid / lo
  const unsigned short* dov;      // dout columns, hi / mid / lo
  long long qplane;
  const float* lse2; const float* dsum;        // (B, H, qsteps * 32)
  const uint8_t* mask;                         // (B, Lk) or null
  float* dq; float* dk; float* dv; float* ws;  // ws: dq partials (splits, B, H, Lq, 32) with splits > 1
  const uint32_t* seed; uint32_t drop_thresh; float inv_keep;
  int Lq, Lk, B, H, ld_dq, ld_dk, ld_dv, ksteps, qsteps, splits;
  float scale;
};

// (The score tiles are products6 of gd4d_attn_pieces.h: the query-side kernel hands it the K pieces as A and the Q pieces as B, as
// the forward; the key-side kernel the other way round, products6<false>, and gets the transposed tile of the same products in the
// same order.)

struct XbQueryShared { float o[XM_WAVES][32][XM_D + 1]; };

// grid (query steps, H * splits, B), 4 waves
__global__ __launch_bounds__(64 * XM_WAVES, 2) void cross_bwd_query_kernel(const CrossBwdParams p) {
  __shared__ XbQueryShared sh;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int qi = lane & 15;            // query column of this lane in a score tile
  const int g = lane >> 4;
  const int qstep = blockIdx.x, q0 = 32 * qstep;
  const int h = blockIdx.y % p.H, split = blockIdx.y / p.H;
  const int b = blockIdx.z;
  const bool drop = p.drop_thresh != 0u;

  Planes3 qp[2], gp[2];                // Q^T and dout^T as B operands: lane (query qi, g), channels 8 g .. 8 g + 7
  float lse2[2], dsum[2];
  uint32_t drow[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const size_t e = xm_frag(p.H, p.qsteps, b, h, qstep, t, lane);
    qp[t] = load_planes(p.qk, p.qplane, e);
    gp[t] = load_planes(p.dok, p.qplane, e);
    const size_t r = (((size_t)b * p.H + h) * p.qsteps + qstep) * 32 + 16 * t + qi;
    lse2[t] = p.lse2[r];                       // +inf past Lq: probability 0
    dsum[t] = p.dsum[r];
    drow[t] = mha_drop_row(b, h, q0 + 16 * t + qi, p.H, p.Lq, p.Lk);
  }
  uint32_t seed_lo = 0, seed_hi = 0;
  if (drop) { seed_lo = p.seed[0]; seed_hi = p.seed[1]; }
  f32x4 a0[2], a1[2];                           // dq^T rows d = 4 g + r, and 16 + 4 g + r
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    a0[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    a1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int s_first = xm_split_first(p.ksteps, p.splits, split), s_last = xm_split_first(p.ksteps, p.splits, split + 1);
  struct StepData { Planes3 k[2], v[2]; KeyStepMask mask; };        // K rows, V rows (K columns: fetched where they are used)
  auto fetch = [&](const int step, StepData& d) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const size_t e = xm_frag(p.H, p.ksteps, b, h, step, t, lane);
      d.k[t] = load_planes(p.kk, p.kplane, e);
      d.v[t] = load_planes(p.vk, p.kplane, e);
    }
    d.mask.fetch(p.mask, b, p.Lk, step, lane);
  };
  auto compute = [&](const int step, const StepData& d) {
    const unsigned bits = d.mask.bits();
    if (bits == 0xffffffffu) return;                                  // every probability of the step is 0
    const unsigned mb = KeyStepMask::of_lane(bits, g);
    Planes3 c[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) c[half] = load_planes(p.kv, p.kplane, xm_frag(p.H, p.ksteps, b, h, step, half, lane));
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float ds[8];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        // S^T and dP^T, lane (qi, g) register r <-> key 16 kt + 4 g + r of the step
        const f32x4 st = products6(d.k[kt], qp[t]);
        const f32x4 dp = xm_x6(d.v[kt], gp[t], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = ((mb >> (16 * kt + r)) & 1u) ? 0.f : __builtin_amdgcn_exp2f(st[r] - lse2[t]);
          float x = dp[r];
          if (drop) {
            const uint32_t key = (uint32_t)(32 * step + 16 * kt + 4 * g + r);
            x = mha_drop_keep(seed_lo, seed_hi, drow[t] + key, p.drop_thresh) ? x * p.inv_keep : 0.f;
          }
          ds[4 * kt + r] = pr * (x - dsum[t]);
        }
      }
      // dq^T += K^T dS^T: A = K^T[d = lane & 15 (+ 16)][k = 8 g + j], B = this lane's own eight dS
      const Planes3 dsp = split_planes3(ds);
      a0[t] = xm_x6(c[0], dsp, a0[t]);
      a1[t] = xm_x6(c[1], dsp, a1[t]);
    }
  };
  walk_steps<XM_WAVES, StepData>(s_first, s_last, wave, fetch, compute);

  // ---- the waves' key slices, summed in wave order ----
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sh.o[wave][16 * t + qi][4 * g + r] = a0[t][r];
      sh.o[wave][16 * t + qi][16 + 4 * g + r] = a1[t][r];
    }
  }
  __syncthreads();
  for (int e = tid; e < 32 * XM_D; e += 64 * XM_WAVES) {
    const int i = e / XM_D, d = e % XM_D;
    if (q0 + i >= p.Lq) continue;
    float s = sh.o[0][i][d];
#pragma unroll
    for (int w = 1; w < XM_WAVES; ++w) s += sh.o[w][i][d];
    if (p.splits == 1) p.dq[((size_t)(q0 + i) * p.B + b) * p.ld_dq + h * XM_D + d] = s * p.scale;
    else p.ws[((((size_t)split * p.B + b) * p.H + h) * p.Lq + (q0 + i)) * XM_D + d] = s;
  }
}

// the key splits' dq partials, summed in split order: one thread per (query, batch, head, channel)
__global__ __launch_bounds__(256) void cross_bwd_merge_kernel(const CrossBwdParams p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)p.Lq * p.B * p.H * XM_D) return;
  const int d = (int)(e % XM_D);
  const int h = (int)(e / XM_D % p.H);
  const int b = (int)(e / XM_D / p.H % p.B);
  const int q = (int)(e / XM_D / p.H / p.B);
  float s = 0.f;
  for (int sp = 0; sp < p.splits; ++sp) s += p.ws[((((size_t)sp * p.B + b) * p.H + h) * p.Lq + q) * XM_D + d];
  p.dq[((size_t)q * p.B + b) * p.ld_dq + h * XM_D + d] = s * p.scale;
}

struct XbKeyShared { float o[XM_WAVES][32][2][XM_D + 1]; };           // [wave][key of its half][dk | dv][channel]

// grid (key blocks of 64, H, B), 4 waves: wave w owns key step 2 block + (w & 1) and takes the query steps (w >> 1), (w >> 1) + 2, ...
__global__ __launch_bounds__(64 * XM_WAVES, 2) void cross_bwd_key_kernel(const CrossBwdParams p) {
  __shared__ XbKeyShared sh;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ki = lane & 15;            // key column of this lane in a score tile
  const int g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int kstep = 2 * blockIdx.x + (wave & 1);
  const bool have = kstep < p.ksteps;                                  // (an odd number of key steps: the last block's second half)
  const bool drop = p.drop_thresh != 0u;

  Planes3 kp[2], vp[2];                // K^T and V^T as B operands: lane (key ki, g), channels 8 g .. 8 g + 7
  bool masked[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    kp[t] = vp[t] = Planes3{};
    const int key = 32 * kstep + 16 * t + ki;
    masked[t] = key >= p.Lk || (p.mask && p.mask[(size_t)b * p.Lk + key]);
    if (have) {
      const size_t e = xm_frag(p.H, p.ksteps, b, h, kstep, t, lane);
      kp[t] = load_planes(p.kk, p.kplane, e);
      vp[t] = load_planes(p.vk, p.kplane, e);
    }
  }
  uint32_t seed_lo = 0, seed_hi = 0;
  if (drop) { seed_lo = p.seed[0]; seed_hi = p.seed[1]; }
  f32x4 dk0[2], dk1[2], dv0[2], dv1[2];         // dk^T, dv^T rows d = 4 g + r and 16 + 4 g + r, column key ki of tile t
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    dk0[t] = dk1[t] = dv0[t] = dv1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bool any = have && __ballot(!(masked[0] && masked[1])) != 0ull;      // wave-uniform: a key of this half is seen

  if (any) {
    for (int qstep = wave >> 1; qstep < p.qsteps; qstep += 2) {
      // ---- first the two products that reduce over channels, for both key tiles: P o M and dS stay, the row fragments go ----
      float pm[2][8], ds[2][8];                 // register j <-> query 16 (j >> 2) + 4 g + (j & 3) of the step
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {          // one query tile's row fragments at a time
        const size_t e = xm_frag(p.H, p.qsteps, b, h, qstep, qt, lane);
        const Planes3 qp = load_planes(p.qk, p.qplane, e), gp = load_planes(p.dok, p.qplane, e);
        const size_t r0 = (((size_t)b * p.H + h) * p.qsteps + qstep) * 32 + 16 * qt + 4 * g;
        const float4 l4 = *reinterpret_cast<const float4*>(p.lse2 + r0), s4 = *reinterpret_cast<const float4*>(p.dsum + r0);
        const float lse2[4] = {l4.x, l4.y, l4.z, l4.w}, dsum[4] = {s4.x, s4.y, s4.z, s4.w};      // lse2 = +inf past Lq
        uint32_t drow[4] = {0u, 0u, 0u, 0u};    // dropout ids of this lane's four queries at key 0, once per query tile
        if (drop) {
#pragma unroll
          for (int r = 0; r < 4; ++r) drow[r] = mha_drop_row(b, h, 32 * qstep + 16 * qt + 4 * g + r, p.H, p.Lq, p.Lk);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {           // this wave's two key tiles
          // S and dP, lane (ki, g) register r <-> query 16 qt + 4 g + r of the step
          const f32x4 st = products6<false>(qp, kp[t]);
          const f32x4 dp = xm_x6(gp, vp[t], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pr = masked[t] ? 0.f : __builtin_amdgcn_exp2f(st[r] - lse2[r]);
            float x = dp[r], y = pr;
            if (drop) {
              const bool keep = mha_drop_keep(seed_lo, seed_hi, drow[r] + (uint32_t)(32 * kstep + 16 * t + ki), p.drop_thresh);
              x = keep ? x * p.inv_keep : 0.f;
              y = keep ? y * p.inv_keep : 0.f;
            }
            pm[t][4 * qt + r] = y;
            ds[t][4 * qt + r] = pr * (x - dsum[r]);
          }
        }
      }
      // ---- then the two that reduce over the step's queries: dv^T += dout^T (P o M), dk^T += Q^T dS.  A = columns
      //      [d = lane & 15 (+ 16)][k = 8 g + j], B = this lane's own eight values ----
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const size_t e = xm_frag(p.H, p.qsteps, b, h, qstep, half, lane);
        const Planes3 gc = load_planes(p.dov, p.qplane, e), qc = load_planes(p.qv, p.qplane, e);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          f32x4& dv = half ? dv1[t] : dv0[t];
          dv = xm_x6(gc, split_planes3(pm[t]), dv);
          f32x4& dk = half ? dk1[t] : dk0[t];
          dk = xm_x6(qc, split_planes3(ds[t]), dk);
        }
      }
    }
  }

  // ---- the two waves of a key half, summed in wave order.  q was packed times scale log2(e): dk = ln(2) Q^T dS ----
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bool z = masked[t];                                          // exact zeros, whatever a non-finite dout or Dq made of 0 x
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sh.o[wave][16 * t + ki][0][4 * g + r] = z ? 0.f : dk0[t][r];
      sh.o[wave][16 * t + ki][0][16 + 4 * g + r] = z ? 0.f : dk1[t][r];
      sh.o[wave][16 * t + ki][1][4 * g + r] = z ? 0.f : dv0[t][r];
      sh.o[wave][16 * t + ki][1][16 + 4 * g + r] = z ? 0.f : dv1[t][r];
    }
  }
  __syncthreads();
  for (int e = tid; e < XB_KEYS * 2 * XM_D; e += 64 * XM_WAVES) {
    const int d = e % XM_D, which = e / XM_D % 2, i = e / (2 * XM_D);
    const int key = XB_KEYS * blockIdx.x + i;
    if (key >= p.Lk) continue;
    const int half = i >> 5, kk = i & 31;
    const float s = sh.o[half][kk][which][d] + sh.o[half + 2][kk][which][d];
    if (which == 0) p.dk[((size_t)key * p.B + b) * p.ld_dk + h * XM_D + d] = s * ATTN_LN2;
    else p.dv[((size_t)key * p.B + b) * p.ld_dv + h * XM_D + d] = s;
  }
}

struct XbPlan {
  int qt, splits, ksteps, qsteps;
  size_t pack_bytes, dq_bytes;
};

static int xb_plan(int Lq, int Lk, int B, int H, int q_tile, int splits, XbPlan* out) {
  if (q_tile == 64) return GD4D_EUNSUPPORTED;                          // the backward's workgroup owns 32 queries
  int qt, s;
  const int rc = xm_plan(Lq, Lk, B, H, q_tile ? q_tile : 32, splits, &qt, &s);
  if (rc != GD4D_OK) return rc;
  out->qt = qt;
  out->splits = s;
  out->ksteps = (Lk + 31) / 32;
  out->qsteps = (Lq + 31) / 32;
  // twelve planes of the queries (q and dout, each as rows x3 and columns x3), then Dq and lse log2(e)
  out->pack_bytes = XB_QPLANES * gd4d_cross_mha_plane_elems(Lq, B, H) * sizeof(unsigned short) + 2 * (size_t)B * H * out->qsteps * 32 * sizeof(float);
  out->dq_bytes = s > 1 ? (size_t)s * B * H * Lq * XM_D * sizeof(float) : 0;
  return GD4D_OK;
}

}  // namespace gd4d

extern "C" int gd4d_cross_mha_bwd_plan(int Lq, int Lk, int B, int H, int q_tile, int splits, int64_t* plan) {
  using namespace gd4d;
  XbPlan x;
  if (!plan) return GD4D_EINVAL;
  const int rc = xb_plan(Lq, Lk, B, H, q_tile, splits, &x);
  if (rc != GD4D_OK) return rc;
  plan[0] = x.qt; plan[1] = x.splits; plan[2] = x.ksteps; plan[3] = x.qsteps;
  plan[4] = x.qsteps; plan[5] = (int64_t)H * x.splits; plan[6] = B; plan[7] = 64 * XM_WAVES;
  plan[8] = XB_KEYS;
  plan[9] = (Lk + XB_KEYS - 1) / XB_KEYS; plan[10] = H; plan[11] = B; plan[12] = 64 * XM_WAVES;
  plan[13] = (int64_t)x.pack_bytes; plan[14] = (int64_t)x.dq_bytes; plan[15] = (int64_t)(x.pack_bytes + x.dq_bytes);
  for (int i = 0; i <= x.splits; ++i) plan[16 + i] = xm_split_first(x.ksteps, x.splits, i);
  return GD4D_OK;
}

extern "C" size_t gd4d_cross_mha_bwd_workspace_bytes(int Lq, int Lk, int B, int H, int q_tile, int splits) {
  gd4d::XbPlan x;
  if (gd4d::xb_plan(Lq, Lk, B, H, q_tile, splits, &x) != GD4D_OK) return 0;
  return x.pack_bytes + x.dq_bytes;
}

namespace gd4d {

// Both K | V packs, one launch of up to four groups: K rows always; V columns in `v_pieces` pieces (2: inference, 3: training), V
// rows and K columns (the backward's) where their planes are given.  grid (steps, groups, B).
static int cross_pack_kv(const float* k, const float* v, int ldk, int ldv, void* k_planes, void* v_planes, int v_pieces, void* vk_planes,
                         void* kv_planes, long long plane_stride, int Lk, int B, int H, int D, void* stream) {
  if (!k || !v || !k_planes || Lk <= 0 || B <= 0 || H <= 0) return GD4D_EINVAL;
  if (D != XM_D || H != 8 || B > 65535) return GD4D_EUNSUPPORTED;
  const int rc = xm_check_layout(ldk < ldv ? ldk : ldv, plane_stride, Lk, B, H,
                                 aligned16(k) && !(ldk % 4) && aligned16(k_planes) && aligned16(v_planes) && aligned16(vk_planes) &&
                                     aligned16(kv_planes) && (!vk_planes || (aligned16(v) && !(ldv % 4))));
  if (rc != GD4D_OK) return rc;
  const int steps = (Lk + 31) / 32;
  CrossPackParams p{};
  int n = 0;
  p.g[n++] = CrossPackGroup{k, static_cast<unsigned short*>(k_planes), ldk, 0, 1.f, 3};
  if (v_planes) p.g[n++] = CrossPackGroup{v, static_cast<unsigned short*>(v_planes), ldv, 1, 1.f, v_pieces};
  if (vk_planes) p.g[n++] = CrossPackGroup{v, static_cast<unsigned short*>(vk_planes), ldv, 0, 1.f, 3};
  if (kv_planes) p.g[n++] = CrossPackGroup{k, static_cast<unsigned short*>(kv_planes), ldk, 1, 1.f, 3};
  p.plane = plane_stride;
  p.groups = n; p.L = Lk; p.B = B; p.H = H; p.steps = steps;
  hipLaunchKernelGGL(cross_pack_kernel, dim3(steps, n, B), dim3(64 * XM_WAVES), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

}  // namespace gd4d

extern "C" int gd4d_cross_mha_pack_kv(const float* k, const float* v, int ldk, int ldv, void* k_planes, void* v_planes,
                                      long long plane_stride, int Lk, int B, int H, int D, void* stream) {
  if (!v_planes) return GD4D_EINVAL;
  return gd4d::cross_pack_kv(k, v, ldk, ldv, k_planes, v_planes, 2, nullptr, nullptr, plane_stride, Lk, B, H, D, stream);
}

extern "C" int gd4d_cross_mha_pack_kv_train(const float* k, const float* v, int ldk, int ldv, void* k_planes, void* v_planes,
                                            void* vk_planes, void* kv_planes, long long plane_stride, int Lk, int B, int H, int D,
                                            void* stream) {
  return gd4d::cross_pack_kv(k, v, ldk, ldv, k_planes, v_planes, 3, vk_planes, kv_planes, plane_stride, Lk, B, H, D, stream);
}

extern "C" int gd4d_cross_mha_bwd(const float* dout, const float* q, const float* out, const float* lse, const void* k_planes,
                                  const void* vk_planes, const void* kv_planes, long long plane_stride,
                                  const void* key_padding_mask, float* dq, float* dk, float* dv, void* workspace,
                                  size_t workspace_bytes, int Lq, int Lk, int B, int H, int D, int ld_dout, int ldq, int ldo,
                                  int ld_dq, int ld_dk, int ld_dv, float scale, float drop_p, const void* seed, int q_tile,
                                  int splits, void* stream) {
  using namespace gd4d;
  if (!dout || !q || !out || !lse || !k_planes || !vk_planes || !kv_planes || !dq || !dk || !dv || Lq <= 0 || Lk <= 0 || B <= 0 || H <= 0)
    return GD4D_EINVAL;
  int rc = attn_check_drop(drop_p, seed, (double)B * H * Lq * Lk);
  if (rc != GD4D_OK) return rc;
  if (D != XM_D || H != 8) return GD4D_EUNSUPPORTED;
  XbPlan x;
  rc = xb_plan(Lq, Lk, B, H, q_tile, splits, &x);
  if (rc != GD4D_OK) return rc;
  int min_ld = ld_dout;
  for (const int ld : {ldq, ldo, ld_dq, ld_dk, ld_dv}) min_ld = ld < min_ld ? ld : min_ld;
  rc = xm_check_layout(min_ld, plane_stride, Lk, B, H,
                       aligned16(dout) && aligned16(q) && aligned16(out) && !(ld_dout % 4) && !(ldq % 4) && !(ldo % 4) && aligned16(k_planes) &&
                           aligned16(vk_planes) && aligned16(kv_planes) && aligned16(workspace));
  if (rc != GD4D_OK) return rc;
  if (!workspace || workspace_bytes < x.pack_bytes + x.dq_bytes) return GD4D_EWORKSPACE;

  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t qplane = gd4d_cross_mha_plane_elems(Lq, B, H);
  unsigned short* planes = static_cast<unsigned short*>(workspace);
  float* rows = reinterpret_cast<float*>(planes + XB_QPLANES * qplane);
  const size_t nrows = (size_t)B * H * x.qsteps * 32;
  const float qscale = scale * ATTN_LOG2E;

  CrossPackParams pk{};
  pk.g[0] = CrossPackGroup{q, planes, ldq, 0, qscale, 3};
  pk.g[1] = CrossPackGroup{dout, planes + 3 * qplane, ld_dout, 0, 1.f, 3};
  pk.g[2] = CrossPackGroup{q, planes + 6 * qplane, ldq, 1, qscale, 3};
  pk.g[3] = CrossPackGroup{dout, planes + 9 * qplane, ld_dout, 1, 1.f, 3};
  pk.plane = (long long)qplane;
  pk.groups = 4; pk.L = Lq; pk.B = B; pk.H = H; pk.steps = x.qsteps;
  pk.dout = dout; pk.out = out; pk.lse = lse; pk.dsum = rows; pk.lse2 = rows + nrows; pk.ld_dout = ld_dout; pk.ld_out = ldo;
  hipLaunchKernelGGL(cross_pack_kernel, dim3(x.qsteps, 5, B), dim3(64 * XM_WAVES), 0, st, pk);

  CrossBwdParams p{static_cast<const unsigned short*>(k_planes), static_cast<const unsigned short*>(vk_planes),
                   static_cast<const unsigned short*>(kv_planes), plane_stride,
                   planes, planes + 3 * qplane, planes + 6 * qplane, planes + 9 * qplane, (long long)qplane,
                   rows + nrows, rows, static_cast<const uint8_t*>(key_padding_mask), dq, dk, dv, rows + 2 * nrows,
                   static_cast<const uint32_t*>(seed), mha_drop_thresh(drop_p), 1.f / (1.f - drop_p),
                   Lq, Lk, B, H, ld_dq, ld_dk, ld_dv, x.ksteps, x.qsteps, x.splits, scale};
  hipLaunchKernelGGL(cross_bwd_query_kernel, dim3(x.qsteps, H * x.splits, B), dim3(64 * XM_WAVES), 0, st, p);
  if (x.splits > 1) {
    const size_t n = (size_t)Lq * B * H * XM_D;
    hipLaunchKernelGGL(cross_bwd_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  }
  hipLaunchKernelGGL(cross_bwd_key_kernel, dim3((Lk + XB_KEYS - 1) / XB_KEYS, H, B), dim3(64 * XM_WAVES), 0, st, p);
  return check_launch();
}
