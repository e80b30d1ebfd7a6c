// Camera-aware DepthNet of Detr3DHeadPECAM (dense_heads/detr3d_head_pe_camaware.py:59-105, built at :198, applied per level at
// :313-320): per level x (N, 256, H, W) of a B = 1 sample,
//     out[n, c] = relu(BN(conv3x3(x) + bias))[n, c] * g[n, c],   g[n] = sigmoid(SE(MLP(s[n]))),
// where s[n] is the camera's scaled pixel size (from its intrinsics and the image-augmentation scale).  The discarded
// context_conv is not computed.  Three entry points:
//
//   gd4d_depth_net_image   the 3x3 weight (256, 256, 3, 3) split once into bf16 hi / lo planes laid out as MFMA A fragments, in the
//                          order the conv walks K: [chunk of 32 input channels][tap][plane][k-group of 8][256 out channels][8 x bf16]
//                          (72 steps x 32 KB = 2.25 MB: fits one XCD's 4-MB L2, which every workgroup of the launch re-reads).
//   gd4d_cam_gate_fwd      g (N, 256) from device buffers (so that a captured graph serves new cameras): one workgroup per camera,
//                          fp32 4x4 inverse (Gauss-Jordan, partial pivoting), then the 1 -> 256 -> 256 MLP and the 256 -> 256 -> 256 SE
//                          as plain fp32 FMAs (~3 MFLOP per sample).
//   gd4d_depth_conv_fwd    the hot path: an implicit GEMM, out channels (M = 256) x output pixels (N) x 9 taps x 256 input channels
//                          (K = 2304), over ALL levels and cameras in ONE launch.
//
// Arithmetic: gd4d_gemm_bf16x3_fwd's - both operands split into bf16 hi + lo, lo hi + hi lo + hi hi accumulated in fp32 on the bf16
// MFMA (v_mfma_f32_32x32x16_bf16; ~2^-16 relative per product).
//
// Tiling.  A workgroup owns a 16 x 16 pixel tile of one (level, camera) and all 256 output channels: 16 waves in 4 (channels) x 4
// (pixels), each wave 2 x 2 tiles of 32 x 32.  The weights are the MFMA's A operand, the pixels its B operand, so a lane of the
// accumulator holds one PIXEL (x fastest) and 16 channels: the NCHW stores of a wave are 16-pixel (64-B) row segments.  The tile's
// work list is the grid itself: blockIdx.x runs over the tiles of level 0, then level 1, ... (a prefix table in the kernel
// arguments), so the 29 x 50 and 15 x 25 levels add their tiles to the same launch instead of launches with ragged tails of their own.
// K is walked chunk by chunk (32 input channels) and, inside a chunk, tap by tap (9): 72 steps.
//   halo   the tile's 18 x 18 input patch of the chunk (zero outside the image: exact padding at every border, and for the ragged
//          pixels of edge tiles, whose outputs are not stored), split hi / lo once and read by all 9 taps: [k-group][324][8 x bf16]
//          per plane, 40.5 KB.  Double-buffered by chunk parity; the next chunk's halo is loaded in two passes of 8 values per
//          thread (before taps 2 and 5) and parked two steps later (after taps 4 and 7): the latency hides under three steps of MFMAs
//          and only 8 registers are held for it.
//   weight one step's (tap, chunk) slice of the image, 32 KB hi + lo, copied to LDS verbatim (two 16-B loads per thread, issued one
//          step ahead into registers and parked after the step's MFMAs), double-buffered by step parity.
// A B fragment of tap (ky, kx) is the halo entry of pixel (py + ky, px + kx): every fragment is one conflict-free ds_read_b128 (16
// lanes read 256 contiguous bytes).  One barrier per step.  145 KB of LDS (+ 5 KB of per-channel epilogue constants): one
// workgroup of 16 waves per CU (four per SIMD).
// Epilogue, the reference's order: + bias, BatchNorm with the running statistics ((y - mean) * weight / sqrt(var + eps) + bias),
// ReLU, x g[n, c]; stored NCHW fp32.
// 124 VGPRs, no scratch (with the two k-halves of a tap unrolled the compiler hoists all 64 fragment registers: 67 spilled).
// Measured (docs/measurements_r07.md): 2.58-2.64 ms per 24-camera sample (0.99-1.02 PFLOP/s of bf16 products, 0.40-0.41 of the
// spec), 1.34-1.37 ms at 12;
// matrix pipe busy 62 %, waves waiting on instruction dependencies 66 % of their cycles; LDS bank conflicts present, not located.
// Training (gd4d_depth_net_train.hip has the rest): depth_conv_kernel<EPI> - the same GEMM with a second epilogue that stores
// y = conv + bias and each tile's per-channel (mean, M2) (125 VGPRs, no scratch) and a third, plain-store one (121 VGPRs, no scratch)
// that is also the input gradient: gd4d_depth_net_image_mode(transposed = 1) lays out w'[ic, oc, 2 - ky, 2 - kx] = w[oc, ic, ky, kx].
// The FPN neck (gd4d_fpn.hip has its other kernels): gd4d_fpn_conv_fwd is two more epilogues of this GEMM, DN_EPI_LEVELS (plain store,
// NCHW) and DN_EPI_LEVELS_CL (the tile stored channels-last, (N, H, W, 256): a lane's 16 channels as four 16-byte runs), in which the
// tile's LEVEL picks the weight image and the bias (level_image / level_bias; the other epilogues never read them and compile to the
// code they were: second instantiations, not a shared one).
// Left off: padding the stages, two workgroups per CU, fusing the epilogue into the position embedding's gate / fuse kernel.
#include "gd4d_common.h"
#include "gd4d_bf16x3.h"
#include "gd4d_conv_common.h"

namespace gd4d {

constexpr int DN_C = 256, DN_KC = 32, DN_CHUNKS = DN_C / DN_KC, DN_TAPS = 9, DN_STEPS = DN_CHUNKS * DN_TAPS;
constexpr int DN_T = 16, DN_HE = DN_T + 2, DN_HALO = DN_HE * DN_HE;          // 16 x 16 tile, 18 x 18 halo
constexpr int DN_THREADS = 1024;
constexpr int DN_W_ARR = 4 * DN_C * 16;                                      // one plane of a step's weights: 16 KB
constexpr int DN_W_STAGE = 2 * DN_W_ARR;                                     // hi + lo: 32 KB
constexpr int DN_H_ARR = 4 * DN_HALO * 16;                                   // one plane of a chunk's halo: 20 736 B
constexpr int DN_H_STAGE = 2 * DN_H_ARR;
constexpr int DN_H_ITEMS = 4 * DN_HALO;                                      // (k-group, halo pixel) items of 8 channels: 1296
constexpr int DN_H_PASSES = (DN_H_ITEMS + DN_THREADS - 1) / DN_THREADS;      // 2
constexpr int DN_EPI = 5 * DN_C * 4;                                         // bias, mean, scale, beta, gate: 5 KB
constexpr int DN_LDS = 2 * DN_W_STAGE + 2 * DN_H_STAGE + DN_EPI;             // 153 600 B
constexpr size_t DN_IMAGE_BYTES = (size_t)DN_STEPS * DN_W_STAGE;             // 2 359 296 B
constexpr int DN_MAX_LEVELS = 4;

static_assert(DN_LDS <= 160 * 1024, "LDS budget of a CU");

// ---- camera gate ------------------------------------------------------------------------------------------------------------
struct CamGateParams {
  const float* intrin;     // (N, 16)
  const float* ida00;      // (n_ida): ida[..., 0, 0]
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *red_w, *red_b, *exp_w, *exp_b;
  float* gate;             // (N, 256)
  float scale;
  int n_ida;
};

// one output channel c of y = b + W v (W (256, 256) row-major), fp32, K in order
__device__ __forceinline__ float dn_row_dot(const float* __restrict__ w, const float* __restrict__ b, const float* v, int c) {
  float acc = 0.f;
  const float4* row = reinterpret_cast<const float4*>(w + (size_t)c * DN_C);
#pragma unroll 8
  for (int j = 0; j < DN_C / 4; ++j) {
    const float4 q = row[j];
    acc = fmaf(q.x, v[4 * j], acc);
    acc = fmaf(q.y, v[4 * j + 1], acc);
    acc = fmaf(q.z, v[4 * j + 2], acc);
    acc = fmaf(q.w, v[4 * j + 3], acc);
  }
  return acc + b[c];
}

__global__ __launch_bounds__(DN_C) void cam_gate_kernel(const CamGateParams p) {
  __shared__ float s_scaled;
  __shared__ float v0[DN_C], v1[DN_C];
  const int cam = blockIdx.x, c = threadIdx.x;
  if (c == 0) {
    // torch.inverse of the camera's 4x4 intrinsics (viewpad), fp32: Gauss-Jordan with partial pivoting
    float a[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[r][k] = p.intrin[cam * 16 + 4 * r + k];
        a[r][4 + k] = r == k ? 1.f : 0.f;
      }
#pragma unroll
    for (int col = 0; col < 4; ++col) {
      int piv = col;
#pragma unroll
      for (int r = col + 1; r < 4; ++r)
        if (fabsf(a[r][col]) > fabsf(a[piv][col])) piv = r;
      if (piv != col)
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float t = a[col][k]; a[col][k] = a[piv][k]; a[piv][k] = t; }
      const float inv = 1.f / a[col][col];
#pragma unroll
      for (int k = 0; k < 8; ++k) a[col][k] *= inv;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r != col) {
          const float f = a[r][col];
#pragma unroll
          for (int k = 0; k < 8; ++k) a[r][k] -= f * a[col][k];
        }
    }
    const float i00 = a[0][4], i11 = a[1][5];
    const float pixel = sqrtf(i00 * i00 + i11 * i11);                   // torch.norm(stack([inv[0,0], inv[1,1]]))
    const float d = p.ida00[p.n_ida == 1 ? 0 : cam];
    // :93-94 reads ida[..., 0, 0] TWICE (not [0,0] and [1,1]): reproduced as written
    const float aug = sqrtf(d * d + d * d);
    s_scaled = pixel * p.scale / aug;
  }
  __syncthreads();
  const float s = s_scaled;
  v0[c] = fmaxf(s * p.fc1_w[c] + p.fc1_b[c], 0.f);                      // mlp.fc1 (1 -> 256) + ReLU
  __syncthreads();
  v1[c] = dn_row_dot(p.fc2_w, p.fc2_b, v0, c);                          // mlp.fc2 (no activation after it)
  __syncthreads();
  const float r = fmaxf(dn_row_dot(p.red_w, p.red_b, v1, c), 0.f);      // se.conv_reduce + ReLU
  __syncthreads();                                                      // (every read of v0 above is done)
  v0[c] = r;
  __syncthreads();
  const float e = dn_row_dot(p.exp_w, p.exp_b, v0, c);                  // se.conv_expand
  p.gate[cam * DN_C + c] = 1.f / (1.f + expf(-e));                      // se.gate
}

// ---- the 3x3 convolution -----------------------------------------------------------------------------------------------------
struct DepthConvParams {
  const float* x[DN_MAX_LEVELS];
  float* out[DN_MAX_LEVELS];
  int h[DN_MAX_LEVELS], w[DN_MAX_LEVELS], tiles_x[DN_MAX_LEVELS], tiles_cam[DN_MAX_LEVELS], start[DN_MAX_LEVELS];
  const char* image;
  const float *bias, *mean, *var, *gamma, *beta, *gate;
  float* partials;         // DN_EPI_STATS: (tiles, 2, 256) per-tile mean and M2 of y, tiles in grid order
  float eps;
  int levels;
  const char* level_image[DN_MAX_LEVELS];   // DN_EPI_LEVELS / DN_EPI_LEVELS_CL: a weight image and a bias (or null) per level
  const float* level_bias[DN_MAX_LEVELS];
};

// The epilogues of the one implicit GEMM.  INFER: + bias, BatchNorm (running statistics), ReLU, x gate.  STATS (training forward):
// stores y = conv + bias and each channel's (mean, M2) over the tile's valid pixels, summed in a fixed order (lanes by an xor
// butterfly, then the four pixel waves).  PLAIN: stores conv (+ bias when given): the frozen-BatchNorm forward and the input gradient.
// LEVELS / LEVELS_CL (the FPN neck's output convolutions): PLAIN with the level's own image and bias, stored NCHW / channels-last.
enum { DN_EPI_INFER = 0, DN_EPI_STATS = 1, DN_EPI_PLAIN = 2, DN_EPI_LEVELS = 3, DN_EPI_LEVELS_CL = 4 };

template <int EPI>
__global__ __launch_bounds__(DN_THREADS) void depth_conv_kernel(const DepthConvParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wbuf = smem;                                   // [2][hi, lo][4][256][16 B]
  char* const hbuf = smem + 2 * DN_W_STAGE;                  // [2][hi, lo][4][324][16 B]
  float* const e_bias = reinterpret_cast<float*>(hbuf + 2 * DN_H_STAGE);
  float* const e_mean = e_bias + DN_C;
  float* const e_scale = e_mean + DN_C;
  float* const e_beta = e_scale + DN_C;
  float* const e_gate = e_beta + DN_C;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;                   // wm: 64 output channels, wn: 64 pixels (4 tile rows)
  const int l32 = lane & 31, kg = lane >> 5;

  // work item: (level, camera, tile row, tile column)
  const int t = blockIdx.x;
  int lv = 0;
#pragma unroll
  for (int l = 1; l < DN_MAX_LEVELS; ++l)
    if (l < p.levels && t >= p.start[l]) lv = l;
  const int H = p.h[lv], W = p.w[lv];
  const size_t HW = (size_t)H * W;
  const int local = t - p.start[lv];
  const int cam = local / p.tiles_cam[lv];
  const int rt = local - cam * p.tiles_cam[lv];
  const int ty0 = (rt / p.tiles_x[lv]) * DN_T, tx0 = (rt % p.tiles_x[lv]) * DN_T;
  const float* const xin = p.x[lv] + (size_t)cam * DN_C * HW;

  if (EPI == DN_EPI_INFER) {
    if (tid < DN_C) {
      const float sc = p.gamma[tid] / sqrtf(p.var[tid] + p.eps);
      e_bias[tid] = p.bias[tid];
      e_mean[tid] = p.mean[tid];
      e_scale[tid] = sc;
      e_beta[tid] = p.beta[tid];
      e_gate[tid] = p.gate[cam * DN_C + tid];
    }
  } else if (tid < DN_C) {
    const float* const b = EPI >= DN_EPI_LEVELS ? p.level_bias[lv] : p.bias;
    e_bias[tid] = b ? b[tid] : 0.f;
  }
  const char* const image = EPI >= DN_EPI_LEVELS ? p.level_image[lv] : p.image;

  // halo staging role: item it = (k-group, halo pixel); 8 channels of one pixel, zero outside the image
  const float* h_src[DN_H_PASSES];
  bool h_in[DN_H_PASSES], h_live[DN_H_PASSES];
#pragma unroll
  for (int ps = 0; ps < DN_H_PASSES; ++ps) {
    const int it = tid + DN_THREADS * ps;
    h_live[ps] = it < DN_H_ITEMS;
    const int kgrp = it / DN_HALO, hp = it % DN_HALO;
    const int y = ty0 - 1 + hp / DN_HE, x = tx0 - 1 + hp % DN_HE;
    h_in[ps] = h_live[ps] && y >= 0 && y < H && x >= 0 && x < W;
    h_src[ps] = xin + (size_t)(kgrp * 8) * HW + (h_in[ps] ? (size_t)y * W + x : 0);
  }
  float hr[8];                                               // one pass of the halo in flight at a time
  auto issue_halo = [&](int chunk, int ps) {
#pragma unroll
    for (int j = 0; j < 8; ++j) hr[j] = h_in[ps] ? h_src[ps][(size_t)(chunk * DN_KC + j) * HW] : 0.f;
  };
  auto park_halo = [&](int buf, int ps) {
    if (h_live[ps]) {
      char* base = hbuf + buf * DN_H_STAGE;
      const int off = (tid + DN_THREADS * ps) * 16;
      u32x4 hi, lo;
      split8(hr, hi, lo);
      *reinterpret_cast<u32x4*>(base + off) = hi;
      *reinterpret_cast<u32x4*>(base + DN_H_ARR + off) = lo;
    }
  };
  u32x4 wr[2];
  auto issue_w = [&](int s) {
    const char* src = image + (size_t)s * DN_W_STAGE + tid * 16;
    wr[0] = *reinterpret_cast<const u32x4*>(src);
    wr[1] = *reinterpret_cast<const u32x4*>(src + DN_W_ARR);
  };
  auto park_w = [&](int buf) {
    char* base = wbuf + buf * DN_W_STAGE + tid * 16;
    *reinterpret_cast<u32x4*>(base) = wr[0];
    *reinterpret_cast<u32x4*>(base + DN_W_ARR) = wr[1];
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  // B fragments: pixel p = 64 wn + 32 ni + l32 of the tile -> (py, px); its halo entry for tap (ky, kx) is (py + ky) * 18 + px + kx
  int pix_hp[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int pp = 64 * wn + 32 * ni + l32;
    pix_hp[ni] = (pp >> 4) * DN_HE + (pp & 15);
  }

#pragma unroll
  for (int ps = 0; ps < DN_H_PASSES; ++ps) {
    issue_halo(0, ps);
    park_halo(0, ps);
  }
  issue_w(0);
  park_w(0);
  issue_w(1);
  __syncthreads();
  for (int chunk = 0; chunk < DN_CHUNKS; ++chunk) {
    const char* hb = hbuf + (chunk & 1) * DN_H_STAGE;
#pragma unroll
    for (int tap = 0; tap < DN_TAPS; ++tap) {
      const int s = chunk * DN_TAPS + tap;
      // the next chunk's halo, pass ps: loaded before tap 2 + 3 ps, in flight under three steps of MFMAs, parked after tap 4 + 3 ps
      const bool more = chunk + 1 < DN_CHUNKS;
#pragma unroll
      for (int ps = 0; ps < DN_H_PASSES; ++ps)
        if (more && tap == 2 + 3 * ps) issue_halo(chunk + 1, ps);
      const char* wb = wbuf + (s & 1) * DN_W_STAGE;
      const int tap_off = (tap / 3) * DN_HE + tap % 3;
#pragma unroll 1                                       // (unrolled, the compiler hoists both halves' 64 fragment registers: 67 spilled)
      for (int ks = 0; ks < 2; ++ks) {
        const int kgrp = 2 * ks + kg;
        u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int aoff = (kgrp * DN_C + 64 * wm + 32 * i + l32) * 16;
          const int boff = (kgrp * DN_HALO + pix_hp[i] + tap_off) * 16;
          ah[i] = *reinterpret_cast<const u32x4*>(wb + aoff);
          al[i] = *reinterpret_cast<const u32x4*>(wb + DN_W_ARR + aoff);
          bh[i] = *reinterpret_cast<const u32x4*>(hb + boff);
          bl[i] = *reinterpret_cast<const u32x4*>(hb + DN_H_ARR + boff);
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma_32x32x16_x3(ah[mi], al[mi], bh[ni], bl[ni], acc[mi][ni]);
      }
      if (s + 1 < DN_STEPS) {
        park_w((s + 1) & 1);                                  // its readers finished before the last barrier
#pragma unroll
        for (int ps = 0; ps < DN_H_PASSES; ++ps)             // its buffer was last read in chunk - 1
          if (more && tap == 4 + 3 * ps) park_halo((chunk + 1) & 1, ps);
        if (s + 2 < DN_STEPS) issue_w(s + 2);
      }
      __syncthreads();
    }
  }

  // C/D of 32x32x16: column (pixel) = l32, rows (channels) 4 kg + (r & 3) + 8 (r >> 2)
  float* const outp = p.out[lv] + (size_t)cam * DN_C * HW;
  if (EPI == DN_EPI_INFER) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int pp = 64 * wn + 32 * ni + l32;
      const int y = ty0 + (pp >> 4), x = tx0 + (pp & 15);
      if (y >= H || x >= W) continue;
      float* const o = outp + (size_t)y * W + x;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = 64 * wm + 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
          float v = acc[mi][ni][r] + e_bias[c];                 // conv bias
          v = (v - e_mean[c]) * e_scale[c] + e_beta[c];          // BatchNorm2d, eval (running statistics)
          v = fmaxf(v, 0.f);                                     // ReLU
          o[(size_t)c * HW] = v * e_gate[c];                     // SELayer: x * gate
        }
    }
  } else if (EPI == DN_EPI_LEVELS_CL) {
    float* const outc = p.out[lv] + (size_t)cam * HW * DN_C;  // (N, H, W, 256)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int pp = 64 * wn + 32 * ni + l32;
      const int y = ty0 + (pp >> 4), x = tx0 + (pp & 15);
      if (y >= H || x >= W) continue;
      float* const o = outc + ((size_t)y * W + x) * DN_C;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = 64 * wm + 32 * mi + 4 * kg + 8 * q;     // registers 4 q .. 4 q + 3: channels c .. c + 3
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = acc[mi][ni][4 * q + j] + e_bias[c + j];
          *reinterpret_cast<f32x4*>(o + c) = v;
        }
    }
  } else {
    // (the main loop's last barrier is behind every wave: the stages are free)
    float* const red = reinterpret_cast<float*>(smem);          // [4 pixel waves][256]
    float* const tmean = red + 4 * DN_C;                        // [256]
    bool ok[2];
    size_t off[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int pp = 64 * wn + 32 * ni + l32;
      const int y = ty0 + (pp >> 4), x = tx0 + (pp & 15);
      ok[ni] = y < H && x < W;
      off[ni] = ok[ni] ? (size_t)y * W + x : 0;
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 64 * wm + 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
        float s = 0.f;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const float v = acc[mi][ni][r] + e_bias[c];
          acc[mi][ni][r] = v;
          if (ok[ni]) {
            outp[(size_t)c * HW + off[ni]] = v;
            s += v;
          }
        }
        if (EPI == DN_EPI_STATS) {
          s = half_wave_sum(s);
          if (l32 == 0) red[wn * DN_C + c] = s;
        }
      }
    if (EPI == DN_EPI_STATS) {
      const int vh = min(DN_T, H - ty0), vw = min(DN_T, W - tx0);
      __syncthreads();
      if (tid < DN_C) tmean[tid] = ((red[tid] + red[DN_C + tid]) + (red[2 * DN_C + tid] + red[3 * DN_C + tid])) / (float)(vh * vw);
      __syncthreads();
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = 64 * wm + 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
          const float m = tmean[c];
          float s = 0.f;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const float d = acc[mi][ni][r] - m;
            if (ok[ni]) s += d * d;
          }
          s = half_wave_sum(s);
          if (l32 == 0) red[wn * DN_C + c] = s;                 // (tmean is read above, red's sums were consumed before the barrier)
        }
      __syncthreads();
      if (tid < DN_C) {
        float* const part = p.partials + (size_t)t * 2 * DN_C;
        part[tid] = tmean[tid];
        part[DN_C + tid] = (red[tid] + red[DN_C + tid]) + (red[2 * DN_C + tid] + red[3 * DN_C + tid]);
      }
    }
  }
}

}  // namespace gd4d

extern "C" size_t gd4d_depth_net_image_bytes(int channels) { return channels == gd4d::DN_C ? gd4d::DN_IMAGE_BYTES : 0; }

extern "C" int gd4d_depth_net_image_mode(const float* conv_w, int channels, int transposed, void* image, void* stream) {
  using namespace gd4d;
  if (!conv_w || !image) return GD4D_EINVAL;
  if (channels != DN_C || (transposed != 0 && transposed != 1)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  // transposed (the input gradient's image): w'[ic, oc, 2 - ky, 2 - kx] = w[oc, ic, ky, kx], so the same kernel run on dy gives dx
  const ConvImage d{DN_C, DN_C, DN_TAPS, DN_C, DN_KC, DN_C, 0, transposed, transposed};
  return pack_conv_image(d, conv_w, image, static_cast<hipStream_t>(stream));
}

extern "C" int gd4d_depth_net_image(const float* conv_w, int channels, void* image, void* stream) {
  return gd4d_depth_net_image_mode(conv_w, channels, 0, image, stream);
}

extern "C" int gd4d_cam_gate_fwd(const float* intrinsics, const float* ida00, int n, int n_ida, float scale_depth_factor,
                                 const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b, const float* se_reduce_w,
                                 const float* se_reduce_b, const float* se_expand_w, const float* se_expand_b, int channels, float* gate,
                                 void* stream) {
  using namespace gd4d;
  if (!intrinsics || !ida00 || !fc1_w || !fc1_b || !fc2_w || !fc2_b || !se_reduce_w || !se_reduce_b || !se_expand_w || !se_expand_b ||
      !gate)
    return GD4D_EINVAL;
  if (channels != DN_C || n <= 0 || (n_ida != 1 && n_ida != n)) return GD4D_EUNSUPPORTED;
  if (!aligned16(fc2_w) || !aligned16(se_reduce_w) || !aligned16(se_expand_w)) return GD4D_EALIGN;
  CamGateParams p{intrinsics, ida00, fc1_w, fc1_b, fc2_w, fc2_b, se_reduce_w, se_reduce_b, se_expand_w, se_expand_b, gate,
                  scale_depth_factor, n_ida};
  hipLaunchKernelGGL(cam_gate_kernel, dim3(n), dim3(DN_C), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

namespace gd4d {

// the level table and the tile count of a launch; GD4D_OK or the error code
static int depth_conv_levels(DepthConvParams& p, const float* const* x, float* const* out, const int32_t* level_hw, int levels, int n,
                             long long& tiles) {
  tiles = 0;
  for (int l = 0; l < levels; ++l) {
    const int h = level_hw[2 * l], w = level_hw[2 * l + 1];
    if (!x[l] || !out[l] || h <= 0 || w <= 0) return GD4D_EINVAL;
    if ((long long)n * DN_C * h * w > (1ll << 40)) return GD4D_EUNSUPPORTED;
    p.x[l] = x[l];
    p.out[l] = out[l];
    p.h[l] = h;
    p.w[l] = w;
    p.tiles_x[l] = (w + DN_T - 1) / DN_T;
    p.tiles_cam[l] = p.tiles_x[l] * ((h + DN_T - 1) / DN_T);
    p.start[l] = (int)tiles;
    tiles += (long long)n * p.tiles_cam[l];
    if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  }
  p.levels = levels;
  return GD4D_OK;
}

template <int EPI>
static int depth_conv_launch(const DepthConvParams& p, long long tiles, void* stream) {
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(depth_conv_kernel<EPI>), DN_LDS)) return GD4D_ELAUNCH;
  hipLaunchKernelGGL(depth_conv_kernel<EPI>, dim3((unsigned)tiles), dim3(DN_THREADS), DN_LDS, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

}  // namespace gd4d

extern "C" int gd4d_depth_conv_fwd(const float* const* x, float* const* out, const int32_t* level_hw, int levels, int n, int channels,
                                   const void* image, const float* bias, const float* bn_mean, const float* bn_var,
                                   const float* bn_weight, const float* bn_bias, float eps, const float* gate, void* stream) {
  using namespace gd4d;
  if (!x || !out || !level_hw || !image || !bias || !bn_mean || !bn_var || !bn_weight || !bn_bias || !gate) return GD4D_EINVAL;
  if (channels != DN_C || levels < 1 || levels > DN_MAX_LEVELS || n <= 0) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  DepthConvParams p{};
  long long tiles = 0;
  const int code = depth_conv_levels(p, x, out, level_hw, levels, n, tiles);
  if (code != GD4D_OK) return code;
  p.image = static_cast<const char*>(image);
  p.bias = bias;
  p.mean = bn_mean;
  p.var = bn_var;
  p.gamma = bn_weight;
  p.beta = bn_bias;
  p.gate = gate;
  p.eps = eps;
  return depth_conv_launch<DN_EPI_INFER>(p, tiles, stream);
}

extern "C" long long gd4d_depth_conv_tiles(const int32_t* level_hw, int levels, int n) {
  if (!level_hw || levels < 1 || n <= 0) return 0;
  long long tiles = 0;
  for (int l = 0; l < levels; ++l) {
    const int h = level_hw[2 * l], w = level_hw[2 * l + 1];
    if (h <= 0 || w <= 0) return 0;
    tiles += (long long)n * ((h + gd4d::DN_T - 1) / gd4d::DN_T) * ((w + gd4d::DN_T - 1) / gd4d::DN_T);
  }
  return tiles;
}

extern "C" int gd4d_depth_conv_raw(const float* const* x, float* const* y, const int32_t* level_hw, int levels, int n, int channels,
                                   const void* image, const float* bias, float* partials, void* stream) {
  using namespace gd4d;
  if (!x || !y || !level_hw || !image) return GD4D_EINVAL;
  if (channels != DN_C || levels < 1 || levels > DN_MAX_LEVELS || n <= 0) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  DepthConvParams p{};
  long long tiles = 0;
  const int code = depth_conv_levels(p, x, y, level_hw, levels, n, tiles);
  if (code != GD4D_OK) return code;
  p.image = static_cast<const char*>(image);
  p.bias = bias;
  p.partials = partials;
  return partials ? depth_conv_launch<DN_EPI_STATS>(p, tiles, stream) : depth_conv_launch<DN_EPI_PLAIN>(p, tiles, stream);
}

// The FPN neck's 3x3 output convolutions (mmdet FPN.fpn_convs; CPFPN keeps level 0's only): the plain-store GEMM above with a weight
// image and a bias per level, all levels in one launch.
extern "C" int gd4d_fpn_conv_fwd(const float* const* x, float* const* out, const int32_t* level_hw, int levels, int n, int channels,
                                 const void* const* images, const float* const* biases, int out_channels_last, void* stream) {
  using namespace gd4d;
  if (!x || !out || !level_hw || !images) return GD4D_EINVAL;
  if (channels != DN_C || levels < 1 || levels > DN_MAX_LEVELS || n <= 0 || (out_channels_last != 0 && out_channels_last != 1))
    return GD4D_EUNSUPPORTED;
  DepthConvParams p{};
  long long tiles = 0;
  const int code = depth_conv_levels(p, x, out, level_hw, levels, n, tiles);
  if (code != GD4D_OK) return code;
  for (int l = 0; l < levels; ++l) {
    if (!images[l]) return GD4D_EINVAL;
    if (!aligned16(images[l]) || (out_channels_last && !aligned16(out[l]))) return GD4D_EALIGN;
    p.level_image[l] = static_cast<const char*>(images[l]);
    p.level_bias[l] = biases ? biases[l] : nullptr;
  }
  return out_channels_last ? depth_conv_launch<DN_EPI_LEVELS_CL>(p, tiles, stream) : depth_conv_launch<DN_EPI_LEVELS>(p, tiles, stream);
}
