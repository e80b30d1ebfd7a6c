// The two weight-gradient GEMM bodies of the convolution families, each written once and instantiated per family by a compile-time
// policy (as vv_gemm_kernel<MT, MODE, EPI> and the row-chain body are per shape).  Both are GEMMs whose K runs over the pixels, on
// the split-bf16 x 3 MFMA (gd4d_bf16x3.h): the MFMA's k index is the pixel, and both operands want 8 consecutive pixels of one
// channel per lane - NCHW as it lies.  The gradient dy (the A operand) is read by exactly one wave of a workgroup, so it goes from
// global memory to registers, is split there and never touches LDS; the input x (the B operand) is shared by the waves and staged in
// LDS, split hi / lo.  The (image, tile) list is cut into P partitions (partition_range); a workgroup walks its partition's tiles in
// order and stores its partial sums into its own slab of a workspace (an empty partition stores zeros), and a second kernel of the
// family adds the P slabs in order.  No atomics anywhere: every sum has a fixed order, two runs give the same bits.
//
//   kernel                     body      policy              BSUM   what the policy fixes
//   depth_wgrad_kernel         3x3       DepthWgradShape     no     256 / 256 channels, 512 threads, tiles of a list of up to 4 levels
//   vt_conv3x3_wgrad_kernel    3x3       VvWgradShape        yes    run-time Cin / Cout / blockDim, tiles of one map
//   fpn_lateral_wgrad_kernel   1x1       LateralWgradShape   yes    256 output channels (no guard), one source map
//   vt_osa_wgrad_kernel        1x1       OsaWgradShape       no     blocks of 256 output channels (guarded), up to VV_MAX_SRC source maps
//   rt_conv3x3_wgrad_kernel    3x3       RtWgradShape        yes    as VvWgradShape, Cout in blocks of up to 256 along blockIdx.y (ResNet)
//   rt_conv1x1_wgrad_kernel    1x1       RtPwWgradShape      yes    blocks of 256 output channels (guarded), x read at stride 1 or 2 (ResNet)
//
// conv3x3_wgrad_body: dW[oc, ic, ky, kx] = sum over tiles and pixels of dy[oc, p] x[ic, p + (ky - 1, kx - 1)].
//   Grid (Cin / 32 chunks of input channels) x P, a tile is 16 x 16 pixels.  A workgroup of Cout / 32 waves owns Cout output
//   channels x 32 input channels x 9 taps: wave w the output channels 32 w .. 32 w + 31 and nine 32 x 32 accumulators (144
//   registers).  One K step of 16 is one row of the tile; dy's row is loaded a row ahead.  The chunk's 18 x 18 halo of x is staged
//   once per tile as THREE copies, one per kx, each shifted by kx pixels ([kx][plane hi, lo][32 channels][18 rows][16 pixels] bf16,
//   rows of 32 B, channels 18 * 32 + 16 = 592 B apart so that 16 lanes of a read fall on 16 distinct slots): tap (ky, kx) of tile row
//   py is then the aligned 16-B read at (row py + ky, pixels 8 kg ..) of copy kx.  Zero fill outside the image makes the padding and
//   the ragged tiles exact; pixels of dy outside the image are zeros.  111 KB of LDS, one workgroup per CU.  Partials go to a
//   (P, 9, Cout, Cin) workspace.  BSUM: a lane also adds the 8 dy values of each row it loads (in pixel order, rows and tiles in
//   order), the two halves of a row are added (pixels 0-7 first) and the workgroups of chunk 0 store (P, Cout).
//   Untuned: dy is read once per input-channel chunk (Cin / 32 times).
//
// conv1x1_wgrad_body: dW[oc, ic] = sum over tiles and pixels of dy[oc, p] x[ic, p].
//   Grid (chunks of 64 input channels x P) x (blocks of 256 output channels), a tile is 64 consecutive pixels of an image.  A
//   workgroup of 4 waves owns 256 output channels x 64 input channels: wave w the output channels 64 w .. 64 w + 63 of the block and
//   2 x 2 accumulators of 32 x 32.  The tile's 64-channel x 64-pixel block of x is staged once ([plane hi, lo][channel][8-pixel
//   group], channels 9 units of 16 B apart): a thread loads 16 pixels of one channel (issue) before the previous tile's MFMAs and
//   splits and stores them after (park).  Four K steps of 16 pixels per tile.  Pixels past the map and channels past K are zeros.
//   Partials go to a (P, Cout, K) workspace.  BSUM: as above per K step, stored by the workgroups of chunk 0 into (P, Cout).
//   Untuned: dy is read once per input-channel chunk (K / 64 times): at K = 512 that, not the MFMA, is what the kernel waits for.
#pragma once
#include "gd4d_bf16x3.h"
#include "gd4d_conv_common.h"

namespace gd4d {

// ---- 3x3 ------------------------------------------------------------------------------------------------------------------------
constexpr int CW3_T = 16, CW3_KC = 32, CW3_HE = CW3_T + 2;
constexpr int CW3_CH_STRIDE = CW3_HE * 32 + 16;               // 18 rows of 16 bf16 + 16 B: 16 lanes of a read on 16 distinct slots
constexpr int CW3_PLANE = CW3_KC * CW3_CH_STRIDE;             // 18 944 B
constexpr int CW3_LDS = 3 * 2 * CW3_PLANE;                    // 113 664 B
constexpr int CW3_ITEMS = 3 * CW3_KC * CW3_HE * 2;            // (kx, channel, halo row, 8-pixel half): 3456
static_assert(CW3_LDS <= 160 * 1024, "LDS budget of a CU");

struct Conv3x3Tile {
  int H, W, ty0, tx0;              // the tile's map and its first pixel
  const float* x;                  // x at (image, chunk * 32)
  const float* dy;                 // dy at (image, oc_a)
};

// Shape: cin(), cout(), chunks() = cin() / 32, threads() (the workgroup's, 64 cout() / 32), tile(t, chunk, oc_a) -> Conv3x3Tile, and
// p with tiles, partitions, ws (and ws_b when BSUM).
template <typename Shape, bool BSUM>
__device__ __forceinline__ void conv3x3_wgrad_body(const Shape& s, char* smem) {
  const int tid = threadIdx.x, threads = s.threads();
  const int lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, kg = lane >> 5;
  const int chunk = blockIdx.x % s.chunks(), part = blockIdx.x / s.chunks();
  int t_begin, t_end;
  partition_range(part, s.p.tiles, s.p.partitions, t_begin, t_end);

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  const int oc_a = 32 * wave + l32;                          // the A operand's row of this lane
  for (int t = t_begin; t < t_end; ++t) {
    const Conv3x3Tile g = s.tile(t, chunk, oc_a);
    const int H = g.H, W = g.W, ty0 = g.ty0, tx0 = g.tx0;
    const size_t HW = (size_t)H * W;

    // one row of the dy tile: 8 pixels of this lane's output channel, zeros outside the image
    auto load_dy = [&](int py, float* v) {
      const int y = ty0 + py;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = tx0 + 8 * kg + j;
        v[j] = (y < H && x < W) ? g.dy[(size_t)y * W + x] : 0.f;
      }
    };
    float a_next[8];
    load_dy(0, a_next);

    __syncthreads();                                         // the previous tile's readers are done
    for (int it = tid; it < CW3_ITEMS; it += threads) {
      const int half = it & 1, q = it >> 1;
      const int hy = q % CW3_HE, q2 = q / CW3_HE;
      const int ic = q2 % CW3_KC, kx = q2 / CW3_KC;
      const int y = ty0 - 1 + hy, x0 = tx0 - 1 + kx + 8 * half;
      const bool row_in = y >= 0 && y < H;
      const float* src = g.x + (size_t)ic * HW + (row_in ? (size_t)y * W : 0);
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = x0 + j;
        v[j] = (row_in && x >= 0 && x < W) ? src[x] : 0.f;
      }
      u32x4 hi, lo;
      split8(v, hi, lo);
      char* dst = smem + (size_t)(kx * 2) * CW3_PLANE + ic * CW3_CH_STRIDE + hy * 32 + half * 16;
      *reinterpret_cast<u32x4*>(dst) = hi;
      *reinterpret_cast<u32x4*>(dst + CW3_PLANE) = lo;
    }
    __syncthreads();

    const char* const bbase = smem + l32 * CW3_CH_STRIDE + kg * 16;
#pragma unroll 1
    for (int py = 0; py < CW3_T; ++py) {
      u32x4 ah, al;
      split8(a_next, ah, al);
      if constexpr (BSUM) {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += a_next[j];
        bsum += sum;
      }
      if (py + 1 < CW3_T) load_dy(py + 1, a_next);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const char* b = bbase + (kx * 2) * CW3_PLANE + (py + ky) * 32;
          const u32x4 bh = *reinterpret_cast<const u32x4*>(b);
          const u32x4 bl = *reinterpret_cast<const u32x4*>(b + CW3_PLANE);
          acc[3 * ky + kx] = mfma_32x32x16_x3(ah, al, bh, bl, acc[3 * ky + kx]);
        }
    }
  }

  // column (input channel) = l32, rows (output channels) by mfma32_row
  float* const ws = s.p.ws + (size_t)part * 9 * s.cout() * s.cin();
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = mfma32_row(kg, r, 32 * wave);
      ws[((size_t)t * s.cout() + oc) * s.cin() + chunk * CW3_KC + l32] = acc[t][r];
    }
  if constexpr (BSUM) {
    const float other = __shfl_xor(bsum, 32);
    if (chunk == 0 && kg == 0) s.p.ws_b[(size_t)part * s.cout() + oc_a] = bsum + other;        // pixels 0-7 of a row, then 8-15
  }
}

// ---- 1x1 ------------------------------------------------------------------------------------------------------------------------
constexpr int CW1_THREADS = 256, CW1_PX = 64, CW1_IC = 64, CW1_OC = 256;
constexpr int CW1_PITCH = 9;                           // 16-byte units per channel of the staged block: 8 pixel groups + 1
constexpr int CW1_B_ARR = CW1_IC * CW1_PITCH;

struct Conv1x1Wgrad {              // what both families pass from their parameter structs
  const float* dy;                 // (N, cout, HW)
  float* ws;                       // (P, cout, k)
  float* ws_b;                     // (P, cout), BSUM only
  int k, hw, tiles_img, tiles, partitions, chunks;
};

struct Conv1x1Source {             // where a staged channel lies
  const float* base;               // its map, (N, channels, HW)
  int channels, local;
};

// Shape: g (a Conv1x1Wgrad), cout(), GUARD (output channels past cout() exist in the block and are skipped), oc0(wave) (the wave's
// first output channel), source(channel of K, whether it is < k) -> Conv1x1Source, and where pixel p of dy's map lies in x's:
// x_plane() (the pixels of one channel of x) and x_pixel(p) (p itself, or the input pixel (2 yo, 2 xo) under output pixel p of a
// stride-2 convolution).  s_b: [hi, lo][channel][pixel group (+ 1)].
template <typename Shape, bool BSUM>
__device__ __forceinline__ void conv1x1_wgrad_body(const Shape& s, u32x4 (&s_b)[2][CW1_B_ARR]) {
  const Conv1x1Wgrad& g = s.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
  const int chunk = blockIdx.x % g.chunks, part = blockIdx.x / g.chunks;
  const int oc0 = s.oc0(wave);
  int t_begin, t_end;
  partition_range(part, g.tiles, g.partitions, t_begin, t_end);
  const size_t HW = (size_t)g.hw;

  // staging role: thread = (channel of the chunk, 16 consecutive pixels of the tile)
  const int s_ic = tid >> 2, s_q = tid & 3;
  const int s_icg = chunk * CW1_IC + s_ic;
  const bool s_ic_ok = s_icg < g.k;
  const Conv1x1Source from = s.source(s_icg, s_ic_ok);
  float hr[16];
  auto issue = [&](int t) {
    const int cam = t / g.tiles_img, p0 = (t - cam * g.tiles_img) * CW1_PX + 16 * s_q;
    const float* src = from.base + ((size_t)cam * from.channels + from.local) * s.x_plane();
#pragma unroll
    for (int j = 0; j < 16; ++j) hr[j] = (s_ic_ok && p0 + j < g.hw) ? src[s.x_pixel(p0 + j)] : 0.f;
  };
  auto park = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4 hi, lo;
      split8(hr + 8 * h, hi, lo);
      s_b[0][s_ic * CW1_PITCH + 2 * s_q + h] = hi;
      s_b[1][s_ic * CW1_PITCH + 2 * s_q + h] = lo;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
  float bsum[2] = {0.f, 0.f};

  bool a_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) a_ok[i] = !Shape::GUARD || oc0 + 32 * i + l32 < s.cout();

  if (t_begin < t_end) issue(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();                                   // the previous tile's readers are done
    park();
    __syncthreads();
    if (t + 1 < t_end) issue(t + 1);
    const int cam = t / g.tiles_img, p0 = (t - cam * g.tiles_img) * CW1_PX;
    const float* const gp = g.dy + ((size_t)cam * s.cout() + (a_ok[0] ? oc0 + l32 : 0)) * HW;  // (a_ok[1] implies a_ok[0])
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int px = p0 + 16 * ks + 8 * kg;
      u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (a_ok[i] && px + j < g.hw) ? gp[(size_t)(32 * i) * HW + px + j] : 0.f;
        if constexpr (BSUM) {
          float sum = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) sum += a[j];
          bsum[i] += sum;
        }
        split8(a, ah[i], al[i]);
        bh[i] = s_b[0][(32 * i + l32) * CW1_PITCH + 2 * ks + kg];
        bl[i] = s_b[1][(32 * i + l32) * CW1_PITCH + 2 * ks + kg];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma_32x32x16_x3(ah[mi], al[mi], bh[ni], bl[ni], acc[mi][ni]);
    }
  }

  // column (input channel) = l32, rows (output channels) by mfma32_row
  float* const ws = g.ws + (size_t)part * s.cout() * g.k;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int ic = chunk * CW1_IC + 32 * ni + l32;
    if (ic >= g.k) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int oc = mfma32_row(kg, r, oc0 + 32 * mi);
        if (!Shape::GUARD || oc < s.cout()) ws[(size_t)oc * g.k + ic] = acc[mi][ni][r];
      }
  }
  if constexpr (BSUM) {
    if (chunk == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float other = __shfl_xor(bsum[i], 32);
        if (kg == 0 && a_ok[i]) g.ws_b[(size_t)part * s.cout() + oc0 + 32 * i + l32] = bsum[i] + other;   // pixels 0-7 of a step, then 8-15
      }
    }
  }
}

// The finishing launch VoVNet's and ResNet's weight gradients share (gd4d_vovnet_train.hip: vt_wgrad_finish_kernel, a workgroup per
// output channel): G = the partitions' slabs of ws (partitions, taps, cout, cin) added in order, dw[c] = scale[c] G[c], dbeta[c] = the
// parts_b rows of ws_b added in order, dgamma[c] = rstd[c] (<weight[c], G[c]> - mean[c] dbeta[c]); bn = (3, cout): scale, rstd, mean.
int vt_finish(const float* ws, const float* ws_b, int partitions, int parts_b, int cin, int cout, int taps, const float* weight,
              const float* bn, float* dw, float* dgamma, float* dbeta, hipStream_t s);

}  // namespace gd4d
