// Training of DCNv2 (gd4d_dcn.hip holds the forward; gd4d_dcn_common.h what both share).  Notation as there: tap k = 3 ky + kx,
// P_k(p) = (y s - 1 + ky + dy_k(p), x s - 1 + kx + dx_k(p)), m_k the modulation after the sigmoid, S[ci, k, p] = bilinear0(x[n, ci], P_k(p))
// the UNmodulated sample, corners at floor and floor + 1 with fractions ly, lx, a corner outside the image counting as value 0.  With
// dout the incoming gradient and y the forward's output:
//     g[co, p]     = dout[co, p] (y[co, p] > 0 when the forward applied its ReLU) (scale[co] when a BatchNorm was folded)
//     c[ci, k, p]  = sum_co w[co, ci, k] g[co, p]
//     dmod_k(p)    = sum_ci c S                      d(dy_k)(p) = m_k sum_ci c ((1 - lx)(v10 - v00) + lx (v11 - v01))
//     dX[ci, corner j of P_k(p)] += m_k wgt_j c      d(dx_k)(p) = m_k sum_ci c ((1 - ly)(v01 - v00) + ly (v11 - v10))
//     dW[co, ci, k] = sum_{n, p} g m_k S             dbias[co]  = sum_{n, p} g
// Floor and fraction are taken of the offset, as in the forward: at an integer sample coordinate (every offset of a fresh layer is
// exactly 0) the offset gradient is the derivative from the right - mmcv's convention, and what fp64 autograd through floor-based
// index arithmetic gives.
//
//   gd4d_dcn_weight_image_t   the weight (Cout, Cin, 3, 3) as the A operand of the data kernel: rows (tap, ci), K = Cout, split bf16 hi / lo,
//                             [tap][chunk of 32 ci][plane][k-group of 8 co][32 ci][8 x bf16]: 9 Cin Cout 4 bytes, no padding.
//   gd4d_dcn_bwd_data         c, the offset / modulation gradients and dX in ONE pass; c is never written to memory.  An implicit GEMM on
//                             the split-bf16 x 3 MFMA: M = 9 Cin (items of 32 rows: one tap, 32 input channels), N = a tile of 64 (Cout
//                             <= 256) or 32 consecutive output pixels of one image, K = Cout.  A workgroup of 8 waves owns a tile: the
//                             prologue forms g from dout, y and scale, splits it and parks it in LDS as B fragments (<= 64 KB); wave v
//                             takes the items v, v + 8, ...: A fragments straight from the image (L2-served, read once per tile), one
//                             32 x 32 accumulator per 32 pixels.  The epilogue of an item, c in the accumulators (lane = pixel, 16 of the
//                             32 channels): the (pixel, tap)'s corner geometry, the four corners of x per channel (global loads, lanes
//                             along the pixels), the three sums over its channels, and m wgt_j c added into dX with atomicAdd (float,
//                             vector lanes; corners outside the image and zero coefficients skipped).  The sums of a lane's two
//                             channel halves are added (low half first), then into the wave's own (27, pixels) LDS slab in item order;
//                             at the end the 8 slabs are added in wave order, the m / sigmoid factors applied and the 27-channel map
//                             written once.  So dX is the ONE output whose bits depend on the run (float atomics; the caller zeroes
//                             it); every other sum has a fixed order.
//   gd4d_dcn_wgrad            dW and dbias: M = Cout, N = (tap, 32 input channels), K = the pixels.  Grid: (9 Cin / 32 items) x P
//                             partitions of the (image, 64-pixel tile) list; a workgroup of 4 waves holds ALL Cout rows of its item
//                             (wave v: row tiles v, v + 4, ...), so each (tap, channel, pixel) is sampled by one workgroup - the
//                             sampling work is the forward's.  The B operand is the modulated sample recomputed as the forward's B stage
//                             does (the same coefficient and combine functions, corner loads at clamped addresses): thread = (pixel,
//                             8 channels), split and parked in LDS (8 KB); the A operand is g, 8 consecutive pixels of a channel per
//                             lane, formed in registers.  Partials go to a (P, Cout, Cin, 9) workspace (+ (P, Cout) for dbias, summed by
//                             the workgroups of item 0 from the g they read); a second kernel adds the P partials in order.  Partitions
//                             beyond the tile count write zeros.  No pipelining between sampling and MFMA (untuned).
//   gd4d_dcn_offset_conv_dgrad   dX += conv_transpose3x3(do, W_off): one thread per element of dX, a plain read-modify-write after the
//                             data kernel on the same stream; 243 fmaf in a fixed order.
//   gd4d_dcn_offset_conv_wgrad   dW_off (27, Cin, 3, 3) and db_off: M = 27 (one 32-row tile), N = (tap, 32 channels), K = pixels; one wave
//                             per (item, partition), both operands gathered from global memory; the same workspace scheme.
// Left open: a deterministic dX (a sorted-record form like the pyramid gradient's); staging A through LDS and a software pipeline in
// the data kernel (each wave waits for its own A loads); overlapping the weight gradient's sampling with its MFMAs; fusing the
// conv_offset kernels into these.
#include "gd4d_common.h"
#include "gd4d_bf16x3.h"
#include "gd4d_conv_common.h"
#include "gd4d_dcn_common.h"

namespace gd4d {

constexpr int DT_THREADS = 512, DT_WAVES = 8, DT_ROWS = 32;      // data kernel: 8 waves, items of 32 (tap, ci) rows
constexpr int DW_THREADS = 256, DW_PX = 64, DW_NC = 32;          // weight gradients: 64-pixel tiles, 32 input channels per item

// g of one element: dout, masked by the forward's ReLU (y > 0) and scaled by the folded BatchNorm
__device__ __forceinline__ float dcn_g(const float* __restrict__ dout, const float* __restrict__ y, size_t i, float scale) {
  float g = dout[i];
  if (y && !(y[i] > 0.f)) g = 0.f;
  return g * scale;
}

// ---- data kernel ------------------------------------------------------------------------------------------------------------
struct DcnBwdDataParams {
  const float* dout;       // (N, Cout, Ho, Wo)
  const float* y;          // the forward's output when it applied its ReLU, else null
  const float* scale;      // (Cout) or null
  const float* x;          // (N, Cin, H, W)
  const float* offmask;    // (N, 27, Ho, Wo)
  const char* image_t;
  float* dx;               // (N, Cin, H, W), zeroed by the caller; null: not wanted
  float* doff;             // (N, 27, Ho, Wo)
  int cin, cout, h, w, ho, wo, stride, sigmoid_grad, tiles_img;
};

template <int NI>
__global__ __launch_bounds__(DT_THREADS) void dcn_bwd_data_kernel(const DcnBwdDataParams p) {
  constexpr int NPIX = 32 * NI;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int kgs = p.cout / 8;
  const int b_arr = kgs * NPIX * 16;
  char* const bbuf = smem;                                         // [hi, lo][k-group of 8 co][pixel][16 B]
  float* const red = reinterpret_cast<float*>(smem + 2 * b_arr);  // [wave][27][pixel]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
  const int img = blockIdx.x / p.tiles_img, p0 = (blockIdx.x - img * p.tiles_img) * NPIX;
  const int H = p.h, W = p.w;
  const size_t HW = (size_t)H * W;
  const int HWo = p.ho * p.wo;

  for (int i = tid; i < DT_WAVES * DCN_OFF_C * NPIX; i += DT_THREADS) red[i] = 0.f;
  // prologue: the tile of g as B fragments
  {
    const float* const dout = p.dout + (size_t)img * p.cout * HWo;
    const float* const yy = p.y ? p.y + (size_t)img * p.cout * HWo : nullptr;
    for (int i = tid; i < kgs * NPIX; i += DT_THREADS) {
      const int pix = i % NPIX, kgrp = i / NPIX, pp = p0 + pix;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int co = kgrp * 8 + j;
        v[j] = pp < HWo ? dcn_g(dout, yy, (size_t)co * HWo + pp, p.scale ? p.scale[co] : 1.f) : 0.f;
      }
      u32x4 hi, lo;
      split8(v, hi, lo);
      *reinterpret_cast<u32x4*>(bbuf + (size_t)i * 16) = hi;
      *reinterpret_cast<u32x4*>(bbuf + b_arr + (size_t)i * 16) = lo;
    }
  }
  __syncthreads();

  const int chunks = p.cin / DT_ROWS, items = DCN_TAPS * chunks, ksteps = p.cout / 16;
  const float* const xin = p.x + (size_t)img * p.cin * HW;
  const float* const om = p.offmask + (size_t)img * DCN_OFF_C * HWo;
  float* const dxp = p.dx ? p.dx + (size_t)img * p.cin * HW : nullptr;

  for (int item = wave; item < items; item += DT_WAVES) {            // (wave-uniform)
    const int tap = item / chunks, chunk = item - tap * chunks;
    const int ky = tap / 3, kx = tap - 3 * ky;
    f32x16 acc[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;
    const char* const wa = p.image_t + (size_t)item * 2 * kgs * 512 + (kg * 32 + l32) * 16;
    for (int ks = 0; ks < ksteps; ++ks) {
      const u32x4 ah = *reinterpret_cast<const u32x4*>(wa + (size_t)ks * 1024);
      const u32x4 al = *reinterpret_cast<const u32x4*>(wa + (size_t)kgs * 512 + (size_t)ks * 1024);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int boff = ((2 * ks + kg) * NPIX + 32 * ni + l32) * 16;
        const u32x4 bh = *reinterpret_cast<const u32x4*>(bbuf + boff);
        const u32x4 bl = *reinterpret_cast<const u32x4*>(bbuf + b_arr + boff);
        acc[ni] = mfma_32x32x16_x3(ah, al, bh, bl, acc[ni]);
      }
    }

    // C/D of 32x32x16: column (pixel) = l32, rows (channels of the item) 4 kg + (r & 3) + 8 (r >> 2)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int pix = 32 * ni + l32, pp = p0 + pix;
      bool live = pp < HWo;
      const int oy = live ? pp / p.wo : 0, ox = live ? pp - oy * p.wo : 0;
      float dy = 0.f, dx = 0.f, m = 0.f;
      if (live) {
        dy = om[(size_t)(2 * tap) * HWo + pp];
        dx = om[(size_t)(2 * tap + 1) * HWo + pp];
        m = om[(size_t)(18 + tap) * HWo + pp];
      }
      live = live && dcn_offset_sane(dy, dx);                      // (an offset the forward does not sample: every gradient 0)
      const DcnCorners c = dcn_corners(dy, dx, m, oy * p.stride - 1 + ky, ox * p.stride - 1 + kx, H, W);
      const float wgt[4] = {c.hy * c.hx, c.hy * c.lx, c.ly * c.hx, c.ly * c.lx};
      bool in[4];
      float coef[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        in[j] = live && c.in[j];
        coef[j] = m * wgt[j];
      }
      float s_mod = 0.f, s_dy = 0.f, s_dx = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = mfma32_row(kg, r, chunk * DT_ROWS);
        const char* const xp = reinterpret_cast<const char*>(xin + (size_t)ci * HW);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = in[j] ? *reinterpret_cast<const float*>(xp + c.off[j]) : 0.f;
        const float cv = acc[ni][r];
        s_mod = fmaf(cv, dcn_combine(wgt, v[0], v[1], v[2], v[3]), s_mod);
        s_dy = fmaf(cv, fmaf(c.lx, v[3] - v[1], c.hx * (v[2] - v[0])), s_dy);
        s_dx = fmaf(cv, fmaf(c.ly, v[3] - v[2], c.hy * (v[1] - v[0])), s_dx);
        if (dxp) {
          char* const dp = reinterpret_cast<char*>(dxp + (size_t)ci * HW);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (in[j] && coef[j] != 0.f) atomicAdd(reinterpret_cast<float*>(dp + c.off[j]), coef[j] * cv);
        }
      }
      // the lane's partner holds the other 16 channels of the same pixel
      s_mod += __shfl_xor(s_mod, 32);
      s_dy += __shfl_xor(s_dy, 32);
      s_dx += __shfl_xor(s_dx, 32);
      if (kg == 0) {                                               // the wave's own slab: no other wave touches it
        float* const rp = red + (size_t)wave * DCN_OFF_C * NPIX + pix;
        rp[(2 * tap) * NPIX] += s_dy;
        rp[(2 * tap + 1) * NPIX] += s_dx;
        rp[(18 + tap) * NPIX] += s_mod;
      }
    }
  }
  __syncthreads();

  float* const doff = p.doff + (size_t)img * DCN_OFF_C * HWo;
  for (int i = tid; i < DCN_OFF_C * NPIX; i += DT_THREADS) {
    const int j = i / NPIX, pix = i - j * NPIX, pp = p0 + pix;
    if (pp >= HWo) continue;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < DT_WAVES; ++v) s += red[(v * DCN_OFF_C + j) * NPIX + pix];
    const int tap = j < 18 ? j >> 1 : j - 18;
    const float m = om[(size_t)(18 + tap) * HWo + pp];
    if (j < 18) s *= m;
    else if (p.sigmoid_grad) s *= m * (1.f - m);
    doff[(size_t)j * HWo + pp] = s;
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
struct DcnWgradParams {
  const float *dout, *y, *scale, *x, *offmask;
  float* ws;               // (P, Cout, Cin, 9)
  float* ws_b;             // (P, Cout)
  int cin, cout, h, w, ho, wo, stride, tiles_img, tiles, partitions, chunks;
};

__global__ __launch_bounds__(DW_THREADS) void dcn_wgrad_kernel(const DcnWgradParams p) {
  __shared__ __attribute__((aligned(16))) char s_b[2 * 8 * DW_NC * 16];   // [hi, lo][group of 8 pixels][channel][8 x bf16]
  constexpr int B_ARR = 8 * DW_NC * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
  const int items = DCN_TAPS * p.chunks;
  const int item = blockIdx.x % items, part = blockIdx.x / items;
  const int tap = item / p.chunks, chunk = item - tap * p.chunks;
  const int ky = tap / 3, kx = tap - 3 * ky;
  int t_begin, t_end;
  partition_range(part, p.tiles, p.partitions, t_begin, t_end);
  const int H = p.h, W = p.w;
  const size_t HW = (size_t)H * W;
  const int HWo = p.ho * p.wo;
  const int s_pix = tid & 63, s_c0 = (tid >> 6) * 8;               // sampling role: a pixel of the tile, 8 channels of the chunk

  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  for (int t = t_begin; t < t_end; ++t) {
    const int img = t / p.tiles_img, p0 = (t - img * p.tiles_img) * DW_PX;
    // the modulated samples of (tap, chunk, tile), as the forward's B stage forms them
    float sv[8];
    {
      const int pp = p0 + s_pix;
      const bool live = pp < HWo;
      const int oy = live ? pp / p.wo : 0, ox = live ? pp - oy * p.wo : 0;
      float dy = 0.f, dx = 0.f, m = 0.f;
      if (live) {
        const float* const om = p.offmask + (size_t)img * DCN_OFF_C * HWo + pp;
        dy = om[(size_t)(2 * tap) * HWo];
        dx = om[(size_t)(2 * tap + 1) * HWo];
        m = om[(size_t)(18 + tap) * HWo];
      }
      const DcnCorners c = dcn_corners(dy, dx, m, oy * p.stride - 1 + ky, ox * p.stride - 1 + kx, H, W);
      float cw[4];
      dcn_modulated_weights(c, m, cw);                             // (m = 0 past the ragged edge: zero weights)
      const char* const xp = reinterpret_cast<const char*>(p.x + ((size_t)img * p.cin + chunk * DW_NC + s_c0) * HW);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const char* const xc = xp + (size_t)j * HW * 4;
        sv[j] = dcn_combine(cw, *reinterpret_cast<const float*>(xc + c.off[0]), *reinterpret_cast<const float*>(xc + c.off[1]),
                            *reinterpret_cast<const float*>(xc + c.off[2]), *reinterpret_cast<const float*>(xc + c.off[3]));
      }
    }
    __syncthreads();                                               // the previous tile's readers are done
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const unsigned hh = cvt_pk_bf16(sv[j], sv[j + 1]);
      const unsigned ll = cvt_pk_bf16(sv[j] - __uint_as_float(hh << 16), sv[j + 1] - __uint_as_float(hh & 0xffff0000u));
      char* const d0 = s_b + ((s_pix >> 3) * DW_NC + s_c0 + j) * 16 + (s_pix & 7) * 2;
      *reinterpret_cast<uint16_t*>(d0) = (uint16_t)hh;
      *reinterpret_cast<uint16_t*>(d0 + 16) = (uint16_t)(hh >> 16);
      *reinterpret_cast<uint16_t*>(d0 + B_ARR) = (uint16_t)ll;
      *reinterpret_cast<uint16_t*>(d0 + B_ARR + 16) = (uint16_t)(ll >> 16);
    }
    __syncthreads();

    const float* const dout = p.dout + (size_t)img * p.cout * HWo;
    const float* const yy = p.y ? p.y + (size_t)img * p.cout * HWo : nullptr;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int px = p0 + 16 * ks + 8 * kg;
      const int boff = ((2 * ks + kg) * DW_NC + l32) * 16;
      const u32x4 bh = *reinterpret_cast<const u32x4*>(s_b + boff);
      const u32x4 bl = *reinterpret_cast<const u32x4*>(s_b + B_ARR + boff);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = 32 * (wave + 4 * i) + l32;
        if (32 * (wave + 4 * i) >= p.cout) continue;                // (wave-uniform)
        const float sc = p.scale ? p.scale[co] : 1.f;
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = px + j < HWo ? dcn_g(dout, yy, (size_t)co * HWo + px + j, sc) : 0.f;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += a[j];
        bsum[i] += s;
        u32x4 ah, al;
        split8(a, ah, al);
        acc[i] = mfma_32x32x16_x3(ah, al, bh, bl, acc[i]);
      }
    }
  }

  // column (input channel) = l32, rows (output channels) by mfma32_row
  float* const ws = p.ws + (size_t)part * p.cout * p.cin * DCN_TAPS;
  const int ci = chunk * DW_NC + l32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (32 * (wave + 4 * i) >= p.cout) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = mfma32_row(kg, r, 32 * (wave + 4 * i));
      ws[((size_t)co * p.cin + ci) * DCN_TAPS + tap] = acc[i][r];
    }
    if (item == 0) {
      const float other = __shfl_xor(bsum[i], 32);
      if (kg == 0) p.ws_b[(size_t)part * p.cout + 32 * (wave + 4 * i) + l32] = bsum[i] + other;   // pixels 0-7 of a step, then 8-15
    }
  }
}

// ---- conv_offset: input gradient ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dcn_offset_dgrad_kernel(const float* __restrict__ doff, const float* __restrict__ woff,
                                                               float* __restrict__ dx, const long long total, const int cin, const int H,
                                                               const int W, const int ho, const int wo, const int stride) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % W), y = (int)((idx / W) % H);
  const long long plane = idx / ((long long)H * W);
  const int ci = (int)(plane % cin);
  const long long img = plane / cin;
  const size_t HWo = (size_t)ho * wo;
  const float* const dimg = doff + (size_t)img * DCN_OFF_C * HWo;
  float s = 0.f;
  for (int ky = 0; ky < 3; ++ky) {
    const int ty = y + 1 - ky;                                     // = oy stride
    if (ty < 0 || ty % stride) continue;
    const int oy = ty / stride;
    if (oy >= ho) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int tx = x + 1 - kx;
      if (tx < 0 || tx % stride) continue;
      const int ox = tx / stride;
      if (ox >= wo) continue;
      const float* const d = dimg + (size_t)oy * wo + ox;
      const float* const wp = woff + (size_t)ci * DCN_TAPS + 3 * ky + kx;
#pragma unroll
      for (int j = 0; j < DCN_OFF_C; ++j) s = fmaf(d[(size_t)j * HWo], wp[(size_t)j * cin * DCN_TAPS], s);
    }
  }
  dx[idx] += s;
}

// ---- conv_offset: weight gradient -------------------------------------------------------------------------------------------------
struct DcnOffsetWgradParams {
  const float *doff, *x;
  float* ws;               // (P, 27, Cin, 9)
  float* ws_b;             // (P, 27)
  int cin, h, w, ho, wo, stride, tiles_img, tiles, partitions, chunks;
};

__global__ __launch_bounds__(64) void dcn_offset_wgrad_kernel(const DcnOffsetWgradParams p) {
  const int lane = threadIdx.x, l32 = lane & 31, kg = lane >> 5;
  const int items = DCN_TAPS * p.chunks;
  const int item = blockIdx.x % items, part = blockIdx.x / items;
  const int tap = item / p.chunks, chunk = item - tap * p.chunks;
  const int ky = tap / 3, kx = tap - 3 * ky;
  int t_begin, t_end;
  partition_range(part, p.tiles, p.partitions, t_begin, t_end);
  const size_t HW = (size_t)p.h * p.w;
  const int HWo = p.ho * p.wo;
  const int ci = chunk * DW_NC + l32;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;
  for (int t = t_begin; t < t_end; ++t) {
    const int img = t / p.tiles_img, p0 = (t - img * p.tiles_img) * DW_PX;
    const float* const xc = p.x + ((size_t)img * p.cin + ci) * HW;
    const float* const dj = p.doff + ((size_t)img * DCN_OFF_C + (l32 < DCN_OFF_C ? l32 : 0)) * HWo;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      float a[8], b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int px = p0 + 16 * ks + 8 * kg + j;
        const bool ok = px < HWo;
        const int oy = ok ? px / p.wo : 0, ox = ok ? px - oy * p.wo : 0;
        const int iy = oy * p.stride - 1 + ky, ix = ox * p.stride - 1 + kx;
        const bool in = ok && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
        b[j] = in ? xc[(size_t)iy * p.w + ix] : 0.f;
        a[j] = ok && l32 < DCN_OFF_C ? dj[px] : 0.f;
      }
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += a[j];
      bsum += s;
      u32x4 ah, al, bh, bl;
      split8(a, ah, al);
      split8(b, bh, bl);
      acc = mfma_32x32x16_x3(ah, al, bh, bl, acc);
    }
  }
  float* const ws = p.ws + (size_t)part * DCN_OFF_C * p.cin * DCN_TAPS;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = mfma32_row(kg, r);
    if (j < DCN_OFF_C) ws[((size_t)j * p.cin + ci) * DCN_TAPS + tap] = acc[r];
  }
  if (item == 0) {
    const float other = __shfl_xor(bsum, 32);
    if (kg == 0 && l32 < DCN_OFF_C) p.ws_b[(size_t)part * DCN_OFF_C + l32] = bsum + other;
  }
}

template <int NI>
static int dcn_bwd_data_launch(DcnBwdDataParams& p, int n, void* stream) {
  const int npix = 32 * NI;
  p.tiles_img = (p.ho * p.wo + npix - 1) / npix;
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  const int lds = 2 * (p.cout / 8) * npix * 16 + DT_WAVES * DCN_OFF_C * npix * 4;
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(dcn_bwd_data_kernel<NI>), lds)) return GD4D_ELAUNCH;
  hipLaunchKernelGGL((dcn_bwd_data_kernel<NI>), dim3((unsigned)tiles), dim3(DT_THREADS), lds, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

}  // namespace gd4d

extern "C" size_t gd4d_dcn_weight_image_t_bytes(int cin, int cout) {
  int mpad, kc;
  if (!gd4d::dcn_cin_ok(cin) || cout == gd4d::DCN_OFF_C || !gd4d::dcn_geometry(cout, mpad, kc)) return 0;
  return (size_t)gd4d::DCN_TAPS * cin * cout * 4;
}

extern "C" int gd4d_dcn_weight_image_t(const float* weight, int cin, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  int mpad, kc;
  if (!dcn_cin_ok(cin) || cout == DCN_OFF_C || !dcn_geometry(cout, mpad, kc)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  const ConvImage d{cin, cout, DCN_TAPS, DT_ROWS, cout, cin, 1, 1, 0};
  return pack_conv_image(d, weight, image, static_cast<hipStream_t>(stream));
}

extern "C" int gd4d_dcn_bwd_data(const float* dout, const float* y, const float* scale, const float* x, const float* offmask, int n, int cin,
                                 int cout, int h, int w, int stride, const void* image_t, int sigmoid_grad, float* dx, float* doff,
                                 void* stream) {
  using namespace gd4d;
  if (!dout || !x || !offmask || !image_t || !doff) return GD4D_EINVAL;
  int ho, wo, mpad, kc;
  if (!dcn_cin_ok(cin) || cout == DCN_OFF_C || !dcn_geometry(cout, mpad, kc) || !dcn_out_hw(n, cin, cout, h, w, stride, ho, wo) ||
      (sigmoid_grad != 0 && sigmoid_grad != 1))
    return GD4D_EUNSUPPORTED;
  if (!aligned16(image_t)) return GD4D_EALIGN;
  DcnBwdDataParams p{dout, y, scale, x, offmask, static_cast<const char*>(image_t), dx, doff, cin, cout, h, w, ho, wo, stride, sigmoid_grad, 0};
  return cout <= 256 ? dcn_bwd_data_launch<2>(p, n, stream) : dcn_bwd_data_launch<1>(p, n, stream);
}

extern "C" long long gd4d_dcn_wgrad_tiles(int n, int h, int w, int stride) {
  if (n <= 0 || h <= 0 || w <= 0 || (stride != 1 && stride != 2)) return 0;
  const long long hwo = (long long)((h - 1) / stride + 1) * ((w - 1) / stride + 1);
  return n * ((hwo + gd4d::DW_PX - 1) / gd4d::DW_PX);
}

extern "C" size_t gd4d_dcn_wgrad_workspace_bytes(int cin, int cout, int partitions) {
  using namespace gd4d;
  int mpad, kc;
  if (!dcn_cin_ok(cin) || cout == DCN_OFF_C || !dcn_geometry(cout, mpad, kc) || !partitions_ok(partitions)) return 0;
  return (size_t)partitions * cout * ((size_t)cin * DCN_TAPS + 1) * sizeof(float);
}

extern "C" int gd4d_dcn_wgrad(const float* dout, const float* y, const float* scale, const float* x, const float* offmask, int n, int cin,
                              int cout, int h, int w, int stride, int partitions, float* workspace, float* dw, float* dbias, void* stream) {
  using namespace gd4d;
  if (!dout || !x || !offmask || !workspace || !dw || !dbias) return GD4D_EINVAL;
  int ho, wo, mpad, kc;
  if (!dcn_cin_ok(cin) || cout == DCN_OFF_C || !dcn_geometry(cout, mpad, kc) || !dcn_out_hw(n, cin, cout, h, w, stride, ho, wo) ||
      !partitions_ok(partitions))
    return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long tiles = gd4d_dcn_wgrad_tiles(n, h, w, stride);
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  DcnWgradParams p{dout, y, scale, x, offmask, workspace, workspace + (size_t)partitions * cout * cin * DCN_TAPS,
                   cin, cout, h, w, ho, wo, stride, (int)(tiles / n), (int)tiles, partitions, cin / DW_NC};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dcn_wgrad_kernel, dim3((unsigned)(DCN_TAPS * p.chunks * partitions)), dim3(DW_THREADS), 0, s, p);
  const int total = cout * cin * DCN_TAPS;
  return sum_partitions(p.ws, p.ws_b, partitions, total, cout, dw, dbias, s);
}

extern "C" int gd4d_dcn_offset_conv_dgrad(const float* doff, const float* weight, int n, int cin, int h, int w, int stride, float* dx,
                                          void* stream) {
  using namespace gd4d;
  if (!doff || !weight || !dx) return GD4D_EINVAL;
  int ho, wo;
  if (!dcn_cin_ok(cin) || !dcn_out_hw(n, cin, DCN_OFF_C, h, w, stride, ho, wo)) return GD4D_EUNSUPPORTED;
  const long long total = (long long)n * cin * h * w;
  if ((total + 255) / 256 > (1ll << 31) - 1) return GD4D_EUNSUPPORTED;
  hipLaunchKernelGGL(dcn_offset_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), doff,
                     weight, dx, total, cin, h, w, ho, wo, stride);
  return check_launch();
}

extern "C" size_t gd4d_dcn_offset_conv_wgrad_workspace_bytes(int cin, int partitions) {
  using namespace gd4d;
  if (!dcn_cin_ok(cin) || !partitions_ok(partitions)) return 0;
  return (size_t)partitions * DCN_OFF_C * ((size_t)cin * DCN_TAPS + 1) * sizeof(float);
}

extern "C" int gd4d_dcn_offset_conv_wgrad(const float* doff, const float* x, int n, int cin, int h, int w, int stride, int partitions,
                                          float* workspace, float* dw, float* db, void* stream) {
  using namespace gd4d;
  if (!doff || !x || !workspace || !dw || !db) return GD4D_EINVAL;
  int ho, wo;
  if (!dcn_cin_ok(cin) || !dcn_out_hw(n, cin, DCN_OFF_C, h, w, stride, ho, wo) || !partitions_ok(partitions)) return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long tiles = gd4d_dcn_wgrad_tiles(n, h, w, stride);
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  DcnOffsetWgradParams p{doff, x, workspace, workspace + (size_t)partitions * DCN_OFF_C * cin * DCN_TAPS,
                         cin, h, w, ho, wo, stride, (int)(tiles / n), (int)tiles, partitions, cin / DW_NC};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dcn_offset_wgrad_kernel, dim3((unsigned)(DCN_TAPS * p.chunks * partitions)), dim3(64), 0, s, p);
  const int total = DCN_OFF_C * cin * DCN_TAPS;
  return sum_partitions(p.ws, p.ws_b, partitions, total, DCN_OFF_C, dw, db, s);
}
