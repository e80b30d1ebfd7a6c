// The GEMM of the VoVNet kernels, vv_gemm_kernel<MT, MODE, EPI>, with its geometry, M tiling and launch helpers: shared by the inference
// entry points (gd4d_vovnet.hip, which describes the kernel: tiling, staging, resources) and the data gradients of training
// (gd4d_vovnet_train.hip).  EPI selects the epilogue only; the main loop is one.
//   VV_FWD   relu(acc * scale[c] + shift[c]), and in MODE OSA each tile's per-channel sums for the pool
//   VV_BWD   (acc (+ add)) ([mask > 0]) (+ add2), plain store: the adjoint of a stride-1 convolution on a transposed (and, 3x3,
//            tap-flipped) weight image, with the gradient that is already there added, the next layer's ReLU mask applied and the
//            residual's gradient added after the mask.  add, mask, add2 are optional maps of the output's shape; add and add2 may be
//            the output itself (an element is read before it is written, by the same thread).
//   VV_RES   the ResNet blocks' (gd4d_resnet.hip): v = acc * scale[c] + shift[c]; v += identity[e] where there is one; max(v, 0) where
//            relu is set; no pool sums.  BatchNorm, then the residual, then the ReLU: the block's own order.
//            The ResNet blocks' adjoints (gd4d_resnet_train.hip) pass a fourth optional map, add_even, of HALF the output's
//            resolution ((ho - 1) / 2 + 1 rows, (wo - 1) / 2 + 1 columns): add_even[y / 2, x / 2] is added where y and x are both even,
//            after the mask - the gradient of a stride-2 downsample branch, which touches the even pixels only.
// MODE VV_P2 is the pointwise convolution with stride 2 (a stage's downsample): an 8 x 16 tile of OUTPUT pixels whose B operand is the
// 128 input pixels (2 y, 2 x), staged as VV_OSA stages its 128 consecutive ones; gd4d_resnet.hip alone instantiates it.
// MODE VV_T2 is the adjoint of the 3x3 convolution with stride 2 (gd4d_resnet_train.hip alone instantiates it, with VV_BWD): VV_S1's
// tile, halo and tap walk over the OUTPUT's (dx's) pixels, whose staged patch is the half-resolution source dz zero-interleaved -
// halo pixel (y, x) is dz[y / 2, x / 2] where y and x are both even, else 0.  The full-resolution interleaved map exists in LDS only.
#pragma once
#include "gd4d_common.h"
#include "gd4d_bf16x3.h"
#include "gd4d_conv_common.h"

namespace gd4d {

constexpr int VV_THREADS = 256, VV_KC = 32, VV_TY = 8, VV_TX = 16, VV_PIX = VV_TY * VV_TX;
constexpr int VV_MAX_SRC = 6;
enum { VV_S1 = 0, VV_S2 = 1, VV_OSA = 2, VV_P2 = 3, VV_T2 = 4 };
enum { VV_FWD = 0, VV_BWD = 1, VV_RES = 2 };

template <int MODE> struct VvGeom;
template <> struct VvGeom<VV_S1> { static constexpr int TAPS = 9, STRIDE = 1, HE_H = VV_TY + 2, HE_W = VV_TX + 2, HBUF = 2; };
template <> struct VvGeom<VV_S2> { static constexpr int TAPS = 9, STRIDE = 2, HE_H = 2 * VV_TY + 1, HE_W = 2 * VV_TX + 1, HBUF = 1; };
template <> struct VvGeom<VV_OSA> { static constexpr int TAPS = 1, STRIDE = 1, HE_H = 1, HE_W = VV_PIX, HBUF = 2; };
template <> struct VvGeom<VV_P2> { static constexpr int TAPS = 1, STRIDE = 2, HE_H = 1, HE_W = VV_PIX, HBUF = 2; };
template <> struct VvGeom<VV_T2> { static constexpr int TAPS = 9, STRIDE = 1, HE_H = VV_TY + 2, HE_W = VV_TX + 2, HBUF = 2; };

template <int MODE> constexpr int vv_halo() { return VvGeom<MODE>::HE_H * VvGeom<MODE>::HE_W; }
template <int MODE> constexpr int vv_h_stage() { return 2 * 4 * vv_halo<MODE>() * 16; }               // hi + lo planes of one chunk
constexpr int vv_w_stage(int mt) { return 2 * 4 * 32 * mt * 16; }                                   // hi + lo planes of one step
template <int MT, int MODE> constexpr int vv_lds() { return 2 * vv_w_stage(MT) + VvGeom<MODE>::HBUF * vv_h_stage<MODE>(); }

static_assert(vv_lds<7, VV_S2>() <= 160 * 1024 && vv_lds<7, VV_S1>() <= 160 * 1024, "LDS budget of a CU");

// the M tiling: MT row blocks of 32 per workgroup, one of {7, 5, 4, 3, 2, 1} that divides Cout / 32.  A workgroup's time goes as
// MT + 0.4 (its MFMAs, and per step the barrier and the B fragments every tiling pays; 0.4 fits the two pairs measured in
// docs/measurements_r22.md), a launch's as that times the workgroups, of which fewer than one per CU cost as much as one per CU:
// with pixels enough the largest count wins (the least B traffic), with few pixels (stage 5, six cameras) the launch is cut into
// more workgroups.  Ties go to the larger count.  The 0.4 is a two-point fit taken on one part (an MI355X, V-99 at 320 x 800 and six
// cameras): a tuning constant, not a model; the result's bits do not depend on the choice.  The CU count is the current device's.
static long long vv_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  return cus;
}
static inline int vv_mt(int cout, long long tiles) {
  const long long VV_CUS = vv_cus();
  const int nb = cout / 32;
  const int pick[6] = {7, 5, 4, 3, 2, 1};
  int best = 1;
  long long best_cost = -1;
  for (int i = 0; i < 6; ++i) {
    if (nb % pick[i]) continue;
    const long long groups = tiles * (nb / pick[i]);
    const long long cost = (groups > VV_CUS ? groups : VV_CUS) * (10 * pick[i] + 4);
    if (best_cost < 0 || cost < best_cost) {
      best = pick[i];
      best_cost = cost;
    }
  }
  return best;
}
// m_blocks of the entry points: 0 = vv_mt's choice, or one of the six counts that divides Cout / 32 (the tests run every tiling)
static inline bool vv_mt_ok(int cout, int m_blocks) {
  return m_blocks == 0 || ((m_blocks == 7 || (m_blocks >= 1 && m_blocks <= 5)) && (cout / 32) % m_blocks == 0);
}

// ---- the GEMM ---------------------------------------------------------------------------------------------------------------
struct VvParams {
  const float* src[VV_MAX_SRC];   // NCHW maps of the same N, H, W; the convolutions have one
  int src_ch[VV_MAX_SRC];         // channels of each map
  int src_chunk0[VV_MAX_SRC];     // the first K chunk of each map
  int n_src, chunks;
  int h, w, ho, wo, tiles_x, tiles_img;
  int cout;
  const char* image;
  const float *scale, *shift;
  float* out;
  float* partials;                // OSA: (N, tiles_img, cout)
  const float *add, *mask, *add2;  // VV_BWD: optional maps of the output's shape (appended: the forward's fields keep their offsets)
  const float* identity;          // VV_RES: an optional map of the output's shape, added before the ReLU
  int relu;                       // VV_RES: whether the ReLU runs
  const float* add_even;          // VV_BWD: an optional map of half the output's resolution, added at the even pixels (appended)
};

template <int MT, int MODE, int EPI = VV_FWD>
__global__ __launch_bounds__(VV_THREADS) void vv_gemm_kernel(const VvParams p) {
  using G = VvGeom<MODE>;
  constexpr int TAPS = G::TAPS, S = G::STRIDE, HE_W = G::HE_W, HALO = vv_halo<MODE>();
  constexpr int ROWS = 32 * MT, W_BLK = 2 * 4 * 32 * 16, W_ARR = W_BLK / 2, W_STAGE = MT * W_BLK;   // a row block's step: hi + lo, 4 KB
  constexpr int H_ITEMS = 4 * HALO, H_ARR = H_ITEMS * 16, H_STAGE = 2 * H_ARR;
  constexpr int H_PASSES = (H_ITEMS + VV_THREADS - 1) / VV_THREADS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wbuf = smem;                                   // [2][MT row blocks][hi, lo][4][32][16 B]
  char* const hbuf = smem + 2 * W_STAGE;                     // [HBUF][hi, lo][4][HALO][16 B]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, kg = lane >> 5;

  // work item: (image, pixel tile) x row tile
  const int img = blockIdx.x / p.tiles_img, rt = blockIdx.x - img * p.tiles_img;
  const int tile_m = blockIdx.y;
  const int ty0 = MODE == VV_OSA ? 0 : (rt / p.tiles_x) * VV_TY;
  const int tx0 = MODE == VV_OSA ? rt * VV_PIX : (rt % p.tiles_x) * VV_TX;     // OSA: the first pixel of the flattened image
  const int H = p.h, W = p.w;
  const int HS = (H - 1) / 2 + 1, WS = (W - 1) / 2 + 1;      // VV_T2: the half-resolution source under an H x W output
  const size_t HW = (size_t)H * W, SHW = MODE == VV_T2 ? (size_t)HS * WS : HW;   // the pixels of one source channel
  const int steps = p.chunks * TAPS;
  const char* const image = p.image + (size_t)tile_m * MT * steps * W_BLK + tid * 16;   // row block j: + j steps W_BLK

  // halo staging role: item (k-group, halo pixel) = 8 channels of one input pixel, zero outside the image
  int h_off[H_PASSES], h_ch[H_PASSES];
  bool h_in[H_PASSES];
#pragma unroll
  for (int ps = 0; ps < H_PASSES; ++ps) {
    const int it = tid + VV_THREADS * ps;
    const int kgrp = it / HALO, hp = it % HALO;
    h_ch[ps] = kgrp * 8;
    if (MODE == VV_OSA) {
      const size_t pix = (size_t)tx0 + hp;
      h_in[ps] = it < H_ITEMS && pix < HW;
      h_off[ps] = h_in[ps] ? (int)pix : 0;
    } else if (MODE == VV_P2) {                               // the input pixel under output pixel hp of the tile: no halo, no padding
      const int y = 2 * (ty0 + hp / VV_TX), x = 2 * (tx0 + hp % VV_TX);
      h_in[ps] = it < H_ITEMS && y < H && x < W;
      h_off[ps] = h_in[ps] ? y * W + x : 0;
    } else if (MODE == VV_T2) {                               // the zero-interleaved source: dz[y / 2, x / 2] at even (y, x), else 0
      const int y = ty0 - 1 + hp / HE_W, x = tx0 - 1 + hp % HE_W;
      h_in[ps] = it < H_ITEMS && y >= 0 && y < H && x >= 0 && x < W && !((y | x) & 1);
      h_off[ps] = h_in[ps] ? (y >> 1) * WS + (x >> 1) : 0;
    } else {
      const int y = ty0 * S - 1 + hp / HE_W, x = tx0 * S - 1 + hp % HE_W;
      h_in[ps] = it < H_ITEMS && y >= 0 && y < H && x >= 0 && x < W;
      h_off[ps] = h_in[ps] ? y * W + x : 0;
    }
  }
  float hr[H_PASSES][8];
  auto issue_halo = [&](int chunk) {
    const float* base = p.src[0];
    int c0 = 0, cs = p.src_ch[0];
    if (MODE == VV_OSA) {
#pragma unroll
      for (int i = 1; i < VV_MAX_SRC; ++i)
        if (i < p.n_src && chunk >= p.src_chunk0[i]) {
          base = p.src[i];
          c0 = p.src_chunk0[i];
          cs = p.src_ch[i];
        }
    }
    const float* const cb = base + ((size_t)img * cs + (size_t)(chunk - c0) * VV_KC) * SHW;
#pragma unroll
    for (int ps = 0; ps < H_PASSES; ++ps)
#pragma unroll
      for (int j = 0; j < 8; ++j) hr[ps][j] = h_in[ps] ? cb[(size_t)(h_ch[ps] + j) * SHW + h_off[ps]] : 0.f;
  };
  auto park_halo = [&](int buf) {
    char* const base = hbuf + buf * H_STAGE;
#pragma unroll
    for (int ps = 0; ps < H_PASSES; ++ps) {
      const int it = tid + VV_THREADS * ps;
      if (it < H_ITEMS) {
        u32x4 hi, lo;
        split8(hr[ps], hi, lo);
        *reinterpret_cast<u32x4*>(base + it * 16) = hi;
        *reinterpret_cast<u32x4*>(base + H_ARR + it * 16) = lo;
      }
    }
  };
  u32x4 wr[MT];
  auto issue_w = [&](int s) {
    const char* const src = image + (size_t)s * W_BLK;
#pragma unroll
    for (int j = 0; j < MT; ++j) wr[j] = *reinterpret_cast<const u32x4*>(src + (size_t)j * steps * W_BLK);
  };
  auto park_w = [&](int buf) {
    char* const base = wbuf + buf * W_STAGE + tid * 16;
#pragma unroll
    for (int j = 0; j < MT; ++j) *reinterpret_cast<u32x4*>(base + j * W_BLK) = wr[j];
  };

  f32x16 acc[MT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

  // B fragments: pixel pp = 32 wave + l32 of the tile; its halo entry for tap (ky, kx) is (S py + ky) * HE_W + S px + kx
  const int pp = 32 * wave + l32;
  const int py = pp >> 4, px = pp & 15;
  const int pix_hp = MODE == VV_OSA || MODE == VV_P2 ? pp : (py * S) * HE_W + px * S;

  issue_halo(0);
  park_halo(0);
  issue_w(0);
  park_w(0);
  if (steps > 1) issue_w(1);
  __syncthreads();
  for (int chunk = 0; chunk < p.chunks; ++chunk) {
    const bool more = chunk + 1 < p.chunks;
    if (more) issue_halo(chunk + 1);                         // in flight under the chunk's MFMAs, parked after its last tap
    const char* const hb = hbuf + (G::HBUF == 2 ? (chunk & 1) : 0) * H_STAGE;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int s = chunk * TAPS + tap;
      const char* const wb = wbuf + (s & 1) * W_STAGE;
      const int tap_off = (tap / 3) * HE_W + tap % 3;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int kgrp = 2 * ks + kg;
        const int boff = (kgrp * HALO + pix_hp + tap_off) * 16;
        const u32x4 bh = *reinterpret_cast<const u32x4*>(hb + boff);
        const u32x4 bl = *reinterpret_cast<const u32x4*>(hb + H_ARR + boff);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
          const int aoff = mi * W_BLK + (kgrp * 32 + l32) * 16;
          const u32x4 ah = *reinterpret_cast<const u32x4*>(wb + aoff);
          const u32x4 al = *reinterpret_cast<const u32x4*>(wb + W_ARR + aoff);
          acc[mi] = mfma_32x32x16_x3(ah, al, bh, bl, acc[mi]);
        }
      }
      if (s + 1 < steps) {
        park_w((s + 1) & 1);                                 // its readers finished before the last barrier
        if (s + 2 < steps) issue_w(s + 2);
      }
      if (tap == TAPS - 1 && more) {
        if (G::HBUF == 1) __syncthreads();                   // one buffer: every wave is done with this chunk's patch
        park_halo(G::HBUF == 2 ? (chunk + 1) & 1 : 0);       // two: the buffer was last read in chunk - 1
      }
      __syncthreads();
    }
  }

  // C/D of 32x32x16: column (pixel) = l32, rows (channels) 4 kg + (r & 3) + 8 (r >> 2)
  bool ok;
  size_t off, plane;
  [[maybe_unused]] int oy, ox;                               // the output pixel (VV_BWD's add_even asks for its parity)
  if (MODE == VV_OSA) {
    const size_t pix = (size_t)tx0 + pp;
    ok = pix < HW;
    off = ok ? pix : 0;
    plane = HW;
    oy = (int)(off / (size_t)W);
    ox = (int)(off - (size_t)oy * W);
  } else {
    const int y = ty0 + py, x = tx0 + px;
    ok = y < p.ho && x < p.wo;
    off = ok ? (size_t)y * p.wo + x : 0;
    plane = (size_t)p.ho * p.wo;
    oy = y;
    ox = x;
  }
  const int crow0 = tile_m * ROWS;
  if constexpr (EPI == VV_BWD) {
    if (!ok) return;
    const size_t o = ((size_t)img * p.cout + crow0) * plane + off;
    // add_even: (N, cout, he, we) with he = (rows - 1) / 2 + 1; this lane's pixel takes part where both its coordinates are even
    const int we = ((MODE == VV_OSA ? W : p.wo) - 1) / 2 + 1, he = ((MODE == VV_OSA ? H : p.ho) - 1) / 2 + 1;
    const size_t plane_e = (size_t)he * we;
    const bool even = p.add_even && !((oy | ox) & 1);
    const size_t oe = ((size_t)img * p.cout + crow0) * plane_e + (size_t)(oy >> 1) * we + (ox >> 1);
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cl = 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
        const size_t e = o + (size_t)cl * plane;
        float v = acc[mi][r];
        if (p.add) v = v + p.add[e];
        if (p.mask && !(p.mask[e] > 0.f)) v = 0.f;           // strict, as torch's ReLU
        if (p.add2) v = v + p.add2[e];
        if (even) v = v + p.add_even[oe + (size_t)cl * plane_e];
        p.out[e] = v;
      }
    return;
  }
  if constexpr (EPI == VV_RES) {
    if (!ok) return;
    const size_t o = ((size_t)img * p.cout + crow0) * plane + off;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cl = 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
        const size_t e = o + (size_t)cl * plane;
        float v = acc[mi][r] * p.scale[crow0 + cl] + p.shift[crow0 + cl];
        if (p.identity) v = v + p.identity[e];
        if (p.relu) v = fmaxf(v, 0.f);
        p.out[e] = v;
      }
    return;
  }
  float* const outp = p.out + ((size_t)img * p.cout + crow0) * plane + off;
  float* const red = reinterpret_cast<float*>(smem);          // OSA: [4 waves][ROWS] (the main loop's last barrier is behind every wave)
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cl = 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
      const float v = fmaxf(acc[mi][r] * p.scale[crow0 + cl] + p.shift[crow0 + cl], 0.f);
      if (ok) outp[(size_t)cl * plane] = v;
      if (MODE == VV_OSA) {
        const float s = half_wave_sum(ok ? v : 0.f);
        if (l32 == 0) red[wave * ROWS + cl] = s;
      }
    }
  if (MODE == VV_OSA) {
    __syncthreads();
    if (tid < ROWS)
      p.partials[((size_t)img * p.tiles_img + rt) * p.cout + crow0 + tid] =
          (red[tid] + red[ROWS + tid]) + (red[2 * ROWS + tid] + red[3 * ROWS + tid]);
  }
}

template <int MT, int MODE, int EPI>
static int vv_launch_mt(const VvParams& p, unsigned tiles, unsigned row_tiles, hipStream_t stream) {
  constexpr int lds = vv_lds<MT, MODE>();
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(vv_gemm_kernel<MT, MODE, EPI>), lds)) return GD4D_ELAUNCH;
  hipLaunchKernelGGL((vv_gemm_kernel<MT, MODE, EPI>), dim3(tiles, row_tiles), dim3(VV_THREADS), lds, stream, p);
  return check_launch();
}

template <int MODE, int EPI = VV_FWD>
static int vv_launch(const VvParams& p, long long tiles, int m_blocks, void* stream) {
  const int mt = m_blocks ? m_blocks : vv_mt(p.cout, tiles);
  const unsigned rows = (unsigned)(p.cout / (32 * mt)), t = (unsigned)tiles;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (mt) {
    case 7: return vv_launch_mt<7, MODE, EPI>(p, t, rows, st);
    case 5: return vv_launch_mt<5, MODE, EPI>(p, t, rows, st);
    case 4: return vv_launch_mt<4, MODE, EPI>(p, t, rows, st);
    case 3: return vv_launch_mt<3, MODE, EPI>(p, t, rows, st);
    case 2: return vv_launch_mt<2, MODE, EPI>(p, t, rows, st);
    default: return vv_launch_mt<1, MODE, EPI>(p, t, rows, st);
  }
}

static bool vv_conv_channels(int cin, int cout) {
  return cin % 32 == 0 && cin >= 32 && cin <= 1024 && cout % 32 == 0 && cout >= 32 && cout <= 256;
}
static bool vv_osa_channels(int k, int cout) {
  return k % 32 == 0 && k >= 32 && k <= 2304 && cout % 32 == 0 && cout >= 32 && cout <= 1024;
}

// w (cout, cin, taps): a (row block of 32 output channels, step = chunk * taps + tap) is 4 KB; the image does not depend on the M tiling
static int vv_image(const float* weight, int cin, int cout, int taps, void* image, void* stream) {
  if (!aligned16(image)) return GD4D_EALIGN;
  const ConvImage d{cin, cout, taps, 32, VV_KC, cout, 0, 0, 0};
  return pack_conv_image(d, weight, image, static_cast<hipStream_t>(stream));
}

}  // namespace gd4d
