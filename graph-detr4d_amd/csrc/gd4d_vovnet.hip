// VoVNet (V-39 / V-57 / V-99, eSE) on the bf16 MFMA: the backbone of the reference's VoVNet configurations
// (models/backbones/vovnet.py, vovnetcp.py), inference with frozen BatchNorm.  One OSA module is
//     x_0 = input, x_i = relu(BN_i(conv3x3_i(x_{i-1})))  (i = 1 .. L),   xt = relu(BN(W . concat(x_0 .. x_L))),
//     out = xt * hsigmoid(fc(avgpool(xt))) (+ input),                     hsigmoid(v) = relu6(v + 3) / 6.
// Entry points (eight launches per OSA module of five layers, all on one stream):
//
//   gd4d_conv3x3_image / gd4d_conv3x3_bn_relu_fwd      3x3, pad 1, stride 1 or 2, no bias, relu(acc * scale[c] + shift[c])
//   gd4d_osa_concat_image / gd4d_osa_concat_conv_fwd   the 1x1 aggregation over up to six separate NCHW maps: the concatenation is
//                                                      never written, the K walk steps from one map to the next at a chunk boundary;
//                                                      same epilogue, plus each tile's per-channel sum of the activated outputs
//   gd4d_ese_gate_fwd                                  mean = sum of those partials in tile order / (H W); gate = hsigmoid(fc_w mean +
//                                                      fc_b), plain fp32 FMAs with K in order (a row per thread, 256 rows per workgroup)
//   gd4d_ese_apply_fwd                                 out = xt * gate[n, c] (+ identity): one pass of 16-byte accesses over the FLAT
//                                                      tensor (H W need not be a multiple of 4: a 16-byte group may span planes, each
//                                                      element takes its own plane's gate); out may be xt
//
// Arithmetic: gd4d_bf16x3.h - both operands split into bf16 hi + lo, lo hi + hi lo + hi hi accumulated in fp32 on
// v_mfma_f32_32x32x16_bf16.  No atomics; every sum has a fixed order (K: chunk by chunk of 32 channels, tap by tap inside a chunk; pool:
// 32 lanes by an xor butterfly, then the four waves, then the tiles in order): two runs give the same bits.
//
// One GEMM kernel, vv_gemm_kernel<MT, MODE>, in the style of depth_conv_kernel (gd4d_depth_net.hip): the weight image is the MFMA's A
// operand, the pixels its B operand, so an accumulator lane holds one pixel and 16 channels and the NCHW stores of a wave are 16-pixel
// row segments.  A workgroup is 4 waves and owns 128 output pixels (8 rows x 16 columns; MODE OSA: 128 consecutive pixels of the
// flattened image) x 32 MT output channels; wave w holds pixels 32 w .. 32 w + 31 and all MT row blocks (MT f32x16 accumulators).
//   M tiling.  Padding M to 256 for every Cout would waste half the MFMAs of stage 2 (Cout = 128, the most pixels).  MT is one of
//          {7, 5, 4, 3, 2, 1} that divides Cout / 32 (vv_mt below), and blockIdx.y walks the Cout / (32 MT) row tiles: with pixels
//          enough to fill the CUs the largest, 64 -> 2, 128 -> 4, 160 -> 5, 192 -> 2 x 3, 224 -> 7, 256 .. 1024 -> 2 .. 8 x 4; with few
//          (stage 5, or six cameras) a smaller one, down to a workgroup per row block.  No padded row is ever multiplied.
//          Six instantiations per mode.  The weight image is laid out per row BLOCK of 32, so it does not depend on the choice, and
//          neither do the bits: a block's K walk is the same in every tiling.
//   weight one step's (chunk, tap) slice of the MT row blocks, 4 KB each (hi + lo), copied to LDS verbatim: MT 16-byte loads per
//          thread, issued one step ahead into registers, parked after the step's MFMAs, double-buffered by step parity.  One barrier
//          per step.
//   halo   the tile's input patch of the chunk, zero outside the image (exact padding, and ragged tiles' unused pixels), split hi / lo
//          once and read by all nine taps: [k-group][halo pixel][8 x bf16] per plane.  Stride 1: 10 x 18 pixels, 22.5 KB, double-buffered
//          by chunk parity.  Stride 2: 17 x 33, 70 KB, ONE buffer and a second barrier per chunk (two would not fit beside MT = 7's
//          weights; only stem_3 has stride 2).  OSA: 128 pixels, 16 KB, double-buffered.  The next chunk's patch is loaded into registers
//          at the top of a chunk and parked after its last tap.
//   A B fragment of tap (ky, kx) is the halo entry (s py + ky, s px + kx): one ds_read_b128 per plane.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): VGPRs + AGPRs, dynamic LDS bytes, waves per SIMD the registers allow.
// Scratch is 0 bytes per lane for every instantiation.  The accumulators are 16 MT of the AGPRs; stride 2 holds the next patch in
// registers (9 passes x 8 values) and fills the 256 VGPRs, the compiler parks the rest in AGPRs (copies, not memory).
//     MT     stride 1                 stride 2                  OSA (1x1)
//     7      146 + 112, 103 424, 1    256 + 152, 129 152, 1     128 + 112, 90 112, 2
//     5      136 +  80,  87 040, 2    256 + 108, 112 768, 1      96 +  80, 73 728, 2
//     4      132 +  64,  78 848, 2    256 +  86, 104 576, 1      92 +  64, 65 536, 3
//     3      128 +  48,  70 656, 2    256 +  72,  96 384, 1      92 +  48, 57 344, 3
//     2      124 +  32,  62 464, 3    256 +  48,  88 192, 1      84 +  32, 49 152, 4
//     1      120 +  16,  54 272, 3    256 +  26,  80 000, 1      80 +  16, 40 960, 5
// vv_ese_gate_kernel 62 VGPRs (4 KB of static LDS), vv_ese_apply_kernel 18; no scratch.  The weight images are packed by
// pack_conv_image (gd4d_conv_common.h has the format).
// Left off: a 2 x 2 register tile per wave (halves the A reads from LDS), a double-buffered stride-2 halo, fusing the gate's matvec
// into the last aggregation tile, NHWC.
#include "gd4d_common.h"
#include "gd4d_bf16x3.h"
#include "gd4d_conv_common.h"

namespace gd4d {

constexpr int VV_THREADS = 256, VV_KC = 32, VV_TY = 8, VV_TX = 16, VV_PIX = VV_TY * VV_TX;
constexpr int VV_MAX_SRC = 6;
enum { VV_S1 = 0, VV_S2 = 1, VV_OSA = 2 };

template <int MODE> struct VvGeom;
template <> struct VvGeom<VV_S1> { static constexpr int TAPS = 9, STRIDE = 1, HE_H = VV_TY + 2, HE_W = VV_TX + 2, HBUF = 2; };
template <> struct VvGeom<VV_S2> { static constexpr int TAPS = 9, STRIDE = 2, HE_H = 2 * VV_TY + 1, HE_W = 2 * VV_TX + 1, HBUF = 1; };
template <> struct VvGeom<VV_OSA> { static constexpr int TAPS = 1, STRIDE = 1, HE_H = 1, HE_W = VV_PIX, HBUF = 2; };

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
};

template <int MT, int MODE>
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
  const size_t HW = (size_t)H * W;
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
    const float* const cb = base + ((size_t)img * cs + (size_t)(chunk - c0) * VV_KC) * HW;
#pragma unroll
    for (int ps = 0; ps < H_PASSES; ++ps)
#pragma unroll
      for (int j = 0; j < 8; ++j) hr[ps][j] = h_in[ps] ? cb[(size_t)(h_ch[ps] + j) * HW + h_off[ps]] : 0.f;
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
  const int pix_hp = MODE == VV_OSA ? pp : (py * S) * HE_W + px * S;

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
  if (MODE == VV_OSA) {
    const size_t pix = (size_t)tx0 + pp;
    ok = pix < HW;
    off = ok ? pix : 0;
    plane = HW;
  } else {
    const int y = ty0 + py, x = tx0 + px;
    ok = y < p.ho && x < p.wo;
    off = ok ? (size_t)y * p.wo + x : 0;
    plane = (size_t)p.ho * p.wo;
  }
  const int crow0 = tile_m * ROWS;
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

// ---- eSE --------------------------------------------------------------------------------------------------------------------
constexpr int VV_ESE_MAX_C = 1024;

__global__ __launch_bounds__(256) void vv_ese_gate_kernel(const float* __restrict__ partials, const int tiles, const int c_all, const int hw,
                                                          const float* __restrict__ fc_w, const float* __restrict__ fc_b,
                                                          float* __restrict__ gate) {
  __shared__ float mean[VV_ESE_MAX_C];
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < c_all; c += 256) {           // every workgroup of the image forms the whole mean: its rows need all of it
    float s = 0.f;
    for (int t = 0; t < tiles; ++t) s += partials[((size_t)n * tiles + t) * c_all + c];
    mean[c] = s / (float)hw;
  }
  __syncthreads();
  const int c = blockIdx.y * 256 + threadIdx.x;               // one row of fc_w per thread
  if (c < c_all) {
    float acc = 0.f;
    const float4* const row = reinterpret_cast<const float4*>(fc_w + (size_t)c * c_all);
#pragma unroll 8
    for (int j = 0; j < c_all / 4; ++j) {
      const float4 q = row[j];
      acc = fmaf(q.x, mean[4 * j], acc);
      acc = fmaf(q.y, mean[4 * j + 1], acc);
      acc = fmaf(q.z, mean[4 * j + 2], acc);
      acc = fmaf(q.w, mean[4 * j + 3], acc);
    }
    const float v = (acc + fc_b[c]) + 3.f;
    gate[(size_t)n * c_all + c] = fminf(fmaxf(v, 0.f), 6.f) / 6.f;
  }
}

// flat 16-byte groups; element e of group i lies in plane (4 i + e) / hw, whose gate it takes.  xt and out may be one buffer: a thread
// reads its group before it writes it and touches no other.
__global__ __launch_bounds__(256) void vv_ese_apply_kernel(const float* xt, const float* __restrict__ gate, const float* identity,
                                                           const size_t total, const int hw, float* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t first = 4 * i;
  if (first >= total) return;
  size_t pl = first / hw;
  int r = (int)(first - pl * hw);
  if (first + 4 <= total) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(xt + first);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = a[e] * gate[pl];
      if (++r == hw) { r = 0; ++pl; }
    }
    if (identity) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(identity + first);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + d[e];
    }
    *reinterpret_cast<f32x4*>(out + first) = o;
  } else {
    for (size_t k = first; k < total; ++k) {                  // the last 1-3 elements of the tensor
      float v = xt[k] * gate[pl];
      if (identity) v = v + identity[k];
      out[k] = v;
      if (++r == hw) { r = 0; ++pl; }
    }
  }
}

template <int MT, int MODE>
static int vv_launch_mt(const VvParams& p, unsigned tiles, unsigned row_tiles, hipStream_t stream) {
  constexpr int lds = vv_lds<MT, MODE>();
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(vv_gemm_kernel<MT, MODE>), lds)) return GD4D_ELAUNCH;
  hipLaunchKernelGGL((vv_gemm_kernel<MT, MODE>), dim3(tiles, row_tiles), dim3(VV_THREADS), lds, stream, p);
  return check_launch();
}

template <int MODE>
static int vv_launch(const VvParams& p, long long tiles, int m_blocks, void* stream) {
  const int mt = m_blocks ? m_blocks : vv_mt(p.cout, tiles);
  const unsigned rows = (unsigned)(p.cout / (32 * mt)), t = (unsigned)tiles;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (mt) {
    case 7: return vv_launch_mt<7, MODE>(p, t, rows, st);
    case 5: return vv_launch_mt<5, MODE>(p, t, rows, st);
    case 4: return vv_launch_mt<4, MODE>(p, t, rows, st);
    case 3: return vv_launch_mt<3, MODE>(p, t, rows, st);
    case 2: return vv_launch_mt<2, MODE>(p, t, rows, st);
    default: return vv_launch_mt<1, MODE>(p, t, rows, st);
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

extern "C" size_t gd4d_conv3x3_image_bytes(int cin, int cout) {
  return gd4d::vv_conv_channels(cin, cout) ? (size_t)cout * cin * 9 * 4 : 0;
}

extern "C" int gd4d_conv3x3_image(const float* weight, int cin, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  if (!vv_conv_channels(cin, cout)) return GD4D_EUNSUPPORTED;
  return vv_image(weight, cin, cout, 9, image, stream);
}

extern "C" int gd4d_conv3x3_bn_relu_fwd(const float* x, int n, int cin, int h, int w, int stride, const void* image, int cout,
                                        const float* scale, const float* shift, float* out, int m_blocks, void* stream) {
  using namespace gd4d;
  if (!x || !image || !scale || !shift || !out) return GD4D_EINVAL;
  if (!vv_conv_channels(cin, cout) || (stride != 1 && stride != 2) || n <= 0 || h <= 0 || w <= 0) return GD4D_EUNSUPPORTED;
  if (!vv_mt_ok(cout, m_blocks)) return GD4D_EUNSUPPORTED;
  if ((long long)h * w > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  VvParams p{};
  p.src[0] = x;
  p.src_ch[0] = cin;
  p.n_src = 1;
  p.chunks = cin / VV_KC;
  p.h = h;
  p.w = w;
  p.ho = (h - 1) / stride + 1;
  p.wo = (w - 1) / stride + 1;
  p.tiles_x = (p.wo + VV_TX - 1) / VV_TX;
  p.tiles_img = p.tiles_x * ((p.ho + VV_TY - 1) / VV_TY);
  p.cout = cout;
  p.image = static_cast<const char*>(image);
  p.scale = scale;
  p.shift = shift;
  p.out = out;
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  return stride == 1 ? vv_launch<VV_S1>(p, tiles, m_blocks, stream) : vv_launch<VV_S2>(p, tiles, m_blocks, stream);
}

extern "C" size_t gd4d_osa_concat_image_bytes(int k, int cout) { return gd4d::vv_osa_channels(k, cout) ? (size_t)cout * k * 4 : 0; }

extern "C" int gd4d_osa_concat_image(const float* weight, int k, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  if (!vv_osa_channels(k, cout)) return GD4D_EUNSUPPORTED;
  return vv_image(weight, k, cout, 1, image, stream);
}

extern "C" long long gd4d_osa_concat_tiles(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return ((long long)h * w + gd4d::VV_PIX - 1) / gd4d::VV_PIX;
}

extern "C" int gd4d_osa_concat_conv_fwd(const float* const* src, const int32_t* src_channels, int n_src, int n, int h, int w,
                                        const void* image, int cout, const float* scale, const float* shift, float* out, float* partials,
                                        int m_blocks, void* stream) {
  using namespace gd4d;
  if (!src || !src_channels || !image || !scale || !shift || !out || !partials) return GD4D_EINVAL;
  if (n_src < 1 || n_src > VV_MAX_SRC || n <= 0 || h <= 0 || w <= 0 || (long long)h * w > (1ll << 30)) return GD4D_EUNSUPPORTED;
  VvParams p{};
  int k = 0;
  for (int i = 0; i < n_src; ++i) {
    if (!src[i]) return GD4D_EINVAL;
    const int c = src_channels[i];
    if (c <= 0 || c % VV_KC || c > 2304) return GD4D_EUNSUPPORTED;
    p.src[i] = src[i];
    p.src_ch[i] = c;
    p.src_chunk0[i] = k / VV_KC;
    k += c;
  }
  if (!vv_osa_channels(k, cout) || !vv_mt_ok(cout, m_blocks)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  p.n_src = n_src;
  p.chunks = k / VV_KC;
  p.h = p.ho = h;
  p.w = p.wo = w;
  p.tiles_x = 1;
  p.tiles_img = (int)gd4d_osa_concat_tiles(h, w);
  p.cout = cout;
  p.image = static_cast<const char*>(image);
  p.scale = scale;
  p.shift = shift;
  p.out = out;
  p.partials = partials;
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  return vv_launch<VV_OSA>(p, tiles, m_blocks, stream);
}

extern "C" int gd4d_ese_gate_fwd(const float* partials, int n, int tiles, int channels, int hw, const float* fc_w, const float* fc_b,
                                 float* gate, void* stream) {
  using namespace gd4d;
  if (!partials || !fc_w || !fc_b || !gate) return GD4D_EINVAL;
  if (n <= 0 || tiles <= 0 || hw <= 0 || channels % 32 || channels < 32 || channels > VV_ESE_MAX_C) return GD4D_EUNSUPPORTED;
  if (!aligned16(fc_w)) return GD4D_EALIGN;
  hipLaunchKernelGGL(vv_ese_gate_kernel, dim3(n, (channels + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), partials, tiles, channels, hw, fc_w,
                     fc_b, gate);
  return check_launch();
}

extern "C" int gd4d_ese_apply_fwd(const float* xt, const float* gate, const float* identity, int n, int channels, int hw, float* out,
                                  void* stream) {
  using namespace gd4d;
  if (!xt || !gate || !out) return GD4D_EINVAL;
  if (n <= 0 || channels <= 0 || hw <= 0) return GD4D_EUNSUPPORTED;
  const size_t total = (size_t)n * channels * hw;
  const size_t groups = (total + 3) / 4;
  if (groups > ((size_t)1 << 38)) return GD4D_EUNSUPPORTED;
  if (!aligned16(xt) || !aligned16(out) || (identity && !aligned16(identity))) return GD4D_EALIGN;
  hipLaunchKernelGGL(vv_ese_apply_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), xt, gate,
                     identity, total, hw, out);
  return check_launch();
}
