// Training of the image neck (gd4d_fpn.hip holds the forward and the two input-gradient kinds of its GEMM; the 3x3 output
// convolutions' gradients are gd4d_fpn_conv_fwd on transposed images and gd4d_depth_conv_wgrad).  With gl_i the gradient of lateral i:
//
//   gd4d_fpn_lateral_wgrad     dW (256, Cin) = sum over cameras and pixels of gl[oc, p] x[ic, p], db (256) = sum of gl[oc, p]:
//                              conv1x1_wgrad_body (gd4d_conv_wgrad.h has the algorithm) with all 256 output channels in one
//                              workgroup (no guard), one input map, and the bias sum: a (P, 256, Cin) + (P, 256) workspace, then
//                              sum_partitions.
//   gd4d_fpn_topdown_bwd       the adjoint of the forward's fused nearest-upsampling add, in place on the coarser gradient: one
//                              thread per coarse element adds its children of the finer gradient in row-major order.  The children
//                              are found by testing candidates (an integer bracket, one pixel wider than the exact-ratio range on
//                              both sides) against fpn_nearest_src, the forward's own index function.
//   gd4d_fpn_extra_conv_wgrad  dW[oc, ic, ky, kx] = sum of dy[oc, p] relu?(x)[ic, 2 p + tap - 1], db = sum of dy: grid (8 chunks of 32
//                              input channels) x (9 taps), K = the flattened (camera, output pixel) list, both operands gathered
//                              straight from global memory (zeros outside the image); no LDS, no partitions: these levels have a few
//                              thousand pixels at most.  Untuned.
//   gd4d_fpn_bias_grad         db (256) = channel sums of an (N, 256, H, W) gradient: one workgroup per plane (strided partial sums,
//                              LDS tree), then the planes of a channel in camera order.
// No atomics: every sum runs in a fixed order, two runs give the same bits.
#include "gd4d_bf16x3.h"
#include "gd4d_common.h"
#include "gd4d_conv_wgrad.h"
#include "gd4d_fpn_index.h"

namespace gd4d {

constexpr int FT_C = 256;
constexpr int FT_MAX_CIN = 2048;

// ---- lateral weight / bias gradient -------------------------------------------------------------------------------------------
struct LateralWgradParams {
  const float* g;          // (N, 256, H, W)
  const float* x;          // (N, Cin, H, W)
  float* ws;               // (P, 256, Cin)
  float* ws_b;             // (P, 256)
  int cin, hw, tiles_cam, tiles, partitions, chunks;
};

// conv1x1_wgrad_body's policy: all 256 output channels in one workgroup, K = the channels of the one input map
struct LateralWgradShape {
  const LateralWgradParams& p;
  const Conv1x1Wgrad g;
  static constexpr bool GUARD = false;
  static constexpr int cout() { return FT_C; }
  __device__ __forceinline__ int oc0(int wave) const { return 64 * wave; }
  __device__ __forceinline__ Conv1x1Source source(int icg, bool ok) const { return {p.x, p.cin, ok ? icg : 0}; }
  __device__ __forceinline__ size_t x_plane() const { return (size_t)g.hw; }
  __device__ __forceinline__ int x_pixel(int px) const { return px; }
};

__global__ __launch_bounds__(CW1_THREADS) void fpn_lateral_wgrad_kernel(const LateralWgradParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 s_b[2][CW1_B_ARR];         // [hi, lo][channel][pixel group (+ 1)]
  conv1x1_wgrad_body<LateralWgradShape, true>(
      LateralWgradShape{p, {p.g, p.ws, p.ws_b, p.cin, p.hw, p.tiles_cam, p.tiles, p.partitions, p.chunks}}, s_b);
}

// ---- top-down adjoint ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fpn_topdown_bwd_kernel(const float* __restrict__ fine, float* __restrict__ coarse,
                                                              const long long total, const int H, const int W, const int Hc, const int Wc,
                                                              const float scale_y, const float scale_x) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int xc = (int)(idx % Wc), yc = (int)((idx / Wc) % Hc);
  const long long plane = idx / ((long long)Hc * Wc);
  // candidates: the exact-ratio range of the coarse pixel, one pixel wider on both sides; fpn_nearest_src decides
  const int y_lo = max(0, (int)((long long)yc * H / Hc) - 1), y_hi = min(H - 1, (int)(((long long)(yc + 1) * H + Hc - 1) / Hc) + 1);
  const int x_lo = max(0, (int)((long long)xc * W / Wc) - 1), x_hi = min(W - 1, (int)(((long long)(xc + 1) * W + Wc - 1) / Wc) + 1);
  const float* const src = fine + (size_t)plane * H * W;
  float v = coarse[idx];
  for (int y = y_lo; y <= y_hi; ++y) {
    if (fpn_nearest_src(y, scale_y, Hc) != yc) continue;
    for (int x = x_lo; x <= x_hi; ++x)
      if (fpn_nearest_src(x, scale_x, Wc) == xc) v += src[(size_t)y * W + x];
  }
  coarse[idx] = v;
}

// ---- stride-2 extra level: weight / bias gradient -----------------------------------------------------------------------------
constexpr int EW_KC = 32, EW_CHUNKS = FT_C / EW_KC, EW_TAPS = 9;

struct ExtraWgradParams {
  const float* dy;         // (N, 256, Ho, Wo)
  const float* x;          // (N, 256, H, W)
  float* dw;               // (256, 256, 3, 3)
  float* db;               // (256)
  int H, W, Ho, Wo, total; // total = N Ho Wo
  int relu_in;
};

__global__ __launch_bounds__(256) void fpn_extra_wgrad_kernel(const ExtraWgradParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
  const int chunk = blockIdx.x % EW_CHUNKS, tap = blockIdx.x / EW_CHUNKS;
  const int ky = tap / 3, kx = tap - 3 * ky;
  const int HWo = p.Ho * p.Wo;
  const size_t HW = (size_t)p.H * p.W;
  const int ic = chunk * EW_KC + l32;
  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float bsum[2] = {0.f, 0.f};

  for (int q0 = 0; q0 < p.total; q0 += 16) {
    float a[2][8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = q0 + 8 * kg + j;
      const bool ok = q < p.total;
      const int cam = ok ? q / HWo : 0, pp = ok ? q - cam * HWo : 0;
      const int oy = pp / p.Wo, ox = pp - oy * p.Wo;
      const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
      const bool in = ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      float v = in ? p.x[((size_t)cam * FT_C + ic) * HW + (size_t)iy * p.W + ix] : 0.f;
      if (p.relu_in) v = fmaxf(v, 0.f);
      b[j] = v;
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i][j] = ok ? p.dy[((size_t)cam * FT_C + 64 * wave + 32 * i + l32) * HWo + pp] : 0.f;
    }
    u32x4 bh, bl;
    split8(b, bh, bl);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += a[i][j];
      bsum[i] += s;
      u32x4 ah, al;
      split8(a[i], ah, al);
      acc[i] = mfma_32x32x16_x3(ah, al, bh, bl, acc[i]);
    }
  }
  // column (input channel) = l32, rows (output channels) by mfma32_row
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = mfma32_row(kg, r, 64 * wave + 32 * i);
      p.dw[((size_t)oc * FT_C + ic) * EW_TAPS + tap] = acc[i][r];
    }
  if (blockIdx.x == 0 && p.db) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float other = __shfl_xor(bsum[i], 32);
      if (kg == 0) p.db[64 * wave + 32 * i + l32] = bsum[i] + other;
    }
  }
}

// ---- channel sums ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fpn_plane_sum_kernel(const float* __restrict__ g, const int hw, float* __restrict__ part) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const float* src = g + (size_t)blockIdx.x * hw;
  float s = 0.f;
  for (int i = tid; i < hw; i += 256) s += src[i];
  s = block_sum_256(s, red);
  if (tid == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(FT_C) void fpn_plane_sum_cams_kernel(const float* __restrict__ part, const int n, float* __restrict__ db) {
  const int c = threadIdx.x;
  float s = 0.f;
  for (int cam = 0; cam < n; ++cam) s += part[(size_t)cam * FT_C + c];
  db[c] = s;
}

static bool ft_cin_ok(int cin) { return cin >= 32 && cin <= FT_MAX_CIN && cin % 32 == 0; }

}  // namespace gd4d

extern "C" size_t gd4d_fpn_lateral_wgrad_workspace_bytes(int cin, int partitions) {
  using namespace gd4d;
  if (!ft_cin_ok(cin) || !partitions_ok(partitions)) return 0;
  return (size_t)partitions * FT_C * ((size_t)cin + 1) * sizeof(float);
}

extern "C" long long gd4d_fpn_lateral_wgrad_tiles(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (long long)n * (((long long)h * w + gd4d::CW1_PX - 1) / gd4d::CW1_PX);
}

extern "C" int gd4d_fpn_lateral_wgrad(const float* g, const float* x, int n, int cin, int h, int w, int partitions, float* workspace,
                                      float* dw, float* db, void* stream) {
  using namespace gd4d;
  if (!g || !x || !workspace || !dw || !db) return GD4D_EINVAL;
  if (h <= 0 || w <= 0) return GD4D_EINVAL;
  if (n <= 0 || !ft_cin_ok(cin) || !partitions_ok(partitions)) return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if ((long long)n * FT_MAX_CIN * hw > (1ll << 40) || hw > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long tiles_cam = (hw + CW1_PX - 1) / CW1_PX;
  if (tiles_cam * n > (1ll << 30)) return GD4D_EUNSUPPORTED;
  LateralWgradParams p{};
  p.g = g;
  p.x = x;
  p.ws = workspace;
  p.ws_b = workspace + (size_t)partitions * FT_C * cin;
  p.cin = cin;
  p.hw = (int)hw;
  p.tiles_cam = (int)tiles_cam;
  p.tiles = (int)(tiles_cam * n);
  p.partitions = partitions;
  p.chunks = (cin + CW1_IC - 1) / CW1_IC;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(fpn_lateral_wgrad_kernel, dim3((unsigned)(p.chunks * partitions)), dim3(CW1_THREADS), 0, s, p);
  return sum_partitions(p.ws, p.ws_b, partitions, FT_C * cin, FT_C, dw, db, s);   // dW (256, Cin) and db (256)
}

extern "C" int gd4d_fpn_topdown_bwd(const float* g_fine, int n, int channels, int h, int w, float* g_coarse, int coarse_h, int coarse_w,
                                    void* stream) {
  using namespace gd4d;
  if (!g_fine || !g_coarse) return GD4D_EINVAL;
  if (h <= 0 || w <= 0 || coarse_h <= 0 || coarse_w <= 0) return GD4D_EINVAL;
  if (channels != FT_C || n <= 0 || coarse_h > h || coarse_w > w) return GD4D_EUNSUPPORTED;     // the top-down path only upsamples
  const long long hw = (long long)h * w;
  if ((long long)n * FT_C * hw > (1ll << 40) || hw > (1ll << 30)) return GD4D_EUNSUPPORTED;
  const long long total = (long long)n * FT_C * coarse_h * coarse_w;
  if (total > (1ll << 38)) return GD4D_EUNSUPPORTED;
  hipLaunchKernelGGL(fpn_topdown_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), g_fine,
                     g_coarse, total, h, w, coarse_h, coarse_w, (float)coarse_h / (float)h, (float)coarse_w / (float)w);
  return check_launch();
}

extern "C" int gd4d_fpn_extra_conv_wgrad(const float* dy, const float* x, int n, int channels, int h, int w, int relu_in, float* dw,
                                         float* db, void* stream) {
  using namespace gd4d;
  if (!dy || !x || !dw) return GD4D_EINVAL;
  if (h <= 0 || w <= 0) return GD4D_EINVAL;
  if (channels != FT_C || n <= 0 || (relu_in != 0 && relu_in != 1)) return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if ((long long)n * FT_C * hw > (1ll << 40) || hw > (1ll << 30)) return GD4D_EUNSUPPORTED;
  ExtraWgradParams p{};
  p.dy = dy;
  p.x = x;
  p.dw = dw;
  p.db = db;
  p.H = h;
  p.W = w;
  p.Ho = (h + 1) / 2;
  p.Wo = (w + 1) / 2;
  const long long total = (long long)n * p.Ho * p.Wo;
  if (total > (1ll << 30)) return GD4D_EUNSUPPORTED;
  p.total = (int)total;
  p.relu_in = relu_in;
  hipLaunchKernelGGL(fpn_extra_wgrad_kernel, dim3(EW_CHUNKS * EW_TAPS), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_fpn_bias_grad(const float* g, int n, int channels, int h, int w, float* workspace, float* db, void* stream) {
  using namespace gd4d;
  if (!g || !workspace || !db) return GD4D_EINVAL;
  if (h <= 0 || w <= 0) return GD4D_EINVAL;
  if (channels != FT_C || n <= 0) return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if ((long long)n * FT_C * hw > (1ll << 40) || hw > (1ll << 30) || (long long)n * FT_C > (1ll << 30)) return GD4D_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(fpn_plane_sum_kernel, dim3((unsigned)(n * FT_C)), dim3(256), 0, s, g, (int)hw, workspace);
  hipLaunchKernelGGL(fpn_plane_sum_cams_kernel, dim3(1), dim3(FT_C), 0, s, workspace, n, db);
  return check_launch();
}
