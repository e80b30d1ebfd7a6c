// Training of mmdet's ResNet blocks behind frozen BatchNorms (gd4d_resnet.hip holds the forward; gd4d_vovnet_gemm.h the GEMM of the
// data gradients; gd4d_conv_wgrad.h the two weight-gradient bodies).  A unit is conv -> folded BatchNorm (s = gamma rstd) (-> + identity)
// (-> ReLU); dz is always the gradient of the BatchNorm's OUTPUT after the ReLU's mask, unscaled.  Given dout, a block runs
//
//   gd4d_relu_mask_bwd            g = dout [out > 0]: the one elementwise pass of a block (dout arrives unmasked: the next block and
//                                 the neck sum into it).
//   gd4d_conv1x1_dgrad            dx = ((s W)^T dz (+ add)) ([mask > 0]) (+ add2) (+ add_even at the even pixels): vv_gemm_kernel<MT,
//                                 VV_OSA, VV_BWD> on the transposed scaled image (gd4d_conv1x1_image_t), one destination; K = the
//                                 forward's Cout and M = its Cin, each a multiple of 32 up to 2048.  Always stride 1: a stride-2
//                                 downsample's adjoint is this launch on the HALF-resolution grid, and the unit below adds its result
//                                 through add_even - no zero-filled full-resolution map is written.
//   gd4d_conv3x3_act_dgrad        the same for the 3x3 (pad 1) at ResNet's widths, K = Cout up to 512 and M = Cin up to 1024.  Stride 1:
//                                 vv_gemm_kernel<MT, VV_S1, VV_BWD>, what gd4d_conv3x3_dgrad launches, behind ResNet's limits.  Stride 2:
//                                 MODE VV_T2, dx[y, x] = sum over (ky, kx) of (s W)^T[ky, kx] dz[(y + 1 - ky) / 2, (x + 1 - kx) / 2] where
//                                 both quotients are whole and inside Ho x Wo, Ho = (H - 1) / 2 + 1.  FIRST VERSION: VV_S1's walk over dz
//                                 zero-interleaved in the staged patch (LDS only; nothing interleaved is written to memory).  All nine
//                                 taps are walked, so the launch does the four parity classes' 1 + 2 + 2 + 4 taps as 4 x 9: four
//                                 times the MFMA work, on one convolution per stage.  Odd H and W are exact: the last row of an odd
//                                 map is an even index and only ky = 1 meets a staged dz row there.
//   gd4d_conv1x1_wgrad            G[co, k] = sum over images and OUTPUT pixels of dz[co, p] x[k, in(p)], in(p) = p at stride 1 and
//                                 (2 yo, 2 xo) at stride 2, read in place: conv1x1_wgrad_body with RtPwWgradShape - blocks of 256
//                                 output channels along blockIdx.y, guarded at Cout (up to 2048), K up to 2048 - and the body's sum of
//                                 dz (dbeta's partials).
//   gd4d_conv3x3_act_wgrad        G[co, ci, tap] for Cout up to 512, Cin up to 1024: conv3x3_wgrad_body with RtWgradShape, whose
//                                 workgroups own a block of Cout / 32 / blocks waves (at most 8: 512 is two blocks of 256, never a
//                                 1024-thread workgroup) along blockIdx.y.  Stride 2, FIRST VERSION: the stride-1 body on dz
//                                 zero-interleaved to the input's resolution (rt_even_scatter_kernel writes it into the workspace):
//                                 exact, four times the MFMA work, on one convolution per stage.
//   (both)                        vt_finish (gd4d_vovnet_train.hip): dW = s (x) G, dbeta = sum dz, dgamma = rstd (<W, G> - mean dbeta).
//   gd4d_even_pixels_scatter      dst (planes, h, w) = src[y / 2, x / 2] at even (y, x), else 0: the DCN bottleneck's tail node hands
//                                 autograd a full-resolution gradient of the block input under a stride-2 downsample.
//
// Arithmetic: gd4d_bf16x3.h's three products, fp32 sums in a fixed order, no atomics: two runs give the same bits.
//
// Resources (tools/kernel_code_sizes.py; gfx950): VGPRs + AGPRs, dynamic LDS bytes.  Scratch is 0 bytes per lane and no register is
// spilled in any instantiation.  VV_S1 / VV_BWD is gd4d_vovnet_train.hip's instantiation, compiled here a second time.
//     MT     3x3 stride 1 adjoint (VV_S1)    3x3 stride 2 adjoint (VV_T2)    1x1 adjoint (VV_OSA)
//     7      260 + 112, 103 424              260 + 112, 103 424              240 + 112, 90 112
//     5      216 +  80,  87 040              216 +  80,  87 040              176 +  80, 73 728
//     4      196 +  64,  78 848              196 +  64,  78 848              152 +  64, 65 536
//     3      176 +  48,  70 656              176 +  48,  70 656              136 +  48, 57 344
//     2      156 +  32,  62 464              156 +  32,  62 464              116 +  32, 49 152
//     1      136 +  16,  54 272              136 +  16,  54 272               92 +  16, 40 960
// rt_conv3x3_wgrad_kernel 206 + 0, 113 664 B (CW3_LDS; one workgroup per CU); rt_conv1x1_wgrad_kernel 196 + 64, 18 432 B static;
// rt_relu_mask_kernel 4 + 0 and rt_even_scatter_kernel 6 + 0, no LDS.
//
// Measured (an MI355X, ResNet-50 at 6 x 3 x 320 x 800, one training step, docs/measurements_r44.md): the 3x3 stride-2 weight gradient
// shipped in its zero-interleaved form (rt_conv3x3_wgrad_kernel: 13 calls 1.39 ms in all, three of them of stride 2, whose
// rt_even_scatter_kernel passes add 0.04 ms); the stride-2 adjoint (VV_T2, MT = 4) 3 calls 0.45 ms.  The largest single item is the shared finishing kernel, 42 calls 3.1 ms: a workgroup per output
// channel adds the partitions' slabs one after the other.
#include "gd4d_conv_wgrad.h"
#include "gd4d_vovnet_gemm.h"

namespace gd4d {

static bool rt_pw_channels(int cin, int cout) {
  return cin % 32 == 0 && cin >= 32 && cin <= 2048 && cout % 32 == 0 && cout >= 32 && cout <= 2048;
}
static bool rt_conv_channels(int cin, int cout) {
  return cin % 32 == 0 && cin >= 32 && cin <= 1024 && cout % 32 == 0 && cout >= 32 && cout <= 512;
}
static bool rt_channels(int taps, int cin, int cout) {
  return taps == 9 ? rt_conv_channels(cin, cout) : taps == 1 ? rt_pw_channels(cin, cout) : false;
}

// ---- the elementwise passes ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rt_relu_mask_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                           const long long count, float* __restrict__ g) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) g[i] = out[i] > 0.f ? dout[i] : 0.f;        // strict, as torch's ReLU
}

// grid (ceil(h w / 256), planes): dst[plane, y, x] = src[plane, y / 2, x / 2] at even (y, x), else 0
__global__ __launch_bounds__(256) void rt_even_scatter_kernel(const float* __restrict__ src, const int h, const int w,
                                                              float* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  const int hs = (h - 1) / 2 + 1, ws = (w - 1) / 2 + 1;
  const size_t plane = blockIdx.y;
  dst[plane * h * w + i] = ((y | x) & 1) ? 0.f : src[plane * hs * ws + (size_t)(y >> 1) * ws + (x >> 1)];
}

static int rt_even_scatter(const float* src, long long planes, int h, int w, float* dst, hipStream_t s) {
  for (long long p0 = 0; p0 < planes; p0 += 65535) {         // gridDim.y's limit
    const long long np = planes - p0 < 65535 ? planes - p0 : 65535;
    const size_t hs = (size_t)((h - 1) / 2 + 1) * ((w - 1) / 2 + 1);
    hipLaunchKernelGGL(rt_even_scatter_kernel, dim3((unsigned)((h * w + 255) / 256), (unsigned)np), dim3(256), 0, s, src + p0 * hs, h, w,
                       dst + (size_t)p0 * h * w);
  }
  return check_launch();
}

// ---- 3x3 weight gradient --------------------------------------------------------------------------------------------------------
constexpr int RT_W3_MAX_WAVES = 8;                           // a workgroup's block of output channels: at most 256

struct RtWgradParams {
  const float* dz;                 // (N, cout, H, W)
  const float* x;                  // (N, cin, H, W)
  int cin, cout, h, w, tiles_x, tiles_img, tiles, partitions, chunks;
  float* ws;                       // (partitions, 9, cout, cin)
  float* ws_b;                     // (partitions, cout)
};

// conv3x3_wgrad_body's policy: VvWgradShape's run-time channel counts over the tiles of a single map, with the workgroup's block of
// blockDim.x / 64 x 32 output channels chosen by blockIdx.y: `p` is the workgroup's view, its dz, ws and ws_b moved to the block's first
// output channel, so the body's wave-relative output channel lands where the whole map's does
struct RtWgradShape {
  const RtWgradParams p;
  __device__ __forceinline__ int cin() const { return p.cin; }
  __device__ __forceinline__ int cout() const { return p.cout; }
  __device__ __forceinline__ int chunks() const { return p.chunks; }
  __device__ __forceinline__ int threads() const { return blockDim.x; }
  __device__ __forceinline__ Conv3x3Tile tile(int t, int chunk, int oc_a) const {
    const size_t HW = (size_t)p.h * p.w;
    const int cam = t / p.tiles_img;
    const int rt = t - cam * p.tiles_img;
    return {p.h, p.w, (rt / p.tiles_x) * CW3_T, (rt % p.tiles_x) * CW3_T, p.x + ((size_t)cam * p.cin + chunk * CW3_KC) * HW,
            p.dz + ((size_t)cam * p.cout + oc_a) * HW};
  }
};

// blockDim = 64 waves, waves <= 8 dividing cout / 32; gridDim.y = cout / (32 waves)
__global__ __launch_bounds__(64 * RT_W3_MAX_WAVES) void rt_conv3x3_wgrad_kernel(const RtWgradParams q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  RtWgradParams p = q;
  const int oc0 = blockIdx.y * (blockDim.x >> 6) * 32;
  p.dz += (size_t)oc0 * p.h * p.w;
  p.ws += (size_t)oc0 * p.cin;
  p.ws_b += oc0;
  conv3x3_wgrad_body<RtWgradShape, true>(RtWgradShape{p}, smem);
}

static int rt_w3_waves(int cout) {
  const int nb = cout / 32;
  for (int wv = RT_W3_MAX_WAVES; wv > 1; --wv)
    if (nb % wv == 0) return wv;
  return 1;
}

// ---- 1x1 weight gradient --------------------------------------------------------------------------------------------------------
struct RtPwWgradParams {
  const float* dz;                 // (N, cout, Ho, Wo)
  const float* x;                  // (N, k, H, W)
  int k, cout, stride, w_in, wo, plane_in, hw, tiles_img, tiles, partitions, chunks;
  float* ws;                       // (partitions, cout, k)
  float* ws_b;                     // (partitions, cout)
};

// conv1x1_wgrad_body's policy: a block of 256 output channels per blockIdx.y, guarded at cout; one source map, read where the
// convolution's stride puts output pixel p: p itself, or input pixel (2 yo, 2 xo)
struct RtPwWgradShape {
  const RtPwWgradParams& p;
  const Conv1x1Wgrad g;
  static constexpr bool GUARD = true;
  __device__ __forceinline__ int cout() const { return p.cout; }
  __device__ __forceinline__ int oc0(int wave) const { return blockIdx.y * CW1_OC + 64 * wave; }
  __device__ __forceinline__ Conv1x1Source source(int icg, bool ok) const { return {p.x, p.k, ok ? icg : 0}; }
  __device__ __forceinline__ size_t x_plane() const { return (size_t)p.plane_in; }
  __device__ __forceinline__ int x_pixel(int px) const {
    if (p.stride == 1) return px;
    const int yo = px / p.wo;
    return 2 * yo * p.w_in + 2 * (px - yo * p.wo);
  }
};

__global__ __launch_bounds__(CW1_THREADS) void rt_conv1x1_wgrad_kernel(const RtPwWgradParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 s_b[2][CW1_B_ARR];         // [hi, lo][channel][pixel group (+ 1)]
  conv1x1_wgrad_body<RtPwWgradShape, true>(
      RtPwWgradShape{p, {p.dz, p.ws, p.ws_b, p.k, p.hw, p.tiles_img, p.tiles, p.partitions, p.chunks}}, s_b);
}

static int rt_image_t(const float* weight, int cin, int cout, int taps, void* image, void* stream) {
  if (!weight || !image) return GD4D_EINVAL;
  if (!rt_channels(taps, cin, cout)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  const ConvImage d{cin, cout, taps, 32, VV_KC, cin, 0, 1, taps > 1 ? 1 : 0};
  return pack_conv_image(d, weight, image, static_cast<hipStream_t>(stream));
}

// the argument checks and the launch of both data gradients; h, w are dx's (the convolution's input's)
static int rt_dgrad(int taps, const float* dz, int n, int cin, int cout, int h, int w, int stride, const void* image_t, const float* add,
                    const float* mask, const float* add2, const float* add_even, float* dx, int m_blocks, void* stream) {
  if (!dz || !image_t || !dx) return GD4D_EINVAL;
  if (!rt_channels(taps, cin, cout) || n <= 0 || h <= 0 || w <= 0 || (stride != 1 && stride != 2)) return GD4D_EUNSUPPORTED;
  if (taps == 1 && stride != 1) return GD4D_EUNSUPPORTED;
  if (!vv_mt_ok(cin, m_blocks)) return GD4D_EUNSUPPORTED;
  if ((long long)h * w > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image_t)) return GD4D_EALIGN;
  VvParams p{};
  p.src[0] = dz;
  p.src_ch[0] = cout;
  p.n_src = 1;
  p.chunks = cout / VV_KC;
  p.h = p.ho = h;
  p.w = p.wo = w;
  const bool flat = taps == 1;
  p.tiles_x = flat ? 1 : (w + VV_TX - 1) / VV_TX;
  p.tiles_img = flat ? (int)(((long long)h * w + VV_PIX - 1) / VV_PIX) : p.tiles_x * ((h + VV_TY - 1) / VV_TY);
  p.cout = cin;
  p.image = static_cast<const char*>(image_t);
  p.out = dx;
  p.add = add;
  p.mask = mask;
  p.add2 = add2;
  p.add_even = add_even;
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (flat) return vv_launch<VV_OSA, VV_BWD>(p, tiles, m_blocks, stream);
  return stride == 1 ? vv_launch<VV_S1, VV_BWD>(p, tiles, m_blocks, stream) : vv_launch<VV_T2, VV_BWD>(p, tiles, m_blocks, stream);
}

static bool rt_wgrad_sizes(int taps, int cin, int cout, int n, int h, int w, int stride, int partitions) {
  if (!rt_channels(taps, cin, cout) || n <= 0 || h <= 0 || w <= 0 || (stride != 1 && stride != 2) || !partitions_ok(partitions)) return false;
  return (long long)h * w <= (1ll << 30) && (long long)n * 2048 * h * w <= (1ll << 40);
}

}  // namespace gd4d

extern "C" size_t gd4d_conv1x1_image_t_bytes(int cin, int cout) { return gd4d::rt_pw_channels(cin, cout) ? (size_t)cout * cin * 4 : 0; }

extern "C" int gd4d_conv1x1_image_t(const float* weight, int cin, int cout, void* image, void* stream) {
  return gd4d::rt_image_t(weight, cin, cout, 1, image, stream);
}

extern "C" size_t gd4d_conv3x3_act_image_t_bytes(int cin, int cout) {
  return gd4d::rt_conv_channels(cin, cout) ? (size_t)cout * cin * 9 * 4 : 0;
}

extern "C" int gd4d_conv3x3_act_image_t(const float* weight, int cin, int cout, void* image, void* stream) {
  return gd4d::rt_image_t(weight, cin, cout, 9, image, stream);
}

extern "C" int gd4d_relu_mask_bwd(const float* dout, const float* out, long long count, float* g, void* stream) {
  using namespace gd4d;
  if (!dout || !out || !g) return GD4D_EINVAL;
  if (count <= 0 || count > (1ll << 38)) return GD4D_EUNSUPPORTED;
  hipLaunchKernelGGL(rt_relu_mask_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dout, out,
                     count, g);
  return check_launch();
}

extern "C" int gd4d_even_pixels_scatter(const float* src, long long planes, int h, int w, float* dst, void* stream) {
  using namespace gd4d;
  if (!src || !dst) return GD4D_EINVAL;
  if (planes <= 0 || h <= 0 || w <= 0 || (long long)h * w > (1ll << 30) || planes * h * w > (1ll << 38)) return GD4D_EUNSUPPORTED;
  return rt_even_scatter(src, planes, h, w, dst, static_cast<hipStream_t>(stream));
}

extern "C" int gd4d_conv1x1_dgrad(const float* dz, int n, int cin, int cout, int h, int w, const void* image_t, const float* add,
                                  const float* mask, const float* add2, const float* add_even, float* dx, int m_blocks, void* stream) {
  return gd4d::rt_dgrad(1, dz, n, cin, cout, h, w, 1, image_t, add, mask, add2, add_even, dx, m_blocks, stream);
}

extern "C" int gd4d_conv3x3_act_dgrad(const float* dz, int n, int cin, int cout, int h, int w, int stride, const void* image_t,
                                      const float* add, const float* mask, const float* add2, const float* add_even, float* dx,
                                      int m_blocks, void* stream) {
  return gd4d::rt_dgrad(9, dz, n, cin, cout, h, w, stride, image_t, add, mask, add2, add_even, dx, m_blocks, stream);
}

extern "C" long long gd4d_resnet_wgrad_tiles(int taps, int n, int h, int w, int stride) {
  if (n <= 0 || h <= 0 || w <= 0 || (stride != 1 && stride != 2)) return 0;
  if (taps == 9) return (long long)n * ((h + gd4d::CW3_T - 1) / gd4d::CW3_T) * ((w + gd4d::CW3_T - 1) / gd4d::CW3_T);
  if (taps != 1) return 0;
  const long long ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
  return (long long)n * ((ho * wo + gd4d::CW1_PX - 1) / gd4d::CW1_PX);
}

extern "C" size_t gd4d_resnet_wgrad_workspace_bytes(int taps, int cin, int cout, int n, int h, int w, int stride, int partitions) {
  using namespace gd4d;
  if (!rt_wgrad_sizes(taps, cin, cout, n, h, w, stride, partitions)) return 0;
  const size_t slabs = (size_t)partitions * ((size_t)taps * cout * cin + cout);
  const size_t scatter = taps == 9 && stride == 2 ? (size_t)n * cout * h * w : 0;       // dz zero-interleaved to the input's resolution
  return (slabs + scatter) * sizeof(float);
}

extern "C" int gd4d_conv3x3_act_wgrad(const float* dz, const float* x, int n, int cin, int cout, int h, int w, int stride, int partitions,
                                      float* workspace, const float* weight, const float* bn, float* dw, float* dgamma, float* dbeta,
                                      void* stream) {
  using namespace gd4d;
  if (!dz || !x || !workspace || !weight || !bn || (!dw && !dgamma && !dbeta)) return GD4D_EINVAL;
  if (!rt_wgrad_sizes(9, cin, cout, n, h, w, stride, partitions)) return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long tiles = gd4d_resnet_wgrad_tiles(9, n, h, w, stride);
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  RtWgradParams p{};
  p.ws = workspace;
  p.ws_b = workspace + (size_t)partitions * 9 * cout * cin;
  p.dz = dz;
  if (stride == 2) {
    float* const wide = p.ws_b + (size_t)partitions * cout;
    const int rc = rt_even_scatter(dz, (long long)n * cout, h, w, wide, s);
    if (rc != GD4D_OK) return rc;
    p.dz = wide;
  }
  p.x = x;
  p.cin = cin;
  p.cout = cout;
  p.h = h;
  p.w = w;
  p.tiles_x = (w + CW3_T - 1) / CW3_T;
  p.tiles_img = p.tiles_x * ((h + CW3_T - 1) / CW3_T);
  p.tiles = (int)tiles;
  p.partitions = partitions;
  p.chunks = cin / CW3_KC;
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(rt_conv3x3_wgrad_kernel), CW3_LDS)) return GD4D_ELAUNCH;
  const int waves = rt_w3_waves(cout);
  hipLaunchKernelGGL(rt_conv3x3_wgrad_kernel, dim3((unsigned)(p.chunks * partitions), (unsigned)(cout / (32 * waves))), dim3(64 * waves),
                     CW3_LDS, s, p);
  return vt_finish(p.ws, p.ws_b, partitions, partitions, cin, cout, 9, weight, bn, dw, dgamma, dbeta, s);
}

extern "C" int gd4d_conv1x1_wgrad(const float* dz, const float* x, int n, int cin, int cout, int h, int w, int stride, int partitions,
                                  float* workspace, const float* weight, const float* bn, float* dw, float* dgamma, float* dbeta,
                                  void* stream) {
  using namespace gd4d;
  if (!dz || !x || !workspace || !weight || !bn || (!dw && !dgamma && !dbeta)) return GD4D_EINVAL;
  if (!rt_wgrad_sizes(1, cin, cout, n, h, w, stride, partitions)) return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long tiles = gd4d_resnet_wgrad_tiles(1, n, h, w, stride);
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
  RtPwWgradParams p{};
  p.dz = dz;
  p.x = x;
  p.k = cin;
  p.cout = cout;
  p.stride = stride;
  p.w_in = w;
  p.wo = wo;
  p.plane_in = h * w;
  p.hw = ho * wo;
  p.tiles_img = (int)(tiles / n);
  p.tiles = (int)tiles;
  p.partitions = partitions;
  p.chunks = (cin + CW1_IC - 1) / CW1_IC;
  p.ws = workspace;
  p.ws_b = workspace + (size_t)partitions * cout * cin;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rt_conv1x1_wgrad_kernel, dim3((unsigned)(p.chunks * partitions), (unsigned)((cout + CW1_OC - 1) / CW1_OC)),
                     dim3(CW1_THREADS), 0, s, p);
  return vt_finish(p.ws, p.ws_b, partitions, partitions, cin, cout, 1, weight, bn, dw, dgamma, dbeta, s);
}
