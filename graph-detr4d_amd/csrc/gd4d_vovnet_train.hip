// Training of VoVNet's OSA module behind frozen BatchNorms (gd4d_vovnet.hip holds the forward; gd4d_vovnet_gemm.h the GEMM both share).
// With s_i = gamma_i rstd_i, t_i = beta_i - mean_i s_i the forward is
//     x_0 = input, x_i = relu(s_i conv3x3_i(x_{i-1}) + t_i)  (i = 1 .. L),   xt = relu(s_c (W_c . cat(x_0 .. x_L)) + t_c),
//     m = mean_hw(xt), v = fc_w m + fc_b, gate = clamp(v + 3, 0, 6) / 6, out = xt gate (+ x_0)
// and the backward, given dout, runs on these entry points:
//
//   gd4d_ese_bwd               dgate[n, c] = sum_hw dout xt (a workgroup per plane: strided partial sums, LDS tree); per image
//                              dv = dgate / 6 where 0 < gate < 1 on the stored fp32 gate (else 0: the clamp's flat parts AND its two
//                              corners pass nothing), dm = fc_w^T dv, with m re-formed from the aggregation's pool partials in the
//                              forward's tile order (the same bits); dfc_w = sum_n dv (x) m, dfc_b = sum_n dv; then one pass per plane
//                              writes dz_c = (dout gate + dm / HW) [xt > 0] and its sum (dbeta_c's partials).
//   gd4d_osa_concat_dgrad      g_i = rows of source i of (s_c W_c)^T dz_c, written straight into the L + 1 maps (the concatenation's
//                              gradient is never formed): vv_gemm_kernel<MT, OSA, BWD> on the transposed image, one launch per
//                              destination map with that map's own M tiling (1024 -> 4, 224 -> 7, ...; the image is laid out per row
//                              block of 32, so a destination's rows are contiguous and the bits do not depend on the tiling).  The
//                              last destination may be masked in the epilogue: dz_L = g_L [x_L > 0].
//   gd4d_conv3x3_dgrad         dx = ((s W)^T, tap-flipped) * dz (+ add) ([mask > 0]) (+ add2): vv_gemm_kernel<MT, S1, BWD> with M = the
//                              forward's Cin (<= 1024) and K = its Cout (<= 256).  One launch per chain step: add = g_{i-1} from the
//                              aggregation, mask = x_{i-1} (the next step's ReLU), add2 = dout for the residual at the input.
//   gd4d_conv3x3_wgrad         G[c, k, tap] = sum over images and pixels of dz[c, p] x_in[k, p + tap] for any Cout <= 256, Cin <= 1024
//                              (multiples of 32): conv3x3_wgrad_body (gd4d_conv_wgrad.h has the algorithm) with Cin, Cout and the
//                              workgroup's Cout / 32 waves at run time, over the (image, 16 x 16 tile) list of one map, and the sum
//                              of dz (dbeta's partials).
//   gd4d_osa_concat_wgrad      the same for the 1x1 aggregation: conv1x1_wgrad_body with blocks of 256 output channels along
//                              blockIdx.y, guarded at Cout, and K = the concatenated channels, each read from the one of the L + 1
//                              maps where it lies; no sum of dz (gd4d_ese_bwd left it in dz_sums).
//   (both)                     the finishing kernel, a workgroup per output channel c: G = the partitions' partials added in order,
//                              dW[c] = s[c] G[c], dbeta[c] = sum dz, dgamma[c] = rstd[c] (<W[c], G[c]> - mean[c] dbeta[c]).  The
//                              identity holds because the pre-BatchNorm map is W * x_in: no such map is stored or recomputed, and
//                              gamma = 0 is exact.  dz is the UNSCALED gradient (of the BatchNorm's output).
// All GEMMs on the split-bf16 x 3 MFMA (gd4d_bf16x3.h).  No atomics; every sum has a fixed order: two runs give the same bits.
#include "gd4d_conv_wgrad.h"
#include "gd4d_vovnet_gemm.h"

namespace gd4d {

// ---- eSE backward -------------------------------------------------------------------------------------------------------------
constexpr int VT_ESE_MAX_C = 1024;

__global__ __launch_bounds__(256) void vt_ese_reduce_kernel(const float* __restrict__ dout, const float* __restrict__ xt, const int hw,
                                                            float* __restrict__ dgate) {
  __shared__ float red[256];
  const size_t base = (size_t)blockIdx.x * hw;
  float s = 0.f;
  for (int i = threadIdx.x; i < hw; i += 256) s += dout[base + i] * xt[base + i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) dgate[blockIdx.x] = s;
}

// grid (n, ceil(C / 256)): every workgroup forms the image's whole dv (its columns of fc_w^T need all of it); the workgroups of
// column block 0 also leave dv and the re-formed mean for the parameter gradients
__global__ __launch_bounds__(256) void vt_ese_gate_kernel(const float* __restrict__ dgate, const float* __restrict__ gate,
                                                          const float* __restrict__ partials, const int tiles, const int c_all, const int hw,
                                                          const float* __restrict__ fc_w, float* __restrict__ dv, float* __restrict__ mean,
                                                          float* __restrict__ dm) {
  __shared__ float s_dv[VT_ESE_MAX_C];
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < c_all; c += 256) {
    const float g = gate[(size_t)n * c_all + c];
    const float d = (g > 0.f && g < 1.f) ? dgate[(size_t)n * c_all + c] / 6.f : 0.f;
    s_dv[c] = d;
    if (blockIdx.y == 0) {
      dv[(size_t)n * c_all + c] = d;
      float s = 0.f;
      for (int t = 0; t < tiles; ++t) s += partials[((size_t)n * tiles + t) * c_all + c];     // the forward's order
      mean[(size_t)n * c_all + c] = s / (float)hw;
    }
  }
  __syncthreads();
  const int k = blockIdx.y * 256 + threadIdx.x;
  if (k < c_all) {
    float acc = 0.f;
    for (int c = 0; c < c_all; ++c) acc = fmaf(fc_w[(size_t)c * c_all + k], s_dv[c], acc);
    dm[(size_t)n * c_all + k] = acc;
  }
}

__global__ __launch_bounds__(256) void vt_ese_param_kernel(const float* __restrict__ dv, const float* __restrict__ mean, const int n,
                                                           const int c_all, float* __restrict__ dfc_w, float* __restrict__ dfc_b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c_all * c_all) return;
  const int c = i / c_all, k = i - c * c_all;
  float s = 0.f, b = 0.f;
  for (int q = 0; q < n; ++q) {
    const float d = dv[(size_t)q * c_all + c];
    s = fmaf(d, mean[(size_t)q * c_all + k], s);
    b += d;
  }
  if (dfc_w) dfc_w[i] = s;
  if (dfc_b && k == 0) dfc_b[c] = b;
}

__global__ __launch_bounds__(256) void vt_ese_apply_kernel(const float* __restrict__ dout, const float* __restrict__ xt,
                                                           const float* __restrict__ gate, const float* __restrict__ dm, const int hw,
                                                           float* __restrict__ dz, float* __restrict__ dz_sums) {
  __shared__ float red[256];
  const size_t base = (size_t)blockIdx.x * hw;
  const float g = gate[blockIdx.x], add = dm[blockIdx.x] / (float)hw;
  float s = 0.f;
  for (int i = threadIdx.x; i < hw; i += 256) {
    const float v = xt[base + i] > 0.f ? dout[base + i] * g + add : 0.f;       // strict, as torch's ReLU
    dz[base + i] = v;
    s += v;
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) dz_sums[blockIdx.x] = s;
}

// ---- 3x3 weight gradient ------------------------------------------------------------------------------------------------------
constexpr int VW_MAX_THREADS = 512;

struct VvWgradParams {
  const float* dz;                 // (N, cout, H, W)
  const float* x;                  // (N, cin, H, W)
  int cin, cout, h, w, tiles_x, tiles_img, tiles, partitions, chunks;
  float* ws;                       // (partitions, 9, cout, cin)
  float* ws_b;                     // (partitions, cout)
};

// conv3x3_wgrad_body's policy: channel counts and the workgroup's size at run time, the tiles of a single map
struct VvWgradShape {
  const VvWgradParams& p;
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

// blockDim = 64 (cout / 32)
__global__ __launch_bounds__(VW_MAX_THREADS) void vt_conv3x3_wgrad_kernel(const VvWgradParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv3x3_wgrad_body<VvWgradShape, true>(VvWgradShape{p}, smem);
}

// ---- aggregation (1x1) weight gradient ----------------------------------------------------------------------------------------
struct VvAggWgradParams {
  const float* dz;                 // (N, cout, H, W)
  const float* src[VV_MAX_SRC];
  int src_ch[VV_MAX_SRC], src_c0[VV_MAX_SRC];
  int n_src, k, cout, hw, tiles_img, tiles, partitions, chunks;
  float* ws;                       // (partitions, cout, k)
};

// conv1x1_wgrad_body's policy: a block of 256 output channels per blockIdx.y, guarded at cout; K is the concatenation of the source
// maps, a staged channel is read from the map it lies in
struct OsaWgradShape {
  const VvAggWgradParams& p;
  const Conv1x1Wgrad g;
  static constexpr bool GUARD = true;
  __device__ __forceinline__ int cout() const { return p.cout; }
  __device__ __forceinline__ int oc0(int wave) const { return blockIdx.y * CW1_OC + 64 * wave; }
  __device__ __forceinline__ Conv1x1Source source(int icg, bool ok) const {
    Conv1x1Source s{p.src[0], p.src_ch[0], ok ? icg : 0};
#pragma unroll
    for (int i = 1; i < VV_MAX_SRC; ++i)
      if (i < p.n_src && ok && icg >= p.src_c0[i]) s = {p.src[i], p.src_ch[i], icg - p.src_c0[i]};
    return s;
  }
  __device__ __forceinline__ size_t x_plane() const { return (size_t)g.hw; }
  __device__ __forceinline__ int x_pixel(int px) const { return px; }
};

__global__ __launch_bounds__(CW1_THREADS) void vt_osa_wgrad_kernel(const VvAggWgradParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 s_b[2][CW1_B_ARR];         // [hi, lo][channel][pixel group (+ 1)]
  conv1x1_wgrad_body<OsaWgradShape, false>(
      OsaWgradShape{p, {p.dz, p.ws, nullptr, p.k, p.hw, p.tiles_img, p.tiles, p.partitions, p.chunks}}, s_b);
}

// ---- the finishing step of both weight gradients: a workgroup per output channel ---------------------------------------------
struct VvFinishParams {
  const float* ws;                 // (partitions, taps, cout, cin)
  const float* ws_b;               // (parts_b, cout)
  const float* weight;             // (cout, cin, taps)
  const float* bn;                 // (3, cout): scale, rstd, mean
  int partitions, parts_b, cin, cout, taps;
  float *dw, *dgamma, *dbeta;      // each optional
};

__global__ __launch_bounds__(256) void vt_wgrad_finish_kernel(const VvFinishParams p) {
  __shared__ float red[256];
  const int c = blockIdx.x, per = p.cin * p.taps;
  const size_t total = (size_t)p.taps * p.cout * p.cin;
  const float scale = p.bn[c];
  float dot = 0.f;
  for (int i = threadIdx.x; i < per; i += 256) {
    const int k = i / p.taps, tap = i - k * p.taps;
    const float* const q0 = p.ws + ((size_t)tap * p.cout + c) * p.cin + k;
    float g = 0.f;
    for (int q = 0; q < p.partitions; ++q) g += q0[(size_t)q * total];
    if (p.dw) p.dw[(size_t)c * per + i] = scale * g;
    dot = fmaf(p.weight[(size_t)c * per + i], g, dot);
  }
  dot = block_sum_256(dot, red);
  if (threadIdx.x == 0) {
    float b = 0.f;
    for (int q = 0; q < p.parts_b; ++q) b += p.ws_b[(size_t)q * p.cout + c];
    if (p.dbeta) p.dbeta[c] = b;
    if (p.dgamma) p.dgamma[c] = p.bn[p.cout + c] * (dot - p.bn[2 * p.cout + c] * b);
  }
}

static int vt_image_t(const float* weight, int cin, int cout, int taps, void* image, void* stream) {
  if (!aligned16(image)) return GD4D_EALIGN;
  const ConvImage d{cin, cout, taps, 32, VV_KC, cin, 0, 1, taps > 1 ? 1 : 0};
  return pack_conv_image(d, weight, image, static_cast<hipStream_t>(stream));
}

static void vt_geometry(VvParams& p, const float* dz, int k_ch, int h, int w, bool osa) {
  p.src[0] = dz;
  p.src_ch[0] = k_ch;
  p.n_src = 1;
  p.chunks = k_ch / VV_KC;
  p.h = p.ho = h;
  p.w = p.wo = w;
  p.tiles_x = osa ? 1 : (w + VV_TX - 1) / VV_TX;
  p.tiles_img = osa ? (int)(((long long)h * w + VV_PIX - 1) / VV_PIX) : p.tiles_x * ((h + VV_TY - 1) / VV_TY);
}

}  // namespace gd4d

extern "C" size_t gd4d_conv3x3_image_t_bytes(int cin, int cout) { return gd4d_conv3x3_image_bytes(cin, cout); }

extern "C" int gd4d_conv3x3_image_t(const float* weight, int cin, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  if (!vv_conv_channels(cin, cout)) return GD4D_EUNSUPPORTED;
  return vt_image_t(weight, cin, cout, 9, image, stream);
}

extern "C" size_t gd4d_osa_concat_image_t_bytes(int k, int cout) { return gd4d_osa_concat_image_bytes(k, cout); }

extern "C" int gd4d_osa_concat_image_t(const float* weight, int k, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  if (!vv_osa_channels(k, cout)) return GD4D_EUNSUPPORTED;
  return vt_image_t(weight, k, cout, 1, image, stream);
}

extern "C" int gd4d_conv3x3_dgrad(const float* dz, int n, int cin, int cout, int h, int w, const void* image_t, const float* add,
                                  const float* mask, const float* add2, float* dx, int m_blocks, void* stream) {
  using namespace gd4d;
  if (!dz || !image_t || !dx) return GD4D_EINVAL;
  if (!vv_conv_channels(cin, cout) || n <= 0 || h <= 0 || w <= 0) return GD4D_EUNSUPPORTED;
  if (!vv_mt_ok(cin, m_blocks)) return GD4D_EUNSUPPORTED;
  if ((long long)h * w > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image_t)) return GD4D_EALIGN;
  VvParams p{};
  vt_geometry(p, dz, cout, h, w, false);
  p.cout = cin;
  p.image = static_cast<const char*>(image_t);
  p.out = dx;
  p.add = add;
  p.mask = mask;
  p.add2 = add2;
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  return vv_launch<VV_S1, VV_BWD>(p, tiles, m_blocks, stream);
}

extern "C" int gd4d_osa_concat_dgrad(const float* dz, int n, int cout, int h, int w, const void* image_t, float* const* dst,
                                     const int32_t* dst_channels, int n_dst, const float* mask_last, int m_blocks, void* stream) {
  using namespace gd4d;
  if (!dz || !image_t || !dst || !dst_channels) return GD4D_EINVAL;
  if (n_dst < 1 || n_dst > VV_MAX_SRC || n <= 0 || h <= 0 || w <= 0 || (long long)h * w > (1ll << 30)) return GD4D_EUNSUPPORTED;
  int k = 0;
  for (int i = 0; i < n_dst; ++i) {
    if (!dst[i]) return GD4D_EINVAL;
    const int c = dst_channels[i];
    if (c <= 0 || c % VV_KC || c > 2304 || !vv_mt_ok(c, m_blocks)) return GD4D_EUNSUPPORTED;
    k += c;
  }
  if (!vv_osa_channels(k, cout)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image_t)) return GD4D_EALIGN;
  VvParams p{};
  vt_geometry(p, dz, cout, h, w, true);
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  const size_t block_bytes = (size_t)p.chunks * 2 * 4 * 32 * 16;             // a row block of 32: chunks steps of 4 KB
  int row0 = 0;
  for (int i = 0; i < n_dst; ++i) {
    p.cout = dst_channels[i];
    p.image = static_cast<const char*>(image_t) + (size_t)(row0 / 32) * block_bytes;
    p.out = dst[i];
    p.mask = i == n_dst - 1 ? mask_last : nullptr;
    const int rc = vv_launch<VV_OSA, VV_BWD>(p, tiles, m_blocks, stream);
    if (rc != GD4D_OK) return rc;
    row0 += dst_channels[i];
  }
  return GD4D_OK;
}

extern "C" long long gd4d_conv3x3_wgrad_tiles(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (long long)n * ((h + gd4d::CW3_T - 1) / gd4d::CW3_T) * ((w + gd4d::CW3_T - 1) / gd4d::CW3_T);
}

extern "C" long long gd4d_osa_concat_wgrad_tiles(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (long long)n * (((long long)h * w + gd4d::CW1_PX - 1) / gd4d::CW1_PX);
}

extern "C" size_t gd4d_conv_wgrad_workspace_bytes(int cin, int cout, int taps, int partitions) {
  using namespace gd4d;
  if (!partitions_ok(partitions)) return 0;
  if (!(taps == 9 ? vv_conv_channels(cin, cout) : taps == 1 ? vv_osa_channels(cin, cout) : false)) return 0;
  return (size_t)partitions * ((size_t)taps * cout * cin + cout) * sizeof(float);
}

namespace gd4d {
// (not static: gd4d_resnet_train.hip finishes its weight gradients with it too; declared in gd4d_conv_wgrad.h)
int vt_finish(const float* ws, const float* ws_b, int partitions, int parts_b, int cin, int cout, int taps, const float* weight,
                     const float* bn, float* dw, float* dgamma, float* dbeta, hipStream_t s) {
  VvFinishParams f{ws, ws_b, weight, bn, partitions, parts_b, cin, cout, taps, dw, dgamma, dbeta};
  hipLaunchKernelGGL(vt_wgrad_finish_kernel, dim3((unsigned)cout), dim3(256), 0, s, f);
  return check_launch();
}
}  // namespace gd4d

extern "C" int gd4d_conv3x3_wgrad(const float* dz, const float* x, int n, int cin, int cout, int h, int w, int partitions,
                                  float* workspace, const float* weight, const float* bn, float* dw, float* dgamma, float* dbeta,
                                  void* stream) {
  using namespace gd4d;
  if (!dz || !x || !workspace || !weight || !bn || (!dw && !dgamma && !dbeta)) return GD4D_EINVAL;
  if (!vv_conv_channels(cin, cout) || n <= 0 || h <= 0 || w <= 0 || !partitions_ok(partitions)) return GD4D_EUNSUPPORTED;
  if ((long long)h * w > (1ll << 30) || (long long)n * 1024 * h * w > (1ll << 40)) return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long tiles = gd4d_conv3x3_wgrad_tiles(n, h, w);
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  VvWgradParams p{};
  p.dz = dz;
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
  p.ws = workspace;
  p.ws_b = workspace + (size_t)partitions * 9 * cout * cin;
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(vt_conv3x3_wgrad_kernel), CW3_LDS)) return GD4D_ELAUNCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vt_conv3x3_wgrad_kernel, dim3((unsigned)(p.chunks * partitions)), dim3(64 * (cout / 32)), CW3_LDS, s, p);
  return vt_finish(p.ws, p.ws_b, partitions, partitions, cin, cout, 9, weight, bn, dw, dgamma, dbeta, s);
}

extern "C" int gd4d_osa_concat_wgrad(const float* dz, const float* dz_sums, const float* const* src, const int32_t* src_channels, int n_src,
                                     int n, int h, int w, int cout, int partitions, float* workspace, const float* weight, const float* bn,
                                     float* dw, float* dgamma, float* dbeta, void* stream) {
  using namespace gd4d;
  if (!dz || !dz_sums || !src || !src_channels || !workspace || !weight || !bn || (!dw && !dgamma && !dbeta)) return GD4D_EINVAL;
  if (n_src < 1 || n_src > VV_MAX_SRC || n <= 0 || h <= 0 || w <= 0 || !partitions_ok(partitions)) return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if (hw > (1ll << 30) || (long long)n * 2304 * hw > (1ll << 40)) return GD4D_EUNSUPPORTED;
  VvAggWgradParams p{};
  int k = 0;
  for (int i = 0; i < n_src; ++i) {
    if (!src[i]) return GD4D_EINVAL;
    const int c = src_channels[i];
    if (c <= 0 || c % VV_KC || c > 2304) return GD4D_EUNSUPPORTED;
    p.src[i] = src[i];
    p.src_ch[i] = c;
    p.src_c0[i] = k;
    k += c;
  }
  if (!vv_osa_channels(k, cout)) return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long tiles = gd4d_osa_concat_wgrad_tiles(n, h, w);
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  p.dz = dz;
  p.n_src = n_src;
  p.k = k;
  p.cout = cout;
  p.hw = (int)hw;
  p.tiles_img = (int)(tiles / n);
  p.tiles = (int)tiles;
  p.partitions = partitions;
  p.chunks = (k + CW1_IC - 1) / CW1_IC;
  p.ws = workspace;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vt_osa_wgrad_kernel, dim3((unsigned)(p.chunks * partitions), (unsigned)((cout + CW1_OC - 1) / CW1_OC)), dim3(CW1_THREADS), 0,
                     s, p);
  return vt_finish(p.ws, dz_sums, partitions, n, k, cout, 1, weight, bn, dw, dgamma, dbeta, s);
}

extern "C" size_t gd4d_ese_bwd_workspace_bytes(int n, int channels) {
  if (n <= 0 || channels % 32 || channels < 32 || channels > gd4d::VT_ESE_MAX_C) return 0;
  return (size_t)4 * n * channels * sizeof(float);             // dgate, dv, mean, dm
}

extern "C" int gd4d_ese_bwd(const float* dout, const float* xt, const float* partials, int tiles, const float* gate, const float* fc_w, int n,
                            int channels, int hw, float* workspace, float* dz, float* dz_sums, float* dfc_w, float* dfc_b, void* stream) {
  using namespace gd4d;
  if (!dout || !xt || !partials || !gate || !fc_w || !workspace || !dz || !dz_sums) return GD4D_EINVAL;
  if (n <= 0 || tiles <= 0 || hw <= 0 || channels % 32 || channels < 32 || channels > VT_ESE_MAX_C) return GD4D_EUNSUPPORTED;
  if (hw > (1 << 30) || (long long)n * channels > (1ll << 30)) return GD4D_EUNSUPPORTED;
  const size_t nc = (size_t)n * channels;
  float *dgate = workspace, *dv = workspace + nc, *mean = workspace + 2 * nc, *dm = workspace + 3 * nc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vt_ese_reduce_kernel, dim3((unsigned)nc), dim3(256), 0, s, dout, xt, hw, dgate);
  hipLaunchKernelGGL(vt_ese_gate_kernel, dim3(n, (channels + 255) / 256), dim3(256), 0, s, dgate, gate, partials, tiles, channels, hw, fc_w, dv,
                     mean, dm);
  if (dfc_w || dfc_b)
    hipLaunchKernelGGL(vt_ese_param_kernel, dim3((unsigned)((channels * channels + 255) / 256)), dim3(256), 0, s, dv, mean, n, channels, dfc_w,
                       dfc_b);
  hipLaunchKernelGGL(vt_ese_apply_kernel, dim3((unsigned)nc), dim3(256), 0, s, dout, xt, gate, dm, hw, dz, dz_sums);
  return check_launch();
}
