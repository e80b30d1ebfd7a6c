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
//                              (multiples of 32), after depth_wgrad_kernel: grid (Cin / 32 chunks) x P partitions of the (image,
//                              16 x 16 tile) list; a workgroup of Cout / 32 waves, wave w = output channels 32 w .. 32 w + 31 and nine
//                              32 x 32 accumulators; K runs over the pixels, a K step is one tile row; dz goes from global memory to
//                              registers (a row ahead) and is also summed there (dbeta); the chunk's 18 x 18 halo of x_in is staged
//                              once per tile, split hi / lo, as three copies shifted by kx.  Partials per partition in a workspace.
//   gd4d_osa_concat_wgrad      the same for the 1x1 aggregation, after fpn_lateral_wgrad_kernel: grid (chunks of 64 concatenated
//                              channels x P partitions of the (image, 64-pixel tile) list) x (blocks of 256 output channels); the
//                              chunk's channels are read from the L + 1 maps where they lie.
//   (both)                     the finishing kernel, a workgroup per output channel c: G = the partitions' partials added in order,
//                              dW[c] = s[c] G[c], dbeta[c] = sum dz, dgamma[c] = rstd[c] (<W[c], G[c]> - mean[c] dbeta[c]).  The
//                              identity holds because the pre-BatchNorm map is W * x_in: no such map is stored or recomputed, and
//                              gamma = 0 is exact.  dz is the UNSCALED gradient (of the BatchNorm's output).
// All GEMMs on the split-bf16 x 3 MFMA (gd4d_bf16x3.h).  No atomics; every sum has a fixed order: two runs give the same bits.
// Untuned: the weight-gradient kernels read dz once per input-channel chunk.
#include "gd4d_vovnet_gemm.h"

namespace gd4d {

// sum over the workgroup's 256 threads in a fixed order: a tree over LDS; the result in every thread
__device__ __forceinline__ float vt_block_sum_256(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// ---- eSE backward -------------------------------------------------------------------------------------------------------------
constexpr int VT_ESE_MAX_C = 1024;

__global__ __launch_bounds__(256) void vt_ese_reduce_kernel(const float* __restrict__ dout, const float* __restrict__ xt, const int hw,
                                                            float* __restrict__ dgate) {
  __shared__ float red[256];
  const size_t base = (size_t)blockIdx.x * hw;
  float s = 0.f;
  for (int i = threadIdx.x; i < hw; i += 256) s += dout[base + i] * xt[base + i];
  s = vt_block_sum_256(s, red);
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
  s = vt_block_sum_256(s, red);
  if (threadIdx.x == 0) dz_sums[blockIdx.x] = s;
}

// ---- 3x3 weight gradient ------------------------------------------------------------------------------------------------------
constexpr int VW_T = 16, VW_KC = 32, VW_HE = VW_T + 2, VW_MAX_THREADS = 512;
constexpr int VW_CH_STRIDE = VW_HE * 32 + 16;                 // 18 rows of 16 bf16 + 16 B: 16 lanes of a read on 16 distinct slots
constexpr int VW_PLANE = VW_KC * VW_CH_STRIDE;                // 18 944 B
constexpr int VW_LDS = 3 * 2 * VW_PLANE;                      // 113 664 B
constexpr int VW_ITEMS = 3 * VW_KC * VW_HE * 2;               // (kx, channel, halo row, 8-pixel half): 3456
static_assert(VW_LDS <= 160 * 1024, "LDS budget of a CU");

struct VvWgradParams {
  const float* dz;                 // (N, cout, H, W)
  const float* x;                  // (N, cin, H, W)
  int cin, cout, h, w, tiles_x, tiles_img, tiles, partitions, chunks;
  float* ws;                       // (partitions, 9, cout, cin)
  float* ws_b;                     // (partitions, cout)
};

// blockDim = 64 (cout / 32)
__global__ __launch_bounds__(VW_MAX_THREADS) void vt_conv3x3_wgrad_kernel(const VvWgradParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, threads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, kg = lane >> 5;
  const int chunk = blockIdx.x % p.chunks, part = blockIdx.x / p.chunks;
  const int t_begin = (int)((long long)part * p.tiles / p.partitions), t_end = (int)((long long)(part + 1) * p.tiles / p.partitions);
  const int H = p.h, W = p.w;
  const size_t HW = (size_t)H * W;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  const int oc_a = 32 * wave + l32;                          // the A operand's row of this lane
  for (int t = t_begin; t < t_end; ++t) {
    const int cam = t / p.tiles_img;
    const int rt = t - cam * p.tiles_img;
    const int ty0 = (rt / p.tiles_x) * VW_T, tx0 = (rt % p.tiles_x) * VW_T;
    const float* const xin = p.x + ((size_t)cam * p.cin + chunk * VW_KC) * HW;
    const float* const dzp = p.dz + ((size_t)cam * p.cout + oc_a) * HW;

    // one row of the dz tile: 8 pixels of this lane's output channel, zeros outside the image
    auto load_dz = [&](int py, float* v) {
      const int y = ty0 + py;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = tx0 + 8 * kg + j;
        v[j] = (y < H && x < W) ? dzp[(size_t)y * W + x] : 0.f;
      }
    };
    float a_next[8];
    load_dz(0, a_next);

    __syncthreads();                                         // the previous tile's readers are done
    for (int it = tid; it < VW_ITEMS; it += threads) {
      const int half = it & 1, q = it >> 1;
      const int hy = q % VW_HE, q2 = q / VW_HE;
      const int ic = q2 % VW_KC, kx = q2 / VW_KC;
      const int y = ty0 - 1 + hy, x0 = tx0 - 1 + kx + 8 * half;
      const bool row_in = y >= 0 && y < H;
      const float* src = xin + (size_t)ic * HW + (row_in ? (size_t)y * W : 0);
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = x0 + j;
        v[j] = (row_in && x >= 0 && x < W) ? src[x] : 0.f;
      }
      u32x4 hi, lo;
      split8(v, hi, lo);
      char* dst = smem + (size_t)(kx * 2) * VW_PLANE + ic * VW_CH_STRIDE + hy * 32 + half * 16;
      *reinterpret_cast<u32x4*>(dst) = hi;
      *reinterpret_cast<u32x4*>(dst + VW_PLANE) = lo;
    }
    __syncthreads();

    const char* const bbase = smem + l32 * VW_CH_STRIDE + kg * 16;
#pragma unroll 1
    for (int py = 0; py < VW_T; ++py) {
      u32x4 ah, al;
      split8(a_next, ah, al);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += a_next[j];
      bsum += s;
      if (py + 1 < VW_T) load_dz(py + 1, a_next);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const char* b = bbase + (kx * 2) * VW_PLANE + (py + ky) * 32;
          const u32x4 bh = *reinterpret_cast<const u32x4*>(b);
          const u32x4 bl = *reinterpret_cast<const u32x4*>(b + VW_PLANE);
          acc[3 * ky + kx] = mfma_32x32x16_x3(ah, al, bh, bl, acc[3 * ky + kx]);
        }
    }
  }

  // C/D of 32x32x16: column (input channel) = l32, rows (output channels) 4 kg + (r & 3) + 8 (r >> 2)
  float* const ws = p.ws + (size_t)part * 9 * p.cout * p.cin;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = 32 * wave + 4 * kg + (r & 3) + 8 * (r >> 2);
      ws[((size_t)t * p.cout + oc) * p.cin + chunk * VW_KC + l32] = acc[t][r];
    }
  const float other = __shfl_xor(bsum, 32);
  if (chunk == 0 && kg == 0) p.ws_b[(size_t)part * p.cout + oc_a] = bsum + other;               // pixels 0-7 of a row, then 8-15
}

// ---- aggregation (1x1) weight gradient ----------------------------------------------------------------------------------------
constexpr int VA_THREADS = 256, VA_PX = 64, VA_IC = 64, VA_OC = 256;
constexpr int VA_PITCH = 9;                            // 16-byte units per channel of the staged block: 8 pixel groups + 1
constexpr int VA_B_ARR = VA_IC * VA_PITCH;

struct VvAggWgradParams {
  const float* dz;                 // (N, cout, H, W)
  const float* src[VV_MAX_SRC];
  int src_ch[VV_MAX_SRC], src_c0[VV_MAX_SRC];
  int n_src, k, cout, hw, tiles_img, tiles, partitions, chunks;
  float* ws;                       // (partitions, cout, k)
};

__global__ __launch_bounds__(VA_THREADS) void vt_osa_wgrad_kernel(const VvAggWgradParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 s_b[2][VA_B_ARR];          // [hi, lo][channel][pixel group (+ 1)]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
  const int chunk = blockIdx.x % p.chunks, part = blockIdx.x / p.chunks;
  const int oc0 = blockIdx.y * VA_OC + 64 * wave;
  const int t_begin = (int)((long long)part * p.tiles / p.partitions), t_end = (int)((long long)(part + 1) * p.tiles / p.partitions);
  const size_t HW = (size_t)p.hw;

  // staging role: thread = (channel of the chunk, 16 consecutive pixels of the tile); the channel lies in one of the source maps
  const int s_ic = tid >> 2, s_q = tid & 3;
  const int s_icg = chunk * VA_IC + s_ic;
  const bool s_ic_ok = s_icg < p.k;
  const float* s_base = p.src[0];
  int s_cs = p.src_ch[0], s_cl = s_ic_ok ? s_icg : 0;
#pragma unroll
  for (int i = 1; i < VV_MAX_SRC; ++i)
    if (i < p.n_src && s_ic_ok && s_icg >= p.src_c0[i]) {
      s_base = p.src[i];
      s_cs = p.src_ch[i];
      s_cl = s_icg - p.src_c0[i];
    }
  float hr[16];
  auto issue = [&](int t) {
    const int cam = t / p.tiles_img, p0 = (t - cam * p.tiles_img) * VA_PX + 16 * s_q;
    const float* src = s_base + ((size_t)cam * s_cs + s_cl) * HW;
#pragma unroll
    for (int j = 0; j < 16; ++j) hr[j] = (s_ic_ok && p0 + j < p.hw) ? src[p0 + j] : 0.f;
  };
  auto park = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4 hi, lo;
      split8(hr + 8 * h, hi, lo);
      s_b[0][s_ic * VA_PITCH + 2 * s_q + h] = hi;
      s_b[1][s_ic * VA_PITCH + 2 * s_q + h] = lo;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  bool a_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) a_ok[i] = oc0 + 32 * i + l32 < p.cout;

  if (t_begin < t_end) issue(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();                                   // the previous tile's readers are done
    park();
    __syncthreads();
    if (t + 1 < t_end) issue(t + 1);
    const int cam = t / p.tiles_img, p0 = (t - cam * p.tiles_img) * VA_PX;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int px = p0 + 16 * ks + 8 * kg;
      u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float* const gp = p.dz + ((size_t)cam * p.cout + (a_ok[i] ? oc0 + 32 * i + l32 : 0)) * HW;
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (a_ok[i] && px + j < p.hw) ? gp[px + j] : 0.f;
        split8(a, ah[i], al[i]);
        bh[i] = s_b[0][(32 * i + l32) * VA_PITCH + 2 * ks + kg];
        bl[i] = s_b[1][(32 * i + l32) * VA_PITCH + 2 * ks + kg];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma_32x32x16_x3(ah[mi], al[mi], bh[ni], bl[ni], acc[mi][ni]);
    }
  }

  // C/D of 32x32x16: column (input channel) = l32, rows (output channels) 4 kg + (r & 3) + 8 (r >> 2)
  float* const ws = p.ws + (size_t)part * p.cout * p.k;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int ic = chunk * VA_IC + 32 * ni + l32;
    if (ic >= p.k) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int oc = oc0 + 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
        if (oc < p.cout) ws[(size_t)oc * p.k + ic] = acc[mi][ni][r];
      }
  }
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
  dot = vt_block_sum_256(dot, red);
  if (threadIdx.x == 0) {
    float b = 0.f;
    for (int q = 0; q < p.parts_b; ++q) b += p.ws_b[(size_t)q * p.cout + c];
    if (p.dbeta) p.dbeta[c] = b;
    if (p.dgamma) p.dgamma[c] = p.bn[p.cout + c] * (dot - p.bn[2 * p.cout + c] * b);
  }
}

static bool vt_parts_ok(int partitions) { return partitions >= 1 && partitions <= 4096; }

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
  return (long long)n * ((h + gd4d::VW_T - 1) / gd4d::VW_T) * ((w + gd4d::VW_T - 1) / gd4d::VW_T);
}

extern "C" long long gd4d_osa_concat_wgrad_tiles(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (long long)n * (((long long)h * w + gd4d::VA_PX - 1) / gd4d::VA_PX);
}

extern "C" size_t gd4d_conv_wgrad_workspace_bytes(int cin, int cout, int taps, int partitions) {
  using namespace gd4d;
  if (!vt_parts_ok(partitions)) return 0;
  if (!(taps == 9 ? vv_conv_channels(cin, cout) : taps == 1 ? vv_osa_channels(cin, cout) : false)) return 0;
  return (size_t)partitions * ((size_t)taps * cout * cin + cout) * sizeof(float);
}

namespace gd4d {
static int vt_finish(const float* ws, const float* ws_b, int partitions, int parts_b, int cin, int cout, int taps, const float* weight,
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
  if (!vv_conv_channels(cin, cout) || n <= 0 || h <= 0 || w <= 0 || !vt_parts_ok(partitions)) return GD4D_EUNSUPPORTED;
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
  p.tiles_x = (w + VW_T - 1) / VW_T;
  p.tiles_img = p.tiles_x * ((h + VW_T - 1) / VW_T);
  p.tiles = (int)tiles;
  p.partitions = partitions;
  p.chunks = cin / VW_KC;
  p.ws = workspace;
  p.ws_b = workspace + (size_t)partitions * 9 * cout * cin;
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(vt_conv3x3_wgrad_kernel), VW_LDS)) return GD4D_ELAUNCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vt_conv3x3_wgrad_kernel, dim3((unsigned)(p.chunks * partitions)), dim3(64 * (cout / 32)), VW_LDS, s, p);
  return vt_finish(p.ws, p.ws_b, partitions, partitions, cin, cout, 9, weight, bn, dw, dgamma, dbeta, s);
}

extern "C" int gd4d_osa_concat_wgrad(const float* dz, const float* dz_sums, const float* const* src, const int32_t* src_channels, int n_src,
                                     int n, int h, int w, int cout, int partitions, float* workspace, const float* weight, const float* bn,
                                     float* dw, float* dgamma, float* dbeta, void* stream) {
  using namespace gd4d;
  if (!dz || !dz_sums || !src || !src_channels || !workspace || !weight || !bn || (!dw && !dgamma && !dbeta)) return GD4D_EINVAL;
  if (n_src < 1 || n_src > VV_MAX_SRC || n <= 0 || h <= 0 || w <= 0 || !vt_parts_ok(partitions)) return GD4D_EUNSUPPORTED;
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
  p.chunks = (k + VA_IC - 1) / VA_IC;
  p.ws = workspace;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vt_osa_wgrad_kernel, dim3((unsigned)(p.chunks * partitions), (unsigned)((cout + VA_OC - 1) / VA_OC)), dim3(VA_THREADS), 0,
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
