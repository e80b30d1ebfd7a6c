// Training of the camera-aware DepthNet stage (gd4d_depth_net.hip holds the implicit GEMM and its epilogues).  Per level, with
//     y = conv3x3(x) + b,  xhat = (y - mu) rstd,  z = gamma xhat + beta,  out = relu(z) g[n, c]:
//
//   gd4d_depth_bn_stats      merges the GEMM's per-tile (mean, M2) partials per (level, channel) with Chan's update in a fixed order
//                            (32 slices of the tile list, then the slices in order), writes mu / rstd / scale = gamma rstd and moves
//                            the running buffers level after level (momentum, unbiased variance) - what L BatchNorm2d calls do.
//                            frozen: mu / rstd / scale from the running buffers, nothing is written back (mmdet's norm_eval).
//   gd4d_depth_bn_act_fwd    out from y, elementwise, in the inference epilogue's order of operations (frozen outputs are its bits).
//   gd4d_depth_bn_bwd        one pass over dout and y per (level, camera, channel) plane: sum dz, sum dz xhat, sum dout relu(z)
//                            (dz = dout g [z > 0]), each plane by one workgroup (strided partial sums, LDS tree: a fixed order);
//                            a one-workgroup kernel adds the planes in (level, camera) order into dbeta, dgamma, dg; a second pass
//                            writes dy = scale (dz - dbeta_l / M - xhat dgamma_l / M) (frozen: scale dz) and sums it per plane for
//                            the convolution bias gradient.
//   gd4d_depth_conv_wgrad    dW[oc, ic, ky, kx] = sum over levels, cameras, pixels of dy[oc, p] x[ic, p + (ky - 1, kx - 1)]: a GEMM
//                            256 x 2304 whose K runs over the pixels, on the split-bf16 x 3 MFMA (gd4d_bf16x3.h).
//
// The weight gradient is conv3x3_wgrad_body (gd4d_conv_wgrad.h has the algorithm) with everything fixed at compile time: 256 / 256
// channels, so a grid of 8 chunks x P and workgroups of 8 waves, over the (level, camera, 16 x 16 tile) list in the forward's order
// (DepthWgradShape finds a tile's level in the table); no bias sum (gd4d_depth_bn_bwd has it).  The FPN's 3x3 convolutions train
// through this entry point too.  depth_wgrad_sum_kernel adds the P partials of the (P, 9, 256, 256) workspace in order and writes the
// (256, 256, 3, 3) layout.
// Register / spill figures of the compiler's resource report: see docs/measurements_r16.md.
#include "gd4d_common.h"
#include "gd4d_conv_wgrad.h"

namespace gd4d {

constexpr int DT_C = 256, DT_T = 16, DT_MAX_LEVELS = 4;

struct DepthPlaneParams {
  const float* a[DT_MAX_LEVELS];   // dout (bn_act: unused)
  const float* y[DT_MAX_LEVELS];
  float* o[DT_MAX_LEVELS];         // out / dy
  int hw[DT_MAX_LEVELS];
  int levels, n;
  const float* stats;              // (levels, 3, 256): mu, rstd, scale
  const float *beta, *gate;
  float* part;                     // (levels * n, 4, 256): sum dz, sum dz xhat, sum dout relu(z), sum dy
  const float* sums;               // (levels, 2, 256): dbeta_l, dgamma_l
  int frozen;
};

// ---- statistics ---------------------------------------------------------------------------------------------------------
struct DepthStatsParams {
  const float* partials;           // (tiles, 2, 256)
  int h[DT_MAX_LEVELS], w[DT_MAX_LEVELS];
  int levels, n;
  const float* gamma;
  float *running_mean, *running_var;
  float* stats;
  float momentum, eps;
  int frozen;
};

constexpr int DT_ST_CH = 32, DT_ST_SL = 32;

__global__ __launch_bounds__(DT_ST_CH* DT_ST_SL) void depth_bn_stats_kernel(const DepthStatsParams p) {
  __shared__ float s_n[DT_ST_SL][DT_ST_CH], s_mean[DT_ST_SL][DT_ST_CH], s_m2[DT_ST_SL][DT_ST_CH];
  const int cl = threadIdx.x % DT_ST_CH, sl = threadIdx.x / DT_ST_CH;
  const int c = blockIdx.x * DT_ST_CH + cl;
  if (p.frozen) {
    if (sl == 0)
      for (int l = 0; l < p.levels; ++l) {
        const float var = p.running_var[c];
        float* st = p.stats + (size_t)l * 3 * DT_C;
        st[c] = p.running_mean[c];
        st[DT_C + c] = 1.f / sqrtf(var + p.eps);
        st[2 * DT_C + c] = p.gamma[c] / sqrtf(var + p.eps);       // the inference epilogue's scale, bit for bit
      }
    return;
  }
  float rm = 0.f, rv = 0.f;
  if (sl == 0) {
    rm = p.running_mean[c];
    rv = p.running_var[c];
  }
  long long tile0 = 0;
  for (int l = 0; l < p.levels; ++l) {
    const int H = p.h[l], W = p.w[l];
    const int tx = (W + DT_T - 1) / DT_T, ty = (H + DT_T - 1) / DT_T;
    const int per_cam = tx * ty, tiles = p.n * per_cam;
    float na = 0.f, ma = 0.f, m2a = 0.f;
    for (int i = sl; i < tiles; i += DT_ST_SL) {
      const int rt = i % per_cam;
      const int vh = min(DT_T, H - (rt / tx) * DT_T), vw = min(DT_T, W - (rt % tx) * DT_T);
      const float nb = (float)(vh * vw);
      const float* part = p.partials + (size_t)(tile0 + i) * 2 * DT_C;
      const float mb = part[c], m2b = part[DT_C + c];
      const float nn = na + nb, d = mb - ma;
      ma = ma + d * (nb / nn);
      m2a = m2a + m2b + d * d * (na * nb / nn);
      na = nn;
    }
    s_n[sl][cl] = na;
    s_mean[sl][cl] = ma;
    s_m2[sl][cl] = m2a;
    __syncthreads();
    if (sl == 0) {
      for (int s = 1; s < DT_ST_SL; ++s) {
        const float nb = s_n[s][cl];
        if (nb == 0.f) continue;
        const float mb = s_mean[s][cl], m2b = s_m2[s][cl];
        const float nn = na + nb, d = mb - ma;
        ma = ma + d * (nb / nn);
        m2a = m2a + m2b + d * d * (na * nb / nn);
        na = nn;
      }
      const float var = m2a / na;
      const float rstd = 1.f / sqrtf(var + p.eps);
      float* st = p.stats + (size_t)l * 3 * DT_C;
      st[c] = ma;
      st[DT_C + c] = rstd;
      st[2 * DT_C + c] = p.gamma[c] * rstd;
      rm = (1.f - p.momentum) * rm + p.momentum * ma;
      rv = (1.f - p.momentum) * rv + p.momentum * (m2a / (na - 1.f));
    }
    __syncthreads();
    tile0 += tiles;
  }
  if (sl == 0) {
    p.running_mean[c] = rm;
    p.running_var[c] = rv;
  }
}

// ---- plane kernels: one workgroup per (level, camera, channel) plane ---------------------------------------------------------------
struct PlaneAt {
  int lv, cam, c, hw;
  size_t base;
  int row;                         // level * n + camera
};

__device__ __forceinline__ PlaneAt plane_at(const DepthPlaneParams& p) {
  PlaneAt a;
  const int per_level = p.n * DT_C;
  a.lv = blockIdx.x / per_level;
  const int r = blockIdx.x - a.lv * per_level;
  a.cam = r / DT_C;
  a.c = r - a.cam * DT_C;
  a.hw = p.hw[0];
#pragma unroll
  for (int l = 1; l < DT_MAX_LEVELS; ++l)
    if (a.lv == l) a.hw = p.hw[l];
  a.base = (size_t)r * a.hw;
  a.row = a.lv * p.n + a.cam;
  return a;
}

template <typename T>
__device__ __forceinline__ T pick(T const (&v)[DT_MAX_LEVELS], int lv) {
  T r = v[0];
#pragma unroll
  for (int l = 1; l < DT_MAX_LEVELS; ++l)
    if (lv == l) r = v[l];
  return r;
}

__global__ __launch_bounds__(256) void depth_bn_act_kernel(const DepthPlaneParams p) {
  const PlaneAt a = plane_at(p);
  const float* st = p.stats + (size_t)a.lv * 3 * DT_C;
  const float mean = st[a.c], scale = st[2 * DT_C + a.c], beta = p.beta[a.c], g = p.gate[a.cam * DT_C + a.c];
  const float* y = pick(p.y, a.lv) + a.base;
  float* o = pick(p.o, a.lv) + a.base;
  for (int i = threadIdx.x; i < a.hw; i += 256) {
    float v = (y[i] - mean) * scale + beta;
    v = fmaxf(v, 0.f);
    o[i] = v * g;
  }
}

__global__ __launch_bounds__(256) void depth_bn_bwd_reduce_kernel(const DepthPlaneParams p) {
  __shared__ float red[256];
  const PlaneAt a = plane_at(p);
  const float* st = p.stats + (size_t)a.lv * 3 * DT_C;
  const float mean = st[a.c], rstd = st[DT_C + a.c], scale = st[2 * DT_C + a.c], beta = p.beta[a.c], g = p.gate[a.cam * DT_C + a.c];
  const float* y = pick(p.y, a.lv) + a.base;
  const float* d = pick(p.a, a.lv) + a.base;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < a.hw; i += 256) {
    const float yc = y[i] - mean;
    const float z = yc * scale + beta;
    if (z > 0.f) {                                           // strict, as torch's ReLU
      const float dz = d[i] * g;
      s0 += dz;
      s1 += dz * (yc * rstd);
      s2 += d[i] * z;
    }
  }
  s0 = block_sum_256(s0, red);
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  if (threadIdx.x == 0) {
    float* part = p.part + (size_t)a.row * 4 * DT_C;
    part[a.c] = s0;
    part[DT_C + a.c] = s1;
    part[2 * DT_C + a.c] = s2;
  }
}

// the planes' sums in (level, camera) order: sums (levels, 2, 256) = dbeta_l, dgamma_l; dbeta, dgamma over the levels; dg (n, 256)
__global__ __launch_bounds__(DT_C) void depth_bn_bwd_sums_kernel(const float* __restrict__ part, int levels, int n, float* __restrict__ sums,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                 float* __restrict__ dg) {
  const int c = threadIdx.x;
  float tb = 0.f, tg = 0.f;
  for (int l = 0; l < levels; ++l) {
    float sb = 0.f, sg = 0.f;
    for (int cam = 0; cam < n; ++cam) {
      const float* q = part + (size_t)(l * n + cam) * 4 * DT_C;
      sb += q[c];
      sg += q[DT_C + c];
    }
    sums[(size_t)l * 2 * DT_C + c] = sb;
    sums[(size_t)l * 2 * DT_C + DT_C + c] = sg;
    tb += sb;
    tg += sg;
  }
  dbeta[c] = tb;
  dgamma[c] = tg;
  for (int cam = 0; cam < n; ++cam) {
    float s = 0.f;
    for (int l = 0; l < levels; ++l) s += part[(size_t)(l * n + cam) * 4 * DT_C + 2 * DT_C + c];
    dg[cam * DT_C + c] = s;
  }
}

__global__ __launch_bounds__(256) void depth_bn_bwd_dy_kernel(const DepthPlaneParams p) {
  __shared__ float red[256];
  const PlaneAt a = plane_at(p);
  const float* st = p.stats + (size_t)a.lv * 3 * DT_C;
  const float mean = st[a.c], rstd = st[DT_C + a.c], scale = st[2 * DT_C + a.c], beta = p.beta[a.c], g = p.gate[a.cam * DT_C + a.c];
  const float inv_m = 1.f / ((float)p.n * (float)a.hw);
  const float mb = p.frozen ? 0.f : p.sums[(size_t)a.lv * 2 * DT_C + a.c] * inv_m;
  const float mg = p.frozen ? 0.f : p.sums[(size_t)a.lv * 2 * DT_C + DT_C + a.c] * inv_m;
  const float* y = pick(p.y, a.lv) + a.base;
  const float* d = pick(p.a, a.lv) + a.base;
  float* o = pick(p.o, a.lv) + a.base;
  float s = 0.f;
  for (int i = threadIdx.x; i < a.hw; i += 256) {
    const float yc = y[i] - mean;
    const float z = yc * scale + beta;
    const float dz = z > 0.f ? d[i] * g : 0.f;
    const float v = scale * (dz - mb - (yc * rstd) * mg);
    o[i] = v;
    s += v;
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) p.part[(size_t)a.row * 4 * DT_C + 3 * DT_C + a.c] = s;
}

__global__ __launch_bounds__(DT_C) void depth_bn_bwd_bias_kernel(const float* __restrict__ part, int rows, float* __restrict__ db) {
  const int c = threadIdx.x;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += part[(size_t)r * 4 * DT_C + 3 * DT_C + c];
  db[c] = s;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------
constexpr int WG_THREADS = 512, WG_CHUNKS = DT_C / CW3_KC;
constexpr int WG_DW = DT_C * DT_C * 9;

struct DepthWgradParams {
  const float* dy[DT_MAX_LEVELS];
  const float* x[DT_MAX_LEVELS];
  int h[DT_MAX_LEVELS], w[DT_MAX_LEVELS], tiles_x[DT_MAX_LEVELS], tiles_cam[DT_MAX_LEVELS], start[DT_MAX_LEVELS];
  int levels, tiles, partitions;
  float* ws;                       // (partitions, 9, 256, 256)
};

// conv3x3_wgrad_body's policy: everything fixed at compile time, a tile looked up in the level table
struct DepthWgradShape {
  const DepthWgradParams& p;
  static constexpr int cin() { return DT_C; }
  static constexpr int cout() { return DT_C; }
  static constexpr int chunks() { return WG_CHUNKS; }
  static constexpr int threads() { return WG_THREADS; }
  __device__ __forceinline__ Conv3x3Tile tile(int t, int chunk, int oc_a) const {
    int lv = 0;
#pragma unroll
    for (int l = 1; l < DT_MAX_LEVELS; ++l)
      if (l < p.levels && t >= p.start[l]) lv = l;
    const int H = pick(p.h, lv), W = pick(p.w, lv), tpc = pick(p.tiles_cam, lv), tpx = pick(p.tiles_x, lv);
    const size_t HW = (size_t)H * W;
    const int local = t - pick(p.start, lv);
    const int cam = local / tpc;
    const int rt = local - cam * tpc;
    return {H, W, (rt / tpx) * DT_T, (rt % tpx) * DT_T, pick(p.x, lv) + ((size_t)cam * DT_C + chunk * CW3_KC) * HW,
            pick(p.dy, lv) + ((size_t)cam * DT_C + oc_a) * HW};
  }
};

__global__ __launch_bounds__(WG_THREADS) void depth_wgrad_kernel(const DepthWgradParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv3x3_wgrad_body<DepthWgradShape, false>(DepthWgradShape{p}, smem);
}

// dW (256, 256, 3, 3) = the partitions' partials added in order
__global__ __launch_bounds__(256) void depth_wgrad_sum_kernel(const float* __restrict__ ws, int partitions, float* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x;              // (tap, oc, ic)
  if (i >= WG_DW) return;
  float s = 0.f;
  for (int q = 0; q < partitions; ++q) s += ws[(size_t)q * WG_DW + i];
  const int tap = i / (DT_C * DT_C), oc = (i / DT_C) % DT_C, ic = i % DT_C;
  dw[((size_t)oc * DT_C + ic) * 9 + tap] = s;
}

static bool plane_levels(DepthPlaneParams& p, const int32_t* level_hw, int levels, int n, long long& planes) {
  planes = 0;
  for (int l = 0; l < levels; ++l) {
    const long long hw = (long long)level_hw[2 * l] * level_hw[2 * l + 1];
    if (level_hw[2 * l] <= 0 || level_hw[2 * l + 1] <= 0 || hw > (1ll << 30)) return false;
    p.hw[l] = (int)hw;
    planes += (long long)n * DT_C;
  }
  p.levels = levels;
  p.n = n;
  return planes <= (1ll << 30);
}

}  // namespace gd4d

extern "C" int gd4d_depth_bn_stats(const float* partials, const int32_t* level_hw, int levels, int n, int channels, const float* bn_weight,
                                   float* running_mean, float* running_var, float momentum, float eps, int frozen, float* stats,
                                   void* stream) {
  using namespace gd4d;
  if (!level_hw || !bn_weight || !running_mean || !running_var || !stats || (!frozen && !partials)) return GD4D_EINVAL;
  if (channels != DT_C || levels < 1 || levels > DT_MAX_LEVELS || n <= 0) return GD4D_EUNSUPPORTED;
  DepthStatsParams p{};
  for (int l = 0; l < levels; ++l) {
    p.h[l] = level_hw[2 * l];
    p.w[l] = level_hw[2 * l + 1];
    if (p.h[l] <= 0 || p.w[l] <= 0) return GD4D_EINVAL;
    if (!frozen && (long long)n * p.h[l] * p.w[l] < 2) return GD4D_EUNSUPPORTED;     // (the unbiased variance of one value)
  }
  p.partials = partials;
  p.levels = levels;
  p.n = n;
  p.gamma = bn_weight;
  p.running_mean = running_mean;
  p.running_var = running_var;
  p.stats = stats;
  p.momentum = momentum;
  p.eps = eps;
  p.frozen = frozen ? 1 : 0;
  hipLaunchKernelGGL(depth_bn_stats_kernel, dim3(DT_C / DT_ST_CH), dim3(DT_ST_CH * DT_ST_SL), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_depth_bn_act_fwd(const float* const* y, float* const* out, const int32_t* level_hw, int levels, int n, int channels,
                                     const float* stats, const float* bn_bias, const float* gate, void* stream) {
  using namespace gd4d;
  if (!y || !out || !level_hw || !stats || !bn_bias || !gate) return GD4D_EINVAL;
  if (channels != DT_C || levels < 1 || levels > DT_MAX_LEVELS || n <= 0) return GD4D_EUNSUPPORTED;
  DepthPlaneParams p{};
  long long planes = 0;
  if (!plane_levels(p, level_hw, levels, n, planes)) return GD4D_EINVAL;
  for (int l = 0; l < levels; ++l) {
    if (!y[l] || !out[l]) return GD4D_EINVAL;
    p.y[l] = y[l];
    p.o[l] = out[l];
  }
  p.stats = stats;
  p.beta = bn_bias;
  p.gate = gate;
  hipLaunchKernelGGL(depth_bn_act_kernel, dim3((unsigned)planes), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" size_t gd4d_depth_bn_bwd_workspace_bytes(int levels, int n) {
  if (levels < 1 || levels > gd4d::DT_MAX_LEVELS || n <= 0) return 0;
  return ((size_t)levels * n * 4 + (size_t)levels * 2) * gd4d::DT_C * sizeof(float);
}

extern "C" int gd4d_depth_bn_bwd(const float* const* dout, const float* const* y, float* const* dy, const int32_t* level_hw, int levels, int n,
                                 int channels, const float* stats, const float* bn_bias, const float* gate, int frozen, float* workspace,
                                 float* dgamma, float* dbeta, float* dgate, float* dbias, void* stream) {
  using namespace gd4d;
  if (!dout || !y || !dy || !level_hw || !stats || !bn_bias || !gate || !workspace || !dgamma || !dbeta || !dgate || !dbias)
    return GD4D_EINVAL;
  if (channels != DT_C || levels < 1 || levels > DT_MAX_LEVELS || n <= 0) return GD4D_EUNSUPPORTED;
  DepthPlaneParams p{};
  long long planes = 0;
  if (!plane_levels(p, level_hw, levels, n, planes)) return GD4D_EINVAL;
  for (int l = 0; l < levels; ++l) {
    if (!dout[l] || !y[l] || !dy[l]) return GD4D_EINVAL;
    p.a[l] = dout[l];
    p.y[l] = y[l];
    p.o[l] = dy[l];
  }
  float* const sums = workspace + (size_t)levels * n * 4 * DT_C;
  p.stats = stats;
  p.beta = bn_bias;
  p.gate = gate;
  p.part = workspace;
  p.sums = sums;
  p.frozen = frozen ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(depth_bn_bwd_reduce_kernel, dim3((unsigned)planes), dim3(256), 0, s, p);
  hipLaunchKernelGGL(depth_bn_bwd_sums_kernel, dim3(1), dim3(DT_C), 0, s, workspace, levels, n, sums, dgamma, dbeta, dgate);
  hipLaunchKernelGGL(depth_bn_bwd_dy_kernel, dim3((unsigned)planes), dim3(256), 0, s, p);
  hipLaunchKernelGGL(depth_bn_bwd_bias_kernel, dim3(1), dim3(DT_C), 0, s, workspace, levels * n, dbias);
  return check_launch();
}

extern "C" size_t gd4d_depth_conv_wgrad_workspace_bytes(int partitions) {
  return partitions < 1 ? 0 : (size_t)partitions * gd4d::WG_DW * sizeof(float);
}

extern "C" int gd4d_depth_conv_wgrad(const float* const* dy, const float* const* x, const int32_t* level_hw, int levels, int n, int channels,
                                     int partitions, float* workspace, float* dw, void* stream) {
  using namespace gd4d;
  if (!dy || !x || !level_hw || !workspace || !dw) return GD4D_EINVAL;
  if (channels != DT_C || levels < 1 || levels > DT_MAX_LEVELS || n <= 0 || !partitions_ok(partitions)) return GD4D_EUNSUPPORTED;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  DepthWgradParams p{};
  long long tiles = 0;
  for (int l = 0; l < levels; ++l) {
    const int h = level_hw[2 * l], w = level_hw[2 * l + 1];
    if (!dy[l] || !x[l] || h <= 0 || w <= 0) return GD4D_EINVAL;
    if ((long long)n * DT_C * h * w > (1ll << 40)) return GD4D_EUNSUPPORTED;
    p.dy[l] = dy[l];
    p.x[l] = x[l];
    p.h[l] = h;
    p.w[l] = w;
    p.tiles_x[l] = (w + DT_T - 1) / DT_T;
    p.tiles_cam[l] = p.tiles_x[l] * ((h + DT_T - 1) / DT_T);
    p.start[l] = (int)tiles;
    tiles += (long long)n * p.tiles_cam[l];
    if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  }
  p.levels = levels;
  p.tiles = (int)tiles;
  p.partitions = partitions;
  p.ws = workspace;
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(depth_wgrad_kernel), CW3_LDS)) return GD4D_ELAUNCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(depth_wgrad_kernel, dim3((unsigned)(WG_CHUNKS * partitions)), dim3(WG_THREADS), CW3_LDS, s, p);
  hipLaunchKernelGGL(depth_wgrad_sum_kernel, dim3((WG_DW + 255) / 256), dim3(256), 0, s, workspace, partitions, dw);
  return check_launch();
}
