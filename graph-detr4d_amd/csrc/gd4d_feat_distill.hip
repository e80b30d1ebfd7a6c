// MixDistill's pyramid feature-distillation loss (distillation/distillers/mix_distill.py:51-55, 118-138) on the device: per level the
// student's map goes through a 1x1 convolution 256 -> 256 with bias and is compared to the teacher's, plainly ('vanilla': mse_loss) or
// weighted by two attention maps taken from the TEACHER ('attention', :131-137).  The converted student map is never written:
//
//   fd_fused_kernel          one workgroup per (camera, 64 pixels) of a level, on the NCHW tensors as they arrive (a camera's level is a
//                            256 x HW matrix, pixels contiguous).  The X tile is loaded once and split into bf16 hi / lo pieces in LDS;
//                            S = W X + b on the split-bf16 MFMAs (gd4d_bf16x3.h) with the weight's fragments read from a fragment-ordered
//                            image; S meets the teacher's tile in the accumulator registers: the tile's loss goes to a per-workgroup
//                            partial, G = dloss/dS = 2 coef (a_c a_s) (S - t) replaces S in the registers, is written once (the weight
//                            gradient's operand) and - split again, through LDS - is the B operand of dX = W^T G, written by the same
//                            launch.  An accumulator tile has its pixel on the lane and its channels in the registers, so registers
//                            8s .. 8s+7 ARE the fragment of k-step s of the second product, in a permuted channel order; the W^T image
//                            is stored in that same order (element j of lane half h of step s: channel 16s + 8(j>>2) + 4h + (j&3)).
//   fd_wgrad_kernel          dW = sum_{camera, pixel} G X^T and db = sum G for one level: 128 x 128 output tiles x `splits` ranges of
//                            32-pixel chunks, each workgroup's partial to the workspace; fd_wgrad_reduce_kernel adds the partials in
//                            index order.
//   fd_stats_*               the attention maps: ONE pass over the teacher gives every pixel's and every channel's sum of |t| (channel
//                            sums as per-workgroup partials, added in index order), a second small kernel the two softmaxes (with the
//                            maximum subtracted): a_c (R, HW) = 256 softmax_p(mean_c |t| / T), a_s (R, 256) = HW softmax_c(mean_p |t| / T).
//   fd_loss_reduce_kernel    every level's per-workgroup partials, already scaled by loss_weight / (levels R 256 HW_l), to ONE scalar.
//
// No floating-point atomics: every sum has a fixed order, two runs give the same bits.  No allocation, no synchronisation: everything
// lives in the caller's workspace, every launch goes to the caller's stream (the term can be captured in a graph).
#include "gd4d_bf16x3.h"
#include "gd4d_common.h"

namespace gd4d {

constexpr int FD_C = 256;                            // channels in and out: nn.Conv2d(256, 256, 1) (:55)
constexpr int FD_PX = 64;                            // pixels per workgroup of the fused kernel
constexpr int FD_PITCH = 33;                         // 16-byte units per pixel of the LDS operand image: 32 k-units + 1 (bank spread)
constexpr int FD_PLANE = FD_C * FD_C / 8;            // 16-byte units of one bf16 plane of a weight
constexpr size_t FD_IMAGE_BYTES = 4 * (size_t)FD_PLANE * 16;      // W hi, W lo, W^T hi, W^T lo
constexpr int FD_FUSED_LDS = 2 * FD_PX * FD_PITCH * 16;
constexpr int FD_SC = 256;                           // pixels per workgroup of the statistics pass
constexpr int FD_WT = 128;                           // output tile of the weight gradient (FD_WT x FD_WT)
constexpr int FD_WK = 32;                            // pixels per k-chunk of the weight gradient
constexpr int FD_WPITCH = 36;                        // floats per LDS row of a chunk (16-byte aligned rows, banks spread)
constexpr int FD_MAX_SPLITS = 128;
constexpr int FD_MAX_LEVELS = 8;

// row of a 32x32 accumulator tile held in register i of lane half h
__device__ __forceinline__ int fd_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

__device__ __forceinline__ float fd_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// weight (levels, 256, 256) fp32 -> per level four planes of MFMA A fragments, 16 bytes per (32-row block mb, k-step, lane):
//   planes 0 / 1 (hi / lo)  S = W X:     rows = output channels, k = input channels in natural order;
//   planes 2 / 3            dX = W^T G:  rows = input channels, k = output channels in the accumulator's order (see the header).
__global__ __launch_bounds__(256) void fd_weight_image_kernel(const float* __restrict__ w, u32x4* __restrict__ image) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int which = idx / FD_PLANE, u = idx - which * FD_PLANE;
  const int lane = u & 63, step = (u >> 6) & 15, mb = u >> 10, r = lane & 31, h = lane >> 5;
  const float* W = w + (size_t)blockIdx.y * FD_C * FD_C;
  float v[8];
  if (which == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W[(32 * mb + r) * FD_C + 16 * step + 8 * h + j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W[(16 * step + 8 * (j >> 2) + 4 * h + (j & 3)) * FD_C + 32 * mb + r];
  }
  u32x4 hi, lo;
  split8(v, hi, lo);
  u32x4* img = image + (size_t)blockIdx.y * 4 * FD_PLANE;
  img[(2 * which) * FD_PLANE + u] = hi;
  img[(2 * which + 1) * FD_PLANE + u] = lo;
}

// ---------------------------------------------------------------------------------------------------------------------------
struct FdFusedParams {
  const float* x;        // (R, 256, HW) student level
  const float* t;        // (R, 256, HW) teacher level
  const float* a_c;      // (R, HW)   attention only
  const float* a_s;      // (R, 256)  attention only
  const float* bias;     // (256)
  const u32x4* image;    // this level's weight image
  float* g;              // (R, 256, HW) dloss/dS
  float* dx;             // (R, 256, HW) dloss/dX
  float* partial;        // (R * tiles) loss partials, scaled
  int HW, tiles;
  float gcoef, lcoef;    // 2 coef and coef = loss_weight / (levels R 256 HW)
};

// the 16 k-steps of a 256-deep product for this wave's 2 x 2 tiles: A fragments from the image planes, B fragments from LDS
__device__ __forceinline__ void fd_product(const u32x4* __restrict__ ah_plane, const u32x4* __restrict__ al_plane, const u32x4* s_hi,
                                           const u32x4* s_lo, int wave, int lane, f32x16 (&acc)[2][2]) {
  const int n = lane & 31, h = lane >> 5;
#pragma unroll 2
  for (int kk = 0; kk < 16; ++kk) {
    u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int u = ((2 * wave + mi) * 16 + kk) * 64 + lane;
      ah[mi] = ah_plane[u];
      al[mi] = al_plane[u];
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int u = (32 * ni + n) * FD_PITCH + 2 * kk + h;
      bh[ni] = s_hi[u];
      bl[ni] = s_lo[u];
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma_32x32x16_x3(ah[mi], al[mi], bh[ni], bl[ni], acc[mi][ni]);
  }
}

// 4 waves; wave w owns channel blocks 2w, 2w + 1 (32 channels each) x both 32-pixel blocks of the tile, in both products.
template <bool ATT>
__global__ __launch_bounds__(256) void fd_fused_kernel(const FdFusedParams p) {
  extern __shared__ __attribute__((aligned(16))) char fd_smem[];
  __shared__ float s_red[4];
  u32x4* s_hi = reinterpret_cast<u32x4*>(fd_smem);
  u32x4* s_lo = s_hi + FD_PX * FD_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
  const int HW = p.HW;
  const int r = blockIdx.x / p.tiles, p0 = (blockIdx.x - r * p.tiles) * FD_PX;
  const size_t cam = (size_t)r * FD_C * HW;
  // the X tile, once: thread = (pixel, group of 8 input channels), split into the B fragments of the first product (pixels past the
  // level's end are zeros)
  {
    const int px = p0 + lane;
    const bool ok = px < HW;
#pragma unroll 2
    for (int i = 0; i < 8; ++i) {
      const int cb = wave + 4 * i;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ok ? p.x[cam + (size_t)(8 * cb + j) * HW + px] : 0.f;
      u32x4 hi, lo;
      split8(v, hi, lo);
      s_hi[lane * FD_PITCH + cb] = hi;
      s_lo[lane * FD_PITCH + cb] = lo;
    }
  }
  __syncthreads();
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float b = p.bias[32 * (2 * wave + mi) + fd_row(i, h)];
      acc[mi][0][i] = b;
      acc[mi][1][i] = b;
    }
  fd_product(p.image, p.image + FD_PLANE, s_hi, s_lo, wave, lane, acc);
  // S against the teacher's tile, in the registers: loss and G
  float lsum = 0.f;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int px = p0 + 32 * ni + n;
      const bool ok = px < HW;
      float ac = 1.0f;
      if (ATT && ok) ac = p.a_c[(size_t)r * HW + px];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = 32 * (2 * wave + mi) + fd_row(i, h);
        float g = 0.f;
        if (ok) {
          const size_t e = cam + (size_t)co * HW + px;
          const float d = acc[mi][ni][i] - p.t[e];
          const float wgt = ATT ? ac * p.a_s[r * FD_C + co] : 1.0f;
          lsum += wgt * d * d;
          g = p.gcoef * wgt * d;
          p.g[e] = g;
        }
        acc[mi][ni][i] = g;
      }
    }
  lsum = wave_sum(lsum);                              // block_sum_put, with the lane / wave indices this kernel already holds
  if (lane == 0) s_red[wave] = lsum;
  __syncthreads();                                    // (also: every wave is done reading the X fragments)
  if (tid == 0) p.partial[blockIdx.x] = block_sum_get<4>(s_red) * p.lcoef;
  // G -> the B fragments of the second product: registers 8s .. 8s+7 of channel block b are k-step 2b + s
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = acc[mi][ni][8 * s + j];
        u32x4 hi, lo;
        split8(v, hi, lo);
        const int u = (32 * ni + n) * FD_PITCH + 2 * (2 * (2 * wave + mi) + s) + h;
        s_hi[u] = hi;
        s_lo[u] = lo;
      }
  __syncthreads();
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;
  fd_product(p.image + 2 * FD_PLANE, p.image + 3 * FD_PLANE, s_hi, s_lo, wave, lane, acc);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int px = p0 + 32 * ni + n;
      if (px >= HW) continue;
#pragma unroll
      for (int i = 0; i < 16; ++i) p.dx[cam + (size_t)(32 * (2 * wave + mi) + fd_row(i, h)) * HW + px] = acc[mi][ni][i];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
struct FdWgradParams {
  const float* g;        // (R, 256, HW)
  const float* x;        // (R, 256, HW)
  float* part;           // (splits, 256, 256)
  float* partb;          // (splits, 256)
  int HW, chunks, splits;
  long long units;       // R * chunks
};

// blockIdx.x = split (a range of (camera, 32-pixel chunk) units), blockIdx.y = output tile (co tile, ci tile).  4 waves, 64 x 64 each.
// A = G[co][pixel], B = X[ci][pixel]: both k-contiguous, staged as fp32 in LDS and split when the fragments are read.
__global__ __launch_bounds__(256) void fd_wgrad_kernel(const FdWgradParams p) {
  __shared__ __attribute__((aligned(16))) float s_g[FD_WT * FD_WPITCH];
  __shared__ __attribute__((aligned(16))) float s_x[FD_WT * FD_WPITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int split = blockIdx.x, co0 = (blockIdx.y >> 1) * FD_WT, ci0 = (blockIdx.y & 1) * FD_WT;
  const int HW = p.HW;
  const long long u0 = p.units * split / p.splits, u1 = p.units * (split + 1) / p.splits;
  const int lrow = tid >> 3, lpx = (tid & 7) * 4;
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  for (long long u = u0; u < u1; ++u) {
    const int r = (int)(u / p.chunks), p0 = (int)(u - (long long)r * p.chunks) * FD_WK;
    __syncthreads();                                  // the previous chunk's fragments are read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = lrow + 32 * i;
      const size_t gro = ((size_t)r * FD_C + co0 + row) * HW, xro = ((size_t)r * FD_C + ci0 + row) * HW;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int px = p0 + lpx + j;
        const bool ok = px < HW;
        const float gv = ok ? p.g[gro + px] : 0.f, xv = ok ? p.x[xro + px] : 0.f;
        s_g[row * FD_WPITCH + lpx + j] = gv;
        s_x[row * FD_WPITCH + lpx + j] = xv;
        bsum[i] += gv;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < FD_WK / 16; ++kk) {
      u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) split8(s_g + (64 * wm + 32 * mi + n) * FD_WPITCH + 16 * kk + 8 * h, ah[mi], al[mi]);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) split8(s_x + (64 * wn + 32 * ni + n) * FD_WPITCH + 16 * kk + 8 * h, bh[ni], bl[ni]);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma_32x32x16_x3(ah[mi], al[mi], bh[ni], bl[ni], acc[mi][ni]);
    }
  }
  float* out = p.part + (size_t)split * FD_C * FD_C;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        out[(co0 + 64 * wm + 32 * mi + fd_row(i, h)) * FD_C + ci0 + 64 * wn + 32 * ni + n] = acc[mi][ni][i];
  if ((blockIdx.y & 1) == 0) {                        // the bias gradient: rows of G, summed by the workgroups of ci tile 0
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      if ((tid & 7) == 0) p.partb[(size_t)split * FD_C + co0 + lrow + 32 * i] = v;
    }
  }
}

__global__ __launch_bounds__(256) void fd_wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ partb,
                                                              float* __restrict__ dw, float* __restrict__ db, int splits) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  float s = 0.f;
  if (e < FD_C * FD_C) {
    for (int k = 0; k < splits; ++k) s += part[(size_t)k * FD_C * FD_C + e];
    dw[e] = s;
  } else if (e < FD_C * FD_C + FD_C) {
    const int c = e - FD_C * FD_C;
    for (int k = 0; k < splits; ++k) s += partb[(size_t)k * FD_C + c];
    db[c] = s;
  }
}

__global__ __launch_bounds__(1024) void fd_loss_reduce_kernel(const float* __restrict__ partial, long long count, float* __restrict__ loss) {
  __shared__ float s_red[16];
  float s = 0.f;
  for (long long i = threadIdx.x; i < count; i += 1024) s += partial[i];
  // (a thread's s starts from +0, and x + y is -0 only for two -0: no wave holds -0, the sum needs no 0 in front)
  block_sum_put(s, s_red);
  __syncthreads();
  if (threadIdx.x == 0) *loss = block_sum_get<16>(s_red);
}

// ---------------------------------------------------------------------------------------------------------------------------
// One pass over the teacher: workgroup = (camera, 256 pixels), wave w takes channels w, w + 4, ...; each lane 4 pixels.
__global__ __launch_bounds__(256) void fd_stats_sums_kernel(const float* __restrict__ t, float* __restrict__ colsum,
                                                            float* __restrict__ rowpart, int HW, int chunks) {
  __shared__ float s_col[4][FD_SC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x / chunks, p0 = (blockIdx.x - r * chunks) * FD_SC;
  float col[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < FD_C / 4; ++k) {
    const int c = wave + 4 * k;
    const float* row = t + ((size_t)r * FD_C + c) * HW;
    float rs = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int px = p0 + lane + 64 * q;
      const float v = px < HW ? fabsf(row[px]) : 0.f;
      col[q] += v;
      rs += v;
    }
    rs = wave_sum(rs);
    if (lane == 0) rowpart[(size_t)blockIdx.x * FD_C + c] = rs;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s_col[wave][lane + 64 * q] = col[q];
  __syncthreads();
  const int px = p0 + tid;
  if (px < HW) colsum[(size_t)r * HW + px] = ((s_col[0][tid] + s_col[1][tid]) + s_col[2][tid]) + s_col[3][tid];
}

// the maximum or the sum (block_sum, gd4d_common.h) over the workgroup's 256 threads, in every thread
__device__ __forceinline__ float fd_block_reduce(float v, bool is_max, float* s_tmp) {
  __syncthreads();                                    // s_tmp's previous readers (block_sum does not end with a barrier)
  if (!is_max) return block_sum<4>(v, s_tmp);
  v = fd_wave_max(v);
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_tmp[0], s_tmp[1]), fmaxf(s_tmp[2], s_tmp[3]));
}

// One workgroup per camera: a_s = HW softmax_c(mean_p |t| / T) from the channel partials, a_c = 256 softmax_p(mean_c |t| / T) in place
// over the pixel sums.
__global__ __launch_bounds__(256) void fd_stats_softmax_kernel(float* __restrict__ a_c, float* __restrict__ a_s,
                                                               const float* __restrict__ rowpart, int HW, int chunks, float temperature) {
  __shared__ float s_tmp[4];
  const int tid = threadIdx.x, r = blockIdx.x;
  float s = 0.f;
  for (int ch = 0; ch < chunks; ++ch) s += rowpart[((size_t)r * chunks + ch) * FD_C + tid];
  const float x = (s / (float)HW) / temperature;
  const float m = fd_block_reduce(x, true, s_tmp);
  const float e = expf(x - m);
  const float z = fd_block_reduce(e, false, s_tmp);
  a_s[(size_t)r * FD_C + tid] = (float)HW * (e / z);
  float* ac = a_c + (size_t)r * HW;
  float pm = -INFINITY;
  for (int px = tid; px < HW; px += 256) pm = fmaxf(pm, (ac[px] / (float)FD_C) / temperature);
  pm = fd_block_reduce(pm, true, s_tmp);
  float pz = 0.f;
  for (int px = tid; px < HW; px += 256) pz += expf((ac[px] / (float)FD_C) / temperature - pm);
  pz = fd_block_reduce(pz, false, s_tmp);
  for (int px = tid; px < HW; px += 256) ac[px] = (float)FD_C * (expf((ac[px] / (float)FD_C) / temperature - pm) / pz);
}

// ---------------------------------------------------------------------------------------------------------------------------
static inline size_t fd_up(size_t b) { return (b + 255) & ~(size_t)255; }

// 0: fine
static int fd_check_levels(const int32_t* level_hw, int levels, int R, int C) {
  if (!level_hw || levels <= 0 || R <= 0) return GD4D_EINVAL;
  if (C != FD_C || levels > FD_MAX_LEVELS) return GD4D_EUNSUPPORTED;
  for (int l = 0; l < levels; ++l) {
    if (level_hw[2 * l] <= 0 || level_hw[2 * l + 1] <= 0) return GD4D_EINVAL;
    if ((long long)R * level_hw[2 * l] * level_hw[2 * l + 1] >= (1ll << 31)) return GD4D_EUNSUPPORTED;
  }
  return GD4D_OK;
}

struct FdLayout {
  size_t partial, image, wpart, wpartb, g, total;
  long long npartial;
};

static FdLayout fd_layout(const int32_t* level_hw, int levels, int R) {
  FdLayout w{};
  long long max_hw = 0;
  for (int l = 0; l < levels; ++l) {
    const long long hw = (long long)level_hw[2 * l] * level_hw[2 * l + 1];
    w.npartial += (long long)R * ((hw + FD_PX - 1) / FD_PX);
    if (hw > max_hw) max_hw = hw;
  }
  size_t off = 0;
  w.partial = off; off += fd_up((size_t)w.npartial * sizeof(float));
  w.image = off;   off += fd_up((size_t)levels * FD_IMAGE_BYTES);
  w.wpart = off;   off += fd_up((size_t)FD_MAX_SPLITS * FD_C * FD_C * sizeof(float));
  w.wpartb = off;  off += fd_up((size_t)FD_MAX_SPLITS * FD_C * sizeof(float));
  w.g = off;       off += fd_up((size_t)R * FD_C * (size_t)max_hw * sizeof(float));
  w.total = off;
  return w;
}

}  // namespace gd4d

extern "C" size_t gd4d_feat_distill_stats_workspace_bytes(const int32_t* level_hw, int levels, int R) {
  using namespace gd4d;
  if (fd_check_levels(level_hw, levels, R, FD_C) != GD4D_OK) return 0;
  size_t most = 0;
  for (int l = 0; l < levels; ++l) {
    const long long hw = (long long)level_hw[2 * l] * level_hw[2 * l + 1];
    const size_t b = (size_t)R * (size_t)((hw + FD_SC - 1) / FD_SC) * FD_C * sizeof(float);
    if (b > most) most = b;
  }
  return fd_up(most);
}

extern "C" int gd4d_feat_distill_stats_fwd(const float* const* teacher, const int32_t* level_hw, int levels, int R, int C,
                                           float temperature, float* const* a_c, float* const* a_s, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  using namespace gd4d;
  if (!teacher || !a_c || !a_s || !workspace) return GD4D_EINVAL;
  const int bad = fd_check_levels(level_hw, levels, R, C);
  if (bad != GD4D_OK) return bad;
  if (!(temperature > 0.f)) return GD4D_EINVAL;
  for (int l = 0; l < levels; ++l)
    if (!teacher[l] || !a_c[l] || !a_s[l]) return GD4D_EINVAL;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  if (workspace_bytes < gd4d_feat_distill_stats_workspace_bytes(level_hw, levels, R)) return GD4D_EWORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* rowpart = static_cast<float*>(workspace);                     // one level at a time: the stream orders the reuse
  for (int l = 0; l < levels; ++l) {
    const int hw = level_hw[2 * l] * level_hw[2 * l + 1], chunks = (hw + FD_SC - 1) / FD_SC;
    hipLaunchKernelGGL(fd_stats_sums_kernel, dim3((unsigned)(R * chunks)), dim3(256), 0, st, teacher[l], a_c[l], rowpart, hw, chunks);
    hipLaunchKernelGGL(fd_stats_softmax_kernel, dim3(R), dim3(256), 0, st, a_c[l], a_s[l], rowpart, hw, chunks, temperature);
  }
  return check_launch();
}

extern "C" size_t gd4d_feat_distill_workspace_bytes(const int32_t* level_hw, int levels, int R) {
  using namespace gd4d;
  if (fd_check_levels(level_hw, levels, R, FD_C) != GD4D_OK) return 0;
  return fd_layout(level_hw, levels, R).total;
}

extern "C" int gd4d_feat_distill_fwd(const float* const* student, const float* const* teacher, const int32_t* level_hw, int levels, int R,
                                     int C, const float* weight, const float* bias, const float* const* a_c, const float* const* a_s,
                                     float loss_weight, float* loss, float* const* grad_student, float* grad_weight, float* grad_bias,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gd4d;
  if (!student || !teacher || !weight || !bias || !loss || !grad_student || !grad_weight || !grad_bias || !workspace) return GD4D_EINVAL;
  if ((a_c == nullptr) != (a_s == nullptr)) return GD4D_EINVAL;        // both attention maps, or neither (vanilla)
  const int bad = fd_check_levels(level_hw, levels, R, C);
  if (bad != GD4D_OK) return bad;
  for (int l = 0; l < levels; ++l) {
    if (!student[l] || !teacher[l] || !grad_student[l]) return GD4D_EINVAL;
    if (a_c && (!a_c[l] || !a_s[l])) return GD4D_EINVAL;
  }
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const FdLayout w = fd_layout(level_hw, levels, R);
  if (workspace_bytes < w.total) return GD4D_EWORKSPACE;
  const void* kern = a_c ? reinterpret_cast<const void*>(fd_fused_kernel<true>) : reinterpret_cast<const void*>(fd_fused_kernel<false>);
  if (!allow_dynamic_lds(kern, FD_FUSED_LDS)) return GD4D_ELAUNCH;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  float* partial = reinterpret_cast<float*>(base + w.partial);
  u32x4* image = reinterpret_cast<u32x4*>(base + w.image);
  float* wpart = reinterpret_cast<float*>(base + w.wpart);
  float* wpartb = reinterpret_cast<float*>(base + w.wpartb);
  float* g = reinterpret_cast<float*>(base + w.g);                      // one level at a time: the stream orders the reuse
  hipLaunchKernelGGL(fd_weight_image_kernel, dim3(2 * FD_PLANE / 256, levels), dim3(256), 0, st, weight, image);
  long long pbase = 0;
  for (int l = 0; l < levels; ++l) {
    const int hw = level_hw[2 * l] * level_hw[2 * l + 1], tiles = (hw + FD_PX - 1) / FD_PX;
    const double coef = (double)loss_weight / ((double)levels * (double)R * (double)FD_C * (double)hw);
    FdFusedParams p{student[l], teacher[l], a_c ? a_c[l] : nullptr, a_s ? a_s[l] : nullptr, bias + (size_t)l * FD_C,
                    image + (size_t)l * 4 * FD_PLANE, g, grad_student[l], partial + pbase, hw, tiles, (float)(2.0 * coef), (float)coef};
    if (a_c) hipLaunchKernelGGL(fd_fused_kernel<true>, dim3((unsigned)(R * tiles)), dim3(256), FD_FUSED_LDS, st, p);
    else hipLaunchKernelGGL(fd_fused_kernel<false>, dim3((unsigned)(R * tiles)), dim3(256), FD_FUSED_LDS, st, p);
    pbase += (long long)R * tiles;
    const int chunks = (hw + FD_WK - 1) / FD_WK;
    const long long units = (long long)R * chunks;
    const int splits = units < FD_MAX_SPLITS ? (int)units : FD_MAX_SPLITS;
    FdWgradParams q{g, student[l], wpart, wpartb, hw, chunks, splits, units};
    hipLaunchKernelGGL(fd_wgrad_kernel, dim3(splits, 4), dim3(256), 0, st, q);
    hipLaunchKernelGGL(fd_wgrad_reduce_kernel, dim3((FD_C * FD_C + FD_C + 255) / 256), dim3(256), 0, st, wpart, wpartb,
                       grad_weight + (size_t)l * FD_C * FD_C, grad_bias + (size_t)l * FD_C, splits);
  }
  hipLaunchKernelGGL(fd_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, partial, w.npartial, loss);
  return check_launch();
}
