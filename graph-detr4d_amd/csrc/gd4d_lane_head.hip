// The lane stages of PETRHeadseg (dense_heads/petr_head_seg.py, losses/Sigmoid_ce_loss.py, detectors/petr3d_seg.py): what the
// reference runs as a long tail of element-wise torch launches behind the two decoders.
//
//   gd4d_lane_mask_loss     Sigmoid_ce_loss (Sigmoid_ce_loss.py:39-43) of every decoder layer against ONE target map, loss and
//                           gradient together, then the nan_to_num of petr_head_seg.py:785:
//     lane_row_weight_kernel   one wave per target row: n1 = #(t == 1), n0 = #(t == 0) by an integer wave reduction, pw = n0 / max(n1, 1)
//                              to the workspace - once per row, shared by the layers;
//     lane_loss_kernel         grid (chunks of LANE_CHUNK elements, layers): term = w (max(x, 0) - x t + log1p(exp(-|x|))) with
//                              w = t pw + (1 - t), and dlogits = coef w (sigmoid(x) - t), coef = loss_weight / (R C).  The terms are
//                              added in fp64: per thread in element order, the workgroup by block_sum (gd4d_common.h); one fp64
//                              partial per workgroup;
//     lane_loss_finish_kernel  one workgroup per layer adds the layer's partials in a fixed order, writes nan_to_num(loss) and - where
//                              the loss was not finite - zeroes the layer's gradient (see include/gd4d.h for this deviation).
//                           No floating-point atomics: two runs give the same bits.  16-byte accesses where C % 4 == 0 and the
//                           tensors are 16-byte aligned, 4-byte ones otherwise.
//
//   gd4d_lane_map_fwd       the map decode of Petr3D_seg.simple_test_pts (petr3d_seg.py:228-246) in one launch: query n = h g + w holds
//                           a 3 x 16 x 16 patch (channel k = 256 c + 16 h1 + w2), which lands at [c, 16 h + h1, 16 w + w2] - the einops
//                           pattern '(h w) c h1 w2 -> c (h h1) (w w2)' as index arithmetic, four consecutive w2 per thread as one
//                           16-byte load and two 16-byte stores.  prob = 1 / (1 + exp(-x)) in fp32, binary = prob >= 0.5 on that value.
//                           With a ground-truth map one workgroup owns a whole (sample, class) plane and reduces inter = sum(binary gt),
//                           sum(binary) (an integer count) and sum(gt) in a fixed order, then writes the IoU of petr3d_seg.py:25-29;
//                           without one the plane's g patch rows are spread over g workgroups.
#include "gd4d_loss_pieces.h"

namespace gd4d {

constexpr int LANE_THREADS = 256;
constexpr int LANE_CHUNK = 4096;                     // elements of one layer per workgroup of lane_loss_kernel: 4 x float4 per thread
constexpr int LANE_PATCH = 768;                      // 3 classes x 16 x 16: what lane_branches' last Linear writes per query
constexpr int LANE_MAP_THREADS = 1024;

// ---- Sigmoid_ce_loss ------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(LANE_THREADS) void lane_row_weight_kernel(const float* __restrict__ t, float* __restrict__ pw, int R, int C) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * (LANE_THREADS / GD4D_WAVE) + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* row = t + (size_t)r * C;
  int n1 = 0, n0 = 0;
  if (VEC) {
    const float4* row4 = reinterpret_cast<const float4*>(row);
    for (int i = lane; i < C / 4; i += GD4D_WAVE) {
      const float4 v = row4[i];
      n1 += (v.x == 1.f) + (v.y == 1.f) + (v.z == 1.f) + (v.w == 1.f);
      n0 += (v.x == 0.f) + (v.y == 0.f) + (v.z == 0.f) + (v.w == 0.f);
    }
  } else {
    for (int i = lane; i < C; i += GD4D_WAVE) {
      const float v = row[i];
      n1 += v == 1.f;
      n0 += v == 0.f;
    }
  }
  n1 = wave_sum(n1);
  n0 = wave_sum(n0);
  if (lane == 0) pw[r] = (float)n0 / fmaxf((float)n1, 1.f);
}

// one element: its term of the mean and its gradient.  Not sigmoid_f / softplus_neg_abs: one e = exp(-|x|) serves both, and the sigmoid
// is the overflow-free e / (1 + e) for x < 0.
__device__ __forceinline__ float lane_term(float x, float t, float pw, float coef, float& grad) {
  const float w = t * pw + (1.f - t);
  const float e = expf(-fabsf(x));                                    // in (0, 1]: never overflows
  const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  grad = coef * w * (sig - t);
  return w * ((fmaxf(x, 0.f) - x * t) + log1pf(e));
}

template <bool VEC>
__global__ __launch_bounds__(LANE_THREADS) void lane_loss_kernel(const float* __restrict__ logits, const float* __restrict__ targets,
                                                                 const float* __restrict__ pw, float* __restrict__ dlogits,
                                                                 double* __restrict__ partial, long long RC, int C, float coef) {
  __shared__ double s_red[LANE_THREADS / GD4D_WAVE];
  const int l = blockIdx.y;
  const float* x = logits + (size_t)l * RC;
  float* dx = dlogits + (size_t)l * RC;
  const long long base = (long long)blockIdx.x * LANE_CHUNK;
  double acc = 0.0;
  if (VEC) {
#pragma unroll
    for (int it = 0; it < LANE_CHUNK / (4 * LANE_THREADS); ++it) {
      const long long i = base + 4 * ((long long)it * LANE_THREADS + threadIdx.x);
      if (i < RC) {                                                     // (C % 4 == 0: the four elements share a row and lie inside)
        const float4 xv = *reinterpret_cast<const float4*>(x + i);
        const float4 tv = *reinterpret_cast<const float4*>(targets + i);
        const float p = pw[i / C];
        float4 g;
        acc += (double)lane_term(xv.x, tv.x, p, coef, g.x);
        acc += (double)lane_term(xv.y, tv.y, p, coef, g.y);
        acc += (double)lane_term(xv.z, tv.z, p, coef, g.z);
        acc += (double)lane_term(xv.w, tv.w, p, coef, g.w);
        *reinterpret_cast<float4*>(dx + i) = g;
      }
    }
  } else {
#pragma unroll 4
    for (int it = 0; it < LANE_CHUNK / LANE_THREADS; ++it) {
      const long long i = base + (long long)it * LANE_THREADS + threadIdx.x;
      if (i < RC) {
        float g;
        acc += (double)lane_term(x[i], targets[i], pw[i / C], coef, g);
        dx[i] = g;
      }
    }
  }
  const double s = block_sum(acc, s_red);
  if (threadIdx.x == 0) partial[(size_t)l * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(LANE_THREADS) void lane_loss_finish_kernel(const double* __restrict__ partial, int chunks, long long RC,
                                                                        double scale, float* __restrict__ loss, float* __restrict__ dlogits) {
  __shared__ double s_red[LANE_THREADS / GD4D_WAVE];
  __shared__ int s_bad;
  const int l = blockIdx.x;
  const double* p = partial + (size_t)l * chunks;
  double acc = 0.0;
  for (int i = threadIdx.x; i < chunks; i += LANE_THREADS) acc += p[i];
  const double s = block_sum(acc, s_red);
  if (threadIdx.x == 0) {
    const float v = (float)(scale * s);                                 // loss_weight * mean
    loss[l] = nan_to_num_f(v);                                          // petr_head_seg.py:785
    s_bad = !finite_f(&v, 1);
  }
  __syncthreads();
  if (s_bad) {
    float* dx = dlogits + (size_t)l * RC;
    for (long long i = threadIdx.x; i < RC; i += LANE_THREADS) dx[i] = 0.f;
  }
}

// ---- the map decode -------------------------------------------------------------------------------------------------------------
template <bool GT>
__global__ __launch_bounds__(LANE_MAP_THREADS) void lane_map_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                                    float* __restrict__ prob, float* __restrict__ binary,
                                                                    float* __restrict__ sums, float* __restrict__ iou, int g) {
  __shared__ float s_inter[LANE_MAP_THREADS / GD4D_WAVE], s_gt[LANE_MAP_THREADS / GD4D_WAVE];
  __shared__ int s_bin[LANE_MAP_THREADS / GD4D_WAVE];
  const int bc = blockIdx.x, b = bc / 3, c = bc - 3 * b;
  const int side = 16 * g;                                              // the map is side x side
  const size_t plane = (size_t)bc * side * side;
  const int per_row = 64 * g;                                           // 16-byte units of one patch row: g queries x 256 channels / 4
  float inter = 0.f, sum_gt = 0.f;
  int sum_bin = 0;
  for (int h = blockIdx.y; h < g; h += gridDim.y) {
    for (int u = threadIdx.x; u < per_row; u += LANE_MAP_THREADS) {
      const int w = u >> 6, j = u & 63, h1 = j >> 2, w2 = (j & 3) * 4;
      const size_t src = ((size_t)b * g * g + (size_t)h * g + w) * LANE_PATCH + 256 * c + 4 * j;
      const size_t dst = plane + (size_t)(16 * h + h1) * side + 16 * w + w2;
      const float4 x = *reinterpret_cast<const float4*>(logits + src);
      float4 p, q;
      p.x = sigmoid_f(x.x);
      p.y = sigmoid_f(x.y);
      p.z = sigmoid_f(x.z);
      p.w = sigmoid_f(x.w);
      q.x = p.x >= 0.5f ? 1.f : 0.f;
      q.y = p.y >= 0.5f ? 1.f : 0.f;
      q.z = p.z >= 0.5f ? 1.f : 0.f;
      q.w = p.w >= 0.5f ? 1.f : 0.f;
      *reinterpret_cast<float4*>(prob + dst) = p;
      *reinterpret_cast<float4*>(binary + dst) = q;
      if (GT) {
        const float4 t = *reinterpret_cast<const float4*>(gt + dst);
        inter += ((q.x * t.x + q.y * t.y) + (q.z * t.z + q.w * t.w));
        sum_gt += ((t.x + t.y) + (t.z + t.w));
        sum_bin += (int)q.x + (int)q.y + (int)q.z + (int)q.w;
      }
    }
  }
  if (GT) {                                                             // (gridDim.y == 1: this workgroup saw the whole plane)
    block_sum_put(inter, s_inter);                                      // the fixed-order workgroup sum of gd4d_common.h, the
    block_sum_put(sum_gt, s_gt);                                        // three values behind one barrier
    block_sum_put(sum_bin, s_bin);
    __syncthreads();
    if (threadIdx.x == 0) {
      constexpr int WAVES = LANE_MAP_THREADS / GD4D_WAVE;
      const float a = block_sum_get<WAVES>(s_inter), t = block_sum_get<WAVES>(s_gt);
      const float nb = (float)block_sum_get<WAVES>(s_bin);
      sums[3 * bc + 0] = a;
      sums[3 * bc + 1] = nb;
      sums[3 * bc + 2] = t;
      iou[bc] = (2.f * a + 0.01f) / ((nb + t) + 0.01f);
    }
  }
}

static int lane_chunks(long long RC) { return (int)((RC + LANE_CHUNK - 1) / LANE_CHUNK); }

}  // namespace gd4d

extern "C" size_t gd4d_lane_mask_loss_workspace_bytes(int L, int R, int C) {
  using namespace gd4d;
  if (L <= 0 || R <= 0 || C <= 0 || L > 65535 || (long long)R * C > (1ll << 40)) return 0;
  const size_t bytes = (size_t)L * lane_chunks((long long)R * C) * sizeof(double) + (size_t)R * sizeof(float);
  return (bytes + 15) & ~(size_t)15;
}

extern "C" int gd4d_lane_mask_loss(const float* logits, const float* targets, float loss_weight, int L, int R, int C, float* loss,
                                   float* dlogits, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gd4d;
  if (!logits || !targets || !loss || !dlogits || L <= 0 || R <= 0 || C <= 0) return GD4D_EINVAL;
  const size_t need = gd4d_lane_mask_loss_workspace_bytes(L, R, C);
  if (need == 0) return GD4D_EUNSUPPORTED;
  if (!workspace || workspace_bytes < need) return GD4D_EWORKSPACE;
  if (!aligned16(workspace)) return GD4D_EALIGN;
  const long long RC = (long long)R * C;
  const int chunks = lane_chunks(RC);
  double* partial = static_cast<double*>(workspace);
  float* pw = reinterpret_cast<float*>(partial + (size_t)L * chunks);
  const bool vec = C % 4 == 0 && aligned16(logits) && aligned16(targets) && aligned16(dlogits);
  const float coef = (float)((double)loss_weight / (double)RC);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 rows((R + 3) / 4), grid(chunks, L);
  if (vec) {
    hipLaunchKernelGGL(lane_row_weight_kernel<true>, rows, dim3(LANE_THREADS), 0, s, targets, pw, R, C);
    hipLaunchKernelGGL(lane_loss_kernel<true>, grid, dim3(LANE_THREADS), 0, s, logits, targets, pw, dlogits, partial, RC, C, coef);
  } else {
    hipLaunchKernelGGL(lane_row_weight_kernel<false>, rows, dim3(LANE_THREADS), 0, s, targets, pw, R, C);
    hipLaunchKernelGGL(lane_loss_kernel<false>, grid, dim3(LANE_THREADS), 0, s, logits, targets, pw, dlogits, partial, RC, C, coef);
  }
  hipLaunchKernelGGL(lane_loss_finish_kernel, dim3(L), dim3(LANE_THREADS), 0, s, partial, chunks, RC,
                     (double)loss_weight / (double)RC, loss, dlogits);
  return check_launch();
}

extern "C" int gd4d_lane_map_fwd(const float* logits, const float* gt_map, int B, int g, float* prob, float* binary, float* sums,
                                 float* iou, void* stream) {
  using namespace gd4d;
  if (!logits || !prob || !binary || B <= 0 || g <= 0) return GD4D_EINVAL;
  if (gt_map && (!sums || !iou)) return GD4D_EINVAL;
  if (g > 2048 || (long long)B * 3 > 0x7fffffffll) return GD4D_EUNSUPPORTED;      // a plane of up to 2^30 elements; int32 counts hold
  if (!aligned16(logits) || !aligned16(prob) || !aligned16(binary) || (gt_map && !aligned16(gt_map))) return GD4D_EALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (gt_map)
    hipLaunchKernelGGL(lane_map_kernel<true>, dim3(3 * B, 1), dim3(LANE_MAP_THREADS), 0, s, logits, gt_map, prob, binary, sums, iou, g);
  else
    hipLaunchKernelGGL(lane_map_kernel<false>, dim3(3 * B, g), dim3(LANE_MAP_THREADS), 0, s, logits, gt_map, prob, binary, sums, iou, g);
  return check_launch();
}
