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
// One GEMM kernel, vv_gemm_kernel<MT, MODE, EPI> (gd4d_vovnet_gemm.h: gd4d_vovnet_train.hip instantiates it too, with the backward
// epilogue), in the style of depth_conv_kernel (gd4d_depth_net.hip): the weight image is the MFMA's A
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
#include "gd4d_vovnet_gemm.h"

namespace gd4d {

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
