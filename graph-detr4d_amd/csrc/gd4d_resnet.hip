// The plain convolutions of mmdet's ResNet blocks (Bottleneck: 1x1, 3x3, 1x1 and the 1x1 downsample; BasicBlock: 3x3, 3x3 and the
// downsample) on the bf16 MFMA, inference with frozen BatchNorm: one launch per convolution, with the folded BatchNorm, the residual
// add and the ReLU in its epilogue - no separate pass over the map.
//
//   gd4d_conv1x1_image / gd4d_conv1x1_bn_act_fwd          1x1, stride 1 or 2, no bias
//   gd4d_conv3x3_act_image / gd4d_conv3x3_bn_act_fwd      3x3, pad 1, stride 1 or 2, no bias
//       out[e] = act(acc * scale[c] + shift[c] (+ identity[e]))        act = ReLU where `relu` is set, else nothing
//
// BatchNorm, then the residual, then the ReLU: the block's order.  `relu` is off for a downsample branch and on everywhere else;
// `identity` is conv3's (BasicBlock: conv2's) second operand, a map of the output's shape.
//
// The kernel is vv_gemm_kernel<MT, MODE, VV_RES> (gd4d_vovnet_gemm.h; gd4d_vovnet.hip describes its tiling and staging): the VoVNet
// GEMM with a third epilogue.  The 3x3 runs in MODE VV_S1 / VV_S2 as VoVNet's does and reads gd4d_conv3x3_image's format; the 1x1 with
// stride 1 runs in MODE VV_OSA with one source (128 consecutive pixels of the flat image per workgroup, no pool sums); the 1x1 with
// stride 2 in the new MODE VV_P2: an 8 x 16 tile of OUTPUT pixels whose B operand is staged from the input pixels (2 y, 2 x) only -
// 128 staged pixels per chunk, 16 KB, double-buffered by chunk parity like VV_OSA's, not the 17 x 33 patch a 3x3 of stride 2 needs.  Odd
// input sizes: Ho = (H - 1) / 2 + 1.  The stride-2 K walk is the stride-1 walk, so the result equals the stride-1 kernel's on
// x[:, :, ::2, ::2] bit for bit.
//
// Channels: 1x1 K a multiple of 32 in [32, 2304] and Cout one in [32, 2048] (conv3 of stage 4 and its downsample: 64 row blocks, which
// the tilings 1, 2 and 4 divide); 3x3 Cin in [32, 1024] and Cout in [32, 512] (stage 4 without DCN, ResNet-18's last stage).  The
// limits are this file's (rn_*_channels): VoVNet's entry points keep theirs.  blockIdx.y walks the Cout / (32 MT) row tiles.
//
// Arithmetic: gd4d_bf16x3.h's three products, fp32 sums, K in a fixed order (chunk by chunk of 32 channels, tap by tap inside a
// chunk), no atomics: two runs give the same bits, and so does every M tiling.  With identity = NULL and relu = 1 the 3x3 gives
// gd4d_conv3x3_bn_relu_fwd's bits.
//
// Resources (tools/kernel_code_sizes.py; gfx950): VGPRs + AGPRs, dynamic LDS bytes.  Scratch is 0 bytes per lane for every
// instantiation.
//     MT     3x3 stride 1 (VV_S1)    3x3 stride 2 (VV_S2)     1x1 stride 1 (VV_OSA)    1x1 stride 2 (VV_P2)
//     7      148 + 112, 103 424      256 + 152, 129 152       128 + 112, 90 112        124 + 112, 90 112
//     5      136 +  80,  87 040      256 + 108, 112 768        96 +  80, 73 728         96 +  80, 73 728
//     4      132 +  64,  78 848      256 +  86, 104 576        88 +  64, 65 536         88 +  64, 65 536
//     3      128 +  48,  70 656      256 +  72,  96 384        88 +  48, 57 344         88 +  48, 57 344
//     2      124 +  32,  62 464      256 +  48,  88 192        84 +  32, 49 152         84 +  32, 49 152
//     1      120 +  16,  54 272      256 +  26,  80 000        76 +  16, 40 960         76 +  16, 40 960
// Left off: folding a downsample into conv3's K walk as one launch (the two BatchNorm scales differ: the weights would have to carry
// them), NHWC, the 7x7 stem (3 input channels) and the max-pooling.
#include "gd4d_vovnet_gemm.h"

namespace gd4d {

static bool rn_pw_channels(int k, int cout) {
  return k % 32 == 0 && k >= 32 && k <= 2304 && cout % 32 == 0 && cout >= 32 && cout <= 2048;
}
static bool rn_conv_channels(int cin, int cout) {
  return cin % 32 == 0 && cin >= 32 && cin <= 1024 && cout % 32 == 0 && cout >= 32 && cout <= 512;
}

// taps 1 or 9: the argument checks and the launch of both entry points
static int rn_conv_bn_act(int taps, const float* x, int n, int cin, int h, int w, int stride, const void* image, int cout,
                          const float* scale, const float* shift, const float* identity, int relu, float* out, int m_blocks,
                          void* stream) {
  if (!x || !image || !scale || !shift || !out) return GD4D_EINVAL;
  if (!(taps == 9 ? rn_conv_channels(cin, cout) : rn_pw_channels(cin, cout)) || (stride != 1 && stride != 2) || n <= 0 || h <= 0 || w <= 0)
    return GD4D_EUNSUPPORTED;
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
  const bool flat = taps == 1 && stride == 1;                 // 128 consecutive pixels of the flat image
  p.tiles_x = flat ? 1 : (p.wo + VV_TX - 1) / VV_TX;
  p.tiles_img = flat ? (int)(((long long)h * w + VV_PIX - 1) / VV_PIX) : p.tiles_x * ((p.ho + VV_TY - 1) / VV_TY);
  p.cout = cout;
  p.image = static_cast<const char*>(image);
  p.scale = scale;
  p.shift = shift;
  p.out = out;
  p.identity = identity;
  p.relu = relu != 0;
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (taps == 9)
    return stride == 1 ? vv_launch<VV_S1, VV_RES>(p, tiles, m_blocks, stream) : vv_launch<VV_S2, VV_RES>(p, tiles, m_blocks, stream);
  return stride == 1 ? vv_launch<VV_OSA, VV_RES>(p, tiles, m_blocks, stream) : vv_launch<VV_P2, VV_RES>(p, tiles, m_blocks, stream);
}

}  // namespace gd4d

extern "C" size_t gd4d_conv1x1_image_bytes(int k, int cout) { return gd4d::rn_pw_channels(k, cout) ? (size_t)cout * k * 4 : 0; }

extern "C" int gd4d_conv1x1_image(const float* weight, int k, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  if (!rn_pw_channels(k, cout)) return GD4D_EUNSUPPORTED;
  return vv_image(weight, k, cout, 1, image, stream);
}

extern "C" int gd4d_conv1x1_bn_act_fwd(const float* x, int n, int cin, int h, int w, int stride, const void* image, int cout,
                                       const float* scale, const float* shift, const float* identity, int relu, float* out,
                                       int m_blocks, void* stream) {
  return gd4d::rn_conv_bn_act(1, x, n, cin, h, w, stride, image, cout, scale, shift, identity, relu, out, m_blocks, stream);
}

extern "C" size_t gd4d_conv3x3_act_image_bytes(int cin, int cout) {
  return gd4d::rn_conv_channels(cin, cout) ? (size_t)cout * cin * 9 * 4 : 0;
}

extern "C" int gd4d_conv3x3_act_image(const float* weight, int cin, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  if (!rn_conv_channels(cin, cout)) return GD4D_EUNSUPPORTED;
  return vv_image(weight, cin, cout, 9, image, stream);
}

extern "C" int gd4d_conv3x3_bn_act_fwd(const float* x, int n, int cin, int h, int w, int stride, const void* image, int cout,
                                       const float* scale, const float* shift, const float* identity, int relu, float* out,
                                       int m_blocks, void* stream) {
  return gd4d::rn_conv_bn_act(9, x, n, cin, h, w, stride, image, cout, scale, shift, identity, relu, out, m_blocks, stream);
}
