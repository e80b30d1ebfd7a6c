// The image neck in front of the decoder, inference: mmdet's FPN and the reference's CPFPN (models/necks/cp_fpn.py) with 256 output
// channels, fp32 NCHW maps in.
//   laterals   lat_i = conv1x1_i(C_{i+s}) + b_i                                                          (cp_fpn.py:162-165)
//   top-down   lat_{i-1} += F.interpolate(lat_i, size=lat_{i-1}.shape[2:], mode='nearest')               (cp_fpn.py:169-178)
//   outputs    conv3x3_i(lat_i) + b_i (FPN: every level; CPFPN: level 0 only, the others are their laterals, :182-184)
//   extras     conv3x3 stride 2 pad 1 of the last output, of relu(...) from the second extra on           (cp_fpn.py:202-207)
//
//   gd4d_fpn_lateral_image   a (256, Cin) weight split once into bf16 hi / lo MFMA A fragments in the order the kernel walks K:
//                            [chunk of 32 input channels][plane][k-group of 8][256 out channels][8 x bf16] - gd4d_depth_net_image's
//                            format with one "tap", so the 3x3 images serve the stride-2 kernel below unchanged.
//   gd4d_fpn_lateral_fwd     one level's lateral AND its top-down add: out = (W x + b) + up[nearest].  A camera's level is a Cin x HW
//                            matrix with the pixels contiguous: they are the MFMA's B operand, the weights its A operand.  A workgroup
//                            (4 waves) owns 64 consecutive pixels of the flattened H W index - a tile crosses image rows - and all
//                            256 output channels (wave w: channels 64 w .. 64 w + 63).  K is walked in chunks of 32 input channels:
//                            thread (pixel, k-group) loads 8 channels of its pixel (for one k-group a wave reads 256 contiguous bytes
//                            per channel), splits them hi / lo and parks them in LDS; the next chunk's loads are issued before the
//                            chunk's MFMAs and parked after them (double-buffered, one barrier per chunk).  A fragments come from the
//                            image in L2 (32 KB per chunk, every workgroup of the launch reads the same ones).  An accumulator lane
//                            holds one pixel x 16 channels; the epilogue adds the bias and then the coarser lateral's value at
//                            (min(floor(y * (Hc / H)), Hc - 1), min(floor(x * (Wc / W)), Wc - 1)), both in fp32 - ATen's index rule
//                            and torch's order of the two additions, so the fused add repeats the unfused one bit for bit.  Launch
//                            order is coarse to fine, one launch per level; up == NULL is the coarsest level.
//   gd4d_fpn_extra_conv_fwd  the stride-2 extra levels, a dedicated small kernel (24 x 8 x 13 output pixels at the R50 pyramid): the
//                            same GEMM skeleton, K = 9 taps x 256 channels in gd4d_depth_net_image's order (72 steps), the B tile of a
//                            step gathered at (2 oy - 1 + ky, 2 ox - 1 + kx) with zeros outside the image and an optional ReLU on
//                            read.  Chosen over im2col + gd4d_gemm_bf16x3_fwd: no (rows, 2304) buffer, no second launch, and the
//                            output lands in NCHW or channels-last directly.
//   gd4d_fpn_conv_fwd        the stride-1 3x3 output convolutions: gd4d_depth_net.hip's implicit GEMM with a weight image and a bias
//                            per level (defined there, next to the kernel it instantiates).
// `up`, the extra convolution's input and every output are NCHW or channels-last ((N, H, W, 256); 16-byte aligned), so that a neck
// asked for channels-last outputs writes them in place: the decoder then gathers them without the per-sample copy.
// Training (gd4d_fpn_train.hip has the weight gradients, the top-down adjoint and the bias sums): two more kinds of the same GEMM.
//   gd4d_fpn_lateral_dgrad     dx (N, Cin, H, W) = W^T g: K = the 256 channels of g (8 steps), the Cin output channels walked in blocks
//                              of 256 (grid y; a ragged last block: the transposed image of gd4d_fpn_lateral_image_mode is zero
//                              beyond Cin, waves past it skip their MFMAs and nothing past Cin is stored).
//   gd4d_fpn_extra_conv_dgrad  the stride-2 level's input gradient: the gather GEMM over gd4d_depth_net_image_mode(transposed = 1)'s
//                              taps, tap (ky', kx') of pixel (y, x) reading dy at ((y - 1 + ky') / 2, (x - 1 + kx') / 2) where both
//                              are even and in range (three taps in four contribute zeros: untuned, the levels are tiny); the
//                              epilogue multiplies by [mask > 0] (the forward's ReLU on read) and adds `add` (the level's own dout).
// Arithmetic: split-bf16 x 3 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (gd4d_bf16x3.h).  No atomics: two runs give the same bits.
#include "gd4d_bf16x3.h"
#include "gd4d_common.h"
#include "gd4d_conv_common.h"
#include "gd4d_fpn_index.h"

namespace gd4d {

constexpr int FPN_C = 256;                           // output channels (every shipped config)
constexpr int FPN_PX = 64;                           // pixels per workgroup
constexpr int FPN_KC = 32;                           // input channels per step
constexpr int FPN_THREADS = 256;
constexpr int FPN_PITCH = 5;                         // 16-byte units per pixel of a staged step: 4 k-groups + 1 (bank spread)
constexpr int FPN_B_ARR = FPN_PX * FPN_PITCH;        // units of one plane of a step's pixels
constexpr int FPN_W_ARR = 4 * FPN_C * 16;            // bytes of one plane of a step's weights: 16 KB
constexpr int FPN_W_STEP = 2 * FPN_W_ARR;            // hi + lo
constexpr int FPN_MAX_CIN = 2048;
constexpr int FPN_TAPS = 9;

struct FpnGemmParams {
  const float* x;          // LATERAL: (N, Cin, H, W); EXTRA: (N, 256, H, W), NCHW or channels-last (x_cs / x_ps)
  const char* image;
  const float* bias;       // (256) or null
  const float* up;         // LATERAL: the coarser lateral (N, 256, Hc, Wc), NCHW or channels-last, or null
  float* out;              // (N, 256, Ho, Wo), NCHW or channels-last
  long long x_cs, x_ps;    // element strides of a channel / a pixel of x
  int cin, H, W, Ho, Wo, Hc, Wc, tiles, steps;
  int relu_in, up_cl, out_cl;
  float scale_y, scale_x;  // float(Hc) / float(Ho), float(Wc) / float(Wo)
  int cout;                // LATERAL_DGRAD: output channels (the lateral's Cin); the other kinds write 256
  const float* mask;       // EXTRA_DGRAD: (N, 256, Ho, Wo) or null: the result is kept where mask > 0
  const float* add;        // EXTRA_DGRAD: (N, 256, Ho, Wo) or null: added after the mask
};

enum { FPN_LATERAL = 0, FPN_EXTRA = 1, FPN_LATERAL_DGRAD = 2, FPN_EXTRA_DGRAD = 3 };

template <int KIND>
__global__ __launch_bounds__(FPN_THREADS) void fpn_gemm_kernel(const FpnGemmParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 s_b[2][2][FPN_B_ARR];     // [step parity][hi, lo][pixel][k-group (+ 1)]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
  const int cam = blockIdx.x / p.tiles, p0 = (blockIdx.x - cam * p.tiles) * FPN_PX;
  const int HWo = p.Ho * p.Wo;
  // LATERAL_DGRAD: grid y walks the output channels in blocks of 256, each with its own run of `steps` weight stages
  const int ocb = KIND == FPN_LATERAL_DGRAD ? (int)blockIdx.y : 0;
  const int cout = KIND == FPN_LATERAL_DGRAD ? p.cout : FPN_C;
  const bool wave_has_channels = KIND != FPN_LATERAL_DGRAD || FPN_C * ocb + 64 * wave < cout;
  const float* const xin = p.x + (size_t)cam * p.cin * p.H * p.W;

  // staging role: thread = (pixel of the tile, k-group): 8 input channels of one pixel per step
  const int s_px = p0 + lane, s_kgrp = wave;
  const bool s_ok = s_px < HWo;
  const int s_oy = s_ok ? s_px / p.Wo : 0, s_ox = s_ok ? s_px - s_oy * p.Wo : 0;
  float hr[8];
  auto issue = [&](int s) {
    int chunk = s;
    bool in = s_ok;
    long long pix = s_px;
    if (KIND == FPN_EXTRA) {
      chunk = s / FPN_TAPS;
      const int tap = s - chunk * FPN_TAPS;
      const int iy = 2 * s_oy - 1 + tap / 3, ix = 2 * s_ox - 1 + tap % 3;
      in = s_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      pix = (long long)iy * p.W + ix;
    }
    if (KIND == FPN_EXTRA_DGRAD) {                      // x is dy (H x W); the tile's pixels are dx's (Ho x Wo)
      chunk = s / FPN_TAPS;
      const int tap = s - chunk * FPN_TAPS;
      const int ty = s_oy - 1 + tap / 3, tx = s_ox - 1 + tap % 3;
      const int iy = ty >> 1, ix = tx >> 1;
      in = s_ok && ty >= 0 && tx >= 0 && !(ty & 1) && !(tx & 1) && iy < p.H && ix < p.W;
      pix = (long long)iy * p.W + ix;
    }
    const float* src = xin + (in ? pix * p.x_ps : 0) + (long long)(chunk * FPN_KC + s_kgrp * 8) * p.x_cs;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = in ? src[j * p.x_cs] : 0.f;
      if (KIND == FPN_EXTRA && p.relu_in) v = fmaxf(v, 0.f);
      hr[j] = v;
    }
  };
  auto park = [&](int buf) {
    u32x4 hi, lo;
    split8(hr, hi, lo);
    s_b[buf][0][lane * FPN_PITCH + s_kgrp] = hi;
    s_b[buf][1][lane * FPN_PITCH + s_kgrp] = lo;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  issue(0);
  park(0);
  __syncthreads();
  for (int s = 0; s < p.steps; ++s) {
    const bool more = s + 1 < p.steps;
    if (more) issue(s + 1);
    const char* const wb = p.image + ((size_t)ocb * p.steps + s) * FPN_W_STEP;
    const u32x4* const bh_plane = s_b[s & 1][0];
    const u32x4* const bl_plane = s_b[s & 1][1];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (!wave_has_channels) break;                   // (wave-uniform; the wave still stages and meets the barriers)
      const int kgrp = 2 * ks + kg;
      u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int aoff = (kgrp * FPN_C + 64 * wave + 32 * i + l32) * 16;
        ah[i] = *reinterpret_cast<const u32x4*>(wb + aoff);
        al[i] = *reinterpret_cast<const u32x4*>(wb + FPN_W_ARR + aoff);
        bh[i] = bh_plane[(32 * i + l32) * FPN_PITCH + kgrp];
        bl[i] = bl_plane[(32 * i + l32) * FPN_PITCH + kgrp];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma_32x32x16_x3(ah[mi], al[mi], bh[ni], bl[ni], acc[mi][ni]);
    }
    if (more) park((s + 1) & 1);                       // its readers (step s - 1) finished before the last barrier
    __syncthreads();
  }

  // C/D of 32x32x16: column (pixel) = l32, rows (channels) 4 kg + (r & 3) + 8 (r >> 2): registers 4 q .. 4 q + 3 are 4 channels in a row
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int px = p0 + 32 * ni + l32;
    if (px >= HWo) continue;
    size_t up_pix = 0;
    if (KIND == FPN_LATERAL && p.up) {
      const int y = px / p.Wo, x = px - y * p.Wo;
      const int sy = fpn_nearest_src(y, p.scale_y, p.Hc), sx = fpn_nearest_src(x, p.scale_x, p.Wc);
      up_pix = (size_t)sy * p.Wc + sx;
    }
    const size_t HWc = (size_t)p.Hc * p.Wc;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = FPN_C * ocb + 64 * wave + 32 * mi + 4 * kg + 8 * q;
        if (KIND == FPN_LATERAL_DGRAD && c >= cout) continue;                 // (cout is a multiple of 32: four channels at once)
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p.bias ? acc[mi][ni][4 * q + j] + p.bias[c + j] : acc[mi][ni][4 * q + j];
        if (KIND == FPN_EXTRA_DGRAD) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const size_t at = ((size_t)cam * FPN_C + c + j) * HWo + px;
            if (p.mask && !(p.mask[at] > 0.f)) v[j] = 0.f;                    // strict, as torch's ReLU
            if (p.add) v[j] = p.add[at] + v[j];
          }
        }
        if (KIND == FPN_LATERAL && p.up) {
          if (p.up_cl) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(p.up + ((size_t)cam * HWc + up_pix) * FPN_C + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] + u[j];
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] + p.up[((size_t)cam * FPN_C + c + j) * HWc + up_pix];
          }
        }
        if (p.out_cl) {
          *reinterpret_cast<f32x4*>(p.out + ((size_t)cam * HWo + px) * FPN_C + c) = v;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) p.out[((size_t)cam * cout + c + j) * HWo + px] = v[j];
        }
      }
  }
}

static bool fpn_flag(int v) { return v == 0 || v == 1; }

}  // namespace gd4d

extern "C" size_t gd4d_fpn_lateral_image_bytes(int cin) {
  using namespace gd4d;
  if (cin < FPN_KC || cin > FPN_MAX_CIN || cin % FPN_KC != 0) return 0;
  return (size_t)(cin / FPN_KC) * FPN_W_STEP;
}

extern "C" size_t gd4d_fpn_lateral_image_mode_bytes(int cin, int transposed) {
  using namespace gd4d;
  if (transposed == 0) return gd4d_fpn_lateral_image_bytes(cin);
  if (transposed != 1 || gd4d_fpn_lateral_image_bytes(cin) == 0) return 0;
  return (size_t)((cin + FPN_C - 1) / FPN_C) * (FPN_C / FPN_KC) * FPN_W_STEP;
}

extern "C" int gd4d_fpn_lateral_image_mode(const float* weight, int cin, int out_channels, int transposed, void* image, void* stream) {
  using namespace gd4d;
  if (transposed == 0) return gd4d_fpn_lateral_image(weight, cin, out_channels, image, stream);
  if (!weight || !image) return GD4D_EINVAL;
  if (out_channels != FPN_C || transposed != 1 || gd4d_fpn_lateral_image_bytes(cin) == 0) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  // W^T: rows = the lateral's input channels in blocks of 256 (zeros beyond cin), K = its 256 output channels
  const ConvImage d{cin, FPN_C, 1, FPN_C, FPN_KC, (cin + FPN_C - 1) / FPN_C * FPN_C, 0, 1, 0};
  return pack_conv_image(d, weight, image, static_cast<hipStream_t>(stream));
}

extern "C" int gd4d_fpn_lateral_image(const float* weight, int cin, int out_channels, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  if (out_channels != FPN_C || gd4d_fpn_lateral_image_bytes(cin) == 0) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  const ConvImage d{cin, FPN_C, 1, FPN_C, FPN_KC, FPN_C, 0, 0, 0};
  return pack_conv_image(d, weight, image, static_cast<hipStream_t>(stream));
}

extern "C" int gd4d_fpn_lateral_fwd(const float* x, int n, int cin, int h, int w, const void* image, const float* bias, const float* up,
                                    int up_h, int up_w, int up_channels_last, float* out, int out_channels, int out_channels_last,
                                    void* stream) {
  using namespace gd4d;
  if (!x || !image || !bias || !out) return GD4D_EINVAL;
  if (h <= 0 || w <= 0 || (up && (up_h <= 0 || up_w <= 0))) return GD4D_EINVAL;
  if (out_channels != FPN_C || n <= 0 || gd4d_fpn_lateral_image_bytes(cin) == 0 || !fpn_flag(up_channels_last) ||
      !fpn_flag(out_channels_last))
    return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if ((long long)n * FPN_MAX_CIN * hw > (1ll << 40) || hw > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (up && (up_h > h || up_w > w)) return GD4D_EUNSUPPORTED;          // the top-down path only upsamples
  if (!aligned16(image) || (out_channels_last && !aligned16(out)) || (up && up_channels_last && !aligned16(up))) return GD4D_EALIGN;
  const long long tiles = (hw + FPN_PX - 1) / FPN_PX;
  if (tiles * n > (1ll << 30)) return GD4D_EUNSUPPORTED;
  FpnGemmParams p{};
  p.x = x;
  p.image = static_cast<const char*>(image);
  p.bias = bias;
  p.up = up;
  p.out = out;
  p.x_cs = hw;
  p.x_ps = 1;
  p.cin = cin;
  p.H = p.Ho = h;
  p.W = p.Wo = w;
  p.Hc = up ? up_h : 1;
  p.Wc = up ? up_w : 1;
  p.tiles = (int)tiles;
  p.steps = cin / FPN_KC;
  p.up_cl = up_channels_last;
  p.out_cl = out_channels_last;
  p.scale_y = (float)p.Hc / (float)h;                                   // ATen's compute_scales_value: float(in) / out
  p.scale_x = (float)p.Wc / (float)w;
  hipLaunchKernelGGL(fpn_gemm_kernel<FPN_LATERAL>, dim3((unsigned)(tiles * n)), dim3(FPN_THREADS), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_fpn_extra_conv_fwd(const float* x, int n, int channels, int h, int w, int in_channels_last, const void* image,
                                       const float* bias, int relu_in, float* out, int out_channels_last, void* stream) {
  using namespace gd4d;
  if (!x || !image || !out) return GD4D_EINVAL;
  if (h <= 0 || w <= 0) return GD4D_EINVAL;
  if (channels != FPN_C || n <= 0 || !fpn_flag(in_channels_last) || !fpn_flag(out_channels_last) || !fpn_flag(relu_in))
    return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if ((long long)n * FPN_C * hw > (1ll << 40) || hw > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image) || (out_channels_last && !aligned16(out))) return GD4D_EALIGN;
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const long long tiles = ((long long)ho * wo + FPN_PX - 1) / FPN_PX;
  if (tiles * n > (1ll << 30)) return GD4D_EUNSUPPORTED;
  FpnGemmParams p{};
  p.x = x;
  p.image = static_cast<const char*>(image);
  p.bias = bias;
  p.out = out;
  p.x_cs = in_channels_last ? 1 : hw;
  p.x_ps = in_channels_last ? FPN_C : 1;
  p.cin = FPN_C;
  p.H = h;
  p.W = w;
  p.Ho = ho;
  p.Wo = wo;
  p.Hc = p.Wc = 1;
  p.tiles = (int)tiles;
  p.steps = (FPN_C / FPN_KC) * FPN_TAPS;
  p.relu_in = relu_in;
  p.out_cl = out_channels_last;
  hipLaunchKernelGGL(fpn_gemm_kernel<FPN_EXTRA>, dim3((unsigned)(tiles * n)), dim3(FPN_THREADS), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_fpn_lateral_dgrad(const float* g, int n, int cin, int h, int w, const void* image_t, float* dx, void* stream) {
  using namespace gd4d;
  if (!g || !image_t || !dx) return GD4D_EINVAL;
  if (h <= 0 || w <= 0) return GD4D_EINVAL;
  if (n <= 0 || gd4d_fpn_lateral_image_bytes(cin) == 0) return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if ((long long)n * FPN_MAX_CIN * hw > (1ll << 40) || hw > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image_t)) return GD4D_EALIGN;
  const long long tiles = (hw + FPN_PX - 1) / FPN_PX;
  if (tiles * n > (1ll << 30)) return GD4D_EUNSUPPORTED;
  FpnGemmParams p{};
  p.x = g;
  p.image = static_cast<const char*>(image_t);
  p.out = dx;
  p.x_cs = hw;
  p.x_ps = 1;
  p.cin = FPN_C;                                                        // K: the channels of g
  p.cout = cin;
  p.H = p.Ho = h;
  p.W = p.Wo = w;
  p.Hc = p.Wc = 1;
  p.tiles = (int)tiles;
  p.steps = FPN_C / FPN_KC;
  hipLaunchKernelGGL(fpn_gemm_kernel<FPN_LATERAL_DGRAD>, dim3((unsigned)(tiles * n), (unsigned)((cin + FPN_C - 1) / FPN_C)),
                     dim3(FPN_THREADS), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_fpn_extra_conv_dgrad(const float* dy, int n, int channels, int h, int w, const void* image_t, const float* mask,
                                         const float* add, float* dx, void* stream) {
  using namespace gd4d;
  if (!dy || !image_t || !dx) return GD4D_EINVAL;
  if (h <= 0 || w <= 0) return GD4D_EINVAL;
  if (channels != FPN_C || n <= 0) return GD4D_EUNSUPPORTED;
  const long long hw = (long long)h * w;
  if ((long long)n * FPN_C * hw > (1ll << 40) || hw > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image_t)) return GD4D_EALIGN;
  const long long tiles = (hw + FPN_PX - 1) / FPN_PX;
  if (tiles * n > (1ll << 30)) return GD4D_EUNSUPPORTED;
  FpnGemmParams p{};
  p.x = dy;
  p.image = static_cast<const char*>(image_t);
  p.out = dx;
  p.mask = mask;
  p.add = add;
  p.H = (h + 1) / 2;                                                    // dy, the forward's output grid
  p.W = (w + 1) / 2;
  p.x_cs = (long long)p.H * p.W;
  p.x_ps = 1;
  p.cin = FPN_C;
  p.Ho = h;                                                             // dx, the forward's input grid
  p.Wo = w;
  p.Hc = p.Wc = 1;
  p.tiles = (int)tiles;
  p.steps = (FPN_C / FPN_KC) * FPN_TAPS;
  hipLaunchKernelGGL(fpn_gemm_kernel<FPN_EXTRA_DGRAD>, dim3((unsigned)(tiles * n)), dim3(FPN_THREADS), 0, static_cast<hipStream_t>(stream),
                     p);
  return check_launch();
}
