// What the DCNv2 forward (gd4d_dcn.hip) and its training kernels (gd4d_dcn_train.hip) share: the limits and the weight image's
// geometry, the output size, the corner geometry of one (pixel, tap) sample and the order in which a sample's four corners are combined.
#pragma once
#include "gd4d_common.h"

namespace gd4d {

constexpr int DCN_TAPS = 9, DCN_OFF_C = 27, DCN_THREADS = 1024, DCN_TW = 16;
constexpr int DCN_MIN_C = 64, DCN_MAX_C = 512;

// the image's geometry for Cout output channels; false: not served
__host__ __device__ inline bool dcn_geometry(int cout, int& mpad, int& kc) {
  if (cout == DCN_OFF_C) { mpad = 32; kc = 16; return true; }
  if (cout < DCN_MIN_C || cout > DCN_MAX_C || cout % 64) return false;
  if (cout <= 256) { mpad = 256; kc = 32; } else { mpad = 512; kc = 16; }
  return true;
}
inline bool dcn_cin_ok(int cin) { return cin >= DCN_MIN_C && cin <= DCN_MAX_C && cin % 64 == 0; }

// the output size of a 3x3 convolution, pad 1; false: a size or a stride the kernels do not take
inline bool dcn_out_hw(int n, int cin, int cout, int h, int w, int stride, int& ho, int& wo) {
  if (n <= 0 || h <= 0 || w <= 0 || (stride != 1 && stride != 2)) return false;
  ho = (h - 1) / stride + 1;
  wo = (w - 1) / stride + 1;
  // the sampler addresses one image of x with 32-bit byte offsets; everything else is size_t
  return (long long)cin * h * w < (1ll << 30) && (long long)n * (cin > cout ? cin : cout) * h * w <= (1ll << 40);
}

// One (pixel, tap) sample at (ybase + dy, xbase + dx), ybase = y s - 1 + ky, xbase = x s - 1 + kx.  Floor and fraction are taken of the
// OFFSET (exact below 2^20), not of the sum with the integer position: the corners are at floor and floor + 1, so at an integer
// coordinate the fraction is 0 and every derivative in the offset is the one from the right (mmcv's convention).  Offsets beyond
// +-2^20 (and NaN) sample nothing: dy = dx = m = 0 and `sane` false.  in[c]: corner c (00, 01, 10, 11: y-major) lies in the image;
// off[c]: its byte offset inside a channel plane, clamped into the image.
struct DcnCorners {
  float ly, lx, hy, hx;
  bool in[4];
  unsigned off[4];
};
__device__ __forceinline__ bool dcn_offset_sane(float dy, float dx) { return fabsf(dy) < 1048576.f && fabsf(dx) < 1048576.f; }
__device__ __forceinline__ DcnCorners dcn_corners(float& dy, float& dx, float& m, int ybase, int xbase, int H, int W) {
  const bool sane = dcn_offset_sane(dy, dx);
  if (!sane) dy = dx = m = 0.f;
  const float fy = floorf(dy), fx = floorf(dx);
  DcnCorners c;
  c.ly = dy - fy;
  c.lx = dx - fx;
  const int y0 = ybase + (int)fy, x0 = xbase + (int)fx;
  const bool ya = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
  const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W;
  const int yA = min(max(y0, 0), H - 1), yB = min(max(y0 + 1, 0), H - 1);
  const int xA = min(max(x0, 0), W - 1), xB = min(max(x0 + 1, 0), W - 1);
  c.hy = 1.f - c.ly;
  c.hx = 1.f - c.lx;
  c.in[0] = ya && xa;
  c.in[1] = ya && xb;
  c.in[2] = yb && xa;
  c.in[3] = yb && xb;
  c.off[0] = (unsigned)(yA * W + xA) * 4u;
  c.off[1] = (unsigned)(yA * W + xB) * 4u;
  c.off[2] = (unsigned)(yB * W + xA) * 4u;
  c.off[3] = (unsigned)(yB * W + xB) * 4u;
  return c;
}
// the forward's corner weights: the modulation folded in, zero for a corner outside the image
__device__ __forceinline__ void dcn_modulated_weights(const DcnCorners& c, float m, float* cw) {
  cw[0] = c.in[0] ? m * (c.hy * c.hx) : 0.f;
  cw[1] = c.in[1] ? m * (c.hy * c.lx) : 0.f;
  cw[2] = c.in[2] ? m * (c.ly * c.hx) : 0.f;
  cw[3] = c.in[3] ? m * (c.ly * c.lx) : 0.f;
}
// the modulated sample from its corner values, in the forward's B stage's order
__device__ __forceinline__ float dcn_combine(const float* cw, float v00, float v01, float v10, float v11) {
  return fmaf(cw[3], v11, fmaf(cw[2], v10, fmaf(cw[1], v01, cw[0] * v00)));
}

}  // namespace gd4d
