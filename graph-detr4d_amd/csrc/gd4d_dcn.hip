// DCNv2, the modulated deformable 3x3 convolution of the R50 / R101 backbones (mmcv 1.x ModulatedDeformConv2dPack as the configs build
// it: dcn=dict(type='DCNv2', deform_groups=1), stage_with_dcn=(False, False, True, True)), inference forward.  With s the stride,
// pad 1, dilation 1, groups = deform_groups = 1 and o = conv_offset(x) (27 channels, the convolution's own stride and padding):
//     dy_k = o[2 k], dx_k = o[2 k + 1], m_k = sigmoid(o[18 + k])                                   (tap k = 3 ky + kx)
//     out[n, co, y, x] = bias[co] + sum_{ci, k} w[co, ci, k] m_k[n, y, x] bilinear0(x[n, ci], y s - 1 + ky + dy_k, x s - 1 + kx + dx_k)
// bilinear0: corners at floor and floor + 1, a corner outside the image contributes 0 (continuous everywhere; equal to
// F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True) at the same pixel coordinates).  Three entry points:
//
//   gd4d_dcn_weight_image     a 3x3 weight (Cout, Cin, 3, 3) split once into bf16 hi / lo planes laid out as MFMA A fragments in the
//                             order the kernels walk K (tap, then chunk of KC input channels):
//                             [tap][chunk][plane][k-group of 8][Mpad out channels][8 x bf16], rows >= Cout zero.  Cout = 27 (conv_offset):
//                             Mpad = 32, KC = 16; Cout <= 256: Mpad = 256, KC = 32; Cout <= 512: Mpad = 512, KC = 16.  Cin and Cout (other
//                             than 27) multiples of 64 up to 512.
//   gd4d_dcn_offset_conv_fwd  the 27-channel 3x3 convolution (M padded to 32), stride 1 or 2: + bias, sigmoid on channels 18..26, one
//                             (N, 27, Ho, Wo) fp32 map.  M = 32 is ONE MFMA row tile, so no element of the B operand is shared between
//                             waves: each lane loads its own fragment (8 channels of its pixel at the tap, zero outside the image)
//                             from global memory and splits it in registers; the A fragments come from the image through L1 / L2 (1 KB per
//                             plane and k-step, the same for every wave).  No LDS, no barrier.  4 waves x 64 pixels: a 16 x 16 tile.
//   gd4d_dcn_fwd              the hot path: the deformable implicit GEMM, M = Cout x N = output pixels x K = 9 Cin.
//
// Arithmetic: gd4d_bf16x3.h's - both operands split into bf16 hi + lo, lo hi + hi lo + hi hi accumulated in fp32 on
// v_mfma_f32_32x32x16_bf16.  The sample m (w00 v00 + w01 v01 + w10 v10 + w11 v11) is formed in fp32 (fmaf, corner order fixed) and
// split afterwards; floor and fraction are taken of the OFFSET (exact), not of the sum with the pixel's integer position.
//
// gd4d_dcn_fwd.  Where the samples come from: GLOBAL memory (L1 / L2-served), lanes along x so that the corner loads of neighbouring
// pixels share cache lines; no LDS-staged input patch (nobody has measured which wins; this one has no second path for samples that
// leave a patch).  A workgroup of 16 waves owns all (padded) output channels of a tile 16 pixels wide: Mpad = 256 -> 4 (channels) x 4
// (pixels) waves, a 16 x 16 tile, KC = 32 input channels per step; Mpad = 512 -> 8 x 2 waves, a 16 x 8 tile, KC = 16 (the weights'
// double buffer is 64 KB either way).  Each wave 2 x 2 tiles of 32 x 32; the weights are the A operand, the pixels the B operand.
// K is walked tap by tap and, inside a tap, chunk by chunk: 9 Cin / KC steps.
//   coefficients  of a (pixel, tap): the four corner weights (out-of-range corners zeroed, the modulation folded in) and the four
//                 corner byte offsets (clamped into the image), 8 registers of the thread that samples that pixel, computed ONCE per
//                 (tile, tap) - 9 times per tile, never per channel.  Pixels past the ragged edge get zero weights.
//   B stage       a step's (tap, chunk) samples, split hi / lo: [k-group][pixel][8 x bf16] per plane, what depth_conv_kernel's halo
//                 is, so a fragment is one ds_read_b128.  Thread t samples pixel t % NPIX for KC NPIX / 1024 consecutive channels
//                 (8 / 2).  A step has 2 KC / 16 phases (k-half, row tile of the wave: 4 / 2), each in front of six MFMAs: a phase
//                 issues the corner loads of the NEXT step's 2 (1) channels - buffer loads: descriptor and channel offset are scalars,
//                 the corner offset is the one address register - and, after the MFMAs, combines, splits and parks them (4 / 2 bytes
//                 per plane).  Double-buffered by step parity.
//   weight stage  one step's slice of the image, 32 KB hi + lo, copied verbatim; a phase moves 8 (16) bytes per thread the same way.
// So 8 + 2 (4 + 4) registers are in flight under the MFMAs instead of a whole step's 32 + 8, which is what fits 128.
// One barrier per step.  LDS: 133 120 B (Mpad = 256) / 86 016 B (Mpad = 512) with the epilogue's per-channel constants: one workgroup
// of 16 waves per CU.
// Epilogue: out = acc * scale[c] + shift[c], ReLU when asked: shift alone is the bias; scale / shift are the folded frozen BatchNorm
// (scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) scale), the bottleneck's relu(bn2(conv2(x))).  NCHW fp32 in and out;
// tiles ragged on every edge.  No atomics; the order of every sum is fixed.
// Compiler (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): dcn_kernel<4, 32> 127 VGPRs, no scratch, no spills;
// dcn_kernel<8, 16> 127 VGPRs, no scratch, no spills; dcn_offset_conv_kernel 42 VGPRs + 32 AGPRs, no scratch, no LDS.  (Held in
// registers across the taps, the sampling thread's pixel position cost one spilled register: coefficients() recomputes it.)
// Known costs, not yet measured apart: the 2-byte parks of the Mpad = 512 shape are 4-way bank-conflicted ds_write_b16; a lane's four
// corner loads are separate dword loads.
// Left off: an LDS-staged input patch; skipping the loads of pixels whose four weights are zero; the conv_offset kernel's reuse of
// its input across taps (it reads x 9 times through L1 / L2); fusing conv_offset into the main kernel.  The backward is
// gd4d_dcn_train.hip; what both share is gd4d_dcn_common.h.
#include "gd4d_common.h"
#include "gd4d_bf16x3.h"
#include "gd4d_conv_common.h"
#include "gd4d_dcn_common.h"

#include <type_traits>

namespace gd4d {

// ---- conv_offset: the 27-channel convolution ---------------------------------------------------------------------------------
struct DcnOffsetParams {
  const float* x;          // (N, Cin, H, W)
  const char* image;       // Mpad = 32, KC = 16
  const float* bias;       // (27) or null
  float* out;              // (N, 27, Ho, Wo): 18 offsets, 9 modulations
  int cin, h, w, ho, wo, stride, tiles_x, tiles_img;
};

__global__ __launch_bounds__(256) void dcn_offset_conv_kernel(const DcnOffsetParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, kg = lane >> 5;
  const int t = blockIdx.x;
  const int img = t / p.tiles_img, rt = t - img * p.tiles_img;
  const int ty0 = (rt / p.tiles_x) * 16, tx0 = (rt % p.tiles_x) * 16;
  const size_t HW = (size_t)p.h * p.w;
  const float* const xin = p.x + (size_t)img * p.cin * HW + (size_t)(8 * kg) * HW;   // this lane's k-half
  const int ksteps = p.cin / 16;

  int oy[2], ox[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int pp = 64 * wave + 32 * ni + l32;
    oy[ni] = ty0 + (pp >> 4);
    ox[ni] = tx0 + (pp & 15);
  }
  f32x16 acc[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;

  for (int tap = 0; tap < DCN_TAPS; ++tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    bool in[2];
    size_t src[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int y = oy[ni] * p.stride - 1 + ky, x = ox[ni] * p.stride - 1 + kx;
      in[ni] = oy[ni] < p.ho && ox[ni] < p.wo && y >= 0 && y < p.h && x >= 0 && x < p.w;
      src[ni] = in[ni] ? (size_t)y * p.w + x : 0;
    }
    const char* const wa = p.image + (size_t)tap * ksteps * 2048 + (kg * 32 + l32) * 16;
    for (int k = 0; k < ksteps; ++k) {
      const u32x4 ah = *reinterpret_cast<const u32x4*>(wa + (size_t)k * 2048);
      const u32x4 al = *reinterpret_cast<const u32x4*>(wa + (size_t)k * 2048 + 1024);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = in[ni] ? xin[(size_t)(16 * k + j) * HW + src[ni]] : 0.f;
        u32x4 bh, bl;
        split8(v, bh, bl);
        acc[ni] = mfma_32x32x16_x3(ah, al, bh, bl, acc[ni]);
      }
    }
  }

  // C/D of 32x32x16: column (pixel) = l32, rows (channels) 4 kg + (r & 3) + 8 (r >> 2)
  const size_t HWo = (size_t)p.ho * p.wo;
  float* const outp = p.out + (size_t)img * DCN_OFF_C * HWo;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    if (oy[ni] >= p.ho || ox[ni] >= p.wo) continue;
    float* const o = outp + (size_t)oy[ni] * p.wo + ox[ni];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = 4 * kg + (r & 3) + 8 * (r >> 2);
      if (c >= DCN_OFF_C) continue;
      float v = acc[ni][r] + (p.bias ? p.bias[c] : 0.f);
      if (c >= 18) v = 1.f / (1.f + expf(-v));
      o[(size_t)c * HWo] = v;
    }
  }
}

// ---- the deformable convolution ----------------------------------------------------------------------------------------------
struct DcnParams {
  const float* x;          // (N, Cin, H, W)
  const float* offmask;    // (N, 27, Ho, Wo)
  const char* image;
  const float *scale, *shift;   // (Cout) or null
  float* out;              // (N, Cout, Ho, Wo)
  int cin, cout, h, w, ho, wo, stride, relu, tiles_x, tiles_img;
};

// WM waves along the (padded) output channels, 64 each; KC input channels per step.  <4, 32>: Mpad 256, a 16 x 16 tile.  <8, 16>: Mpad
// 512, a 16 x 8 tile.
template <int WM, int KC>
struct DcnShape {
  static constexpr int MPAD = 64 * WM, WN = 16 / WM, NPIX = 64 * WN, TH = NPIX / DCN_TW;
  static constexpr int KG = KC / 8, KS = KC / 16;
  static constexpr int CPT = KC * NPIX / DCN_THREADS;            // channels of its pixel a thread samples per step: 8 / 2
  static constexpr int CPH = CPT / (2 * KS);                     // ... per phase (k-half, row tile of the wave): 2 / 1
  static constexpr int WB = 16 / KS;                             // bytes of a weight plane a thread copies per phase: 8 / 16
  typedef typename std::conditional<KS == 2, uint2, u32x4>::type wvec;
  static constexpr int W_ARR = KG * MPAD * 16, W_STAGE = 2 * W_ARR;   // 16 KB per plane
  static constexpr int B_ARR = KG * NPIX * 16, B_STAGE = 2 * B_ARR;
  static constexpr int EPI = 2 * MPAD * 4;
  static constexpr int LDS = 2 * W_STAGE + 2 * B_STAGE + EPI;
  static_assert(W_STAGE == DCN_THREADS * 32, "two 16-byte loads per thread copy a weight stage");
  static_assert(CPT * DCN_THREADS == KC * NPIX && CPH * 2 * KS == CPT && (CPH == 1 || CPH == 2), "sampling roles");
  static_assert(LDS <= 160 * 1024, "LDS budget of a CU");
};

template <int WM, int KC>
__global__ __launch_bounds__(DCN_THREADS) void dcn_kernel(const DcnParams p) {
  using S = DcnShape<WM, KC>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wbuf = smem;                                   // [2][hi, lo][KG][MPAD][16 B]
  char* const bbuf = smem + 2 * S::W_STAGE;                  // [2][hi, lo][KG][NPIX][16 B]
  float* const e_scale = reinterpret_cast<float*>(bbuf + 2 * S::B_STAGE);
  float* const e_shift = e_scale + S::MPAD;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / S::WN, wn = wave % S::WN;            // wm: 64 output channels, wn: 64 pixels (4 tile rows)
  const int l32 = lane & 31, kg = lane >> 5;

  const int t = blockIdx.x;
  const int img = t / p.tiles_img, rt = t - img * p.tiles_img;
  const int ty0 = (rt / p.tiles_x) * S::TH, tx0 = (rt % p.tiles_x) * DCN_TW;
  const int H = p.h, W = p.w;
  const size_t HW = (size_t)H * W, HWo = (size_t)p.ho * p.wo;
  const int chunks = p.cin / KC, steps = DCN_TAPS * chunks;

  if (tid < S::MPAD) {
    e_scale[tid] = p.scale && tid < p.cout ? p.scale[tid] : 1.f;
    e_shift[tid] = p.shift && tid < p.cout ? p.shift[tid] : 0.f;
  }

  // sampling role: pixel tid % NPIX of the tile, channels s_c0 .. s_c0 + CPT - 1 of every chunk.  What is needed 9 times per tile is
  // recomputed from tid there instead of held in registers.
  const int s_c0 = __builtin_amdgcn_readfirstlane((tid / S::NPIX) * S::CPT);   // (NPIX is a multiple of the wave)
  const unsigned plane_bytes = (unsigned)HW * 4u, oplane_bytes = (unsigned)HWo * 4u;
  // (buffer loads: descriptors and channel offsets are scalars, a load needs ONE address register; the descriptors' bounds checks are
  //  a second guard behind the clamped corners)
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.x + (size_t)img * p.cin * HW), 0, (unsigned)p.cin * plane_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.offmask + (size_t)img * DCN_OFF_C * HWo), 0, DCN_OFF_C * oplane_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(p.image), 0, (unsigned)steps * S::W_STAGE, 0x00020000);
  float cw[4];                                               // corner weights x modulation, zero for a corner outside the image
  unsigned co[4];                                            // corner byte offsets inside a channel plane, always in the image
  auto coefficients = [&](int tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    int t_here = tid;
    asm volatile("" : "+v"(t_here));                         // (keeps the compiler from hoisting what follows back into registers)
    const int s_pix = t_here % S::NPIX;
    const int s_y = ty0 + s_pix / DCN_TW, s_x = tx0 + s_pix % DCN_TW;
    const bool s_live = s_y < p.ho && s_x < p.wo;
    float dy = 0.f, dx = 0.f, m = 0.f;
    if (s_live) {
      const unsigned o = (unsigned)(s_y * p.wo + s_x) * 4u;
      dy = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(orsrc, o, (unsigned)(2 * tap) * oplane_bytes, 0));
      dx = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(orsrc, o, (unsigned)(2 * tap + 1) * oplane_bytes, 0));
      m = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(orsrc, o, (unsigned)(18 + tap) * oplane_bytes, 0));
    }
    // (gd4d_dcn_common.h: offsets beyond +-2^20 and NaN sample nothing; floor and fraction of the offset itself are exact)
    const DcnCorners c = dcn_corners(dy, dx, m, s_y * p.stride - 1 + ky, s_x * p.stride - 1 + kx, H, W);
    dcn_modulated_weights(c, m, cw);
#pragma unroll
    for (int j = 0; j < 4; ++j) co[j] = c.off[j];
  };
  float sr[4 * S::CPH];                                      // one phase's corner values in flight
  auto issue_samples = [&](int chunk, int ph) {
    const unsigned soff = (unsigned)(s_c0 + chunk * KC + ph * S::CPH) * plane_bytes;
#pragma unroll
    for (int j = 0; j < S::CPH; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        sr[4 * j + c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, co[c], soff + j * plane_bytes, 0));
  };
  auto park_samples = [&](int buf, int ph) {
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < S::CPH; ++j)
      v[j] = dcn_combine(cw, sr[4 * j], sr[4 * j + 1], sr[4 * j + 2], sr[4 * j + 3]);
    const unsigned hh = cvt_pk_bf16(v[0], v[1]);
    const unsigned ll = cvt_pk_bf16(v[0] - __uint_as_float(hh << 16), v[1] - __uint_as_float(hh & 0xffff0000u));
    const int ch = s_c0 + ph * S::CPH;                       // channel inside the chunk
    char* const dst = bbuf + buf * S::B_STAGE + ((ch >> 3) * S::NPIX + tid % S::NPIX) * 16 + (ch & 7) * 2;
    if (S::CPH == 2) {
      *reinterpret_cast<unsigned*>(dst) = hh;
      *reinterpret_cast<unsigned*>(dst + S::B_ARR) = ll;
    } else {
      *reinterpret_cast<uint16_t*>(dst) = (uint16_t)hh;
      *reinterpret_cast<uint16_t*>(dst + S::B_ARR) = (uint16_t)ll;
    }
  };
  // a weight stage is 32 bytes per thread, 16 of each plane: phase (ks, mi) moves WB bytes of plane mi
  typedef typename S::wvec wvec;
  wvec wr;
  auto issue_w = [&](int s, int ks, int mi) {
    const unsigned soff = (unsigned)s * S::W_STAGE + mi * S::W_ARR + ks * S::WB;
    if constexpr (S::KS == 2)
      wr = __builtin_bit_cast(wvec, __builtin_amdgcn_raw_buffer_load_b64(wrsrc, (unsigned)tid * 16u, soff, 0));
    else
      wr = __builtin_bit_cast(wvec, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (unsigned)tid * 16u, soff, 0));
  };
  auto park_w = [&](int buf, int ks, int mi) {
    *reinterpret_cast<wvec*>(wbuf + buf * S::W_STAGE + mi * S::W_ARR + tid * 16 + ks * S::WB) = wr;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  coefficients(0);
#pragma unroll 1
  for (int ks = 0; ks < S::KS; ++ks)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      issue_samples(0, 2 * ks + mi);
      issue_w(0, ks, mi);
      park_samples(0, 2 * ks + mi);
      park_w(0, ks, mi);
    }
  __syncthreads();
  int n_tap = 0, n_chunk = 1;                                // the (tap, chunk) of step s + 1
  if (n_chunk == chunks) { n_chunk = 0; n_tap = 1; }
  for (int s = 0; s < steps; ++s) {
    const bool more = s + 1 < steps;
    if (more && n_chunk == 0) coefficients(n_tap);           // once per (tile, tap)
    const char* wb = wbuf + (s & 1) * S::W_STAGE;
    const char* bb = bbuf + (s & 1) * S::B_STAGE;
#pragma unroll 1                                             // (as depth_conv_kernel: unrolled, both halves' fragments are hoisted and spill)
    for (int ks = 0; ks < S::KS; ++ks) {
      const int kgrp = 2 * ks + kg;
      u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int aoff = (kgrp * S::MPAD + 64 * wm + 32 * i + l32) * 16;
        const int boff = (kgrp * S::NPIX + 64 * wn + 32 * i + l32) * 16;
        ah[i] = *reinterpret_cast<const u32x4*>(wb + aoff);
        al[i] = *reinterpret_cast<const u32x4*>(wb + S::W_ARR + aoff);
        bh[i] = *reinterpret_cast<const u32x4*>(bb + boff);
        bl[i] = *reinterpret_cast<const u32x4*>(bb + S::B_ARR + boff);
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        // the next step's phase (ks, mi): its loads are in flight under these MFMAs; the stages they are parked in were last read
        // in step s - 1
        if (more) {
          issue_samples(n_chunk, 2 * ks + mi);
          issue_w(s + 1, ks, mi);
        }
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma_32x32x16_x3(ah[mi], al[mi], bh[ni], bl[ni], acc[mi][ni]);
        if (more) {
          park_samples((s + 1) & 1, 2 * ks + mi);
          park_w((s + 1) & 1, ks, mi);
        }
      }
    }
    if (more && ++n_chunk == chunks) { n_chunk = 0; ++n_tap; }
    __syncthreads();
  }

  // C/D of 32x32x16: column (pixel) = l32, rows (channels) 4 kg + (r & 3) + 8 (r >> 2)
  float* const outp = p.out + (size_t)img * p.cout * HWo;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int pp = 64 * wn + 32 * ni + l32;
    const int y = ty0 + pp / DCN_TW, x = tx0 + pp % DCN_TW;
    if (y >= p.ho || x >= p.wo) continue;
    float* const o = outp + (size_t)y * p.wo + x;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      if (64 * wm + 32 * mi >= p.cout) continue;             // (Cout is a multiple of 64: a 32-row tile is all padding or none)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 64 * wm + 32 * mi + 4 * kg + (r & 3) + 8 * (r >> 2);
        float v = acc[mi][ni][r] * e_scale[c] + e_shift[c];
        if (p.relu) v = fmaxf(v, 0.f);
        o[(size_t)c * HWo] = v;
      }
    }
  }
}

template <int WM, int KC>
static int dcn_launch(DcnParams& p, int n, void* stream) {
  using S = DcnShape<WM, KC>;
  p.tiles_x = (p.wo + DCN_TW - 1) / DCN_TW;
  p.tiles_img = p.tiles_x * ((p.ho + S::TH - 1) / S::TH);
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  if (!allow_dynamic_lds(reinterpret_cast<const void*>(dcn_kernel<WM, KC>), S::LDS)) return GD4D_ELAUNCH;
  hipLaunchKernelGGL((dcn_kernel<WM, KC>), dim3((unsigned)tiles), dim3(DCN_THREADS), S::LDS, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

}  // namespace gd4d

extern "C" size_t gd4d_dcn_weight_image_bytes(int cin, int cout) {
  int mpad, kc;
  if (!gd4d::dcn_cin_ok(cin) || !gd4d::dcn_geometry(cout, mpad, kc)) return 0;
  return (size_t)gd4d::DCN_TAPS * cin * mpad * 4;
}

extern "C" int gd4d_dcn_weight_image(const float* weight, int cin, int cout, void* image, void* stream) {
  using namespace gd4d;
  if (!weight || !image) return GD4D_EINVAL;
  int mpad, kc;
  if (!dcn_cin_ok(cin) || !dcn_geometry(cout, mpad, kc)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  const ConvImage d{cin, cout, DCN_TAPS, mpad, kc, mpad, 1, 0, 0};
  return pack_conv_image(d, weight, image, static_cast<hipStream_t>(stream));
}

extern "C" int gd4d_dcn_offset_conv_fwd(const float* x, int n, int cin, int h, int w, int stride, const void* image, const float* bias,
                                        float* offmask, void* stream) {
  using namespace gd4d;
  if (!x || !image || !offmask) return GD4D_EINVAL;
  int ho, wo;
  if (!dcn_cin_ok(cin) || !dcn_out_hw(n, cin, DCN_OFF_C, h, w, stride, ho, wo)) return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  DcnOffsetParams p{x, static_cast<const char*>(image), bias, offmask, cin, h, w, ho, wo, stride, 0, 0};
  p.tiles_x = (wo + 15) / 16;
  p.tiles_img = p.tiles_x * ((ho + 15) / 16);
  const long long tiles = (long long)n * p.tiles_img;
  if (tiles > (1ll << 30)) return GD4D_EUNSUPPORTED;
  hipLaunchKernelGGL(dcn_offset_conv_kernel, dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_dcn_fwd(const float* x, const float* offmask, int n, int cin, int cout, int h, int w, int stride, const void* image,
                            const float* scale, const float* shift, int relu, float* out, void* stream) {
  using namespace gd4d;
  if (!x || !offmask || !image || !out) return GD4D_EINVAL;
  int ho, wo, mpad, kc;
  if (!dcn_cin_ok(cin) || cout == DCN_OFF_C || !dcn_geometry(cout, mpad, kc) || !dcn_out_hw(n, cin, cout, h, w, stride, ho, wo) ||
      (relu != 0 && relu != 1))
    return GD4D_EUNSUPPORTED;
  if (!aligned16(image)) return GD4D_EALIGN;
  DcnParams p{x, offmask, static_cast<const char*>(image), scale, shift, out, cin, cout, h, w, ho, wo, stride, relu, 0, 0};
  return mpad == 256 ? dcn_launch<4, 32>(p, n, stream) : dcn_launch<8, 16>(p, n, stream);
}
