// gd4d_petr_keys_fwd: the key side of PETRHead / PETRv2Head in ONE kernel (dense_heads/petr_head.py:383-403, petrv2_head.py:444-469
// of the reference).  Per tile of 128 pixels of the R = bs n cameras:
//     pe      = position_encoder(frustum coordinates)            192 -> 1024 -> 256, the inputs generated in registers (Mlp2Fr)
//     gate    = conv_expand(relu(conv_reduce(x)))                256 ->  256 -> 256, x = input_proj(feat) read from its NCHW map
//     key_pos = pe * sigmoid(gate) + sine                        (no gate image - PETRHead, with_fpe=False: pe + sine)
//     memory  = x                                                the transpose of the tile
// both written as the KEY-MAJOR rows PETRTransformer's decoder takes, row (cam H W + pix) bs + b of (n H W, bs, 256): the two permute
// copies of (bs, n, 256, H, W) tensors PETRTransformer.forward makes are not made, and neither the (R, S, 192) frustum tensor, the
// (R, S, 1024) hidden activation nor the (R, S, 256) embedding between the two MLPs exists.
//
// The body is gd4d_mlp2_pe_se_fwd's: ml_frustum_split + ml_phase<12> for the embedding, which waits in 128 registers while
// ml_phase<16> runs the gate (gd4d_mlp2_body.h); what is new is the epilogue - no `feat +` term, two outputs - and the row map.
// Differences to the Detr3DHeadPE fuse: the gate reads input_proj's output, not the raw level, and the result is the transformer's
// key_pos, not a new feature map.
//
// Epilogue layout (C / D of v_mfma_f32_32x32x16): a lane holds, per tile of 32 channels, 4 groups of 4 consecutive pixels of ONE
// channel.  x's four pixels are one 16-byte read per lane from the NCHW map (the lines the gate's A operand was loaded from a
// moment ago; with no gate their first read), stored as `memory` - 32 consecutive channels of a key row per half-wave, 128 bytes -
// next to key_pos.  A bit copy: memory == x.permute exactly.
#include "gd4d_mlp2_body.h"

namespace gd4d {

struct PetrKeys {
  const char* pe_w1; const char* pe_w2; const float* pe_b2; int pe_h;       // position_encoder: gd4d_mlp2_image of (W1 permuted, b1, W2)
  const char* se_w1; const char* se_w2; const float* se_b2; int se_h;       // fpe.conv_reduce / conv_expand (GATE only)
  const float* x;           // (R, 256, S) NCHW
  const float* sine;        // (R, S, 256) channels-last rows
  float* memory;            // (n S, bs, 256)
  float* key_pos;           // (n S, bs, 256)
  int M, S, bs, n;
};

// THE row map: row m = (b n + cam) S + pix of the camera-major inputs -> key row (cam S + pix) bs + b.
__host__ __device__ __forceinline__ long long petr_key_row(int m, int S, int bs, int n) {
  const int r = m / S, pix = m - r * S;
  const int b = r / n, cam = r - b * n;
  return ((long long)cam * S + pix) * bs + b;
}

template <bool GATE>
__global__ __launch_bounds__(ML_THREADS, 1) void petr_keys_kernel(const PetrKeys p, const Mlp2Fr fr) {
  extern __shared__ __attribute__((aligned(16))) char ml_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, kg = lane >> 5;
  const int m0 = blockIdx.x * ML_BM + wave * 32;
  const int m = min(m0 + l32, p.M - 1);
  // ---- position_encoder(frustum) ----
  f32x16 pe[ML_NT];
#pragma unroll
  for (int t = 0; t < ML_NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) pe[t][r] = 0.f;
  {
    u32x4 fh[12], fl[12];
    ml_frustum_split(fr, m, kg, fh, fl);
    ml_phase<12>(p.pe_w1, p.pe_w2, p.pe_h / ML_HC, ml_smem, fh, fl, pe, wave, lane);
  }
#pragma unroll
  for (int t = 0; t < ML_NT; ++t) {
    const float bv = p.pe_b2 ? p.pe_b2[32 * t + l32] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) pe[t][r] += bv;
  }
  // ---- the gate: conv_expand(relu(conv_reduce(x))) ----
  f32x16 acc[ML_NT];                                       // (unused, and removed by the compiler, without a gate)
  if (GATE) {
#pragma unroll
    for (int t = 0; t < ML_NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float xr[16][8];
    {
      // NCHW map: channel c of this lane's pixel is S floats further - a wave instruction reads 32 consecutive pixels of two channels
      const int r = m / p.S, pix = m - r * p.S;
      const float* xc = p.x + ((size_t)r * ML_N2 + 8 * kg) * p.S + pix;
#pragma unroll
      for (int st = 0; st < 16; ++st)
#pragma unroll
        for (int e = 0; e < 8; ++e) xr[st][e] = xc[(size_t)(16 * st + e) * p.S];
    }
    u32x4 xh[16], xl[16];
#pragma unroll
    for (int st = 0; st < 16; ++st) split8(xr[st], xh[st], xl[st]);
    ml_phase<16>(p.se_w1, p.se_w2, p.se_h / ML_HC, ml_smem, xh, xl, acc, wave, lane);
  }
  // ---- memory = x^T, key_pos = pe * sigmoid(gate) + sine, both at the key-major row ----
  typedef float ml_f4u __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int mj = m0 + 4 * kg + 8 * j;
    if (mj >= p.M) continue;
    const int r = mj / p.S, pix = mj - r * p.S;
    const float* xm = p.x + (size_t)r * ML_N2 * p.S + pix;
    const bool whole = pix + 3 < p.S && mj + 3 < p.M;          // the 4 pixels are one camera's: rows bs apart, one 16-byte read of x
    if (whole) {
      const size_t row = (size_t)petr_key_row(mj, p.S, p.bs, p.n) * ML_N2;
      const size_t step = (size_t)p.bs * ML_N2;
      // every read of the group's 8 tiles is requested before the first is used (one wave per SIMD: nothing else hides a round trip)
      ml_f4u f4[ML_NT];
      float sv[ML_NT][4];
#pragma unroll
      for (int t = 0; t < ML_NT; ++t) {
        const int n = 32 * t + l32;
        f4[t] = *reinterpret_cast<const ml_f4u*>(xm + (size_t)n * p.S);
#pragma unroll
        for (int i = 0; i < 4; ++i) sv[t][i] = p.sine[(size_t)(mj + i) * ML_N2 + n];
      }
#pragma unroll
      for (int t = 0; t < ML_NT; ++t) {
        const int n = 32 * t + l32;
        const float bv = GATE && p.se_b2 ? p.se_b2[n] : 0.f;
        const float fv[4] = {f4[t].x, f4[t].y, f4[t].z, f4[t].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const size_t o = row + i * step + n;
          p.memory[o] = fv[i];
          const float pv = pe[t][4 * j + i];
          p.key_pos[o] = GATE ? pv * ml_sigmoid(acc[t][4 * j + i] + bv) + sv[t][i] : pv + sv[t][i];
        }
      }
      continue;
    }
    for (int i = 0; i < 4; ++i) {                         // a group across the end of a camera / of the rows: pixel by pixel
      const int mi = mj + i;
      if (mi >= p.M) break;
      const int ri = mi / p.S, pi = mi - ri * p.S;
      const size_t row = (size_t)petr_key_row(mi, p.S, p.bs, p.n) * ML_N2;
#pragma unroll
      for (int t = 0; t < ML_NT; ++t) {
        const int n = 32 * t + l32;
        float a = 0.f, pv = 0.f;                           // register 4 j + i with a runtime i: a select, not an indexed register
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pv = i == k ? pe[t][4 * j + k] : pv;
          if (GATE) a = i == k ? acc[t][4 * j + k] : a;
        }
        const float sv = p.sine[(size_t)mi * ML_N2 + n];
        p.memory[row + n] = p.x[((size_t)ri * ML_N2 + n) * p.S + pi];
        p.key_pos[row + n] = GATE ? pv * ml_sigmoid(a + (p.se_b2 ? p.se_b2[n] : 0.f)) + sv : pv + sv;
      }
    }
  }
}

static bool petr_keys_shape(int bs, int n, int H, int W, int* M) {
  if (bs <= 0 || n <= 0 || H <= 0 || W <= 0) return false;
  const long long m = (long long)bs * n * H * W;
  if (m >= (1ll << 31) - ML_BM) return false;
  *M = (int)m;
  return true;
}

}  // namespace gd4d

// The launch geometry, on the host (no GPU work): *grid = workgroups (one per tile of 128 rows), *rows_per_block = 128; key_rows, when
// not NULL, receives for every input row m = (b n + cam) H W + pix the key row the kernel writes it to, bs n H W entries.
extern "C" int gd4d_petr_keys_plan(int bs, int n, int H, int W, int32_t* grid, int32_t* rows_per_block, int64_t* key_rows) {
  using namespace gd4d;
  int M = 0;
  if (bs <= 0 || n <= 0 || H <= 0 || W <= 0) return GD4D_EINVAL;
  if (!petr_keys_shape(bs, n, H, W, &M)) return GD4D_EUNSUPPORTED;
  if (grid) *grid = (M + ML_BM - 1) / ML_BM;
  if (rows_per_block) *rows_per_block = ML_BM;
  if (key_rows)
    for (int m = 0; m < M; ++m) key_rows[m] = petr_key_row(m, H * W, bs, n);
  return GD4D_OK;
}

extern "C" int gd4d_petr_keys_fwd(const float* x, const float* img2lidar, int bs, int n, int C, int H, int W, float pad_h, float pad_w,
                                  int D, float depth_start, const double* position_range, const void* pe_image, const float* pe_b2,
                                  int pe_H, const void* se_image, const float* se_b2, int se_H, const float* sine, float* memory,
                                  float* key_pos, void* stream) {
  using namespace gd4d;
  if (!x || !img2lidar || !position_range || !pe_image || !sine || !memory || !key_pos || bs <= 0 || n <= 0 || H <= 0 || W <= 0)
    return GD4D_EINVAL;
  int M = 0;
  if (C != ML_N2 || D != 64 || pe_H != 1024 || (se_image && se_H != ML_N2) || !petr_keys_shape(bs, n, H, W, &M)) return GD4D_EUNSUPPORTED;
  if (!aligned16(pe_image) || (se_image && !aligned16(se_image))) return GD4D_EALIGN;
  const int K1 = 3 * D, S = H * W;
  Mlp2Fr fr{};
  for (int l = 0; l < 4; ++l) { fr.h[l] = H; fr.w[l] = W; fr.hw[l] = S; fr.start[l] = l ? S : 0; }
  fr.start[4] = S;
  fr.S = S; fr.i2l = img2lidar; fr.pad_h = pad_h; fr.pad_w = pad_w; fr.depth_start = depth_start;
  // (the frustum kernel's constants: Python-float arithmetic of the reference, rounded to fp32 when it meets the tensor)
  fr.bin_size = (float)((position_range[3] - (double)depth_start) / ((double)D * (1.0 + (double)D)));
  for (int k = 0; k < 3; ++k) { fr.lo[k] = (float)position_range[k]; fr.span[k] = (float)(position_range[k + 3] - position_range[k]); }
  const char* pi = static_cast<const char*>(pe_image);
  const char* si = static_cast<const char*>(se_image);
  PetrKeys p{pi, pi + (size_t)pe_H * K1 * 4 + (size_t)(pe_H / ML_HC) * 1024, pe_b2, pe_H,
             si, si ? si + (size_t)se_H * ML_N2 * 4 + (size_t)(se_H / ML_HC) * 1024 : nullptr, se_b2, se_H,
             x, sine, memory, key_pos, M, S, bs, n};
  const int grid = (M + ML_BM - 1) / ML_BM;
  auto go = [&](auto kern, int lds) -> int {
    if (!allow_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return GD4D_ELAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ML_THREADS), lds, static_cast<hipStream_t>(stream), p, fr);
    return check_launch();
  };
  if (se_image) return go(petr_keys_kernel<true>, 2 * (16 * 2048 + 1024 + ML_S2));      // the second MLP's stage pair (the larger)
  return go(petr_keys_kernel<false>, 2 * (12 * 2048 + 1024 + ML_S2));
}
