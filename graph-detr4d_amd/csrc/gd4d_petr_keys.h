// What gd4d_petr_head.hip (inference) and gd4d_petr_head_train.hip (training) share: THE row map of the key side (petr_key_row),
// the key-side kernel with its training flag, the frustum geometry of a request and the launch.  See gd4d_petr_head.hip for the
// kernel's description.
#ifndef GD4D_PETR_KEYS_H_
#define GD4D_PETR_KEYS_H_
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
  float* pe_out;            // TRAIN: (M, 256) camera-major rows, the embedding after b2 and before the gate (GATE only)
  float* logit_out;         // TRAIN: (M, 256) camera-major rows, the gate's logits after se_b2 (GATE only)
};

// THE row map: row m = (b n + cam) S + pix of the camera-major inputs -> key row (cam S + pix) bs + b.
__host__ __device__ __forceinline__ long long petr_key_row(int m, int S, int bs, int n) {
  const int r = m / S, pix = m - r * S;
  const int b = r / n, cam = r - b * n;
  return ((long long)cam * S + pix) * bs + b;
}

// TRAIN (gd4d_petr_keys_train_fwd): with a gate, what the epilogue holds in registers is stored as well - the embedding and the gate's
// logits, which the backward's row kernel reads.  Without a gate nothing more is stored (dpe = dkey_pos): <false, true> is never
// instantiated, the training entry point launches the inference kernel.
template <bool GATE, bool TRAIN>
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
          if (GATE && TRAIN) {
            p.pe_out[(size_t)(mj + i) * ML_N2 + n] = pv;
            p.logit_out[(size_t)(mj + i) * ML_N2 + n] = acc[t][4 * j + i] + bv;
          }
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
        if (GATE && TRAIN) {
          p.pe_out[(size_t)mi * ML_N2 + n] = pv;
          p.logit_out[(size_t)mi * ML_N2 + n] = a + (p.se_b2 ? p.se_b2[n] : 0.f);
        }
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

// The frustum geometry of one (H, W) level of R cameras, as the frustum kernels take it.
static Mlp2Fr petr_frustum(const float* img2lidar, int H, int W, float pad_h, float pad_w, int D, float depth_start,
                           const double* position_range) {
  const int S = H * W;
  Mlp2Fr fr{};
  for (int l = 0; l < 4; ++l) { fr.h[l] = H; fr.w[l] = W; fr.hw[l] = S; fr.start[l] = l ? S : 0; }
  fr.start[4] = S;
  fr.S = S; fr.i2l = img2lidar; fr.pad_h = pad_h; fr.pad_w = pad_w; fr.depth_start = depth_start;
  // (the frustum kernel's constants: Python-float arithmetic of the reference, rounded to fp32 when it meets the tensor)
  fr.bin_size = (float)((position_range[3] - (double)depth_start) / ((double)D * (1.0 + (double)D)));
  for (int k = 0; k < 3; ++k) { fr.lo[k] = (float)position_range[k]; fr.span[k] = (float)(position_range[k + 3] - position_range[k]); }
  return fr;
}

// gd4d_petr_keys_fwd (TRAIN = false; pe_out = logit_out = NULL) and gd4d_petr_keys_train_fwd: the checks and the launch.
template <bool TRAIN>
static int petr_keys_launch(const float* x, const float* img2lidar, int bs, int n, int C, int H, int W, float pad_h, float pad_w, int D,
                            float depth_start, const double* position_range, const void* pe_image, const float* pe_b2, int pe_H,
                            const void* se_image, const float* se_b2, int se_H, const float* sine, float* memory, float* key_pos,
                            float* pe_out, float* logit_out, void* stream) {
  if (!x || !img2lidar || !position_range || !pe_image || !sine || !memory || !key_pos || bs <= 0 || n <= 0 || H <= 0 || W <= 0)
    return GD4D_EINVAL;
  if (TRAIN && se_image && (!pe_out || !logit_out)) return GD4D_EINVAL;
  int M = 0;
  if (C != ML_N2 || D != 64 || pe_H != 1024 || (se_image && se_H != ML_N2) || !petr_keys_shape(bs, n, H, W, &M)) return GD4D_EUNSUPPORTED;
  if (!aligned16(pe_image) || (se_image && !aligned16(se_image))) return GD4D_EALIGN;
  const int K1 = 3 * D, S = H * W;
  const Mlp2Fr fr = petr_frustum(img2lidar, H, W, pad_h, pad_w, D, depth_start, position_range);
  const char* pi = static_cast<const char*>(pe_image);
  const char* si = static_cast<const char*>(se_image);
  PetrKeys p{pi, pi + (size_t)pe_H * K1 * 4 + (size_t)(pe_H / ML_HC) * 1024, pe_b2, pe_H,
             si, si ? si + (size_t)se_H * ML_N2 * 4 + (size_t)(se_H / ML_HC) * 1024 : nullptr, se_b2, se_H,
             x, sine, memory, key_pos, M, S, bs, n, pe_out, logit_out};
  const int grid = (M + ML_BM - 1) / ML_BM;
  auto go = [&](auto kern, int lds) -> int {
    if (!allow_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return GD4D_ELAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ML_THREADS), lds, static_cast<hipStream_t>(stream), p, fr);
    return check_launch();
  };
  if (se_image) return go(petr_keys_kernel<true, TRAIN>, 2 * (16 * 2048 + 1024 + ML_S2));      // the second MLP's stage pair (the larger)
  if constexpr (TRAIN) return GD4D_EINVAL;               // (no gate: gd4d_petr_keys_train_fwd calls gd4d_petr_keys_fwd - one kernel, one copy)
  else return go(petr_keys_kernel<false, false>, 2 * (12 * 2048 + 1024 + ML_S2));
}

}  // namespace gd4d

#endif  // GD4D_PETR_KEYS_H_
