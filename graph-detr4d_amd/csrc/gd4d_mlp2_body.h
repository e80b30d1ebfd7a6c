// The shared bodies of the two-layer-MLP kernels (gd4d_mlp2.hip, gd4d_petr_head.hip): the tile constants, the frustum geometry
// (Mlp2Fr, ml_frustum_split), the sigmoid of the epilogues and ml_phase - one MLP's walk over its hidden chunks with the weight
// image staged through LDS.  See gd4d_mlp2.hip for the layout of the image and what was measured.
#ifndef GD4D_MLP2_BODY_H_
#define GD4D_MLP2_BODY_H_
#include "gd4d_common.h"
#include "gd4d_bf16x3.h"

#ifndef ML_AHEAD
#define ML_AHEAD 1           // (ml_phase) groups of phase B whose fragments are in flight (2, 3: the same 2.94-2.97 ms)
#endif
#ifndef ML_SPLIT_WAIT
#define ML_SPLIT_WAIT 1      // same box: position MLP 2.12-2.15 -> 2.08 ms, SE gate + fuse 1.30 -> 1.22 ms, the one-kernel form 2.89 = 2.89
#endif

namespace gd4d {

constexpr int ML_WAVES = 4, ML_THREADS = 64 * ML_WAVES, ML_BM = 32 * ML_WAVES, ML_HC = 32, ML_N2 = 256, ML_NT = ML_N2 / 32;
constexpr int ML_S2 = ML_NT * 2 * 2 * 1024;          // bytes of a chunk of W2's image: [tile][step][plane][1 KB]

// sigmoid on the transcendental unit (v_exp_f32, v_rcp_f32: ~1e-7 absolute - the library's expf and an IEEE division are ~45
// instructions per element, and with one wave per SIMD the epilogue's arithmetic is not hidden by anything)
__device__ __forceinline__ float ml_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896340736f));
}

// The FRUSTUM form (gd4d_mlp2_frustum_fwd): X is not read at all.  Row m = camera r, level l, pixel (y, x); its 3 D = 192 inputs are the
// head's frustum coordinates (dense_heads/detr3d_head_pe.py:427-491: pixel centre x depth bin -> lidar frame by the camera's img2lidar
// matrix -> pc_range units -> inverse_sigmoid) - a function of 12 matrix entries and the pixel index, generated in registers when the
// tile's rows would have been loaded (gd4d_frustum_pe_input_fwd's arithmetic, operation for operation; the (R, S, 192) tensor it wrote
// and this kernel re-read - 568 MB each way at 24 cameras - does not exist).  Lane (row, kg) holds input channels 96 kg + j,
// j = 8 step + e: depth bin 32 kg + j / 3, axis j % 3 - so which axis a register holds is known at compile time; W1's image is made
// from W1 with its columns in that order (ops.mlp2_frustum_image).
struct Mlp2Fr {
  const float* i2l;         // (R, 16) img2lidar
  int w[4], h[4], hw[4];
  int start[5];
  int S;
  float pad_h, pad_w, depth_start, bin_size;
  float lo[3], span[3];
};

// hidden unit (inside its chunk of 32) that accumulator register r of a lane with k-group kg holds after phase A: the C / D row
// of v_mfma_f32_32x32x16 - and, read as r = 8 s + e, the k-slot e of phase B's step s
__host__ __device__ __forceinline__ int ml_hidden_of(int kg, int r) { return 4 * kg + (r & 3) + 8 * (r >> 2); }

// The 192 frustum inputs of row m (a lane = one pixel, k-group kg: depth bins 32 kg .. 32 kg + 31), split into bf16 hi / lo as the
// B operand of ml_phase<12>'s first product: gd4d_frustum_pe_input_fwd's arithmetic, operation for operation (see Mlp2Fr).
__device__ __forceinline__ void ml_frustum_split(const Mlp2Fr& fr, const int m, const int kg, u32x4 (&fh)[12], u32x4 (&fl)[12]) {
  const int r = m / fr.S;
  const int rem = m - r * fr.S;
  const int l = (rem >= fr.start[1]) + (rem >= fr.start[2]) + (rem >= fr.start[3]);
  const int pix = rem - fr.start[l];
  const int W = fr.w[l], H = fr.h[l];
  const int y = pix / W, x = pix - y * W;
  const float* mt = fr.i2l + (size_t)r * 16;
  float mm[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) mm[i] = mt[i];
  const float ch = ((float)y * fr.pad_h) / (float)H;
  const float cw = ((float)x * fr.pad_w) / (float)W;
  const float fi0 = kg ? 32.0f : 0.0f;
  float xf[12][8];
#pragma unroll
  for (int dd = 0; dd < 32; ++dd) {
    const float fi = fi0 + (float)dd;
    const float depth = fr.depth_start + (fr.bin_size * fi) * (fi + 1.0f);
    const float sdep = fmaxf(depth, 1e-5f);
    const float px = cw * sdep, py = ch * sdep;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = ((mm[4 * k] * px + mm[4 * k + 1] * py) + mm[4 * k + 2] * depth) + mm[4 * k + 3];
      const float c = (v - fr.lo[k]) / fr.span[k];
      const int j = 3 * dd + k;
      xf[j >> 3][j & 7] = inv_sigmoid_fast(c);
    }
  }
#pragma unroll
  for (int st = 0; st < 12; ++st) split8(xf[st], fh[st], fl[st]);
}

// A phase = one MLP's walk over its hidden chunks (mlp2_kernel's chunk body, one tile per workgroup, no ring across tiles): acc +=
// relu(X W1^T + b1) W2^T for the 32 rows whose X fragments (bf16 hi / lo, the B operand of the transposed first product) the wave holds.
template <int STEPS1>
__device__ __forceinline__ void ml_phase(const char* __restrict__ w1img, const char* __restrict__ w2img, const int nchunks, char* smem,
                                         const u32x4 (&xh)[STEPS1], const u32x4 (&xl)[STEPS1], f32x16 (&acc)[ML_NT],
                                         const int wave, const int lane) {
  typedef __attribute__((address_space(3))) void lds_void_t;
  typedef const __attribute__((address_space(1))) void glb_void_t;
  constexpr int S1 = STEPS1 * 2048 + 1024;
  constexpr int STAGE = S1 + ML_S2;
  constexpr int n1 = S1 >> 10, npieces = STAGE >> 10;
  constexpr int PER_WAVE = (npieces + ML_WAVES - 1) / ML_WAVES;
  const int kg = lane >> 5;
  auto stage_piece = [&](int c, int buf, int k) {
    const int i = wave + ML_WAVES * k;
    if (i >= npieces) return;
    const char* src = i < n1 ? w1img + (size_t)c * S1 + ((size_t)i << 10) : w2img + (size_t)c * ML_S2 + ((size_t)(i - n1) << 10);
    __builtin_amdgcn_global_load_lds((glb_void_t*)(src + lane * 16), (lds_void_t*)(smem + buf * STAGE + (i << 10)), 16, 0, 0);
  };
  __syncthreads();                                     // (the previous phase's stages are done with)
  for (int k = 0; k < PER_WAVE; ++k) stage_piece(0, 0, k);
  for (int c = 0; c < nchunks; ++c) {
    if (ML_SPLIT_WAIT) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // (W1's pieces: see mlp2_kernel)
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool more = c + 1 < nchunks;
    const char* s1 = smem + (c & 1) * STAGE;
    const char* s2 = s1 + S1;
    f32x16 h;
#pragma unroll
    for (int r = 0; r < 16; ++r) h[r] = 0.f;
    const char* f1 = s1 + lane * 16;
    u32x4 wh = *reinterpret_cast<const u32x4*>(f1), wl = *reinterpret_cast<const u32x4*>(f1 + 1024);
#pragma unroll
    for (int st = 0; st < STEPS1; ++st) {
      u32x4 nh = wh, nl = wl;
      if (st + 1 < STEPS1) {
        nh = *reinterpret_cast<const u32x4*>(f1 + (st + 1) * 2048);
        nl = *reinterpret_cast<const u32x4*>(f1 + (st + 1) * 2048 + 1024);
      }
      h = mfma_32x32x16_x3(wh, wl, xh[st], xl[st], h);
      __builtin_amdgcn_sched_barrier(0);
      wh = nh; wl = nl;
    }
    u32x4 ah[2], al[2];
    {
      const float* b1c = reinterpret_cast<const float*>(s1 + STEPS1 * 2048);
      float4 bq[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bq[j] = *reinterpret_cast<const float4*>(b1c + 4 * kg + 8 * j);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float4 ba = bq[2 * s], bb = bq[2 * s + 1];
        const float v[8] = {fmaxf(h[8 * s] + ba.x, 0.f), fmaxf(h[8 * s + 1] + ba.y, 0.f), fmaxf(h[8 * s + 2] + ba.z, 0.f),
                            fmaxf(h[8 * s + 3] + ba.w, 0.f), fmaxf(h[8 * s + 4] + bb.x, 0.f), fmaxf(h[8 * s + 5] + bb.y, 0.f),
                            fmaxf(h[8 * s + 6] + bb.z, 0.f), fmaxf(h[8 * s + 7] + bb.w, 0.f)};
        split8(v, ah[s], al[s]);
      }
    }
    if (ML_SPLIT_WAIT) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    constexpr int GROUPS = 2 * ML_NT;
    const char* f2 = s2 + lane * 16;
    // group g's fragments: [tile][step][plane]; requested ML_AHEAD groups before their MFMAs
    auto frag_at = [&](int g) -> const char* { return f2 + (((g % ML_NT) * 2 + g / ML_NT) * 2) * 1024; };
    u32x4 qh[ML_AHEAD + 1], ql[ML_AHEAD + 1];
#pragma unroll
    for (int a = 0; a < ML_AHEAD; ++a) {
      qh[a] = *reinterpret_cast<const u32x4*>(frag_at(a));
      ql[a] = *reinterpret_cast<const u32x4*>(frag_at(a) + 1024);
    }
#pragma unroll
    for (int grp = 0; grp < GROUPS; ++grp) {
      const int s = grp / ML_NT, t = grp % ML_NT;
      if (grp + ML_AHEAD < GROUPS) {
        qh[ML_AHEAD] = *reinterpret_cast<const u32x4*>(frag_at(grp + ML_AHEAD));
        ql[ML_AHEAD] = *reinterpret_cast<const u32x4*>(frag_at(grp + ML_AHEAD) + 1024);
      }
      acc[t] = mfma_32x32x16_x3(ah[s], al[s], qh[0], ql[0], acc[t]);
      if (more && grp < PER_WAVE) stage_piece(c + 1, (c + 1) & 1, grp);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int a = 0; a < ML_AHEAD; ++a) { qh[a] = qh[a + 1]; ql[a] = ql[a + 1]; }
    }
    if (more)
      for (int k = GROUPS; k < PER_WAVE; ++k) stage_piece(c + 1, (c + 1) & 1, k);
  }
}

}  // namespace gd4d

#endif  // GD4D_MLP2_BODY_H_
