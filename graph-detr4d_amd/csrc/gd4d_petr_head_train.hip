// Training the key side of PETRHead / PETRv2Head (autograd.PetrKeysFunction): three launches next to gd4d_petr_keys_fwd.
//
//   gd4d_petr_keys_train_fwd   petr_keys_kernel's training instantiation (gd4d_petr_keys.h): memory / key_pos as the inference launch
//                              writes them, bit for bit, and the embedding and the gate's logits it holds in registers.  Without a
//                              gate nothing more is stored, and the entry point is gd4d_petr_keys_fwd.
//   gd4d_petr_keys_bwd_rows    one pass over the rows: the gradients of key_pos = pe sigmoid(logit) + sine at the camera-major rows
//                              the MLPs' backward reads, and dmemory transposed into input_proj's NCHW map.
//   gd4d_mlp2_wgrad            the weight and bias gradients of y = relu(X W1^T + b1) W2^T + b2 from dY, the hidden activation never
//                              written and X either read (the sine expansion, K1 = 384) or generated in registers (the frustum, 192).
//
// gd4d_mlp2_wgrad.  Hidden columns do not interact, so a workgroup owns a chunk c of 32 hidden units and a partition of the 128-row
// tiles and keeps dW2[:, c] (256 x 32), dW1[c, :] (32 x K1) and db1[c] in accumulators while it walks its tiles.  Per tile:
//     hid  = relu(X W1[c]^T + b1[c])          K = K1    each wave its 32 rows; W1[c] split once per workgroup, in LDS
//     dhid = (dY W2[:, c]) [hid > 0]          K = 256   W2[:, c] split once per workgroup, in registers (generated X: 3 of the 16
//                                                       steps in LDS - the frustum's arithmetic needs the registers)
//     dW2[:, c] += dY^T hid                   K = rows  wave w: output channels 64 w .. 64 w + 63
//     dW1[c, :] += dhid^T X                   K = rows  wave w: input channels 32 (w + 4 q) ..
// The two K = rows products take operands with 8 consecutive rows of ONE column per lane.  hid / dhid leave phase A as C / D tiles with
// the hidden unit along the lanes and 4 consecutive rows per register group: they are split to bf16 hi / lo and stored as [column][row]
// planes in LDS (8-byte stores), the 16-byte row chunks of a column XOR-swizzled by the column so that 32 columns read 32 banks' worth.
// dY and a stored X are read from memory in that form directly (8 rows of one column per lane, the lanes along the columns: 128-byte
// lines); the generated X is stored to LDS planes like hid.  Rows beyond M: hid = dhid = 0 and dY is read as 0.
// Each (chunk, partition) leaves one partial in the workspace; mlp2_wgrad_reduce_kernel adds them in partition order.  No atomics,
// every sum in a fixed order.  Three bf16 products per product (gd4d_bf16x3.h).
#include "gd4d_petr_keys.h"

namespace gd4d {

// ---- gd4d_petr_keys_bwd_rows ------------------------------------------------------------------------------------------------
struct PetrBwdRows {
  const float* dkey_pos;    // (n S, bs, 256)
  const float* dmemory;     // (n S, bs, 256) or NULL: zeros
  const float* pe;          // GATE: (M, 256) the forward's embedding
  const float* logit;       // GATE: (M, 256) the forward's gate logits
  float* dpe;               // (M, 256) or NULL (no gate: dpe = dsine)
  float* dlogit;            // GATE: (M, 256)
  float* dsine;             // (M, 256) or NULL (bs = 1: dkey_pos is it)
  float* dx0;               // (R, 256, S) NCHW
  int M, S, bs, n;
};

constexpr int PB_ROWS = 32, PB_THREADS = 256;

template <bool GATE>
__global__ __launch_bounds__(PB_THREADS) void petr_keys_bwd_rows_kernel(const PetrBwdRows p) {
  __shared__ float tile[ML_N2][PB_ROWS + 1];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * PB_ROWS;
  const int c4 = (tid & 63) * 4;
  // ---- the row gradients: 16-byte reads at the key row, 16-byte writes at the camera-major row ----
  for (int it = 0; it < PB_ROWS / 4; ++it) {
    const int row = it * 4 + (tid >> 6);
    const int m = m0 + row;
    float4 dm = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < p.M) {
      const size_t k = (size_t)petr_key_row(m, p.S, p.bs, p.n) * ML_N2 + c4;
      const size_t o = (size_t)m * ML_N2 + c4;
      const float4 g = *reinterpret_cast<const float4*>(p.dkey_pos + k);
      if (p.dmemory) dm = *reinterpret_cast<const float4*>(p.dmemory + k);
      if (p.dsine) *reinterpret_cast<float4*>(p.dsine + o) = g;
      if (GATE) {
        const float4 pv = *reinterpret_cast<const float4*>(p.pe + o);
        const float4 lv = *reinterpret_cast<const float4*>(p.logit + o);
        const float gv[4] = {g.x, g.y, g.z, g.w}, pe[4] = {pv.x, pv.y, pv.z, pv.w}, lg[4] = {lv.x, lv.y, lv.z, lv.w};
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = ml_sigmoid(lg[i]);
          a[i] = gv[i] * s;
          b[i] = (gv[i] * pe[i]) * (s * (1.0f - s));
        }
        *reinterpret_cast<float4*>(p.dpe + o) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4*>(p.dlogit + o) = make_float4(b[0], b[1], b[2], b[3]);
      } else if (p.dpe) {
        *reinterpret_cast<float4*>(p.dpe + o) = g;
      }
    }
    tile[c4][row] = dm.x; tile[c4 + 1][row] = dm.y; tile[c4 + 2][row] = dm.z; tile[c4 + 3][row] = dm.w;
  }
  __syncthreads();
  // ---- dx0 = dmemory transposed into the NCHW map ----
  const int r0 = m0 / p.S, pix0 = m0 - r0 * p.S;
  const bool whole = m0 + PB_ROWS <= p.M && pix0 + PB_ROWS <= p.S && (p.S & 3) == 0 && (pix0 & 3) == 0;
  if (whole) {                                            // the 32 pixels are one camera's, 16-byte aligned in every channel
    float* base = p.dx0 + (size_t)r0 * ML_N2 * p.S + pix0;
    for (int it = 0; it < ML_N2 * PB_ROWS / 4 / PB_THREADS; ++it) {
      const int idx = it * PB_THREADS + tid, ch = idx >> 3, q = idx & 7;
      *reinterpret_cast<float4*>(base + (size_t)ch * p.S + 4 * q) =
          make_float4(tile[ch][4 * q], tile[ch][4 * q + 1], tile[ch][4 * q + 2], tile[ch][4 * q + 3]);
    }
    return;
  }
  for (int it = 0; it < ML_N2 * PB_ROWS / PB_THREADS; ++it) {      // across the end of a camera / of the rows: pixel by pixel
    const int idx = it * PB_THREADS + tid, ch = idx >> 5, row = idx & 31;
    const int m = m0 + row;
    if (m >= p.M) continue;
    const int r = m / p.S, pix = m - r * p.S;
    p.dx0[((size_t)r * ML_N2 + ch) * p.S + pix] = tile[ch][row];
  }
}

// ---- gd4d_mlp2_wgrad ----------------------------------------------------------------------------------------------------------
constexpr int MW_HC = 32, MW_BM = 128, MW_THREADS = 256, MW_COL = 256;       // MW_COL: bytes of a column of a [column][row] bf16 plane
constexpr int MW_MAX_PART = 4096;

struct Mlp2Wg {
  const float* x;           // (M, K1) or NULL: generated
  const float* w1;          // (H, K1)
  const float* b1;          // (H)
  const float* w2;          // (256, H)
  const float* dy;          // (M, 256)
  float* ws;
  int M, H, P, tiles;
};

__host__ __device__ __forceinline__ int mw_tile_begin(int part, int tiles, int P) { return (int)((long long)part * tiles / P); }
__host__ __device__ __forceinline__ size_t mw_part_floats(int K1) { return (size_t)ML_N2 * MW_HC + (size_t)MW_HC * K1 + MW_HC; }

// byte offset of rows 8 chunk .. 8 chunk + 7 of column `col` inside a plane
__device__ __forceinline__ int mw_chunk(int col, int chunk) { return col * MW_COL + ((chunk ^ (col & 15)) << 4); }

template <bool GEN>
__global__ __launch_bounds__(MW_THREADS, 1) void mlp2_wgrad_kernel(const Mlp2Wg p, const Mlp2Fr fr) {
  constexpr int STEPS1 = GEN ? 12 : 24, K1 = 16 * STEPS1, NT1 = K1 / 32, T1W = (NT1 + 3) / 4;
  constexpr int PLANE = MW_HC * MW_COL, XPLANE = K1 * MW_COL;
  extern __shared__ __attribute__((aligned(16))) char mw_smem[];
  char* w1s = mw_smem;                                   // [step][hi, lo][lane] 16 bytes: W1[c] as the B operand of phase A
  char* hidT = w1s + STEPS1 * 2048;                      // [hi, lo][32 hidden][128 rows] bf16
  char* dhidT = hidT + 2 * PLANE;
  char* xT = dhidT + 2 * PLANE;                          // GEN: [hi, lo][192 channels][128 rows] bf16
  // GEN: W2[:, c]'s last steps wait in LDS, not in registers (the frustum's arithmetic needs them; 160 KB of LDS hold the rest)
  constexpr int W2REG = GEN ? 13 : 16;
  char* w2s = xT + (GEN ? 2 * XPLANE : 0);               // [16 - W2REG steps][hi, lo][lane] 16 bytes
  float* red = reinterpret_cast<float*>(hidT);           // 256 floats, after the last tile
  const int c = blockIdx.x, part = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, kg = lane >> 5;
  const int t_lo = mw_tile_begin(part, p.tiles, p.P), t_hi = mw_tile_begin(part + 1, p.tiles, p.P);

  // ---- W1[c] -> LDS, W2[:, c] -> registers, both split once ----
  for (int st = wave; st < STEPS1; st += ML_WAVES) {
    // (the generated X holds input channel 96 kg + 8 st + e in k-slot e of step st: ml_frustum_split)
    const float* src = p.w1 + (size_t)(c * MW_HC + l32) * K1 + (GEN ? 96 * kg + 8 * st : 16 * st + 8 * kg);
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u32x4 h, l;
    split8(v, h, l);
    *reinterpret_cast<u32x4*>(w1s + st * 2048 + lane * 16) = h;
    *reinterpret_cast<u32x4*>(w1s + st * 2048 + 1024 + lane * 16) = l;
  }
  u32x4 w2h[W2REG], w2l[W2REG];
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    if (st >= W2REG && wave != 0) continue;                // (the steps kept in LDS: wave 0 loads and stores them)
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = p.w2[(size_t)(16 * st + 8 * kg + e) * p.H + c * MW_HC + l32];
    if (st < W2REG) {
      split8(v, w2h[st], w2l[st]);
    } else {
      u32x4 h, l;
      split8(v, h, l);
      *reinterpret_cast<u32x4*>(w2s + (st - W2REG) * 2048 + lane * 16) = h;
      *reinterpret_cast<u32x4*>(w2s + (st - W2REG) * 2048 + 1024 + lane * 16) = l;
    }
  }
  const float b1v = p.b1[c * MW_HC + l32];
  f32x16 aw2[2], aw1[T1W];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    aw2[0][r] = 0.f; aw2[1][r] = 0.f;
#pragma unroll
    for (int q = 0; q < T1W; ++q) aw1[q][r] = 0.f;
  }
  float adb1 = 0.f, adb2[2] = {0.f, 0.f};
  __syncthreads();

  for (int tile = t_lo; tile < t_hi; ++tile) {
    const int row0 = tile * MW_BM, rw = row0 + wave * 32;
    const int m = min(rw + l32, p.M - 1);
    // ---- phase A: this wave's 32 rows of hid, the hidden unit along the lanes ----
    f32x16 hid;
#pragma unroll
    for (int r = 0; r < 16; ++r) hid[r] = 0.f;
    if (GEN) {
      u32x4 xh[12], xl[12];
      ml_frustum_split(fr, m, kg, xh, xl);
      const int trow = wave * 32 + l32;
#pragma unroll
      for (int st = 0; st < 12; ++st) {
        const unsigned hw[4] = {xh[st].x, xh[st].y, xh[st].z, xh[st].w}, lw[4] = {xl[st].x, xl[st].y, xl[st].z, xl[st].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = 96 * kg + 8 * st + e;
          const int o = mw_chunk(k, trow >> 3) + (trow & 7) * 2;
          *reinterpret_cast<unsigned short*>(xT + o) = (unsigned short)(e & 1 ? hw[e >> 1] >> 16 : hw[e >> 1] & 0xffffu);
          *reinterpret_cast<unsigned short*>(xT + XPLANE + o) = (unsigned short)(e & 1 ? lw[e >> 1] >> 16 : lw[e >> 1] & 0xffffu);
        }
      }
#pragma unroll
      for (int st = 0; st < 12; ++st) {
        const u32x4 wh = *reinterpret_cast<const u32x4*>(w1s + st * 2048 + lane * 16);
        const u32x4 wl = *reinterpret_cast<const u32x4*>(w1s + st * 2048 + 1024 + lane * 16);
        hid = mfma_32x32x16_x3(xh[st], xl[st], wh, wl, hid);
      }
    } else {
      const float* xr = p.x + (size_t)m * K1 + 8 * kg;
#pragma unroll 4
      for (int st = 0; st < STEPS1; ++st) {
        const float4 a = *reinterpret_cast<const float4*>(xr + 16 * st), b = *reinterpret_cast<const float4*>(xr + 16 * st + 4);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        u32x4 xh, xl;
        split8(v, xh, xl);
        const u32x4 wh = *reinterpret_cast<const u32x4*>(w1s + st * 2048 + lane * 16);
        const u32x4 wl = *reinterpret_cast<const u32x4*>(w1s + st * 2048 + 1024 + lane * 16);
        hid = mfma_32x32x16_x3(xh, xl, wh, wl, hid);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) hid[r] = mfma32_row(kg, r, rw) < p.M ? fmaxf(hid[r] + b1v, 0.f) : 0.f;
    // ---- dhid = (dY W2[:, c]) where hid > 0 ----
    f32x16 dh;
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] = 0.f;
    {
      const float* dr = p.dy + (size_t)m * ML_N2 + 8 * kg;
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const float4 a = *reinterpret_cast<const float4*>(dr + 16 * st), b = *reinterpret_cast<const float4*>(dr + 16 * st + 4);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        u32x4 ah, al;
        split8(v, ah, al);
        if (st < W2REG) {
          dh = mfma_32x32x16_x3(ah, al, w2h[st], w2l[st], dh);
        } else {
          const u32x4 wh = *reinterpret_cast<const u32x4*>(w2s + (st - W2REG) * 2048 + lane * 16);
          const u32x4 wl = *reinterpret_cast<const u32x4*>(w2s + (st - W2REG) * 2048 + 1024 + lane * 16);
          dh = mfma_32x32x16_x3(ah, al, wh, wl, dh);
        }
      }
    }
    float colsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dh[r] = hid[r] > 0.f ? dh[r] : 0.f;
      colsum += dh[r];
    }
    adb1 += colsum;
    // ---- hid, dhid -> [hidden][row] planes: register group g = rows 4 kg + 8 g .. + 3 of this wave's 32, one 8-byte store each ----
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      float hv[8], dv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { hv[e] = hid[8 * gp + e]; dv[e] = dh[8 * gp + e]; }
      u32x4 hh, hl, dh_h, dh_l;
      split8(hv, hh, hl);
      split8(dv, dh_h, dh_l);
#pragma unroll
      for (int g2 = 0; g2 < 2; ++g2) {
        const int o = mw_chunk(l32, wave * 4 + 2 * gp + g2) + kg * 8;
        *reinterpret_cast<uint2*>(hidT + o) = g2 ? make_uint2(hh.z, hh.w) : make_uint2(hh.x, hh.y);
        *reinterpret_cast<uint2*>(hidT + PLANE + o) = g2 ? make_uint2(hl.z, hl.w) : make_uint2(hl.x, hl.y);
        *reinterpret_cast<uint2*>(dhidT + o) = g2 ? make_uint2(dh_h.z, dh_h.w) : make_uint2(dh_h.x, dh_h.y);
        *reinterpret_cast<uint2*>(dhidT + PLANE + o) = g2 ? make_uint2(dh_l.z, dh_l.w) : make_uint2(dh_l.x, dh_l.y);
      }
    }
    __syncthreads();
    // ---- dW2[:, c] += dY^T hid and dW1[c, :] += dhid^T X over the tile's 128 rows, 16 per step ----
#pragma unroll 1
    for (int s = 0; s < MW_BM / 16; ++s) {
      const int fo = mw_chunk(l32, 2 * s + kg);
      const int rk = row0 + 16 * s + 8 * kg;               // this lane's 8 rows of the step
      const u32x4 bh = *reinterpret_cast<const u32x4*>(hidT + fo), bl = *reinterpret_cast<const u32x4*>(hidT + PLANE + fo);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const float* dc = p.dy + (size_t)rk * ML_N2 + 32 * (2 * wave + tt) + l32;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = rk + e < p.M ? dc[(size_t)e * ML_N2] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) adb2[tt] += v[e];
        u32x4 ah, al;
        split8(v, ah, al);
        aw2[tt] = mfma_32x32x16_x3(ah, al, bh, bl, aw2[tt]);
      }
      const u32x4 ah = *reinterpret_cast<const u32x4*>(dhidT + fo), al = *reinterpret_cast<const u32x4*>(dhidT + PLANE + fo);
#pragma unroll
      for (int q = 0; q < T1W; ++q) {
        const int tn = wave + ML_WAVES * q;
        if (tn >= NT1) continue;                            // (wave-uniform)
        const int k = 32 * tn + l32;
        u32x4 xh, xl;
        if (GEN) {
          const int xo = mw_chunk(k, 2 * s + kg);
          xh = *reinterpret_cast<const u32x4*>(xT + xo);
          xl = *reinterpret_cast<const u32x4*>(xT + XPLANE + xo);
        } else {
          const float* xc = p.x + (size_t)rk * K1 + k;
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = rk + e < p.M ? xc[(size_t)e * K1] : 0.f;
          split8(v, xh, xl);
        }
        aw1[q] = mfma_32x32x16_x3(ah, al, xh, xl, aw1[q]);
      }
    }
    __syncthreads();
  }

  // ---- this (chunk, partition)'s partial sums ----
  float* base = p.ws + ((size_t)part * (p.H / MW_HC) + c) * mw_part_floats(K1);
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 16; ++r) base[(size_t)mfma32_row(kg, r, 32 * (2 * wave + tt)) * MW_HC + l32] = aw2[tt][r];
  float* b1p = base + ML_N2 * MW_HC;
#pragma unroll
  for (int q = 0; q < T1W; ++q) {
    const int tn = wave + ML_WAVES * q;
    if (tn >= NT1) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) b1p[(size_t)mfma32_row(kg, r) * K1 + 32 * tn + l32] = aw1[q][r];
  }
  red[tid] = adb1;
  __syncthreads();
  if (tid < MW_HC) {
    float s = 0.f;
    for (int w = 0; w < ML_WAVES; ++w) s += red[64 * w + tid] + red[64 * w + 32 + tid];
    b1p[(size_t)MW_HC * K1 + tid] = s;
  }
  if (c == 0) {                                            // db2 = the column sums of dY: chunk 0's workgroups
    float* db2p = p.ws + (size_t)p.P * (p.H / MW_HC) * mw_part_floats(K1) + (size_t)part * ML_N2;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const float s = adb2[tt] + __shfl_xor(adb2[tt], 32, 64);
      if (kg == 0) db2p[32 * (2 * wave + tt) + l32] = s;
    }
  }
}

// dW2 (256, H), dW1 (H, K1), db1 (H), db2 (256): one thread per element, the partitions' partial sums added in partition order
__global__ void mlp2_wgrad_reduce_kernel(const float* __restrict__ ws, int K1, int H, int P, float* __restrict__ dw2,
                                         float* __restrict__ db2, float* __restrict__ dw1, float* __restrict__ db1) {
  const size_t per = mw_part_floats(K1);
  const int nch = H / MW_HC;
  const long long n2 = (long long)ML_N2 * H, n1 = (long long)H * K1;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const float* src;
  float* dst;
  size_t stride = (size_t)nch * per;
  if (i < n2) {
    const int n = (int)(i / H), h = (int)(i - (long long)n * H);
    src = ws + (size_t)(h / MW_HC) * per + (size_t)n * MW_HC + h % MW_HC;
    dst = dw2 + i;
  } else if ((i -= n2) < n1) {
    const int h = (int)(i / K1), k = (int)(i - (long long)h * K1);
    src = ws + (size_t)(h / MW_HC) * per + (size_t)ML_N2 * MW_HC + (size_t)(h % MW_HC) * K1 + k;
    dst = dw1 + i;
  } else if ((i -= n1) < H) {
    src = ws + (size_t)(i / MW_HC) * per + (size_t)ML_N2 * MW_HC + (size_t)MW_HC * K1 + i % MW_HC;
    dst = db1 + i;
  } else if ((i -= H) < ML_N2 && db2) {
    src = ws + (size_t)P * nch * per + i;
    dst = db2 + i;
    stride = ML_N2;
  } else {
    return;
  }
  float s = 0.f;
  for (int q = 0; q < P; ++q) s += src[(size_t)q * stride];
  *dst = s;
}

static bool mlp2_wgrad_shape(int K1, int H, int N2, int partitions) {
  return (K1 == 192 || K1 == 384) && H >= MW_HC && H % MW_HC == 0 && H <= 4096 && N2 == ML_N2 && partitions >= 1 &&
         partitions <= MW_MAX_PART;
}

}  // namespace gd4d

extern "C" int gd4d_petr_keys_train_fwd(const float* x, const float* img2lidar, int bs, int n, int C, int H, int W, float pad_h,
                                        float pad_w, int D, float depth_start, const double* position_range, const void* pe_image,
                                        const float* pe_b2, int pe_H, const void* se_image, const float* se_b2, int se_H,
                                        const float* sine, float* memory, float* key_pos, float* pe_out, float* logit_out,
                                        void* stream) {
  // without a gate nothing more is stored: the inference launch itself (no second copy of that kernel in this file's code object)
  if (!se_image)
    return gd4d_petr_keys_fwd(x, img2lidar, bs, n, C, H, W, pad_h, pad_w, D, depth_start, position_range, pe_image, pe_b2, pe_H, nullptr,
                              se_b2, se_H, sine, memory, key_pos, stream);
  return gd4d::petr_keys_launch<true>(x, img2lidar, bs, n, C, H, W, pad_h, pad_w, D, depth_start, position_range, pe_image, pe_b2, pe_H,
                                      se_image, se_b2, se_H, sine, memory, key_pos, pe_out, logit_out, stream);
}

extern "C" int gd4d_petr_keys_bwd_rows(const float* dkey_pos, const float* dmemory, const float* pe, const float* logit, int bs, int n,
                                       int H, int W, float* dpe, float* dlogit, float* dsine, float* dx0, void* stream) {
  using namespace gd4d;
  if (!dkey_pos || !dx0 || bs <= 0 || n <= 0 || H <= 0 || W <= 0) return GD4D_EINVAL;
  if (logit ? (!pe || !dpe || !dlogit) : (pe || dlogit)) return GD4D_EINVAL;      // the gate's four tensors come together
  int M = 0;
  if (!petr_keys_shape(bs, n, H, W, &M)) return GD4D_EUNSUPPORTED;
  for (const void* q : {(const void*)dkey_pos, (const void*)dmemory, (const void*)pe, (const void*)logit, (const void*)dpe,
                        (const void*)dlogit, (const void*)dsine, (const void*)dx0})
    if (!aligned16(q)) return GD4D_EALIGN;
  const PetrBwdRows p{dkey_pos, dmemory, pe, logit, dpe, dlogit, dsine, dx0, M, H * W, bs, n};
  const dim3 grid((M + PB_ROWS - 1) / PB_ROWS);
  if (logit) hipLaunchKernelGGL(petr_keys_bwd_rows_kernel<true>, grid, dim3(PB_THREADS), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(petr_keys_bwd_rows_kernel<false>, grid, dim3(PB_THREADS), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" size_t gd4d_mlp2_wgrad_workspace_bytes(int K1, int H, int N2, int partitions) {
  using namespace gd4d;
  if (!mlp2_wgrad_shape(K1, H, N2, partitions)) return 0;
  return ((size_t)partitions * (H / MW_HC) * mw_part_floats(K1) + (size_t)partitions * ML_N2) * sizeof(float);
}

extern "C" int gd4d_mlp2_wgrad_plan(long long M, int H, int partitions, int32_t* grid, int32_t* tile_ranges) {
  using namespace gd4d;
  if (M <= 0 || H <= 0 || partitions <= 0) return GD4D_EINVAL;
  if (H % MW_HC || H > 4096 || partitions > MW_MAX_PART || M >= (1ll << 31) - MW_BM) return GD4D_EUNSUPPORTED;
  const int tiles = (int)((M + MW_BM - 1) / MW_BM);
  if (grid) { grid[0] = H / MW_HC; grid[1] = partitions; }
  if (tile_ranges)
    for (int q = 0; q < partitions; ++q) {
      tile_ranges[2 * q] = mw_tile_begin(q, tiles, partitions);
      tile_ranges[2 * q + 1] = mw_tile_begin(q + 1, tiles, partitions);
    }
  return GD4D_OK;
}

extern "C" int gd4d_mlp2_wgrad(const float* x, int K1, const float* img2lidar, int R, int fH, int fW, float pad_h, float pad_w, int D,
                               float depth_start, const double* position_range, const float* w1, const float* b1, const float* w2,
                               const float* dy, long long M, int H, int N2, int partitions, float* workspace, size_t workspace_bytes,
                               float* dw2, float* db2, float* dw1, float* db1, void* stream) {
  using namespace gd4d;
  if (!w1 || !b1 || !w2 || !dy || !workspace || !dw2 || !dw1 || !db1 || M <= 0 || partitions <= 0) return GD4D_EINVAL;
  if (!x && (!img2lidar || !position_range || R <= 0 || fH <= 0 || fW <= 0)) return GD4D_EINVAL;
  if (!mlp2_wgrad_shape(K1, H, N2, partitions) || M >= (1ll << 31) - MW_BM) return GD4D_EUNSUPPORTED;
  if (x ? K1 != 384 : (K1 != 192 || D != 64)) return GD4D_EUNSUPPORTED;       // one instantiation per source of X
  if (!x && (long long)R * fH * fW != M) return GD4D_EINVAL;
  if (workspace_bytes < gd4d_mlp2_wgrad_workspace_bytes(K1, H, N2, partitions)) return GD4D_EWORKSPACE;
  for (const void* q : {(const void*)x, (const void*)w1, (const void*)dy, (const void*)workspace})
    if (!aligned16(q)) return GD4D_EALIGN;
  const int tiles = (int)((M + MW_BM - 1) / MW_BM);
  const Mlp2Wg p{x, w1, b1, w2, dy, workspace, (int)M, H, partitions, tiles};
  Mlp2Fr fr{};
  if (!x) fr = petr_frustum(img2lidar, fH, fW, pad_h, pad_w, D, depth_start, position_range);
  const dim3 grid(H / MW_HC, partitions);
  auto go = [&](auto kern, int lds) -> int {
    if (!allow_dynamic_lds(reinterpret_cast<const void*>(kern), lds)) return GD4D_ELAUNCH;
    hipLaunchKernelGGL(kern, grid, dim3(MW_THREADS), lds, static_cast<hipStream_t>(stream), p, fr);
    return check_launch();
  };
  const int planes = 4 * MW_HC * MW_COL;                                     // hid, dhid (hi, lo)
  const int rc = x ? go(mlp2_wgrad_kernel<false>, 24 * 2048 + planes)
                   : go(mlp2_wgrad_kernel<true>, 12 * 2048 + planes + 2 * 192 * MW_COL + 3 * 2048);     // + X^T and 3 steps of W2
  if (rc != GD4D_OK) return rc;
  const long long total = (long long)ML_N2 * H + (long long)H * K1 + H + ML_N2;
  hipLaunchKernelGGL(mlp2_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     workspace, K1, H, partitions, dw2, db2, dw1, db1);
  return check_launch();
}
