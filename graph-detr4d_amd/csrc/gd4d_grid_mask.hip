// GridMask (models/utils/grid_mask.py:84-123) on the device: the image augmentation `Detr3D.extract_img_feat` applies to the folded
// (B*N, 3, H, W) images in front of the backbone (detectors/detr3d.py:36, 53-54).
//
// The reference builds a 1.5H x 1.5W mask on the host (rows [d i + st_h, d i + st_h + l) and the same columns zeroed for
// i < hh // d, :93-105), crops its centre (:111), uploads it and multiplies.  With rotate = 1 the angle is always 0, so the cropped
// mask has a closed form and the kernel takes five integers instead of a tensor.  With hh = int(1.5 H), Y = y + (hh - H) // 2:
//     row y is in a band      <=>  use_h, k = Y - st_h >= 0, k // d < hh // d, k % d < l       (columns: ww, st_w, use_w)
//     mask = 0 in a band row or a band column, else 1;  mode 1: mask = 1 - mask
//     out = x mask                      or, with an offset map,  out = mask ? x : offset[y, x]                      (:116-121)
// k // d < hh // d is the reference's `for i in range(hh // d)`: for d > hh / 2 the crop reaches rows where a second band would start
// that was never drawn.
//
//   gm_apply_kernel   a wave owns 64 column groups (V elements each: 16 bytes of input per lane where W and the pointers allow,
//                     single elements otherwise) of a run of rows.  Which of a lane's V columns lie in a column band is decided ONCE
//                     per lane (a V-bit word), the row's band from counters that advance with the row: no division per element or per
//                     row.  A lane whose elements are all masked does not load; in place, a lane whose elements are all kept does
//                     nothing.  The cast to fp16 / bf16 (round to nearest even) rides in the same pass.  The parameters come by value
//                     or - `block` given - from eight device words read at run time, so a captured launch follows the block.
//   gm_draw_kernel    one lane: the step's draws (gd4d_grid_mask_rng.h) from {seed_lo, seed_hi, step, thresh} into the block, step + 1.
#include "gd4d_common.h"
#include "gd4d_grid_mask_rng.h"

namespace gd4d {

constexpr int GM_ROWS_MAX = 8;                       // rows per wave, at most
constexpr int GM_UNROLL = 4;                         // rows whose loads are in flight together

struct gm_bf16 { uint16_t v; };
typedef uint32_t gm_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t gm_u32x4 __attribute__((ext_vector_type(4)));
template <int BYTES> struct GmRaw;
template <> struct GmRaw<2> { typedef uint16_t type; };
template <> struct GmRaw<4> { typedef uint32_t type; };
template <> struct GmRaw<8> { typedef gm_u32x2 type; };
template <> struct GmRaw<16> { typedef gm_u32x4 type; };

__device__ __forceinline__ float gm_to_float(float v) { return v; }
__device__ __forceinline__ float gm_to_float(_Float16 v) { return (float)v; }
__device__ __forceinline__ float gm_to_float(gm_bf16 v) { return bf16_to_f32(v.v); }
__device__ __forceinline__ void gm_from_float(float f, float& o) { o = f; }
__device__ __forceinline__ void gm_from_float(float f, _Float16& o) { o = (_Float16)f; }      // v_cvt_f16_f32: round to nearest even
__device__ __forceinline__ void gm_from_float(float f, gm_bf16& o) { o.v = f32_to_bf16(f); }

template <typename T, int V>
__device__ __forceinline__ void gm_load(const T* p, float (&f)[V]) {
  typedef typename GmRaw<sizeof(T) * V>::type R;
  union { R r; T e[V]; } u;
  u.r = *reinterpret_cast<const R*>(p);
#pragma unroll
  for (int j = 0; j < V; ++j) f[j] = gm_to_float(u.e[j]);
}

template <typename T, int V>
__device__ __forceinline__ void gm_store(T* p, const float (&f)[V]) {
  typedef typename GmRaw<sizeof(T) * V>::type R;
  union { R r; T e[V]; } u;
#pragma unroll
  for (int j = 0; j < V; ++j) gm_from_float(f[j], u.e[j]);
  *reinterpret_cast<R*>(p) = u.r;
}

// position k = (padded coordinate) - start along one axis, with k // d and k % d kept by counting
struct GmBand {
  int k, q, r;
};
__device__ __forceinline__ GmBand gm_band_at(int k, int d) {
  GmBand b{k, 0, 0};
  if (k > 0) {
    b.q = k / d;
    b.r = k - b.q * d;
  }
  return b;
}
__device__ __forceinline__ void gm_band_next(GmBand& b, int d) {
  if (++b.k > 0 && ++b.r == d) {
    b.r = 0;
    ++b.q;
  }
}
__device__ __forceinline__ bool gm_band_in(const GmBand& b, int bands, int l) { return b.k >= 0 && b.q < bands && b.r < l; }

struct GmParams {
  const void* x;
  void* out;
  const float* offset;      // (H, W) or nullptr
  const int32_t* block;     // {apply, d, l, st_h, st_w, seed_lo, seed_hi, step} on the device, or nullptr: the values below
  long long rows;           // R * C * H
  int H, W, hh, ww;
  int apply, d, l, st_h, st_w;
  int use_h, use_w, mode;
  int gen_offset;           // offsets from the block's (seed, step) instead of a tensor
  int rows_per_wave;
};

template <typename TI, typename TO, int V>
__global__ __launch_bounds__(256) void gm_apply_kernel(const GmParams p) {
  int apply = p.apply, d = p.d, l = p.l, st_h = p.st_h, st_w = p.st_w;
  uint32_t seed_lo = 0, key = 0;
  if (p.block) {
    apply = p.block[0];
    d = p.block[1];
    l = p.block[2];
    st_h = p.block[3];
    st_w = p.block[4];
    seed_lo = (uint32_t)p.block[5];
    key = gm_step_key((uint32_t)p.block[6], (uint32_t)p.block[7]);
  }
  const bool inplace = static_cast<const void*>(p.out) == p.x;
  if (!apply && inplace) return;
  if (d < 1) d = 1;                                   // a block nobody has drawn into: any mask, but no division by zero
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = (blockIdx.y * 64 + lane) * V;        // V divides W when V > 1 (the host's choice): a group is inside the row or not
  if (c0 >= p.W) return;
  const unsigned all = (1u << V) - 1u;
  // the lane's columns, once
  unsigned colbits = 0;
  if (apply && p.use_w) {
    const int bands = p.ww / d;
    GmBand b = gm_band_at(c0 + (p.ww - p.W) / 2 - st_w, d);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (gm_band_in(b, bands, l)) colbits |= 1u << j;
      gm_band_next(b, d);
    }
  }
  const unsigned keep_in_band = !apply ? all : (p.mode == 1 ? all : 0u);                        // the lane's kept elements of a band row
  const unsigned keep_outside = !apply ? all : (p.mode == 1 ? colbits : (all & ~colbits));      // ... of any other row
  const int hbands = p.hh / d, htop = (p.hh - p.H) / 2 - st_h;
  const bool use_h = apply && p.use_h;
  const long long row0 = ((long long)blockIdx.x * 4 + wave) * p.rows_per_wave;
  long long row1 = row0 + p.rows_per_wave;
  if (row1 > p.rows) row1 = p.rows;
  if (row0 >= row1) return;
  int y = (int)(row0 % p.H);
  GmBand hb = gm_band_at(htop + y, d);
  const TI* x = static_cast<const TI*>(p.x);
  TO* out = static_cast<TO*>(p.out);
  const bool has_off = apply && (p.offset != nullptr || p.gen_offset);
  for (long long row = row0; row < row1; row += GM_UNROLL) {
    float v[GM_UNROLL][V];
    unsigned keep[GM_UNROLL];
    int ys[GM_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_UNROLL; ++u) {
      keep[u] = all;
      ys[u] = y;
      if (row + u < row1) {
        keep[u] = (use_h && gm_band_in(hb, hbands, l)) ? keep_in_band : keep_outside;
        if (++y == p.H) {
          y = 0;
          hb = gm_band_at(htop, d);
        } else {
          gm_band_next(hb, d);
        }
        if (keep[u] != 0 && !(inplace && keep[u] == all)) {
          gm_load<TI, V>(x + (size_t)(row + u) * p.W + c0, v[u]);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) v[u][j] = 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < GM_UNROLL; ++u) {
      if (row + u >= row1) continue;
      if (inplace && keep[u] == all) continue;        // every element of the group stays what it is
      if (keep[u] != all) {
        if (has_off) {
          const int px = ys[u] * p.W + c0;
          float o[V];
          if (p.offset) {
            constexpr int OV = V > 4 ? 4 : V;         // 16 bytes of the fp32 map at a time
#pragma unroll
            for (int c = 0; c < V / OV; ++c) gm_load<float, OV>(p.offset + px + c * OV, *reinterpret_cast<float(*)[OV]>(&o[c * OV]));
          } else {
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = gm_offset_value(gm_hash_keyed(seed_lo, key, (uint32_t)(px + j)));
          }
#pragma unroll
          for (int j = 0; j < V; ++j) v[u][j] = ((keep[u] >> j) & 1u) ? v[u][j] : o[j];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) v[u][j] = ((keep[u] >> j) & 1u) ? v[u][j] : 0.f;
        }
      }
      gm_store<TO, V>(out + (size_t)(row + u) * p.W + c0, v[u]);
    }
  }
}

__global__ void gm_draw_kernel(uint32_t* __restrict__ state, int32_t* __restrict__ block, int H, double ratio) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t seed_lo = state[0], seed_hi = state[1], step = state[2], thresh = state[3];
  const GmDraw r = gm_draw(seed_lo, seed_hi, step, thresh, H, ratio);
  block[0] = r.apply;
  block[1] = r.d;
  block[2] = r.l;
  block[3] = r.st_h;
  block[4] = r.st_w;
  block[5] = (int32_t)seed_lo;
  block[6] = (int32_t)seed_hi;
  block[7] = (int32_t)step;
  state[2] = step + 1u;
}

static int gm_dtype_bytes(int dtype) { return dtype == GD4D_F32 ? 4 : ((dtype == GD4D_BF16 || dtype == GD4D_F16) ? 2 : 0); }

template <typename TI, typename TO>
static void gm_launch(const GmParams& p, bool vec, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(TI);
  const int groups = vec ? p.W / V : p.W;
  const dim3 grid((unsigned)((p.rows + 4 * p.rows_per_wave - 1) / (4 * p.rows_per_wave)), (unsigned)((groups + 63) / 64));
  if (vec) hipLaunchKernelGGL((gm_apply_kernel<TI, TO, V>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((gm_apply_kernel<TI, TO, 1>), grid, dim3(256), 0, st, p);
}

}  // namespace gd4d

extern "C" int gd4d_grid_mask_fwd(const void* x, void* out, int in_dtype, int out_dtype, int R, int C, int H, int W, int apply, int d,
                                  int l, int st_h, int st_w, int use_h, int use_w, int mode, const float* offset, const int32_t* block,
                                  int gen_offset, void* stream) {
  using namespace gd4d;
  if (!x || !out || R <= 0 || C <= 0 || W <= 0) return GD4D_EINVAL;
  if (H < 3) return GD4D_EINVAL;                      // randint(2, h) needs h >= 3 (grid_mask.py:91)
  if (mode != 0 && mode != 1) return GD4D_EINVAL;
  const int si = gm_dtype_bytes(in_dtype), so = gm_dtype_bytes(out_dtype);
  if (!si || !so) return GD4D_EUNSUPPORTED;
  if (in_dtype != out_dtype && in_dtype != GD4D_F32) return GD4D_EUNSUPPORTED;                  // same type, or fp32 -> fp16 / bf16
  if (x == out && in_dtype != out_dtype) return GD4D_EINVAL;
  if (gen_offset && (!block || offset)) return GD4D_EINVAL;                                      // the seed and step live in the block
  if (!block) {
    if (d < 2 || l < 1 || l > d - 1 || st_h < 0 || st_h >= d || st_w < 0 || st_w >= d) return GD4D_EINVAL;
  }
  if ((long long)H * W >= (1ll << 31) || (long long)R * C * H >= (1ll << 31)) return GD4D_EUNSUPPORTED;
  GmParams p{};
  p.x = x;
  p.out = out;
  p.offset = offset;
  p.block = block;
  p.rows = (long long)R * C * H;
  p.H = H;
  p.W = W;
  p.hh = (int)(1.5 * (double)H);
  p.ww = (int)(1.5 * (double)W);
  p.apply = apply != 0;
  p.d = d;
  p.l = l;
  p.st_h = st_h;
  p.st_w = st_w;
  p.use_h = use_h != 0;
  p.use_w = use_w != 0;
  p.mode = mode;
  p.gen_offset = gen_offset != 0;
  // 16 bytes of input per lane: rows that keep the alignment (V divides W) and 16-byte aligned tensors (the output's groups are then
  // 16 or 8 bytes, aligned as well); anything else takes the element-wise form
  const int V = 16 / si;
  const bool vec = W % V == 0 && aligned16(x) && (reinterpret_cast<uintptr_t>(out) % (size_t)(V * so)) == 0 && (!offset || aligned16(offset));
  // enough waves for 256 compute units (8 per unit and more) before a wave takes more than one row
  const long long strips = ((vec ? W / V : W) + 63) / 64;
  long long rpw = p.rows * strips / (256 * 8);
  p.rows_per_wave = (int)(rpw < 1 ? 1 : (rpw > GM_ROWS_MAX ? GM_ROWS_MAX : rpw));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (in_dtype == GD4D_F32 && out_dtype == GD4D_F32) gm_launch<float, float>(p, vec, st);
  else if (in_dtype == GD4D_F32 && out_dtype == GD4D_F16) gm_launch<float, _Float16>(p, vec, st);
  else if (in_dtype == GD4D_F32) gm_launch<float, gm_bf16>(p, vec, st);
  else if (in_dtype == GD4D_F16) gm_launch<_Float16, _Float16>(p, vec, st);
  else gm_launch<gm_bf16, gm_bf16>(p, vec, st);
  return check_launch();
}

extern "C" int gd4d_grid_mask_draw(uint32_t* state, int32_t* block, int H, double ratio, void* stream) {
  using namespace gd4d;
  if (!state || !block) return GD4D_EINVAL;
  if (H < 3) return GD4D_EINVAL;
  if (!(ratio >= 0.0 && ratio <= 65536.0)) return GD4D_EINVAL;
  hipLaunchKernelGGL(gm_draw_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, block, H, ratio);
  return check_launch();
}
