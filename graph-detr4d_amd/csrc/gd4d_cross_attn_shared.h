// The query front end of the cross-attention kernels, written once.  Five translation units start a query with the same
// work - block -> query, camera matrices and weights into LDS, the softmax of the head logits, the metre-space points, their
// projection and mask, the compacted list of a head's visible items, the bilinear cell of an item on a level - and two of
// them (plus gd4d_detr3d.hip) run its adjoint:
//   gd4d_cross_attn.hip             gather from projected values          gd4d_cross_attn_bwd.hip          its backward
//   gd4d_cross_attn_late.hip        aggregate raw features per head       gd4d_cross_attn_sliced_bwd.hip   the plan's backward
//   gd4d_cross_attn_sliced.hip      plan + channel-sliced gathers         gd4d_detr3d.hip                  projection, softmax_lp, both adjoints
// INVARIANT: every kernel that names a (camera, head, point) entry's visibility, image coordinates, softmax weight or corner
// weights takes them from the helpers below, so the bits agree between kernels by construction: item m of head h in the
// plan's backward IS item m of the plan, and the mask of every forward form is the same bytes.  All units are built with
// -ffp-contract=off: project_camera() reproduces the reference's un-fused fp32 arithmetic bit for bit.
// The helpers take pointers into the caller's LDS; none declares LDS of its own.  Where two callers round differently on
// purpose (the softmax's two summation orders, the corner weight's product order) the helper exposes the choice or the
// factors and each caller keeps what it had.
#pragma once
#include "gd4d_common.h"

namespace gd4d {

struct CrossAttnParams {
  const void* value;
  const float* ref;
  const float* offsets;
  const float* attn_logits;
  const float* cam_logits;
  const float* lidar2img;
  float* out;
  uint8_t* mask_out;
  float* uv_out;
  const int32_t* order;   // optional permutation of [0, B*Q): locality order of the queries (gd4d_query_order_fwd)
  int B, N, Q, L, S, P;
  int raw_cam;         // 1: camera weights are the raw logits (Deform3DCrossAttnMP's neighbour pass), 0: sigmoid
  int head_major;      // value layout: 0 = (B*N, S, Hh, Dh) pixel-major, 1 = (B*N, Hh, S, Dh) head-major planes
  int lvl_h[GD4D_MAX_LEVELS];
  int lvl_w[GD4D_MAX_LEVELS];
  int lvl_start[GD4D_MAX_LEVELS];
  float rng_scale[3];  // float(double(hi) - double(lo))
  float rng_lo[3];     // float(lo)
  float img_h, img_w;
  float* agg;          // gd4d_cross_attn_agg_fwd only: (B*Q, Hh, C) per-head aggregates of the raw features
  float* wsum;         //                               (B*Q, Hh) sum of the in-bounds sampling weights per head
  const float* vp_w;   // gd4d_cross_attn_agg_fwd, optional: value_proj weight (C, C) / bias (C) applied to the aggregates in
  const float* vp_b;   //   the kernel's epilogue: out (B*Q, C) = W_h agg_h + b_h wsum_h  (agg / wsum may then be NULL)
  unsigned dbg_wrap;   // dev (GD4D_AGG_DBG_WRAP): pixel indices are ANDed with this mask (0 = off): an all-L2-hit run
};

constexpr int kPoints = 4;   // sampling points per head (reference configs: num_points=4)
constexpr int kChannels = 256;
constexpr float kDepthEps = 1e-5f;   // a point is in front of a camera when its depth exceeds this

// ---- projection of one metre-space point by rows 0-2 of a lidar2img matrix ---------------------
// Order of operations is the reference's torch-CPU arithmetic:
//   c = ((m0*X + m1*Y) + m2*Z) + m3;  u = (cx / max(cz, eps)) / W;  v = (cy / max(cz, eps)) / H; all IEEE, no contraction
// (HIP's __fmul_rn/__fadd_rn are plain operators that the compiler would otherwise contract into v_fma_f32: seen in the ISA).
// The visibility rule is the caller's: project_entry's below, gd4d_detr3d.hip's on u, v mapped to [-1, 1].
__device__ __forceinline__ void project_camera(const float* __restrict__ m, float X, float Y, float Z, float img_w, float img_h,
                                               float& cx, float& cy, float& cz, float& u, float& v) {
  cx = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
  cy = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
  cz = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
  const float zc = fmaxf(cz, kDepthEps);
  u = (cx / zc) / img_w;         // IEEE-correct division (v_div_scale/fmas/fixup)
  v = (cy / zc) / img_h;
}

// Deform3DCrossAttn's rule (:240-258): in front of the camera and strictly inside the image
__device__ __forceinline__ bool in_image(float cz, float u, float v) {
  return cz > kDepthEps && (u > 0.f) && (u < 1.f) && (v > 0.f) && (v < 1.f);
}

template <class P>
__device__ __forceinline__ bool project_entry(const P& p, const float* __restrict__ m, float X, float Y, float Z, float& u, float& v) {
  float cx, cy, cz;
  project_camera(m, X, Y, Z, p.img_w, p.img_h, cx, cy, cz, u, v);
  return in_image(cz, u, v);
}

// Adjoint of project_camera for a point in front of the camera: (gu, gv) = dL/d(u, v) -> g = dL/d(X, Y, Z).
// u = cx / (cz Wimg), v = cy / (cz Himg); iz = 1 / cz (a caller that also runs invisible points, gu = gv = 0, passes 0).
__device__ __forceinline__ void project_adjoint(const float* __restrict__ m, float cx, float cy, float iz, float gu, float gv,
                                                float img_w, float img_h, float g[3]) {
  const float gcx = gu * iz / img_w;
  const float gcy = gv * iz / img_h;
  const float gcz = -(gu * cx * iz * iz / img_w + gv * cy * iz * iz / img_h);
  g[0] = gcx * m[0] + gcy * m[4] + gcz * m[8];
  g[1] = gcx * m[1] + gcy * m[5] + gcz * m[9];
  g[2] = gcx * m[2] + gcy * m[6] + gcz * m[10];
}

template <typename VT> struct Quad;  // 4 consecutive channels of one pixel/head
template <> struct Quad<float> {
  static __device__ __forceinline__ float4 load(const float* p) { return *reinterpret_cast<const float4*>(p); }
};
template <> struct Quad<uint16_t> {
  static __device__ __forceinline__ float4 load(const uint16_t* p) {
    uint2 r = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u),
                       __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u));
  }
};

// ---- block -> query -----------------------------------------------------------------------------
// Workgroup i runs on XCD i % 8 (round-robin dispatch), each XCD with a private L2.  With a locality order of the queries
// every XCD takes a contiguous range of it, so queries that look at the same camera region share an L2 (the backward's
// atomic adds meet there like the forward's reads).  False: this workgroup has no query.  EXACT_GRID: without an order the
// grid is exactly B*Q workgroups (no test).
template <bool EXACT_GRID>
__device__ __forceinline__ bool query_of_block(const int32_t* __restrict__ order, int nq, int& bq) {
  bq = blockIdx.x;
  if (order) {
    const int per_xcd = (nq + 7) >> 3;
    const int pos = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per_xcd || pos >= nq) return false;
    bq = order[pos];
  } else if (!EXACT_GRID && bq >= nq) {
    return false;
  }
  return true;
}

// ---- cameras ------------------------------------------------------------------------------------
template <class P>
__device__ __forceinline__ float camera_weight(const P& p, float cl) { return p.raw_cam ? cl : 1.0f / (1.0f + expf(-cl)); }

// camera n's logit of query (b, q): cam_logits is read in the reference's raw-view scramble (:211-212)
template <class P>
__device__ __forceinline__ float camera_logit(const P& p, int b, int q, int n) {
  return p.cam_logits[(size_t)b * p.Q * p.N + (size_t)n * p.Q + q];
}

// rows 0-2 of the sample's N lidar2img matrices -> s_mat [N][12] (once through LDS instead of 12 global loads per entry)
template <int THREADS, class P>
__device__ __forceinline__ void stage_matrices(const P& p, int b, float* s_mat) {
  for (int i = threadIdx.x; i < p.N * 12; i += THREADS) s_mat[i] = p.lidar2img[((size_t)b * p.N + i / 12) * 16 + i % 12];
}

template <int THREADS, class P>
__device__ __forceinline__ void stage_cameras(const P& p, int b, int q, float* s_mat, float* s_cw) {
  stage_matrices<THREADS>(p, b, s_mat);
  if (threadIdx.x < p.N) s_cw[threadIdx.x] = camera_weight(p, camera_logit(p, b, q, threadIdx.x));
}

// ---- softmax over the L * P logits of a head ----------------------------------------------------
__device__ __forceinline__ void softmax_lp(const float* __restrict__ logits, int n, float* w) {
  float mx = logits[0];
  for (int i = 1; i < n; ++i) mx = fmaxf(mx, logits[i]);
  float sum = 0.f;
  for (int i = 0; i < n; ++i) { w[i] = expf(logits[i] - mx); sum += w[i]; }
  float inv = 1.0f / sum;
  for (int i = 0; i < n; ++i) w[i] *= inv;
}

// can SHUFFLE be chosen at all (the callers add their own conditions: they do not agree, and the two paths round the sum
// differently, so every kernel keeps the choice it has)
constexpr bool softmax_can_shuffle(int lp) { return (lp & (lp - 1)) == 0 && lp <= 32; }
// the plan and its backward (one rule for both: same weights bit for bit): their [B][HH][LP] table is walked by a loop of
// whole waves
template <int HH, int LP> constexpr bool kPlanSoftmaxShuffles = softmax_can_shuffle(LP) && (HH * LP) % GD4D_WAVE == 0;

// s_aw [nb][HH][LP] = softmax of the logits at logits + bb * batch_stride + hd * n_lp, bb < nb.  SHUFFLE: one thread per
// logit (n_lp == LP, a power of two <= 32), groups of LP lanes reduce with xor shuffles; nb * HH * LP is a multiple of the
// wave or at most THREADS.  Otherwise one thread per (bb, head) runs softmax_lp over n_lp <= LP logits.
template <int HH, int LP, bool SHUFFLE, int THREADS>
__device__ __forceinline__ void head_softmax_to_lds(const float* __restrict__ logits, size_t batch_stride, int nb, int n_lp, float* s_aw) {
  if (SHUFFLE) {
    for (int t = threadIdx.x; t < nb * HH * LP; t += THREADS) {
      const int bh = t / LP, i = t % LP;
      const int bb = bh / HH, hd = bh - bb * HH;
      const float x = logits[(size_t)bb * batch_stride + hd * LP + i];
      float mx = x;
#pragma unroll
      for (int o = 1; o < LP; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      const float e = expf(x - mx);
      float sum = e;
#pragma unroll
      for (int o = 1; o < LP; o <<= 1) sum += __shfl_xor(sum, o);
      s_aw[t] = e * (1.0f / sum);
    }
  } else {
    for (int t = threadIdx.x; t < nb * HH; t += THREADS) {
      const int bb = t / HH, hd = t - bb * HH;
      float w[LP];
      softmax_lp(logits + (size_t)bb * batch_stride + hd * n_lp, n_lp, w);
#pragma unroll
      for (int i = 0; i < LP; ++i)
        if (i < n_lp) s_aw[t * LP + i] = w[i];
    }
  }
}

// ---- metre-space points and their projection ----------------------------------------------------
// point hp = (head, point) of query bq: two roundings, then the offset (:222-229)
template <int E, class P>
__device__ __forceinline__ void query_point(const P& p, int bq, int hp, float& X, float& Y, float& Z) {
  const float* rp = p.ref + (size_t)bq * 3;
  const float* offs = p.offsets + ((size_t)bq * E + hp) * 3;
  X = (rp[0] * p.rng_scale[0] + p.rng_lo[0]) + offs[0];
  Y = (rp[1] * p.rng_scale[1] + p.rng_lo[1]) + offs[1];
  Z = (rp[2] * p.rng_scale[2] + p.rng_lo[2]) + offs[2];
}

struct NoWaveHook { __device__ __forceinline__ void operator()(int, bool) const {} };

// Entry e = (camera, head, point) of the query -> s_uv [N][E] ((-1, -1): not visible) and, with OUTPUTS, mask_out / uv_out.
// X, Y, Z: the point of thread's (head, point) = threadIdx.x % E, which never changes between its entries.  s_mat must be
// visible to the workgroup.  hook(e0, vis) runs once per wave iteration on all lanes (E consecutive entries are one camera).
template <int E, int THREADS, bool OUTPUTS = true, class P, class Hook = NoWaveHook>
__device__ __forceinline__ void project_query(const P& p, int b, int q, const float* s_mat, float2* s_uv, float X, float Y, float Z,
                                              Hook hook = Hook()) {
  static_assert(E <= GD4D_WAVE && GD4D_WAVE % E == 0 && THREADS % E == 0, "a thread keeps its (head, point)");
  const int total = p.N * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hp = threadIdx.x % E;
  for (int e0 = wave * GD4D_WAVE; e0 < total; e0 += THREADS) {
    const int e = e0 + lane;
    bool vis = false;
    if (e < total) {
      const int n = e / E;
      float u, v;
      vis = project_entry(p, s_mat + n * 12, X, Y, Z, u, v);
      s_uv[e] = vis ? make_float2(u, v) : make_float2(-1.f, -1.f);
      if (OUTPUTS) {
        const size_t o = (((size_t)b * p.N + n) * p.Q + q) * E + hp;
        if (p.mask_out) p.mask_out[o] = vis ? 1 : 0;
        if (p.uv_out) { p.uv_out[o * 2] = u; p.uv_out[o * 2 + 1] = v; }
      }
    }
    hook(e0, vis);
  }
}

// release / acquire of a wave-private LDS region: no workgroup barrier
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The calling wave compacts head h's visible (camera, point) pairs, in candidate order camera * PT + point, into its own
// list items[] = {u, v, (b * N + camera) * PT + point, camera weight}; returns their number.  The list is fenced for the wave.
template <int PT>
__device__ __forceinline__ int compact_head_items(const float2* s_uv, const float* s_cw, int E, int N, int b, int h, float4* items) {
  const int lane = threadIdx.x & 63;
  const int ncand = N * PT;
  int M = 0;
  for (int c0 = 0; c0 < ncand; c0 += GD4D_WAVE) {
    const int cand = c0 + lane;
    const int n = min(cand, ncand - 1) / PT, k = cand % PT;
    const float2 uvc = s_uv[n * E + h * PT + k];
    const bool vis = cand < ncand && uvc.x >= 0.f;
    const unsigned long long bal = __ballot(vis);
    if (vis) items[M + __popcll(bal & ((1ull << lane) - 1ull))] = make_float4(uvc.x, uvc.y, __int_as_float((b * N + n) * PT + k), s_cw[n]);
    M += __popcll(bal);
  }
  wave_lds_fence();
  return M;
}

// ---- the bilinear cell of image point (u, v) on a W x H level (mmcv MSDA: align_corners=False, zero padding) -------------
// Corner c = (x0 + (c & 1), y0 + (c >> 1)).  The cell exposes the factors; a caller forms its products in its own order
// (((1-dx)*(1-dy)) and ((wl*wx)*wy)*in round differently).
struct BilinearCell {
  int x0, y0;
  float dx, dy;
  __device__ __forceinline__ BilinearCell(float u, float v, float W, float H) {
    const float x = fmaf(u, W, -0.5f);
    const float y = fmaf(v, H, -0.5f);
    const float xf = floorf(x), yf = floorf(y);
    dx = x - xf; dy = y - yf;
    x0 = (int)xf; y0 = (int)yf;
  }
  // clamped form: corners outside the map contribute 0 (zero padding); their loads are clamped onto the map
  struct Corner {
    int xi, yi, xc, yc;
    bool in;          // on the map
    float wx, wy;
  };
  __device__ __forceinline__ Corner corner(int c, int W, int H) const {
    Corner k;
    k.xi = x0 + (c & 1); k.yi = y0 + (c >> 1);
    k.xc = min(max(k.xi, 0), W - 1); k.yc = min(max(k.yi, 0), H - 1);
    k.in = k.xc == k.xi && k.yc == k.yi;
    k.wx = (c & 1) ? dx : 1.f - dx; k.wy = (c >> 1) ? dy : 1.f - dy;
    return k;
  }
  // four-bits form: 1 = x0 on the map, 2 = x0 + 1, 4 = y0, 8 = y0 + 1 (corner_ok below)
  __device__ __forceinline__ unsigned ok_bits(int W, int H) const {
    const bool x0ok = x0 >= 0, x1ok = x0 + 1 < W;
    const bool y0ok = y0 >= 0, y1ok = y0 + 1 < H;
    return (x0ok ? 1u : 0u) | (x1ok ? 2u : 0u) | (y0ok ? 4u : 0u) | (y1ok ? 8u : 0u);
  }
  // the four corner weights (1-dx)(1-dy), dx(1-dy), (1-dx)dy, dx dy
  __device__ __forceinline__ void weights(float bw[4]) const {
    bw[0] = (1.f - dx) * (1.f - dy); bw[1] = dx * (1.f - dy); bw[2] = (1.f - dx) * dy; bw[3] = dx * dy;
  }
};
__device__ __forceinline__ bool corner_ok(unsigned bits, int c) {
  const unsigned need = (1u << (c & 1)) | (4u << (c >> 1));
  return (bits & need) == need;
}

// The four corners of one (item, level) of the sliced gather as {byte offset inside the level, weight} pairs: corner c goes to
// dst[c * stride] when `store`.  wl = softmax weight x camera weight; live = 1 / 0 (an item past the list's end or a level slot
// that is off weighs 0 but keeps its clamped address: its line is in flight already).  The plan's pairs form and the items
// gather's step run exactly this, so their pairs and wsum agree bit for bit.
__device__ __forceinline__ void corner_pairs(const BilinearCell& cell, int lw, int lh, float wl, float live, unsigned rbase,
                                             unsigned pix_stride, bool store, uint2* dst, int stride, float& wsum_lane) {
#pragma unroll
  for (int c_of = 0; c_of < 4; ++c_of) {
    const BilinearCell::Corner k = cell.corner(c_of, lw, lh);
    const float in = k.in ? live : 0.f;
    const float w = (wl * k.wx * k.wy) * in;
    const unsigned off = rbase + (unsigned)(k.yc * lw + k.xc) * pix_stride;
    wsum_lane += w;
    if (store) dst[c_of * stride] = make_uint2(off, __float_as_uint(w));
  }
}

// Backward of the cell: d[c] = dL/d(corner c's weight) (0 for a corner outside the map) -> T = sum_c bw_c d_c and its
// derivatives by x and y (pixel units).  Cell: BilinearCell, or gd4d_detr3d.hip's GridCell - anything with dx, dy and weights().
template <class Cell>
__device__ __forceinline__ void bilinear_adjoint(const Cell& cell, const float d[4], float& T, float& dTdx, float& dTdy) {
  const float dx = cell.dx, dy = cell.dy;
  float bw[4];
  cell.weights(bw);
  T = (bw[0] * d[0] + bw[1] * d[1]) + (bw[2] * d[2] + bw[3] * d[3]);
  dTdx = (1.f - dy) * (d[1] - d[0]) + dy * (d[3] - d[2]);
  dTdy = (1.f - dx) * (d[2] - d[0]) + dx * (d[3] - d[1]);
}

}  // namespace gd4d
