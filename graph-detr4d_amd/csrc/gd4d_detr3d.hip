// gd4d_detr3d_fwd / _bwd and gd4d_detr3d_v2_fwd / _bwd: the sampling cores of DETR3D's two cross-attention modules for gfx950,
// forward and backward.  SURVEY.md Appendix A.2.
//   v1  feature_sampling (detr3d_transformer.py:397-438) fused with the sigmoid weighting and the sum over cameras and levels
//       of Detr3DCrossAtten.forward (:373-383)
//   v2  Detr3DCrossAttenV2 (:441-710), the 2-D-offset deformable variant
//
// The feature maps stay in the layout the reference's caller provides: per level (B*N, C, H, W) NCHW.  One workgroup = one
// (batch, query); thread c = channel c, so every global load of a wave walks 64 channel planes at the same (y, x): strided by
// H*W floats, but only the few pixels a query projects to are ever touched (about 1 camera x 4 levels x 4 corners per query),
// which is far less traffic than re-laying-out the whole pyramid first.  The projection is spread over the first N threads
// (bit-exact arithmetic, translation unit built with -ffp-contract=off).
//
// What the four kernels share is written once: the parameters every one of them reads (Detr3dCommon, filled and validated
// by fill_common), the query front end (project_cameras_fwd / _bwd over camera_grid_point) and the grid-sample cell
// (GridCell).  From gd4d_cross_attn_shared.h come project_camera, project_adjoint, softmax_lp and bilinear_adjoint.
#include "gd4d_common.h"
#include "gd4d_cross_attn_shared.h"

namespace gd4d {

// what every kernel of this unit reads; each kernel's struct adds its own outputs and operands
struct Detr3dCommon {
  const float* feats[GD4D_MAX_LEVELS];
  const float* ref;
  const float* attn_logits;   // v1: (B, Q, N, P=1, L); v2: (B, Q, N, Hh, L*P)
  const float* lidar2img;
  int B, N, Q, C, L;
  int lvl_h[GD4D_MAX_LEVELS];
  int lvl_w[GD4D_MAX_LEVELS];
  float rng_scale[3];
  float rng_lo[3];
  float img_h, img_w;
};

struct Detr3dParams : Detr3dCommon {
  float* out;                 // (B, Q, C) or null
  uint8_t* mask_out;          // (B, N, Q) or null
  float* sampled_out;         // (B, C, Q, N, 1, L) or null
};

struct Detr3dV2Params : Detr3dCommon {
  const float* offsets;       // (B, Q, N, Hh, L, P, 2) pixels of the level
  float* out;                 // (B, Q, C)
  uint8_t* mask_out;          // (B, N, Q) or null
  int Hh;
};

struct Detr3dBwdParams : Detr3dCommon {
  float* gfeats[GD4D_MAX_LEVELS];   // zero-initialised by the caller, or NULL
  const float* grad_out;            // (B, Q, C)
  float* grad_logits;               // v1: (B, Q, N, 1, L); v2: (B, Q, N, Hh, L*P)
  float* grad_ref;                  // (B, Q, 3) or NULL
};

struct Detr3dV2BwdParams : Detr3dBwdParams {
  const float* offsets;             // (B, Q, N, Hh, L, P, 2)
  float* grad_offsets;              // (B, Q, N, Hh, L, P, 2)
  int Hh;
};

// ---- the query front end ----------------------------------------------------------------------------------------------
// project_camera, then DETR3D's own rule (detr3d_transformer.py:421, :676): u, v mapped to grid coordinates in [-1, 1]; visible =
// in front of the camera and strictly inside
__device__ __forceinline__ bool project_grid(const float* __restrict__ m, float X, float Y, float Z, float img_w, float img_h,
                                             float& cx, float& cy, float& cz, float& u, float& v) {
  project_camera(m, X, Y, Z, img_w, img_h, cx, cy, cz, u, v);
  u = (u - 0.5f) * 2.f;
  v = (v - 0.5f) * 2.f;
  return cz > kDepthEps && (u > -1.f) && (u < 1.f) && (v > -1.f) && (v < 1.f);
}

// reference point of query bq -> metres -> camera n of sample b: camera coordinates, grid coordinates, visibility
template <class P>
__device__ __forceinline__ bool camera_grid_point(const P& p, int b, int bq, int n, float& cx, float& cy, float& cz, float2& g) {
  const float* rp = p.ref + (size_t)bq * 3;
  const float X = rp[0] * p.rng_scale[0] + p.rng_lo[0];
  const float Y = rp[1] * p.rng_scale[1] + p.rng_lo[1];
  const float Z = rp[2] * p.rng_scale[2] + p.rng_lo[2];
  return project_grid(p.lidar2img + ((size_t)b * p.N + n) * 16, X, Y, Z, p.img_w, p.img_h, cx, cy, cz, g.x, g.y);
}

// Thread n < N projects camera n.  The forward kernels keep s_uv [N], s_vis [N] and write mask_out if there is one ...
template <class P>
__device__ __forceinline__ void project_cameras_fwd(const P& p, int b, int q, float2* s_uv, int* s_vis) {
  const int n = threadIdx.x;
  if (n < p.N) {
    float cx, cy, cz;
    float2 g;
    const bool vis = camera_grid_point(p, b, b * p.Q + q, n, cx, cy, cz, g);
    s_uv[n] = g;
    s_vis[n] = vis ? 1 : 0;
    if (p.mask_out) p.mask_out[((size_t)b * p.N + n) * p.Q + q] = vis ? 1 : 0;
  }
  __syncthreads();
}

// ... the backward kernels s_uv [N], s_cam [N][4] = cx, cy, cz, vis (the projection's adjoint needs them), and clear s_pt [3]
template <class P>
__device__ __forceinline__ void project_cameras_bwd(const P& p, int b, int bq, float2* s_uv, float* s_cam, float* s_pt) {
  const int n = threadIdx.x;
  if (n < p.N) {
    float cx, cy, cz;
    float2 g;
    const bool vis = camera_grid_point(p, b, bq, n, cx, cy, cz, g);
    s_uv[n] = g;
    s_cam[4 * n] = cx; s_cam[4 * n + 1] = cy; s_cam[4 * n + 2] = cz; s_cam[4 * n + 3] = vis ? 1.f : 0.f;
  }
  if (n < 3) s_pt[n] = 0.f;
  __syncthreads();
}

// thread 0, visible camera n: dL/d(u, v) in [0, 1] image units -> metres, added to s_pt
template <class P>
__device__ __forceinline__ void add_point_gradient(const P& p, int b, int n, const float* s_cam, float gu, float gv, float* s_pt) {
  const float* m = p.lidar2img + ((size_t)b * p.N + n) * 16;
  const float cx = s_cam[4 * n], cy = s_cam[4 * n + 1], cz = s_cam[4 * n + 2];
  float gp[3];
  project_adjoint(m, cx, cy, 1.0f / cz, gu, gv, p.img_w, p.img_h, gp);   // visible: cz > eps
  s_pt[0] += gp[0]; s_pt[1] += gp[1]; s_pt[2] += gp[2];
}

// ---- the grid-sample cell -----------------------------------------------------------------------------------------------
// ATen grid_sampler, bilinear / zeros / align_corners=False, on grid coordinate g in [-1, 1]:
//   x = ((g + 1) * size - 1) / 2 ; corners floor(x), floor(x)+1 ; out-of-map corners contribute 0.
// Corner c = (x0 + (c & 1), y0 + (c >> 1)), (x0, y0) = (xf, yf).  Not BilinearCell: that one takes image coordinates through
// fmaf(u, W, -0.5f) and compares integers; here the corners are tested in float and only a corner on the map is ever cast to
// int, because far-away points exceed the int range.
// The forward's sample() adds its four terms in sequence, the backward's value (bilinear_adjoint's T over taps()) adds
// them pairwise: they round differently, and each caller keeps what it had.
struct GridCell {
  float dx, dy;
  float xf, yf;                    // floor(x), floor(y): corner 0, still in float
  bool x0ok, x1ok, y0ok, y1ok;
  __device__ __forceinline__ GridCell(float gx, float gy, int W, int H) {
    const float x = ((gx + 1.f) * (float)W - 1.f) / 2.f, y = ((gy + 1.f) * (float)H - 1.f) / 2.f;
    xf = floorf(x); yf = floorf(y);
    dx = x - xf; dy = y - yf;
    x0ok = xf >= 0.f && xf <= (float)(W - 1); x1ok = xf + 1.f >= 0.f && xf + 1.f <= (float)(W - 1);
    y0ok = yf >= 0.f && yf <= (float)(H - 1); y1ok = yf + 1.f >= 0.f && yf + 1.f <= (float)(H - 1);
  }
  __device__ __forceinline__ bool any() const { return (x0ok || x1ok) && (y0ok || y1ok); }
  __device__ __forceinline__ bool ok(int c) const { return ((c & 1) ? x1ok : x0ok) && ((c >> 1) ? y1ok : y0ok); }
  // corner c's index in a plane; only for a corner that is on the map (ok(c)): that is what makes the int casts defined
  __device__ __forceinline__ int at(int c, int W) const { return ((int)yf + (c >> 1)) * W + (int)xf + (c & 1); }
  __device__ __forceinline__ float wx(int c) const { return (c & 1) ? dx : 1.f - dx; }
  __device__ __forceinline__ float wy(int c) const { return (c >> 1) ? dy : 1.f - dy; }
  // the four corner weights (1-dx)(1-dy), dx(1-dy), (1-dx)dy, dx dy
  __device__ __forceinline__ void weights(float bw[4]) const {
#pragma unroll
    for (int c = 0; c < 4; ++c) bw[c] = wx(c) * wy(c);
  }
  // the bilinear sample of one channel plane
  __device__ __forceinline__ float sample(const float* __restrict__ plane, int W) const {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (ok(c)) s += wx(c) * wy(c) * plane[at(c, W)];
    return s;
  }
  // the four corner values, 0 outside the map
  __device__ __forceinline__ void taps(const float* __restrict__ plane, int W, float v[4]) const {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = ok(c) ? plane[at(c, W)] : 0.f;
  }
  // gplane[corner c] += (gw * wx) * wy
  __device__ __forceinline__ void scatter(float* gplane, int W, float gw) const {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (ok(c)) atomicAdd(gplane + at(c, W), gw * wx(c) * wy(c));
  }
};

// s_w [N][Hh][L*P] of the v2 kernels: softmax over level x point per (camera, head), zeros for an invisible camera
template <class P, class Vis>
__device__ __forceinline__ void head_weights_to_lds(const P& p, int bq, int LP, float* s_w, Vis visible) {
  for (int e = threadIdx.x; e < p.N * p.Hh; e += blockDim.x) {     // one thread per (camera, head)
    float* w = s_w + (size_t)e * LP;
    if (visible(e / p.Hh)) softmax_lp(p.attn_logits + ((size_t)bq * p.N * p.Hh + e) * LP, LP, w);
    else for (int i = 0; i < LP; ++i) w[i] = 0.f;
  }
  __syncthreads();
}

// ---- v1 forward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detr3d_fwd_kernel(const Detr3dParams p) {
  extern __shared__ float s_mem[];
  float2* s_uv = reinterpret_cast<float2*>(s_mem);            // [N] grid coords in [-1,1]
  float* s_w = s_mem + 2 * p.N;                               // [N*L] sigmoid(logit) * vis
  int* s_vis = reinterpret_cast<int*>(s_w + p.N * p.L);       // [N]

  const int bq = blockIdx.x;
  const int b = bq / p.Q, q = bq - b * p.Q;
  const int t = threadIdx.x;

  project_cameras_fwd(p, b, q, s_uv, s_vis);
  for (int e = t; e < p.N * p.L; e += blockDim.x) {
    const int n = e / p.L;
    const float lg = p.attn_logits[(size_t)bq * p.N * p.L + e];
    s_w[e] = s_vis[n] ? 1.0f / (1.0f + expf(-lg)) : 0.f;
  }
  __syncthreads();

  const bool want_all = p.sampled_out != nullptr;     // feature_sampling() returns every camera
  for (int c = t; c < p.C; c += blockDim.x) {
    float acc = 0.f;
    for (int n = 0; n < p.N; ++n) {
      if (!want_all && !s_vis[n]) continue;                   // workgroup-uniform
      const float2 g = s_uv[n];
      for (int l = 0; l < p.L; ++l) {
        const int H = p.lvl_h[l], W = p.lvl_w[l];
        const GridCell cell(g.x, g.y, W, H);
        const float s = cell.any() ? cell.sample(p.feats[l] + ((size_t)(b * p.N + n) * p.C + c) * H * W, W) : 0.f;
        if (want_all)
          p.sampled_out[((((size_t)b * p.C + c) * p.Q + q) * p.N + n) * p.L + l] = s;
        acc = fmaf(s_w[n * p.L + l], s, acc);
      }
    }
    if (p.out) p.out[(size_t)bq * p.C + c] = acc;
  }
}

// ---- v2 forward ---------------------------------------------------------------------------------------------------------
// Same work mapping as above (workgroup = query, thread = channel, NCHW maps untouched); head h = c / Dh reads its
// own sampling locations: grid coordinate of the projected reference point + offset / (W_l, H_l) (:696-700), weights =
// softmax over level x point per (camera, head) times the camera's visibility (:602-611, :617).
// Quirk reproduced: the reference stacks samples as (..., point, level) and multiplies them with weights laid out
// (..., level, point) (:611 against :705-707), so the sample at (point i, level j) meets weight (level i, point j) -
// well-formed only for num_levels == num_points, which the host enforces.
__global__ __launch_bounds__(256) void detr3d_v2_fwd_kernel(const Detr3dV2Params p) {
  extern __shared__ float s_mem[];
  const int LP = p.L * p.L;                                   // num_points == num_levels
  float2* s_uv = reinterpret_cast<float2*>(s_mem);            // [N] grid coords in [-1,1]
  float* s_w = s_mem + 2 * p.N;                               // [N][Hh][L*P] softmax * vis
  int* s_vis = reinterpret_cast<int*>(s_w + p.N * p.Hh * LP); // [N]
  const int bq = blockIdx.x;
  const int b = bq / p.Q, q = bq - b * p.Q;
  const int t = threadIdx.x;
  project_cameras_fwd(p, b, q, s_uv, s_vis);
  head_weights_to_lds(p, bq, LP, s_w, [&](int n) { return s_vis[n] != 0; });
  const int Dh = p.C / p.Hh;
  for (int c = t; c < p.C; c += blockDim.x) {
    const int h = c / Dh;
    float acc = 0.f;
    for (int n = 0; n < p.N; ++n) {
      if (!s_vis[n]) continue;                                // workgroup-uniform
      const float2 g = s_uv[n];
      const float* w = s_w + ((size_t)n * p.Hh + h) * LP;
      const float* off = p.offsets + (((size_t)bq * p.N + n) * p.Hh + h) * LP * 2;
      for (int l = 0; l < p.L; ++l) {
        const int H = p.lvl_h[l], W = p.lvl_w[l];
        const float* plane = p.feats[l] + ((size_t)(b * p.N + n) * p.C + c) * H * W;
        for (int pt = 0; pt < p.L; ++pt) {
          const GridCell cell(g.x + off[(l * p.L + pt) * 2] / (float)W, g.y + off[(l * p.L + pt) * 2 + 1] / (float)H, W, H);   // :699-700
          const float s = cell.any() ? cell.sample(plane, W) : 0.f;
          acc = fmaf(w[pt * p.L + l], s, acc);                // weight of (level = pt, point = l): the reference's pairing
        }
      }
    }
    p.out[(size_t)bq * p.C + c] = acc;
  }
}

// ---- v1 backward --------------------------------------------------------------------------------------------------------
// Backward of detr3d_fwd_kernel's `out` (the reference: autograd through feature_sampling's F.grid_sample per level, the
// sigmoid weights, the mask product and the sums, detr3d_transformer.py:373-383, :397-438).
// Same work mapping (workgroup = (batch, query), thread = channel).  With g = dL/d out (C), w = sigmoid(logit) * vis and
// s[c, n, l] the bilinear sample:
//   dL/d feats[l][b*N+n, c, corner] += g[c] w[n,l] b_corner                (atomic fp32 add; ~1 camera x L levels x 4 corners)
//   dL/d logit[n,l] = vis w (1 - w) sum_c g[c] s[c,n,l]
//   dL/d (x, y)     = w sum_c g[c] ds/d(x, y)  (pixel units) -> grid coordinate -> u = cx / (cz W_img), v = cy / (cz H_img)
//                     -> lidar2img -> metres -> reference point.  The mask is piecewise constant (no gradient).
// The sums over channels meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void detr3d_bwd_kernel(const Detr3dBwdParams p) {
  extern __shared__ float s_mem[];
  float2* s_uv = reinterpret_cast<float2*>(s_mem);            // [N]
  float* s_cam = s_mem + 2 * p.N;                             // [N][4]: cx, cy, cz, vis
  float* s_red = s_cam + 4 * p.N;                             // [4 waves][3]
  float* s_pt = s_red + 12;                                   // [3] dL/d (metre point), accumulated by thread 0
  const int bq = blockIdx.x;
  const int b = bq / p.Q;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  project_cameras_bwd(p, b, bq, s_uv, s_cam, s_pt);
  // (any C: thread t owns channels t, t + 256, ...; every one of them adds into part[] before the reduction, so there is no
  //  limit on C here and the host sets none - C = 320 and C = 100 are tested as kernels, tests/test_detr3d_kernels_gpu.py)
  for (int n = 0; n < p.N; ++n) {
    const bool vis = s_cam[4 * n + 3] != 0.f;                 // workgroup-uniform
    if (!vis) {
      if (t < p.L) p.grad_logits[((size_t)bq * p.N + n) * p.L + t] = 0.f;
      continue;
    }
    const float2 g2 = s_uv[n];
    float gu = 0.f, gv = 0.f;                                 // dL/d(u, v) in [0, 1] image units, summed over the levels (thread 0)
    for (int l = 0; l < p.L; ++l) {
      const int H = p.lvl_h[l], W = p.lvl_w[l];
      const GridCell cell(g2.x, g2.y, W, H);
      const float lg = p.attn_logits[((size_t)bq * p.N + n) * p.L + l];
      const float w = 1.0f / (1.0f + expf(-lg));
      float part[3] = {0.f, 0.f, 0.f};                        // sum_c g s, sum_c g ds/dx, sum_c g ds/dy
      if (cell.any()) {
        for (int c = t; c < p.C; c += 256) {
          const size_t plane = ((size_t)(b * p.N + n) * p.C + c) * H * W;
          const float g = p.grad_out[(size_t)bq * p.C + c];
          float v[4], T, dTdx, dTdy;
          cell.taps(p.feats[l] + plane, W, v);
          bilinear_adjoint(cell, v, T, dTdx, dTdy);
          part[0] += g * T;
          part[1] += g * dTdx;
          part[2] += g * dTdy;
          if (p.gfeats[l]) cell.scatter(p.gfeats[l] + plane, W, g * w);
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) part[k] = wave_sum(part[k]);
      __syncthreads();                                        // (s_red of the previous level has been read)
      if (lane == 0) { s_red[wave * 3] = part[0]; s_red[wave * 3 + 1] = part[1]; s_red[wave * 3 + 2] = part[2]; }
      __syncthreads();
      if (t == 0) {
        float tot[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) tot[k] = ((s_red[k] + s_red[3 + k]) + s_red[6 + k]) + s_red[9 + k];
        p.grad_logits[((size_t)bq * p.N + n) * p.L + l] = w * (1.f - w) * tot[0];
        // x = ((gx + 1) W - 1) / 2, gx = (u - 0.5) 2  ->  dx/du = W ; likewise dy/dv = H
        gu += w * tot[1] * (float)W;
        gv += w * tot[2] * (float)H;
      }
    }
    if (t == 0) add_point_gradient(p, b, n, s_cam, gu, gv, s_pt);
  }
  __syncthreads();
  if (t < 3 && p.grad_ref) p.grad_ref[(size_t)bq * 3 + t] = s_pt[t] * p.rng_scale[t];
}

// ---- v2 backward --------------------------------------------------------------------------------------------------------
// Backward of detr3d_v2_fwd_kernel (the reference: autograd through Detr3DCrossAttenV2's per-level F.grid_sample of every
// head's channel slice, the softmax over level x point, the (point, level) x (level, point) pairing and the sums,
// detr3d_transformer.py:597-710).  Same work mapping as the forward (workgroup = (batch, query), thread = channel,
// head h = c / Dh).  With g = dL/d out (C), W[n,h,i] = softmax_i(logits[n,h,:]) * vis[n] and
// s[c,n,l,pt] the bilinear sample of channel c at grid g_n + offsets[n,h,l,pt] / (W_l, H_l):
//   dL/d feats[l][b*N+n, c, corner] += g[c] W[n,h,pt*L+l] b_corner               (atomic fp32 add)
//   dL/d W[n,h,pt*L+l]   = sum_{c in h} g[c] s[c,n,l,pt]      ->  softmax backward -> dL/d logits[n,h,:]
//   dL/d offsets[n,h,l,pt] = W[n,h,pt*L+l] sum_{c in h} g[c] ds/d(x, y) / 2       (x = ((gx + 1) W - 1) / 2, gx = g.x + off / W)
//   dL/d g_n = sum_{h,l,pt} W sum_c g ds/d(x, y) (W_l, H_l) / 2  -> u, v -> lidar2img -> metres -> reference point
// The sums over a head's channels meet in LDS in channel order (deterministic).  C <= 256.
__global__ __launch_bounds__(256) void detr3d_v2_bwd_kernel(const Detr3dV2BwdParams p) {
  extern __shared__ float s_mem[];
  const int LP = p.L * p.L;                                   // num_points == num_levels
  float2* s_uv = reinterpret_cast<float2*>(s_mem);            // [N]
  float* s_cam = s_mem + 2 * p.N;                             // [N][4]: cx, cy, cz, vis
  float* s_w = s_cam + 4 * p.N;                               // [N][Hh][LP] softmax (zeros for an invisible camera)
  float* s_part = s_w + p.N * p.Hh * LP;                      // [3][256]
  float* s_dw = s_part + 3 * 256;                             // [Hh][LP] dL/dW of the current camera
  float* s_g = s_dw + p.Hh * LP;                              // [Hh][2] dL/d(grid x, y) of the current camera, per head
  float* s_pt = s_g + 2 * p.Hh;                               // [3]
  const int bq = blockIdx.x;
  const int b = bq / p.Q;
  const int t = threadIdx.x;
  project_cameras_bwd(p, b, bq, s_uv, s_cam, s_pt);
  head_weights_to_lds(p, bq, LP, s_w, [&](int n) { return s_cam[4 * n + 3] != 0.f; });   // as the forward
  const int Dh = p.C / p.Hh;
  const int c = t;                                            // C <= 256: one channel per thread
  const bool c_ok = c < p.C;
  const int h = c_ok ? c / Dh : 0;
  const float g = c_ok ? p.grad_out[(size_t)bq * p.C + c] : 0.f;
  for (int n = 0; n < p.N; ++n) {
    const size_t row = ((size_t)bq * p.N + n) * p.Hh;
    if (s_cam[4 * n + 3] == 0.f) {                            // workgroup-uniform: no gradient through an invisible camera
      for (int e = t; e < p.Hh * LP; e += blockDim.x) {
        p.grad_logits[row * LP + e] = 0.f;
        p.grad_offsets[(row * LP + e) * 2] = 0.f;
        p.grad_offsets[(row * LP + e) * 2 + 1] = 0.f;
      }
      continue;
    }
    const float2 g2 = s_uv[n];
    if (t < 2 * p.Hh) s_g[t] = 0.f;
    for (int l = 0; l < p.L; ++l) {
      const int H = p.lvl_h[l], W = p.lvl_w[l];
      for (int pt = 0; pt < p.L; ++pt) {
        float part0 = 0.f, part1 = 0.f, part2 = 0.f;
        if (c_ok) {
          const float* off = p.offsets + ((row + h) * LP + (l * p.L + pt)) * 2;
          const GridCell cell(g2.x + off[0] / (float)W, g2.y + off[1] / (float)H, W, H);
          if (cell.any()) {
            const size_t plane = ((size_t)(b * p.N + n) * p.C + c) * H * W;
            float v[4], T, dTdx, dTdy;
            cell.taps(p.feats[l] + plane, W, v);
            bilinear_adjoint(cell, v, T, dTdx, dTdy);
            part0 = g * T;
            part1 = g * dTdx;
            part2 = g * dTdy;
            if (p.gfeats[l])                                  // weight (level = pt, point = l)
              cell.scatter(p.gfeats[l] + plane, W, g * s_w[((size_t)n * p.Hh + h) * LP + pt * p.L + l]);
          }
        }
        s_part[t] = part0; s_part[256 + t] = part1; s_part[512 + t] = part2;
        __syncthreads();
        if (t < p.Hh) {                                       // head t: its Dh channels in order
          float tot0 = 0.f, tot1 = 0.f, tot2 = 0.f;
          for (int k = 0; k < Dh; ++k) { tot0 += s_part[t * Dh + k]; tot1 += s_part[256 + t * Dh + k]; tot2 += s_part[512 + t * Dh + k]; }
          const float w = s_w[((size_t)n * p.Hh + t) * LP + pt * p.L + l];
          s_dw[t * LP + pt * p.L + l] = tot0;
          float* go = p.grad_offsets + ((row + t) * LP + (l * p.L + pt)) * 2;
          go[0] = 0.5f * w * tot1;                            // dx / d off_x = (W / 2) (1 / W)
          go[1] = 0.5f * w * tot2;
          s_g[2 * t] += w * tot1 * (0.5f * (float)W);         // dx / d gx = W / 2
          s_g[2 * t + 1] += w * tot2 * (0.5f * (float)H);
        }
        __syncthreads();
      }
    }
    if (t < p.Hh) {                                           // softmax backward of (camera n, head t)
      const float* w = s_w + ((size_t)n * p.Hh + t) * LP;
      float dot = 0.f;
      for (int i = 0; i < LP; ++i) dot += w[i] * s_dw[t * LP + i];
      for (int i = 0; i < LP; ++i) p.grad_logits[(row + t) * LP + i] = w[i] * (s_dw[t * LP + i] - dot);
    }
    if (t == 0) {
      float ggx = 0.f, ggy = 0.f;
      for (int hh = 0; hh < p.Hh; ++hh) { ggx += s_g[2 * hh]; ggy += s_g[2 * hh + 1]; }
      add_point_gradient(p, b, n, s_cam, 2.f * ggx, 2.f * ggy, s_pt);   // g = (u - 0.5) 2
    }
    __syncthreads();
  }
  if (t < 3 && p.grad_ref) p.grad_ref[(size_t)bq * 3 + t] = s_pt[t] * p.rng_scale[t];
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// Validates and fills what the four entry points share, in the order their callers rely on: EINVAL for a missing pointer or
// a non-positive size, then EUNSUPPORTED for a shape the kernels do not take - before any level entry is read -, then
// EINVAL for a null or empty level.  own_args / own_shape: the entry point's own pointers and sizes / its own limits.
static int fill_common(Detr3dCommon& p, const void* const* feats, const int32_t* level_hw, const float* ref, const float* attn_logits,
                       const float* lidar2img, const double* pc_range, float img_h, float img_w, int B, int N, int Q, int C, int L,
                       bool own_args, bool own_shape) {
  if (!feats || !level_hw || !ref || !attn_logits || !lidar2img || !pc_range || !own_args) return GD4D_EINVAL;
  if (B <= 0 || N <= 0 || Q <= 0 || C <= 0 || L <= 0 || !(img_h > 0.f) || !(img_w > 0.f)) return GD4D_EINVAL;
  if (L > GD4D_MAX_LEVELS || N > 256 || !own_shape) return GD4D_EUNSUPPORTED;
  for (int l = 0; l < L; ++l) {
    if (!feats[l] || level_hw[2 * l] <= 0 || level_hw[2 * l + 1] <= 0) return GD4D_EINVAL;
    p.feats[l] = static_cast<const float*>(feats[l]);
    p.lvl_h[l] = level_hw[2 * l];
    p.lvl_w[l] = level_hw[2 * l + 1];
  }
  p.ref = ref; p.attn_logits = attn_logits; p.lidar2img = lidar2img;
  p.B = B; p.N = N; p.Q = Q; p.C = C; p.L = L;
  fill_metre_range(p, pc_range);
  p.img_h = img_h; p.img_w = img_w;
  return GD4D_OK;
}

static void fill_gradients(Detr3dBwdParams& p, const float* grad_out, void* const* grad_feats, float* grad_logits, float* grad_ref) {
  for (int l = 0; l < p.L; ++l) p.gfeats[l] = grad_feats ? static_cast<float*>(grad_feats[l]) : nullptr;
  p.grad_out = grad_out; p.grad_logits = grad_logits; p.grad_ref = grad_ref;
}

}  // namespace gd4d

extern "C" int gd4d_detr3d_fwd(const void* const* feats, const int32_t* level_hw, const float* ref,
                               const float* attn_logits, const float* lidar2img,
                               const double* pc_range, float img_h, float img_w, float* out,
                               uint8_t* mask_out, float* sampled_out, int B, int N, int Q, int C,
                               int L, int P, void* stream) {
  using namespace gd4d;
  Detr3dParams p{};
  if (int rc = fill_common(p, feats, level_hw, ref, attn_logits, lidar2img, pc_range, img_h, img_w, B, N, Q, C, L,
                           out || sampled_out || mask_out, P == 1))
    return rc;
  p.out = out; p.mask_out = mask_out; p.sampled_out = sampled_out;
  const size_t lds = sizeof(float) * (size_t)(2 * N + N * L) + sizeof(int) * (size_t)N;
  hipLaunchKernelGGL(detr3d_fwd_kernel, dim3(B * Q), dim3(256), lds, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_detr3d_bwd(const void* const* feats, const int32_t* level_hw, const float* ref, const float* attn_logits,
                               const float* lidar2img, const double* pc_range, float img_h, float img_w, const float* grad_out,
                               void* const* grad_feats, float* grad_logits, float* grad_ref, int B, int N, int Q, int C, int L,
                               int P, void* stream) {
  using namespace gd4d;
  Detr3dBwdParams p{};
  if (int rc = fill_common(p, feats, level_hw, ref, attn_logits, lidar2img, pc_range, img_h, img_w, B, N, Q, C, L,
                           grad_out && grad_logits, P == 1))
    return rc;
  fill_gradients(p, grad_out, grad_feats, grad_logits, grad_ref);
  const size_t lds = sizeof(float) * (size_t)(2 * N + 4 * N + 12 + 3);
  hipLaunchKernelGGL(detr3d_bwd_kernel, dim3(B * Q), dim3(256), lds, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_detr3d_v2_fwd(const void* const* feats, const int32_t* level_hw, const float* ref,
                                  const float* attn_logits, const float* offsets, const float* lidar2img,
                                  const double* pc_range, float img_h, float img_w, float* out, uint8_t* mask_out,
                                  int B, int N, int Q, int C, int Hh, int L, int P, void* stream) {
  using namespace gd4d;
  Detr3dV2Params p{};
  if (int rc = fill_common(p, feats, level_hw, ref, attn_logits, lidar2img, pc_range, img_h, img_w, B, N, Q, C, L,
                           offsets && out && Hh > 0, P == L && Hh > 0 && C % Hh == 0))
    return rc;
  p.offsets = offsets; p.out = out; p.mask_out = mask_out; p.Hh = Hh;
  const size_t lds = sizeof(float) * (size_t)(2 * N + N * Hh * L * L) + sizeof(int) * (size_t)N;
  if (lds > 64 * 1024) return GD4D_EUNSUPPORTED;
  hipLaunchKernelGGL(detr3d_v2_fwd_kernel, dim3(B * Q), dim3(256), lds, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_detr3d_v2_bwd(const void* const* feats, const int32_t* level_hw, const float* ref, const float* attn_logits,
                                  const float* offsets, const float* lidar2img, const double* pc_range, float img_h, float img_w,
                                  const float* grad_out, void* const* grad_feats, float* grad_logits, float* grad_offsets,
                                  float* grad_ref, int B, int N, int Q, int C, int L, int Hh, void* stream) {
  using namespace gd4d;
  Detr3dV2BwdParams p{};
  if (int rc = fill_common(p, feats, level_hw, ref, attn_logits, lidar2img, pc_range, img_h, img_w, B, N, Q, C, L,
                           offsets && grad_out && grad_logits && grad_offsets && Hh > 0 && C % Hh == 0, C <= 256 && Hh <= 64))
    return rc;
  fill_gradients(p, grad_out, grad_feats, grad_logits, grad_ref);
  p.offsets = offsets; p.grad_offsets = grad_offsets; p.Hh = Hh;
  const size_t lds = sizeof(float) * ((size_t)6 * N + (size_t)N * Hh * L * L + 3 * 256 + (size_t)Hh * L * L + 2 * Hh + 3);
  if (lds > 65536 && !allow_dynamic_lds(reinterpret_cast<const void*>(detr3d_v2_bwd_kernel), (int)lds)) return GD4D_ELAUNCH;
  hipLaunchKernelGGL(detr3d_v2_bwd_kernel, dim3(B * Q), dim3(256), lds, static_cast<hipStream_t>(stream), p);
  return check_launch();
}
