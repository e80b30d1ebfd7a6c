// The pieces the matching-cost and loss kernels are made of, each written once with the reference line it restates:
// gd4d_criterion.hip, gd4d_distill.hip and gd4d_lane_head.hip include this header.  The library is built with -ffp-contract=off, so
// an expression keeps its bits inside an inline function as long as its operations keep their order: a piece is shared only between
// sites whose expression trees are the same.  Three sites are NOT these pieces, on purpose, and say so where they stand:
// head_loss_kernel's BCE (subtracts t ? v : 0, not v y), bce_pos_neg (pos = neg - x) and lane_term (the overflow-free sigmoid).
//   normalize_box, distill_teacher_box     the box code of the ground truth and of the teacher's pseudo ground truth
//   sigmoid_f, softplus_neg_abs            the two transcendental halves of a BCE-with-logits term
//   nan_to_num_f, finite_f                 torch.nan_to_num on a float; torch.isfinite(...).all() over a short array
//   l1_sign                                d|x|/dx as torch's L1 backward writes it
// The sums these kernels make over a workgroup are block_sum_put / block_sum_get (gd4d_common.h): their order is defined there.
#pragma once
#include <float.h>

#include "gd4d_common.h"

namespace gd4d {

// core/bbox/util.py:38-58: (cx, cy, cz, w, l, h, rot[, vx, vy]) -> (cx, cy, log w, log l, cz, log h, sin, cos[, vx, vy]).  Reads
// b[0 .. gt_dim) and nothing past it.
__device__ __forceinline__ void normalize_box(const float* b, int gt_dim, float* o) {
  o[0] = b[0]; o[1] = b[1]; o[2] = logf(b[3]); o[3] = logf(b[4]); o[4] = b[2]; o[5] = logf(b[5]);
  o[6] = sinf(b[6]); o[7] = cosf(b[6]);
  o[8] = gt_dim > 7 ? b[7] : 0.f;
  o[9] = gt_dim > 8 ? b[8] : 0.f;
}

// teacher pseudo ground truth: normalize_bbox(denormalize_bbox(t)) (core/bbox/util.py:38-87) for a 10-entry box code.  The round
// trip is not the identity: sin / cos come back divided by hypot(sin, cos), w / l / h go through log(exp(.)) (exp may overflow to
// inf, or underflow to 0 and give -inf).
__device__ __forceinline__ void distill_teacher_box(const float* t, float* o) {
  const float rot = atan2f(t[6], t[7]);
  o[0] = t[0]; o[1] = t[1]; o[2] = logf(expf(t[2])); o[3] = logf(expf(t[3])); o[4] = t[4]; o[5] = logf(expf(t[5]));
  o[6] = sinf(rot); o[7] = cosf(rot); o[8] = t[8]; o[9] = t[9];
}

// torch.sigmoid in fp32 as the reference's kernels evaluate it: 1 / (1 + exp(-x)); exp(-x) = inf gives 0
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// log(1 + exp(-|x|)): the last term of binary_cross_entropy_with_logits, max(x, 0) - x y + log1p(exp(-|x|))
__device__ __forceinline__ float softplus_neg_abs(float x) { return log1pf(expf(-fabsf(x))); }

// torch.nan_to_num(x, nan, posinf, neginf); the defaults are torch's for float32, what the loss terms go through
// (detr3d_head_pe.py:844-845, :923-924, petr_head_seg.py:785)
__device__ __forceinline__ float nan_to_num_f(float x, float nan = 0.f, float posinf = FLT_MAX, float neginf = -FLT_MAX) {
  if (x != x) return nan;
  if (x == INFINITY) return posinf;
  if (x == -INFINITY) return neginf;
  return x;
}

// torch.isfinite(x[0 .. n)).all() (detr3d_head_pe.py:837, :916): NaN compares false
__device__ __forceinline__ bool finite_f(const float* x, int n) {
  bool ok = true;
  for (int k = 0; k < n; ++k) ok = ok && (fabsf(x[k]) <= FLT_MAX);
  return ok;
}

// The two row-loop loss kernels (head_loss_kernel, distill_loss_kernel): one workgroup of this size per decoder layer.  One constant
// for the launch, __launch_bounds__, the extent of the LDS partials and the wave count block_sum_get unrolls over.
constexpr int LOSS_ROW_THREADS = 1024;
constexpr int LOSS_ROW_WAVES = LOSS_ROW_THREADS / GD4D_WAVE;

// torch.sign(d): the gradient of |d| (L1Loss backward); 0 at 0, and 0 for NaN
__device__ __forceinline__ float l1_sign(float d) { return d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f); }

}  // namespace gd4d
