// Training-side step right after the path: the matching cost of HungarianAssigner3D and the
// per-layer focal / L1 losses of Detr3DHeadPE.loss_single, for ALL decoder layers in one launch each.
//
// The reference runs, per decoder layer and sample: ~15 small torch kernels for the cost matrix, a device -> host copy
// (a synchronisation), scipy on the CPU, two host -> device copies, ~40 small kernels for targets and losses and two
// scalar all-reduces each followed by .item() (two more synchronisations): 6 layers -> 18+ syncs per step
// (hungarian_assigner_3d.py:117-144, detr3d_head_pe.py:782-845).  With these two kernels a step has ONE device -> host
// copy (all layers' cost matrices), the assignment on the host, ONE host -> device copy, one loss launch that also
// produces the gradients, and no .item(): the normalisers are read from device memory.
#include "gd4d_loss_pieces.h"

namespace gd4d {

constexpr int MC_MAX_GT = 1024;      // ground-truth boxes per sample held in LDS
constexpr int MC_QB = 64;            // queries per workgroup

struct MatchCostParams {
  const float* cls;          // (NL, B, Q, C) logits
  const float* box;          // (NL, B, Q, code) head outputs (normalised box code)
  const float* gt_boxes;     // (sumG, gt_dim)
  const int32_t* gt_labels;  // (sumG)
  const int32_t* gt_start;   // device, (B + 1) prefix offsets into the ground-truth arrays
  float* cost;               // block (l, b) at Q * (l * sumG + start_b), shape (Q, G_b) row-major
  int NL, B, Q, C, code, gt_dim, sumG;
  float cls_weight, reg_weight, alpha;
};

// mmdet FocalLossCost (alpha, gamma = 2, eps = 1e-12) + BBox3DL1Cost over the first 8 code entries, then nan_to_num
// The focal term is the reference's own fp32 formula, -log(1 - p + 1e-12) with p = 1 / (1 + expf(-x)): ill-conditioned by construction
// once 1 - p loses its bits (x above ~6) and a constant once p rounds to 1 (x >= 24 ln 2); the cost then follows the rounding of p, not
// the real-number formula.  The blocks of the non-empty samples tile the buffer: every element is written.
__global__ __launch_bounds__(256) void match_cost_kernel(const MatchCostParams p) {
  __shared__ float s_gt[MC_MAX_GT * 8];
  __shared__ int s_lab[MC_MAX_GT];
  const int b = blockIdx.y, l = blockIdx.z;
  const int g0 = p.gt_start[b], G = p.gt_start[b + 1] - g0;
  if (G <= 0) return;
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    float o[10];
    normalize_box(p.gt_boxes + (size_t)(g0 + g) * p.gt_dim, p.gt_dim, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) s_gt[8 * g + k] = o[k];
    s_lab[g] = p.gt_labels[g0 + g];
  }
  __syncthreads();
  const int q0 = blockIdx.x * MC_QB;
  const int nq = min(MC_QB, p.Q - q0);
  const size_t row0 = ((size_t)l * p.B + b) * p.Q;
  float* out = p.cost + (size_t)p.Q * ((size_t)l * p.sumG + g0);
  for (int e = threadIdx.x; e < nq * G; e += blockDim.x) {
    const int ql = e / G, g = e - ql * G;
    const int q = q0 + ql;
    const int lab = s_lab[g];
    if (lab < 0 || lab >= p.C) {                          // the reference's cls_pred[:, gt_labels] raises here; the host
      out[(size_t)q * G + g] = __builtin_nanf("");        // sees the NaN (valid costs are never NaN) and raises too
      continue;
    }
    const float x = p.cls[(row0 + q) * p.C + lab];
    const float pr = sigmoid_f(x);
    const float neg = -logf(1.0f - pr + 1e-12f) * (1.0f - p.alpha) * (pr * pr);
    const float pos = -logf(pr + 1e-12f) * p.alpha * ((1.0f - pr) * (1.0f - pr));
    const float* bx = p.box + (row0 + q) * p.code;
    float l1 = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) l1 += fabsf(bx[k] - s_gt[8 * g + k]);
    const float c = (pos - neg) * p.cls_weight + l1 * p.reg_weight;
    out[(size_t)q * G + g] = nan_to_num_f(c, 100.0f, 100.0f, -100.0f);     // hungarian_assigner_3d.py:139
  }
}

struct HeadLossParams {
  const float* cls;            // (NL, B, Q, C)
  const float* box;            // (NL, B, Q, code)
  const int32_t* assigned;     // (NL, B, Q): index into the ground-truth arrays, or -1 = background
  const float* gt_boxes;
  const int32_t* gt_labels;
  const float* code_weights;   // (10)
  const float* avg_factors;    // device, 2 floats: cls_avg_factor, num_total_pos (both clamped to >= 1 here)
  float* loss;                 // (NL, 2): loss_cls, loss_bbox
  float* grad_cls;             // like cls
  float* grad_box;             // like box
  int NL, B, Q, C, code, gt_dim, sumG;
  float alpha, cls_weight, box_weight;
};

// One workgroup per decoder layer, one thread per (sample, query) row: sigmoid focal loss (gamma = 2) over the classes
// with label `num_classes` = background, L1 on the positives against the normalised ground truth (rows whose target is
// not finite are dropped, :837-842), both already divided by their normalisers; gradients written in the same pass.
// A matched row whose stored label is C is background for the focal term and KEEPS its box term (the reference's one_hot does the
// same); labels outside [0, C] and assigned outside [0, sumG) make the reference raise and are background here.  The compared columns
// are the first nk = min(gt_dim > 7 ? 10 : 8, code) of both sides (the reference only runs for (gt_dim, code) = (7, 8), (9, >= 10),
// where this is its rule; an 8-entry box has vy = 0); gradient columns >= nk are +0.  The gradients are those of the two terms BEFORE
// nan_to_num: a layer whose term was replaced keeps finite gradients wherever its own inputs are finite (torch zeroes the layer).
__global__ __launch_bounds__(LOSS_ROW_THREADS) void head_loss_kernel(const HeadLossParams p) {
  __shared__ float s_red[2][LOSS_ROW_WAVES];
  const int l = blockIdx.x;
  const float cls_avg = fmaxf(p.avg_factors[0], 1.0f), pos_avg = fmaxf(p.avg_factors[1], 1.0f);
  const float kc = p.cls_weight / cls_avg, kb = p.box_weight / pos_avg;
  float sum_cls = 0.f, sum_box = 0.f;
  for (int r = threadIdx.x; r < p.B * p.Q; r += blockDim.x) {
    const size_t row = (size_t)l * p.B * p.Q + r;
    int a = p.assigned[row];
    if (a >= p.sumG) a = -1;                               // never index past the ground truth (host validates; memory safety)
    int label = a >= 0 ? p.gt_labels[a] : p.C;
    if (label < 0 || label > p.C) label = p.C;
    const float* x = p.cls + row * p.C;
    float* gx = p.grad_cls + row * p.C;
    for (int c = 0; c < p.C; ++c) {
      const float v = x[c];
      const bool t = c == label;
      const float pr = sigmoid_f(v);
      const float pt = t ? 1.0f - pr : pr;
      const float aw = t ? p.alpha : 1.0f - p.alpha;
      const float fw = aw * (pt * pt);
      // binary_cross_entropy_with_logits: max(v, 0) - v t + log(1 + exp(-|v|)).  Its own spelling: v t as a select (t is 0 or 1),
      // which is 0 where the product v * 0 of distill_loss_kernel's soft-label form is NaN (v = +-inf)
      const float bce = fmaxf(v, 0.f) - (t ? v : 0.f) + softplus_neg_abs(v);
      sum_cls += bce * fw;
      const float dpt = (t ? -1.0f : 1.0f) * pr * (1.0f - pr);
      gx[c] = kc * (fw * (pr - (t ? 1.0f : 0.f)) + bce * aw * 2.0f * pt * dpt);
    }
    float* gb = p.grad_box + row * p.code;
    for (int k = 0; k < p.code; ++k) gb[k] = 0.f;
    if (a >= 0) {
      float tgt[10];
      normalize_box(p.gt_boxes + (size_t)a * p.gt_dim, p.gt_dim, tgt);
      const int nk = min(p.gt_dim > 7 ? 10 : 8, p.code);
      if (finite_f(tgt, nk)) {
        const float* bx = p.box + row * p.code;
        for (int k = 0; k < nk; ++k) {
          const float d = bx[k] - tgt[k], w = p.code_weights[k];
          sum_box += fabsf(d) * w;
          gb[k] = kb * w * l1_sign(d);
        }
      }
    }
  }
  // the fixed-order workgroup sum of gd4d_common.h, both values behind one barrier; thread k finishes term k
  block_sum_put(sum_cls, s_red[0]);
  block_sum_put(sum_box, s_red[1]);
  __syncthreads();
  if (threadIdx.x < 2) {
    // `0.f +`: this site's sum always started from +0, and a term can be -0 (a negative code weight times fabsf(0)): kept, not argued away
    const float s = (0.f + block_sum_get<LOSS_ROW_WAVES>(s_red[threadIdx.x])) * (threadIdx.x == 0 ? kc : kb);
    p.loss[2 * l + threadIdx.x] = nan_to_num_f(s);         // torch.nan_to_num on the two loss terms (:844-845)
  }
}

}  // namespace gd4d

extern "C" int gd4d_match_cost_fwd(const float* cls, const float* box, const float* gt_boxes, const int32_t* gt_labels,
                                   const int32_t* gt_start, float* cost, int NL, int B, int Q, int C, int code,
                                   int gt_dim, int sum_gt, int max_gt, float cls_weight, float reg_weight, float alpha,
                                   void* stream) {
  using namespace gd4d;
  if (!cls || !box || !gt_boxes || !gt_labels || !gt_start || !cost) return GD4D_EINVAL;
  if (NL <= 0 || B <= 0 || Q <= 0 || C <= 0 || sum_gt <= 0 || max_gt <= 0) return GD4D_EINVAL;
  if (code < 8 || gt_dim < 7 || gt_dim > 9 || max_gt > MC_MAX_GT || B > 65535 || NL > 65535) return GD4D_EUNSUPPORTED;
  MatchCostParams p{cls, box, gt_boxes, gt_labels, gt_start, cost, NL, B, Q, C, code, gt_dim, sum_gt,
                    cls_weight, reg_weight, alpha};
  const dim3 grid((Q + MC_QB - 1) / MC_QB, B, NL);
  hipLaunchKernelGGL(match_cost_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_head_loss_fwd_bwd(const float* cls, const float* box, const int32_t* assigned, const float* gt_boxes,
                                      const int32_t* gt_labels, const float* code_weights, const float* avg_factors,
                                      float* loss, float* grad_cls, float* grad_box, int NL, int B, int Q, int C,
                                      int code, int gt_dim, int sum_gt, float alpha, float loss_cls_weight,
                                      float loss_bbox_weight, void* stream) {
  using namespace gd4d;
  if (!cls || !box || !assigned || !gt_boxes || !gt_labels || !code_weights || !avg_factors || !loss || !grad_cls ||
      !grad_box)
    return GD4D_EINVAL;
  if (NL <= 0 || B <= 0 || Q <= 0 || C <= 0 || sum_gt <= 0) return GD4D_EINVAL;
  if (code < 8 || code > 16 || gt_dim < 7 || gt_dim > 9) return GD4D_EUNSUPPORTED;
  HeadLossParams p{cls, box, assigned, gt_boxes, gt_labels, code_weights, avg_factors, loss, grad_cls, grad_box,
                   NL, B, Q, C, code, gt_dim, sum_gt, alpha, loss_cls_weight, loss_bbox_weight};
  hipLaunchKernelGGL(head_loss_kernel, dim3(NL), dim3(LOSS_ROW_THREADS), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}
