// Detr4D_Distiller's instance distillation term (distillation/distillers/detr4d_distiller.py:143-166) on the device:
//
//   gd4d_distill_match_cost_fwd  DistillHungarianAssigner3D's cost (core/bbox/assigners/distill_hungarian_assigner_3d.py:106-114) for
//                                every (decoder layer, sample) block in one launch;
//   gd4d_lsa_dense_fwd           an exact linear sum assignment for DENSE problems (900 x 900 at the shipped size): a parallel warm
//                                start, then one shortest augmenting path per row it left free;
//   gd4d_distill_loss_fwd_bwd    Detr3DHeadPE.loss_distill_single (dense_heads/detr3d_head_pe.py:851-925) with its targets
//                                (:927-1012) - both loss terms of every layer and their gradients in one launch.
//
// The reference copies each of the 6 x B cost matrices to the host and solves it with scipy, then calls .item() once per layer.
#include <limits.h>

#include "gd4d_loss_pieces.h"

namespace gd4d {

// ---------------------------------------------------------------------------------------------------------------------------
// BCE-with-logits against 1 and against 0 (match_cost.py:52-75): max(x, 0) - x + log1p(exp(-|x|)) and max(x, 0) + log1p(exp(-|x|)).
// Its own association: pos = (max + softplus) - x, where distill_loss_kernel's term is (max - v y) + softplus.
__device__ __forceinline__ void bce_pos_neg(float x, float& pos, float& neg) {
  const float sp = softplus_neg_abs(x);
  neg = fmaxf(x, 0.f) + sp;
  pos = neg - x;
}

constexpr int DC_TILE = 64;          // student rows x teacher columns per workgroup
constexpr int DC_MAX_C = 64;

struct DistillCostParams {
  const float* s_cls;   // (NL, B, Qs, C)
  const float* s_box;   // (NL, B, Qs, code)
  const float* t_cls;   // (NL, B, Qt, C): the soft labels are sigmoid(t_cls[l, 0]) for EVERY sample (detr4d_distiller.py:159)
  const float* t_box;   // (NL, B, Qt, 10)
  float* cost;          // block (l, b) at Qs * (l * B * Qt + b * Qt), (Qs, Qt) row-major
  int NL, B, Qs, Qt, C, code;
  int pseudo_gt;        // 1: t_cls holds the soft labels of sample b itself, t_box the denormalised boxes (NL, B, Qt, 9) - assign()'s inputs
  float cls_weight, reg_weight;
};

// cost[q, t] = cls_weight * sum_c (pos[q, c] p[t, c] + neg[q, c] (1 - p[t, c])) + reg_weight * sum_{k<8} |s_box[q, k] - tn[t, k]|
// (the reference's cost is NOT passed through nan_to_num: +inf stays - scipy accepts it while the problem stays feasible - and NaN or
// -inf, which scipy refuses, are written as NaN: gd4d_match_cost_fwd's marker, status 1 of the solvers)
__global__ __launch_bounds__(256) void distill_match_cost_kernel(const DistillCostParams p) {
  __shared__ float s_pos[DC_TILE][DC_MAX_C + 1], s_neg[DC_TILE][DC_MAX_C + 1], s_sb[DC_TILE][8];
  __shared__ float s_p[DC_TILE][DC_MAX_C + 1], s_tb[DC_TILE][8];
  const int nqt = (p.Qt + DC_TILE - 1) / DC_TILE;
  const int q0 = (blockIdx.x / nqt) * DC_TILE, t0 = (blockIdx.x % nqt) * DC_TILE;
  const int b = blockIdx.y, l = blockIdx.z, C = p.C;
  const size_t srow = ((size_t)l * p.B + b) * p.Qs, trow = ((size_t)l * p.B + b) * p.Qt, t0row = (size_t)l * p.B * p.Qt;
  for (int e = threadIdx.x; e < DC_TILE * C; e += blockDim.x) {
    const int r = e / C, c = e - r * C;
    if (q0 + r < p.Qs) bce_pos_neg(p.s_cls[(srow + q0 + r) * C + c], s_pos[r][c], s_neg[r][c]);
    if (t0 + r < p.Qt) s_p[r][c] = p.pseudo_gt ? p.t_cls[(trow + t0 + r) * C + c] : sigmoid_f(p.t_cls[(t0row + t0 + r) * C + c]);
  }
  for (int r = threadIdx.x; r < DC_TILE; r += blockDim.x) {
    if (q0 + r < p.Qs)
      for (int k = 0; k < 8; ++k) s_sb[r][k] = p.s_box[(srow + q0 + r) * p.code + k];
    if (t0 + r < p.Qt) {
      float o[10];
      if (p.pseudo_gt) normalize_box(p.t_box + (trow + t0 + r) * 9, 7, o);       // (gt_dim 7: the velocity columns are not read)
      else distill_teacher_box(p.t_box + (trow + t0 + r) * 10, o);
      for (int k = 0; k < 8; ++k) s_tb[r][k] = o[k];
    }
  }
  __syncthreads();
  const int t = threadIdx.x & (DC_TILE - 1);
  if (t0 + t >= p.Qt) return;
  float* out = p.cost + (size_t)p.Qs * ((size_t)l * p.B * p.Qt + (size_t)b * p.Qt);
  for (int r = threadIdx.x / DC_TILE; r < DC_TILE && q0 + r < p.Qs; r += 256 / DC_TILE) {
    float pos = 0.f, neg = 0.f;
    for (int c = 0; c < C; ++c) {
      pos += s_pos[r][c] * s_p[t][c];
      neg += s_neg[r][c] * (1.0f - s_p[t][c]);
    }
    float l1 = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) l1 += fabsf(s_sb[r][k] - s_tb[t][k]);
    float cst = (pos + neg) * p.cls_weight + l1 * p.reg_weight;
    if (cst == -INFINITY) cst = __builtin_nanf("");
    out[(size_t)(q0 + r) * p.Qt + t0 + t] = cst;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// gd4d_lsa_dense_fwd.  One 1024-thread workgroup per problem; thread tid owns columns tid, tid + 1024, ... (<= 4) and keeps their dual
// v, their tentative distance and their "scanned" flag in registers; row duals (fp64), both matchings and the path live in LDS.
//
// Warm start (parallel, exact):
//   square (nr == nc): column reduction - v_j = min_i c_ij, u = 0; each column offers itself to its first arg-min row, a row keeps the
//                     LOWEST offering column.  Reduced costs c - u - v >= 0 and every kept pair has reduced cost 0.
//   rectangular (nr < nc, the shorter side as rows as the host solver does): row reduction - u_i = min_j c_ij, v = 0; a row takes its
//                     first arg-min column unless a lower row took it.  Unmatched columns keep v = 0, which the rectangular optimum needs.
// Then, for every row still free, in row order, the shortest augmenting path of scipy's solver (Crouse 2016; the loop of
// gd4d_hungarian_assign_fwd) from the current duals: r = ((min_val + c) - u_i) - v_j in fp64 from the fp32 cost, the dual update and
// the augmentation as there.  The result is an optimal assignment: the same as scipy's whenever the optimum is unique (continuous
// costs), and of the same total cost (up to fp64 rounding) when it is not - the tie it settles on may differ.
// One scan step = every thread updates its columns from the row's costs (one coalesced fp32 row read), then a lexicographic arg-min
// (distance, column already matched, column index) over the workgroup: a wave reduction, ONE barrier, a 16-entry read of the wave
// results (double-buffered slots, so no second barrier).
constexpr int LD_THREADS = 1024;
constexpr int LD_CPT = 4;                       // columns per thread: nc <= 4096
constexpr int LD_WAVES = LD_THREADS / 64;

struct LsaDenseParams {
  const float* cost;
  const int32_t* gt_start;
  int32_t* assigned;
  int32_t* status;
  float* work;                                  // per problem Q * max_gt floats: the transposed copy when G < Q
  int NL, B, Q, sum_gt, max_gt;
};

// fp64 -> uint64 with the same order (negative values included)
__device__ __forceinline__ unsigned long long ld_order(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ld_unorder(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ unsigned long long ld_shfl_xor64(unsigned long long x, int o) {
  const int lo = __shfl_xor((int)(x & 0xffffffffull), o), hi = __shfl_xor((int)(x >> 32), o);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ bool ld_less(unsigned long long ka, int ta, unsigned long long kb, int tb) {
  return ka < kb || (ka == kb && ta < tb);
}

__global__ __launch_bounds__(LD_THREADS) void lsa_dense_kernel(const LsaDenseParams p) {
  extern __shared__ __attribute__((aligned(16))) char ld_smem[];
  __shared__ unsigned long long s_key[2][LD_WAVES];
  __shared__ int s_tie[2][LD_WAVES];
  __shared__ int s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x, l = prob / p.B, b = prob - l * p.B;
  const int g0 = p.gt_start[b], G = p.gt_start[b + 1] - g0, Q = p.Q;
  int32_t* out = p.assigned + (size_t)prob * Q;
  for (int q = tid; q < Q; q += LD_THREADS) out[q] = -1;
  if (G <= 0 || Q <= 0) { if (tid == 0) p.status[prob] = 0; return; }
  if (G > p.max_gt) { if (tid == 0) p.status[prob] = 2; return; }
  const float* c = p.cost + (size_t)Q * ((size_t)l * p.sum_gt + g0);        // (Q, G) row-major
  const bool transposed = G < Q;
  const int nr = transposed ? G : Q, nc = transposed ? Q : G;
  const float* m = c;
  if (tid == 0) s_flag = 0;
  __syncthreads();
  bool bad = false;
  if (transposed) {
    float* w = p.work + (size_t)prob * Q * p.max_gt;                         // (nr, nc) = (G, Q)
    for (int idx = tid; idx < nr * nc; idx += LD_THREADS) {
      const int q = idx / G, g = idx - q * G;                                // coalesced read of (Q, G)
      const float x = c[idx];
      bad = bad || (x != x) || (x == -INFINITY);
      w[(size_t)g * nc + q] = x;
    }
    m = w;
  } else {
    for (int idx = tid; idx < nr * nc; idx += LD_THREADS) {
      const float x = c[idx];
      bad = bad || (x != x) || (x == -INFINITY);
    }
  }
  if (bad) s_flag = 1;
  double* u = reinterpret_cast<double*>(ld_smem);
  int* col4row = reinterpret_cast<int*>(u + nr);
  int* row4col = col4row + nr;
  int* path = row4col + nc;
  for (int r = tid; r < nr; r += LD_THREADS) { u[r] = 0.0; col4row[r] = INT_MAX; }
  for (int j = tid; j < nc; j += LD_THREADS) { row4col[j] = INT_MAX; path[j] = -1; }
  __threadfence_block();                                                     // (the transposed copy: read back by other threads)
  __syncthreads();
  if (s_flag) { if (tid == 0) p.status[prob] = 1; return; }                 // scipy: "matrix contains invalid numeric entries"
  const double inf = __builtin_inf();
  double vj[LD_CPT], sh[LD_CPT];
  bool sc[LD_CPT];
#pragma unroll
  for (int k = 0; k < LD_CPT; ++k) { vj[k] = 0.0; sh[k] = inf; sc[k] = false; }
  // ---- warm start ----
  bool infeasible = false;
  if (nr == nc) {
#pragma unroll
    for (int k = 0; k < LD_CPT; ++k) {
      const int j = tid + k * LD_THREADS;
      if (j >= nc) break;
      double best = inf;
      int arg = -1;
#pragma unroll 8
      for (int i = 0; i < nr; ++i) {
        const double x = (double)m[(size_t)i * nc + j];
        if (x < best) { best = x; arg = i; }
      }
      vj[k] = best;
      if (arg < 0) infeasible = true;                                        // a column of +inf: it can never be matched
      else atomicMin(&col4row[arg], j);
    }
  } else {
    for (int i = tid; i < nr; i += LD_THREADS) {
      const float* ci = m + (size_t)i * nc;
      double best = inf;
      int arg = -1;
      for (int j = 0; j < nc; ++j) {
        const double x = (double)ci[j];
        if (x < best) { best = x; arg = j; }
      }
      u[i] = best;
      if (arg < 0) infeasible = true;
      else atomicMin(&row4col[arg], i);
    }
  }
  if (infeasible) s_flag = 2;
  __syncthreads();
  if (s_flag) { if (tid == 0) p.status[prob] = 2; return; }
  if (nr == nc) {                                                            // the rows' kept columns -> both matchings
    for (int r = tid; r < nr; r += LD_THREADS) if (col4row[r] == INT_MAX) col4row[r] = -1;
    for (int j = tid; j < nc; j += LD_THREADS) row4col[j] = -1;
    __syncthreads();
    for (int r = tid; r < nr; r += LD_THREADS) if (col4row[r] >= 0) row4col[col4row[r]] = r;
  } else {
    for (int r = tid; r < nr; r += LD_THREADS) col4row[r] = -1;
    __syncthreads();
    for (int j = tid; j < nc; j += LD_THREADS) {
      if (row4col[j] == INT_MAX) row4col[j] = -1;
      else col4row[row4col[j]] = j;
    }
  }
  __syncthreads();
  // ---- one shortest augmenting path per free row ----
  int parity = 0;
  for (int cur = 0; cur < nr; ++cur) {
    if (col4row[cur] >= 0) continue;                                         // (uniform: LDS read after a barrier)
#pragma unroll
    for (int k = 0; k < LD_CPT; ++k) { sh[k] = inf; sc[k] = false; }
    double min_val = 0.0;
    int i = cur, sink = -1;
    while (sink < 0) {
      const double ui = u[i];
      const float* ci = m + (size_t)i * nc;
      float x[LD_CPT];
#pragma unroll
      for (int k = 0; k < LD_CPT; ++k) {
        const int j = tid + k * LD_THREADS;
        x[k] = (j < nc && !sc[k]) ? ci[j] : 0.f;
      }
      unsigned long long key = ~0ull;
      int tie = INT_MAX;
#pragma unroll
      for (int k = 0; k < LD_CPT; ++k) {
        const int j = tid + k * LD_THREADS;
        if (j >= nc || sc[k]) continue;
        const double r = ((min_val + (double)x[k]) - ui) - vj[k];
        if (r < sh[k]) { sh[k] = r; path[j] = i; }
        const unsigned long long kk = ld_order(sh[k]);
        const int tt = ((row4col[j] >= 0) << 20) | j;                         // equal distances: an unmatched column first
        if (ld_less(kk, tt, key, tie)) { key = kk; tie = tt; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k2 = ld_shfl_xor64(key, o);
        const int t2 = __shfl_xor(tie, o);
        if (ld_less(k2, t2, key, tie)) { key = k2; tie = t2; }
      }
      if (lane == 0) { s_key[parity][wave] = key; s_tie[parity][wave] = tie; }
      __syncthreads();
      key = s_key[parity][0]; tie = s_tie[parity][0];
#pragma unroll
      for (int w = 1; w < LD_WAVES; ++w) {
        const unsigned long long k2 = s_key[parity][w];
        const int t2 = s_tie[parity][w];
        if (ld_less(k2, t2, key, tie)) { key = k2; tie = t2; }
      }
      parity ^= 1;
      min_val = ld_unorder(key);
      if (tie == INT_MAX || min_val == inf) { infeasible = true; break; }
      const int j = tie & 0xfffff;
#pragma unroll
      for (int k = 0; k < LD_CPT; ++k) if (j == tid + k * LD_THREADS) sc[k] = true;
      const int rj = row4col[j];
      if (rj < 0) sink = j; else i = rj;
    }
    if (infeasible) break;
    // dual update: the rows the search passed through are the ones matched to its scanned columns (the sink is unmatched)
#pragma unroll
    for (int k = 0; k < LD_CPT; ++k) {
      const int j = tid + k * LD_THREADS;
      if (j >= nc || !sc[k]) continue;
      const int r = row4col[j];
      if (r >= 0) u[r] += min_val - sh[k];
      vj[k] -= min_val - sh[k];
    }
    if (tid == 0) u[cur] += min_val;
    __syncthreads();
    if (tid == 0) {
      int j = sink;                                                          // augment along the path
      while (true) {
        const int r = path[j];
        row4col[j] = r;
        const int t = col4row[r]; col4row[r] = j; j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  if (infeasible) { if (tid == 0) p.status[prob] = 2; return; }
  for (int r = tid; r < nr; r += LD_THREADS) {
    if (transposed) out[col4row[r]] = r + g0;
    else out[r] = col4row[r] + g0;
  }
  if (tid == 0) p.status[prob] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
struct DistillLossParams {
  const float* s_cls;          // (NL, B, Qs, C)
  const float* s_box;          // (NL, B, Qs, code >= 10)
  const float* t_cls;          // (NL, B, Qt, C)
  const float* t_box;          // (NL, B, Qt, 10)
  const int32_t* assigned;     // (NL, B, Qs): b * Qt + teacher index, or -1
  const float* code_weights;   // (10)
  const float* avg_factors;    // device: cls_avg_factor, num_total_pos (reduce_mean-ed; both clamped to >= 1 here)
  float* loss;                 // (NL, 2)
  float* grad_cls;
  float* grad_box;
  int NL, B, Qs, Qt, C, code, reweight;
  float cls_weight, reg_weight;
};

// One workgroup per decoder layer, one thread per (sample, query) row, fixed-order reductions (a replay equals an eager run bit for bit).
//   labels[q]  = sigmoid(t_cls[l, 0, t]) for a matched row (teacher t; batch 0 for every sample, the reference's quirk), else num_classes
//   loss_cls   = w_cls * sum BCE-with-logits(s_cls, labels) / max(cls_avg_factor, 1)               (distill_cross_entropy_loss.py:139-147)
//   loss_reg   = w_reg * sum_{rows with finite normalised target} |s_box[:10] - tn| * bbox_weight / divisor
//                bbox_weight = code_weights (x max_c labels with reweight_score) on matched rows, 0 elsewhere; the target of an unmatched
//                row is zeros -> log(0) = -inf: dropped by the isfinite filter (detr3d_head_pe.py:916-921);
//                divisor = max(num_total_pos, 1), or with reweight_score the local sum of max_c labels over rows with labels[:, 0] != 10
//                (:908-911, not clamped);
//   both terms through nan_to_num (:923-924).
// Reference quirks kept on purpose (tests/test_loss_kernels_gpu.py pins each): the soft labels come from batch 0 for every sample; the
// divisor rule compares with the literal 10, so with C != 10 every unmatched row (labels = C) adds C to it; the divisor is not clamped.
// The gradients are those of the two terms BEFORE nan_to_num; when a layer's divisor is 0 (reweight, C == 10, nothing matched) or not
// finite the second pass makes grad_box[:, :10] NaN in EVERY row of that layer (0 * inf), where torch leaves 0 in the rows its
// isfinite filter drops.  assigned outside [b Qt, (b + 1) Qt) counts as unmatched.  Gradient columns >= 10 are +0.
__global__ __launch_bounds__(LOSS_ROW_THREADS) void distill_loss_kernel(const DistillLossParams p) {
  __shared__ float s_red[3][LOSS_ROW_WAVES];
  __shared__ float s_div;
  const int l = blockIdx.x, C = p.C;
  const float kc = p.cls_weight / fmaxf(p.avg_factors[0], 1.0f);
  float sum_cls = 0.f, sum_reg = 0.f, den = 0.f;
  const int rows = p.B * p.Qs;
  for (int row = threadIdx.x; row < rows; row += blockDim.x) {
    const int b = row / p.Qs;
    const size_t r = (size_t)l * rows + row;
    int a = p.assigned[r];
    int t = a - b * p.Qt;
    if (a < 0 || t < 0 || t >= p.Qt) t = -1;                                 // (memory safety: never read past the teacher)
    const float* x = p.s_cls + r * C;
    float* gx = p.grad_cls + r * C;
    const float* tl = p.t_cls + ((size_t)l * p.B * p.Qt + (t < 0 ? 0 : t)) * C;     // batch 0 of layer l
    float lmax = -INFINITY, l0 = (float)C;
    for (int c = 0; c < C; ++c) {
      const float y = t >= 0 ? sigmoid_f(tl[c]) : (float)C;
      if (c == 0) l0 = y;
      lmax = fmaxf(lmax, y);
      const float v = x[c];
      sum_cls += fmaxf(v, 0.f) - v * y + softplus_neg_abs(v);
      gx[c] = kc * (sigmoid_f(v) - y);
    }
    if (p.reweight && l0 != 10.0f) den += lmax;
    float* gb = p.grad_box + r * p.code;
    for (int k = 0; k < p.code; ++k) gb[k] = 0.f;
    if (t >= 0) {
      float tn[10];
      distill_teacher_box(p.t_box + ((size_t)(l * p.B + b) * p.Qt + t) * 10, tn);
      if (finite_f(tn, 10)) {
        const float* bx = p.s_box + r * p.code;
        const float rw = p.reweight ? lmax : 1.0f;
        for (int k = 0; k < 10; ++k) {
          const float d = bx[k] - tn[k], w = 1.0f * p.code_weights[k] * rw;
          sum_reg += fabsf(d) * w;
          gb[k] = w * l1_sign(d);                                             // scaled by reg_weight / divisor below
        }
      }
    }
  }
  // the fixed-order workgroup sum of gd4d_common.h, the three values behind one barrier
  block_sum_put(sum_cls, s_red[0]);
  block_sum_put(sum_reg, s_red[1]);
  block_sum_put(den, s_red[2]);
  __syncthreads();
  if (threadIdx.x == 0) {
    // `0.f +`: these sums always started from +0, and a term of sum_reg can be -0 (a negative code weight times fabsf(0)): kept
    // (the constant wave count unrolls the three chains of LDS reads, so they overlap as they did in one loop: docs/measurements_r47.md)
    constexpr int W = LOSS_ROW_WAVES;
    const float sc_ = 0.f + block_sum_get<W>(s_red[0]), sr_ = 0.f + block_sum_get<W>(s_red[1]), d_ = 0.f + block_sum_get<W>(s_red[2]);
    const float div = p.reweight ? d_ : fmaxf(p.avg_factors[1], 1.0f);
    s_div = div;
    p.loss[2 * l] = nan_to_num_f(sc_ * kc);
    p.loss[2 * l + 1] = nan_to_num_f(p.reg_weight * (sr_ / div));
  }
  __syncthreads();
  const float kb = p.reg_weight / s_div;
  for (int row = threadIdx.x; row < rows; row += blockDim.x) {
    float* gb = p.grad_box + ((size_t)l * rows + row) * p.code;
    for (int k = 0; k < 10; ++k) gb[k] *= kb;
  }
}

}  // namespace gd4d

extern "C" int gd4d_distill_match_cost_fwd(const float* s_cls, const float* s_box, const float* t_cls, const float* t_box, float* cost,
                                           int NL, int B, int Qs, int Qt, int C, int code, int pseudo_gt, float cls_weight,
                                           float reg_weight, void* stream) {
  using namespace gd4d;
  if (!s_cls || !s_box || !t_cls || !t_box || !cost || NL <= 0 || B <= 0 || Qs <= 0 || Qt <= 0 || C <= 0) return GD4D_EINVAL;
  if (code < 8 || C > DC_MAX_C || B > 65535 || NL > 65535) return GD4D_EUNSUPPORTED;
  const long long tiles = (long long)((Qs + DC_TILE - 1) / DC_TILE) * ((Qt + DC_TILE - 1) / DC_TILE);
  if (tiles > INT_MAX) return GD4D_EUNSUPPORTED;
  DistillCostParams p{s_cls, s_box, t_cls, t_box, cost, NL, B, Qs, Qt, C, code, pseudo_gt ? 1 : 0, cls_weight, reg_weight};
  hipLaunchKernelGGL(distill_match_cost_kernel, dim3((unsigned)tiles, B, NL), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" size_t gd4d_lsa_dense_workspace_bytes(int NL, int B, int Q, int max_gt) {
  if (NL <= 0 || B <= 0 || Q <= 0 || max_gt <= 0) return 0;
  return (size_t)NL * B * Q * max_gt * sizeof(float);
}

extern "C" int gd4d_lsa_dense_fwd(const float* cost, const int32_t* gt_start, int32_t* assigned, int32_t* status, void* workspace,
                                  size_t workspace_bytes, int NL, int B, int Q, int sum_gt, int max_gt, void* stream) {
  using namespace gd4d;
  if (!cost || !gt_start || !assigned || !status || NL <= 0 || B <= 0 || Q <= 0 || sum_gt < 0 || max_gt < 0) return GD4D_EINVAL;
  if (max_gt > 0 && (!workspace || workspace_bytes < gd4d_lsa_dense_workspace_bytes(NL, B, Q, max_gt))) return GD4D_EWORKSPACE;
  const int nc = Q > max_gt ? Q : max_gt, nr = Q > max_gt ? max_gt : Q;
  if (nc > LD_THREADS * LD_CPT || (long long)NL * B > INT_MAX) return GD4D_EUNSUPPORTED;
  const size_t lds = (size_t)nr * (8 + 4) + (size_t)nc * (4 + 4) + 64;
  if (lds > 65536 && !allow_dynamic_lds(reinterpret_cast<const void*>(lsa_dense_kernel), (int)lds)) return GD4D_ELAUNCH;
  LsaDenseParams p{cost, gt_start, assigned, status, static_cast<float*>(workspace), NL, B, Q, sum_gt, max_gt};
  hipLaunchKernelGGL(lsa_dense_kernel, dim3(NL * B), dim3(LD_THREADS), lds, static_cast<hipStream_t>(stream), p);
  return check_launch();
}

extern "C" int gd4d_distill_loss_fwd_bwd(const float* s_cls, const float* s_box, const float* t_cls, const float* t_box,
                                         const int32_t* assigned, const float* code_weights, const float* avg_factors, float* loss,
                                         float* grad_cls, float* grad_box, int NL, int B, int Qs, int Qt, int C, int code, int reweight,
                                         float loss_cls_weight, float loss_reg_weight, void* stream) {
  using namespace gd4d;
  if (!s_cls || !s_box || !t_cls || !t_box || !assigned || !code_weights || !avg_factors || !loss || !grad_cls || !grad_box)
    return GD4D_EINVAL;
  if (NL <= 0 || B <= 0 || Qs <= 0 || Qt <= 0 || C <= 0) return GD4D_EINVAL;
  if (code < 10 || code > 16) return GD4D_EUNSUPPORTED;
  DistillLossParams p{s_cls, s_box, t_cls, t_box, assigned, code_weights, avg_factors, loss, grad_cls, grad_box,
                      NL, B, Qs, Qt, C, code, reweight ? 1 : 0, loss_cls_weight, loss_reg_weight};
  hipLaunchKernelGGL(distill_loss_kernel, dim3(NL), dim3(LOSS_ROW_THREADS), 0, static_cast<hipStream_t>(stream), p);
  return check_launch();
}
