// The optimizer step of the reference's training recipe over ONE flat parameter / gradient buffer: gradient-norm clipping
// (mmcv's GradientCumulativeOptimizerHook -> torch.nn.utils.clip_grad_norm_, max_norm 35, L2) followed by AdamW (lr 2e-4,
// weight decay 0.01) - projects/configs/detr4d/detr4d_res50_deform_pe_testaug_320_fullset_ceph.py:205-213.
//
// Two launches whatever the number of parameters (torch's clip + foreach AdamW: ~12 multi-tensor launches over 230 tensors):
//   gd4d_adamw_flat  (1) per-block sums of squares of the gradients, in a fixed order; one thread advances the step counter
//                    (2) every block adds the partial sums in the same order (the same norm everywhere, run-to-run identical),
//                        forms the clip coefficient min(1, max_norm / (norm + 1e-6)) and updates its slice:
//                            g = coef * grad;  p *= 1 - lr * wd;  m = m + (1 - b1) (g - m);  v = b2 v + (1 - b2) g g
//                            p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The step counter lives on the device (a replayed hipGraph cannot change a kernel argument).
//
//   gd4d_adamw_recipe_flat  the same two launches with everything else a run changes on the device as well (gd4d_recipe_state):
//                    (1) sums of squares of g / scale and a "saw a non-finite g / scale" flag per block; one thread evaluates the
//                        learning-rate schedule for this iteration (double), advances the iteration counter and latches the loss scale
//                    (2) every block combines sums and flags in the same order; non-finite: nothing but the skipped-step count moves;
//                        else the update above with g = coef * grad / scale and the element's group's lr * lr_mult, wd * decay_mult
//                        (a sorted range table, looked up once per change of range); one thread updates the loss scale as
//                        torch.amp.GradScaler.update does.  What pass 2's blocks read (lr, scale_in_use, step_in_flight) is written
//                        by pass 1 only; what pass 2's one thread writes no block of this step reads.
#include <algorithm>
#include <cmath>

#include "gd4d_common.h"

namespace gd4d {

constexpr int OPT_THREADS = 256;
constexpr int OPT_BLOCKS = 512;          // partial sums (<= 1024)

__global__ __launch_bounds__(OPT_THREADS) void adamw_sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ partial,
                                                                  float* __restrict__ state) {
  __shared__ float red[OPT_THREADS / 64];
  const long long per = ((n + 3) / 4 + gridDim.x - 1) / gridDim.x * 4;        // a block's contiguous range (multiple of 4)
  const long long lo = (long long)blockIdx.x * per, hi = min(n, lo + per);
  float s = 0.f;
  for (long long i = lo + 4ll * threadIdx.x; i < hi; i += 4ll * OPT_THREADS) {
    if (i + 3 < hi) {
      const float4 v = *reinterpret_cast<const float4*>(g + i);
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    } else {
      for (long long j = i; j < hi; ++j) s += g[j] * g[j];
    }
  }
  block_sum_put(s, red);                                                      // (a sum of squares: no wave holds -0)
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = block_sum_get<OPT_THREADS / 64>(red);
    if (blockIdx.x == 0) state[0] += 1.0f;                                    // the step this update is
  }
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_apply_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                  float* __restrict__ v, long long n, const float* __restrict__ partial,
                                                                  int nparts, float* __restrict__ state, float lr, float b1, float b2,
                                                                  float eps, float wd, float max_norm) {
  __shared__ float s_coef, s_c1, s_c2;
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < nparts; ++i) t += (double)partial[i];                 // the same order in every block
    const float norm = (float)sqrt(t);
    float coef = 1.f;
    if (max_norm > 0.f) coef = fminf(1.f, max_norm / (norm + 1e-6f));         // clip_grad_norm_'s clamp
    const float step = state[0];
    s_coef = coef;
    s_c1 = (float)((double)lr / (1.0 - pow((double)b1, (double)step)));     // (bias corrections in double, as torch's host code)
    s_c2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, (double)step)));
    if (blockIdx.x == 0) state[1] = norm;                                     // (for the host: the norm before clipping)
  }
  __syncthreads();
  const float coef = s_coef, step_size = s_c1, inv_bc2 = s_c2, decay = 1.f - lr * wd;
  for (long long i = 4ll * ((long long)blockIdx.x * OPT_THREADS + threadIdx.x); i < n; i += 4ll * OPT_THREADS * gridDim.x) {
    const int cnt = (int)min(4ll, n - i);
    float pv[4], gv[4], mv[4], vv[4];
    if (cnt == 4) {
      *reinterpret_cast<float4*>(pv) = *reinterpret_cast<const float4*>(p + i);
      *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(g + i);
      *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(m + i);
      *reinterpret_cast<float4*>(vv) = *reinterpret_cast<const float4*>(v + i);
    } else {
      for (int j = 0; j < cnt; ++j) { pv[j] = p[i + j]; gv[j] = g[i + j]; mv[j] = m[i + j]; vv[j] = v[i + j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) break;
      const float gj = gv[j] * coef;
      const float pd = pv[j] * decay;
      const float mj = mv[j] + (1.f - b1) * (gj - mv[j]);
      const float vj = b2 * vv[j] + (1.f - b2) * gj * gj;
      pv[j] = pd - step_size * (mj / (sqrtf(vj) * inv_bc2 + eps));
      mv[j] = mj; vv[j] = vj;
    }
    if (cnt == 4) {
      *reinterpret_cast<float4*>(p + i) = *reinterpret_cast<const float4*>(pv);
      *reinterpret_cast<float4*>(m + i) = *reinterpret_cast<const float4*>(mv);
      *reinterpret_cast<float4*>(v + i) = *reinterpret_cast<const float4*>(vv);
    } else {
      for (int j = 0; j < cnt; ++j) { p[i + j] = pv[j]; m[i + j] = mv[j]; v[i + j] = vv[j]; }
    }
  }
}

// ---- the recipe step: schedule, loss scale, overflow decision, clip, per-group AdamW from device-resident state ----
// mmcv 1.x LrUpdaterHook, restated (include/gd4d.h has the formulas): it = iterations finished before this one
__device__ double recipe_lr(const gd4d_recipe_config& c, long long it) {
  const long long ep = it / c.iters_per_epoch;
  double r = c.base_lr;
  if (c.policy == GD4D_LR_COSINE) {
    const double f = c.by_epoch ? (double)ep / (double)c.max_epochs : (double)it / (double)c.max_iters;
    r = c.end_lr + 0.5 * (c.base_lr - c.end_lr) * (cos(3.14159265358979323846 * f) + 1.0);
  } else if (c.policy == GD4D_LR_STEP) {
    const long long prog = c.by_epoch ? ep : it;
    long long e = 0;
    if (c.step_every > 0) e = prog / c.step_every;
    else for (int i = 0; i < c.n_milestones; ++i) e += c.milestones[i] <= prog;
    r = c.base_lr * pow(c.gamma, (double)e);
  }
  if (c.warmup != GD4D_WARMUP_NONE && it < c.warmup_iters) {
    const double x = (double)it / (double)c.warmup_iters;
    if (c.warmup == GD4D_WARMUP_LINEAR) r *= 1.0 - (1.0 - x) * (1.0 - c.warmup_ratio);
    else if (c.warmup == GD4D_WARMUP_CONSTANT) r *= c.warmup_ratio;
    else r *= pow(c.warmup_ratio, 1.0 - x);
  }
  return r;
}

__global__ __launch_bounds__(OPT_THREADS) void recipe_sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ partial,
                                                                   int* __restrict__ flags, gd4d_recipe_state* __restrict__ st,
                                                                   gd4d_recipe_config cfg) {
  __shared__ float red[OPT_THREADS / 64];
  const float inv = (float)(1.0 / (double)st->loss_scale);                     // (nobody writes loss_scale in this launch)
  const long long per = ((n + 3) / 4 + gridDim.x - 1) / gridDim.x * 4;        // adamw_sumsq_kernel's ranges and order
  const long long lo = (long long)blockIdx.x * per, hi = min(n, lo + per);
  float s = 0.f;
  int bad = 0;
  for (long long i = lo + 4ll * threadIdx.x; i < hi; i += 4ll * OPT_THREADS) {
    if (i + 3 < hi) {
      float4 v = *reinterpret_cast<const float4*>(g + i);
      v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      bad |= !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
    } else {
      for (long long j = i; j < hi; ++j) { const float a = g[j] * inv; s += a * a; bad |= !isfinite(a); }
    }
  }
  block_sum_put(s, red);                                                      // (a sum of squares: no wave holds -0)
  bad = __syncthreads_or(bad);                                                // the barrier between put and get
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = block_sum_get<OPT_THREADS / 64>(red);
    flags[blockIdx.x] = bad;
    if (blockIdx.x == 0) {                                                    // this iteration: its rate, its scale, the step it would be
      const long long it = st->iteration;
      st->lr = (float)recipe_lr(cfg, it);
      st->iteration = it + 1;
      st->scale_in_use = st->loss_scale;
      st->step_in_flight = st->optimizer_steps + 1;
    }
  }
}

__global__ __launch_bounds__(OPT_THREADS) void recipe_apply_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                                   float* __restrict__ v, long long n, const float* __restrict__ partial,
                                                                   const int* __restrict__ flags, int nparts,
                                                                   gd4d_recipe_state* __restrict__ st,
                                                                   const gd4d_recipe_range* __restrict__ ranges, int n_ranges,
                                                                   gd4d_recipe_config cfg) {
  __shared__ float s_coef, s_c2, s_inv, s_lr;
  __shared__ double s_bc1;
  int bad = 0;
  for (int i = threadIdx.x; i < nparts; i += OPT_THREADS) bad |= flags[i];
  bad = __syncthreads_or(bad);                                                // the same decision in every block (and on every rank)
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < nparts; ++i) t += (double)partial[i];                 // the same order in every block
    const float norm = (float)sqrt(t);
    float coef = 1.f;
    if (cfg.max_norm > 0.f) coef = fminf(1.f, cfg.max_norm / (norm + 1e-6f));
    const double step = (double)st->step_in_flight;
    s_coef = coef;
    s_bc1 = 1.0 - pow((double)cfg.beta1, step);
    s_c2 = (float)(1.0 / sqrt(1.0 - pow((double)cfg.beta2, step)));
    s_inv = (float)(1.0 / (double)st->scale_in_use);
    s_lr = st->lr;
    if (blockIdx.x == 0) {                                                    // words no block of this step reads
      st->grad_norm = norm;
      st->found_inf = bad;
      if (bad) st->skipped_steps += 1; else st->optimizer_steps = st->step_in_flight;
      float sc = st->loss_scale;                                              // torch.amp.GradScaler.update
      int tr = st->growth_tracker;
      if (!cfg.dynamic_scale) {
        sc = (float)cfg.init_scale;
      } else if (bad) {
        sc = (float)((double)sc * cfg.backoff_factor);
        tr = 0;
      } else if (tr + 1 == cfg.growth_interval) {
        const float grown = (float)((double)sc * cfg.growth_factor);
        if (isfinite(grown)) sc = grown;
        tr = 0;
      } else {
        tr += 1;
      }
      st->loss_scale = sc;
      st->growth_tracker = tr;
    }
  }
  __syncthreads();
  const long long first = 4ll * ((long long)blockIdx.x * OPT_THREADS + threadIdx.x), stride = 4ll * OPT_THREADS * gridDim.x;
  if (bad) {                                                                  // skipped: p, m, v and Adam's t stay as they were
    if (cfg.zero_grads)
      for (long long i = first; i < n; i += stride) {
        if (n - i >= 4) *reinterpret_cast<float4*>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        else for (long long j = i; j < n; ++j) g[j] = 0.f;
      }
    return;
  }
  const float coef = s_coef, inv = s_inv, inv_bc2 = s_c2, lr = s_lr, b1 = cfg.beta1, b2 = cfg.beta2, eps = cfg.eps;
  const double bc1 = s_bc1;
  long long r_lo = 0, r_hi = 0;                                               // the range the last quad was in
  float decay = 1.f, step_size = 0.f;
  for (long long i = first; i < n; i += stride) {
    if (i >= r_hi || i < r_lo) {                                              // (ranges cover [0, n) without gaps: the first end > i)
      int a = 0, b = n_ranges - 1;
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (ranges[mid].end > i) b = mid; else a = mid + 1;
      }
      const gd4d_recipe_range r = ranges[a];
      r_lo = r.begin; r_hi = r.end;
      const float lr_g = lr * r.lr_mult, wd_g = cfg.weight_decay * r.decay_mult;
      decay = 1.f - lr_g * wd_g;
      step_size = (float)((double)lr_g / bc1);
    }
    const int cnt = (int)min(4ll, n - i);
    float pv[4], gv[4], mv[4], vv[4];
    if (cnt == 4) {
      *reinterpret_cast<float4*>(pv) = *reinterpret_cast<const float4*>(p + i);
      *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(g + i);
      *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(m + i);
      *reinterpret_cast<float4*>(vv) = *reinterpret_cast<const float4*>(v + i);
    } else {
      for (int j = 0; j < cnt; ++j) { pv[j] = p[i + j]; gv[j] = g[i + j]; mv[j] = m[i + j]; vv[j] = v[i + j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) break;
      const float gj = gv[j] * inv * coef;
      const float pd = pv[j] * decay;
      const float mj = mv[j] + (1.f - b1) * (gj - mv[j]);
      const float vj = b2 * vv[j] + (1.f - b2) * gj * gj;
      pv[j] = pd - step_size * (mj / (sqrtf(vj) * inv_bc2 + eps));
      mv[j] = mj; vv[j] = vj;
    }
    if (cnt == 4) {
      *reinterpret_cast<float4*>(p + i) = *reinterpret_cast<const float4*>(pv);
      *reinterpret_cast<float4*>(m + i) = *reinterpret_cast<const float4*>(mv);
      *reinterpret_cast<float4*>(v + i) = *reinterpret_cast<const float4*>(vv);
      if (cfg.zero_grads) *reinterpret_cast<float4*>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int j = 0; j < cnt; ++j) { p[i + j] = pv[j]; m[i + j] = mv[j]; v[i + j] = vv[j]; if (cfg.zero_grads) g[i + j] = 0.f; }
    }
  }
}

}  // namespace gd4d

extern "C" size_t gd4d_adamw_flat_workspace_bytes(void) { return (size_t)gd4d::OPT_BLOCKS * sizeof(float); }

extern "C" int gd4d_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* state, void* workspace,
                               size_t workspace_bytes, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                               float max_norm, void* stream) {
  using namespace gd4d;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !workspace || n <= 0) return GD4D_EINVAL;
  if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(weight_decay >= 0.f)) return GD4D_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq)) return GD4D_EALIGN;
  if (workspace_bytes < gd4d_adamw_flat_workspace_bytes()) return GD4D_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(adamw_sumsq_kernel, dim3(OPT_BLOCKS), dim3(OPT_THREADS), 0, s, grads, (long long)n, partial, state);
  if (int rc = check_launch()) return rc;
  const long long quads = (n + 3) / 4;
  const int blocks = (int)std::min<long long>((quads + OPT_THREADS - 1) / OPT_THREADS, 2048);
  hipLaunchKernelGGL(adamw_apply_kernel, dim3(blocks), dim3(OPT_THREADS), 0, s, params, grads, exp_avg, exp_avg_sq, (long long)n, partial,
                     OPT_BLOCKS, state, lr, beta1, beta2, eps, weight_decay, max_norm);
  return check_launch();
}

extern "C" size_t gd4d_adamw_recipe_flat_workspace_bytes(void) { return (size_t)gd4d::OPT_BLOCKS * (sizeof(float) + sizeof(int)); }
extern "C" size_t gd4d_adamw_recipe_flat_state_bytes(void) { return sizeof(gd4d_recipe_state); }

extern "C" int gd4d_adamw_recipe_flat(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* state, size_t state_bytes,
                                      void* workspace, size_t workspace_bytes, int64_t n, const gd4d_recipe_config* config,
                                      const gd4d_recipe_range* ranges, const gd4d_recipe_range* ranges_dev, int n_ranges, void* stream) {
  using namespace gd4d;
  static_assert(sizeof(gd4d_recipe_state) == 64 && sizeof(gd4d_recipe_range) == 24, "layouts include/gd4d.h documents");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !workspace || !config || !ranges || !ranges_dev || n <= 0) return GD4D_EINVAL;
  if (n_ranges < 1 || n_ranges > GD4D_RECIPE_MAX_RANGES) return GD4D_EINVAL;
  const gd4d_recipe_config& c = *config;
  if (!(c.base_lr >= 0.0) || !(c.beta1 >= 0.f && c.beta1 < 1.f) || !(c.beta2 >= 0.f && c.beta2 < 1.f) || !(c.eps > 0.f) ||
      !(c.weight_decay >= 0.f) || !std::isfinite(c.max_norm))
    return GD4D_EINVAL;
  if (c.policy < GD4D_LR_FIXED || c.policy > GD4D_LR_STEP || c.warmup < GD4D_WARMUP_NONE || c.warmup > GD4D_WARMUP_EXP) return GD4D_EINVAL;
  if (c.iters_per_epoch < 1 || c.warmup_iters < 0 || (c.warmup != GD4D_WARMUP_NONE && !(c.warmup_ratio > 0.0))) return GD4D_EINVAL;
  if (c.policy == GD4D_LR_COSINE && ((c.by_epoch ? c.max_epochs : c.max_iters) < 1 || !(c.end_lr >= 0.0))) return GD4D_EINVAL;
  if (c.policy == GD4D_LR_STEP) {
    if (!(c.gamma > 0.0) || c.step_every < 0 || c.n_milestones < 0 || c.n_milestones > GD4D_RECIPE_MAX_MILESTONES) return GD4D_EINVAL;
    if (c.step_every == 0 && c.n_milestones == 0) return GD4D_EINVAL;
    for (int i = 1; i < c.n_milestones; ++i)
      if (c.milestones[i] <= c.milestones[i - 1]) return GD4D_EINVAL;
  }
  if (!(c.init_scale > 0.0) || !std::isfinite((float)c.init_scale)) return GD4D_EINVAL;
  if (!(c.growth_factor > 1.0) || !(c.backoff_factor > 0.0 && c.backoff_factor < 1.0) || c.growth_interval < 1) return GD4D_EINVAL;
  // the table: sorted, no overlap, no gap, every range starting on a 16-byte quad (a quad never straddles two groups)
  int64_t at = 0;
  for (int i = 0; i < n_ranges; ++i) {
    if (ranges[i].begin != at || ranges[i].end <= ranges[i].begin || (ranges[i].begin & 3)) return GD4D_EINVAL;
    if (!(ranges[i].lr_mult >= 0.f) || !(ranges[i].decay_mult >= 0.f)) return GD4D_EINVAL;
    at = ranges[i].end;
  }
  if (at != n) return GD4D_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
      (reinterpret_cast<uintptr_t>(state) & 7u) || (reinterpret_cast<uintptr_t>(ranges_dev) & 7u) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
    return GD4D_EALIGN;
  if (state_bytes < gd4d_adamw_recipe_flat_state_bytes() || workspace_bytes < gd4d_adamw_recipe_flat_workspace_bytes()) return GD4D_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  int* flags = reinterpret_cast<int*>(partial + OPT_BLOCKS);
  gd4d_recipe_state* st = static_cast<gd4d_recipe_state*>(state);
  hipLaunchKernelGGL(recipe_sumsq_kernel, dim3(OPT_BLOCKS), dim3(OPT_THREADS), 0, s, grads, (long long)n, partial, flags, st, c);
  if (int rc = check_launch()) return rc;
  const long long quads = (n + 3) / 4;
  const int blocks = (int)std::min<long long>((quads + OPT_THREADS - 1) / OPT_THREADS, 2048);
  hipLaunchKernelGGL(recipe_apply_kernel, dim3(blocks), dim3(OPT_THREADS), 0, s, params, grads, exp_avg, exp_avg_sq, (long long)n, partial,
                     flags, OPT_BLOCKS, st, ranges_dev, n_ranges, c);
  return check_launch();
}
