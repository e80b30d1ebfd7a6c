// The pieces the dense softmax-attention kernels are made of, each written once: gd4d_self_attn.hip (with gd4d_mha_body.h),
// gd4d_cross_mha.hip and gd4d_cross_mha_train.hip include this header.  One exception, decided by a timing rule
// (docs/measurements_r41.md, section 3): the self-attention kernels keep their own LDS merge and the split-bf16 body its own
// softmax update (gd4d_mha_body.h) - the same operations in the same order as combine_key_slices<false> and softmax_step<8>.
//   softmax_step            one tile of the base-2 online softmax
//   KeySliceShared, publish_key_slice, merge_key_slices, combine_key_slices, store_attn
//                           the merge of the (m, l, O) triples of waves (LDS) or of key splits (workspace) that saw different keys
//   walk_steps              a wave's round-robin steps with one step of look-ahead
//   Planes3, load_planes, split_planes3, products6, xm_x6
//                           hi / mid / lo bf16 pieces of a fragment and the six-product arithmetic on them
//   KeyStepMask             the 32 mask bits of a key step
//   attn_check_drop         the dropout arguments of an entry point
// The register layout they all assume: a score tile is S^T (MFMA rows = keys, columns = queries), lane (qi = lane & 15,
// g = lane >> 4) holds query qi's scores of the keys 4 g + r (+ 16 per further tile), and O^T rows d = 4 g + r and 16 + 4 g + r.
#pragma once
#include "gd4d_common.h"
#include "gd4d_bf16x3.h"

namespace gd4d {

constexpr int ATTN_D = 32;        // head dimension of every kernel here
constexpr float ATTN_LOG2E = 1.4426950408889634f, ATTN_LN2 = 0.6931471805599453f;

// ------------------------------------------------------------ softmax ------------------------------------------------------------
// x[0 .. N) reduced as a balanced tree: ((x0 . x1) . (x2 . x3)) . ((x4 . x5) . (x6 . x7)).  The shape is part of the result of a sum.
template <int N>
__device__ __forceinline__ float tree_max(const float* x) {
  if constexpr (N == 1) return x[0];
  else return fmaxf(tree_max<N / 2>(x), tree_max<N / 2>(x + N / 2));
}
template <int N>
__device__ __forceinline__ float tree_sum(const float* x) {
  if constexpr (N == 1) return x[0];
  else return tree_sum<N / 2>(x) + tree_sum<N / 2>(x + N / 2);
}

// One tile of the online softmax.  s: this lane's N scores of one query (already times scale log2(e), masked keys at -inf), replaced
// by their probabilities exp2(s - m); m: the query's running maximum (the same in its four lanes), l: this lane's partial sum of
// probabilities.  Returns the factor exp2(m_old - m_new) the caller owes its O registers; dropout, if any, is the caller's too and
// comes after this call, so that l (and the saved lse) stay those of the full softmax.
// The softmax runs in base 2 - a probability is ONE v_exp_f32 instead of expf's range reduction + exp2 + ldexp (~15 instructions;
// the fp32 kernel issued 195 vector instructions per tile and was bound by them, profiles/r04_pmc_step_inflight1.txt).
// GUARD: while every key so far is masked, m_new is -inf and exp2(-inf - -inf) would be NaN: the weights are taken against 0
// instead and stay at exactly 0.  A caller that skips the steps without an unmasked key (gd4d_cross_mha.hip) never has m_new = -inf
// and leaves the two instructions out.
template <int N, bool GUARD = true>
__device__ __forceinline__ float softmax_step(float (&s)[N], float& m, float& l) {
  static_assert(N == 4 || N == 8, "a lane holds one or two tiles of four scores");
  float tmax = tree_max<N>(s);
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
  const float m_new = fmaxf(m, tmax);
  const float m_use = (GUARD && m_new == -__builtin_inff()) ? 0.f : m_new;
  const float corr = __builtin_amdgcn_exp2f(m - m_use);              // m = -inf -> 0
#pragma unroll
  for (int j = 0; j < N; ++j) s[j] = __builtin_amdgcn_exp2f(s[j] - m_use);
  l = l * corr + tree_sum<N>(s);
  m = m_new;
  return corr;
}

// ------------------------------------------------------- merge of key slices -------------------------------------------------------
// (mm, num, den) of n slices of one query's keys, slice w holding (m_of(w), l_of(w), o_of(w)): the common maximum, and O and l
// summed with the factors exp2(m_w - mm), in slice order.  out = num / den, lse = mm ln 2 + log den (store_attn).
// A slice that saw no unmasked key holds (-inf, 0, 0).  GUARD: its factor must be 0, so the common maximum is replaced by 0 when
// it is -inf itself - a row with every key masked then gives out = 0 / 0 = NaN and lse = -inf (the cross-attention core's
// contract).  Without GUARD the same row forms exp2(-inf - -inf) = NaN: out and lse are both NaN, as ATen's softmax of a row of
// -inf (the self-attention core's contract, tests/test_dense_gpu.py pins it; its kernels carry this form as their own code).
template <bool GUARD, class M, class L, class O>
__device__ __forceinline__ void combine_key_slices(const int n, M m_of, L l_of, O o_of, float& mm, float& num, float& den) {
  mm = m_of(0);
  for (int w = 1; w < n; ++w) mm = fmaxf(mm, m_of(w));
  const float m_use = (GUARD && mm == -__builtin_inff()) ? 0.f : mm;
  num = 0.f;
  den = 0.f;
  for (int w = 0; w < n; ++w) {
    const float f = __builtin_amdgcn_exp2f(m_of(w) - m_use);
    num += o_of(w) * f;
    den += l_of(w) * f;
  }
}

// row = q B + b of (Lq, B, H * 32) `out` with row stride ldo and of the optional (Lq, B, H) `lse` (natural units: what the backward
// kernels read); the thread of channel 0 writes the lse
__device__ __forceinline__ void store_attn(float* out, float* lse, const size_t row, const int ldo, const int H, const int h, const int d,
                                           const float mm, const float num, const float den) {
  out[row * ldo + h * ATTN_D + d] = num / den;
  if (lse && d == 0) lse[row * H + h] = mm * ATTN_LN2 + logf(den);
}

// LDS of a workgroup of WAVES waves that own ROWS queries and split their keys: one row of 33 floats per (wave, query), so that
// both the lanes of a tile (query qi, channels 4 g + r) and the merge's threads (consecutive channels) spread over the banks
template <int WAVES, int ROWS>
struct KeySliceShared {
  float m[WAVES][ROWS];
  float l[WAVES][ROWS];
  float o[WAVES][ROWS][ATTN_D + 1];
};

// lane (qi, g) of `wave` hands over one query tile: row = 16 tile + qi, its m, its partial l (summed over the query's four lanes here)
// and its eight O^T registers
template <int WAVES, int ROWS>
__device__ __forceinline__ void publish_key_slice(KeySliceShared<WAVES, ROWS>& sh, const int wave, const int row, const int g, const float m,
                                                  float l, const f32x4& o0, const f32x4& o1) {
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (g == 0) { sh.m[wave][row] = m; sh.l[wave][row] = l; }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sh.o[wave][row][4 * g + r] = o0[r];
    sh.o[wave][row][16 + 4 * g + r] = o1[r];
  }
}

// ... and, once every wave has published, the workgroup's 64 WAVES threads take the (query i, channel d) pairs in turn -
// consecutive threads, consecutive channels - and hand sink(i, d, mm, num, den) each pair of the first `rows` queries
template <bool GUARD, int WAVES, int ROWS, class Sink>
__device__ __forceinline__ void merge_key_slices(const KeySliceShared<WAVES, ROWS>& sh, const int tid, const int rows, Sink sink) {
  __syncthreads();
  for (int e = tid; e < ROWS * ATTN_D; e += 64 * WAVES) {
    const int i = e / ATTN_D, d = e % ATTN_D;
    if (i >= rows) continue;
    float mm, num, den;
    combine_key_slices<GUARD>(WAVES, [&](int w) { return sh.m[w][i]; }, [&](int w) { return sh.l[w][i]; },
                              [&](int w) { return sh.o[w][i][d]; }, mm, num, den);
    sink(i, d, mm, num, den);
  }
}

// ---------------------------------------------------------- step walker ----------------------------------------------------------
// Wave `wave` of WAVES takes the steps first + wave, first + wave + WAVES, ... below `last`: fetch(step, data) requests a step's
// operands, compute(step, data) consumes them, and the next step's are requested before this step's are consumed.  q / k / v arrive
// cold from other XCDs (~2 us per round trip) and a wave has only a few steps: "request, wait, compute" per step was a chain of
// exposed round trips.
template <int WAVES, class Step, class Fetch, class Compute>
__device__ __forceinline__ void walk_steps(const int first, const int last, const int wave, Fetch fetch, Compute compute) {
  Step cur, nxt;
  if (first + wave < last) fetch(first + wave, cur);
  for (int step = first + wave; step < last; step += WAVES) {
    if (step + WAVES < last) fetch(step + WAVES, nxt);
    compute(step, cur);
    cur = nxt;
  }
}

// ------------------------------------------------- hi / mid / lo planes (gd4d_cross_mha.h) -------------------------------------------------
struct Planes3 { u32x4 h, m, l; };     // one lane's 8 bf16 of a fragment in each piece (x = h + m + l; two pieces: h + l, m unused)

// a fragment's pieces from PLANES planes `plane` elements apart; e = xm_frag(...), this lane's first element
template <int PLANES = 3>
__device__ __forceinline__ Planes3 load_planes(const unsigned short* base, const long long plane, const size_t e) {
  Planes3 x{};
  x.h = *reinterpret_cast<const u32x4*>(base + e);
  if constexpr (PLANES == 3) x.m = *reinterpret_cast<const u32x4*>(base + plane + e);
  x.l = *reinterpret_cast<const u32x4*>(base + (PLANES - 1) * plane + e);
  return x;
}

__device__ __forceinline__ Planes3 split_planes3(const float* v) {
  Planes3 x;
  split8x3(v, x.h, x.m, x.l);
  return x;
}

// a b with both operands as hi + mid + lo: six products (lo x lo, lo x mid, mid x lo dropped), smallest terms first, in ONE order
// of the pieces of K and of its partner wherever a score is formed - the forward and both backward kernels must rebuild the same
// bits.  K_IS_A: K's pieces are the A operand (S^T = K Q^T); otherwise they are B (S = Q K^T: the transposed tile of the same products
// in the same order).  Products that are not scores (P V, dout V^T, K^T dS^T, ...) use the K_IS_A order.
// Three products hold a score to ~2^-17 of the sum of its terms' magnitudes - 1.6e-4 on a score of 57, which is the log-sum-exp
// of a row one key dominates; six hold fp32 to ~2^-24 (the arithmetic of GD4D_CHAIN_EXACT).
template <bool K_IS_A = true>
__device__ __forceinline__ f32x4 products6(const Planes3& a, const Planes3& b) {
  f32x4 t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.m), frag(b.m), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  if constexpr (K_IS_A) {
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.l), frag(b.h), t, 0, 0, 0);      // k_lo q_hi
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.h), frag(b.l), t, 0, 0, 0);      // k_hi q_lo
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.m), frag(b.h), t, 0, 0, 0);      // k_mid q_hi
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.h), frag(b.m), t, 0, 0, 0);      // k_hi q_mid
  } else {
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.h), frag(b.l), t, 0, 0, 0);      // q_hi k_lo
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.l), frag(b.h), t, 0, 0, 0);      // q_lo k_hi
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.h), frag(b.m), t, 0, 0, 0);      // q_hi k_mid
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.m), frag(b.h), t, 0, 0, 0);      // q_mid k_hi
  }
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a.h), frag(b.h), t, 0, 0, 0);
}

// acc + a b: the six products are summed on their own before they meet the accumulator
__device__ __forceinline__ f32x4 xm_x6(const Planes3& a, const Planes3& b, const f32x4 acc) { return acc + products6(a, b); }

// ------------------------------------------------------------- key mask -------------------------------------------------------------
// The (B, Lk) key-padding mask of one 32-key step: 32 lanes read one byte each (with the step's operands), a ballot turns them
// into the step's 32 bits.  A key past Lk counts as masked.
struct KeyStepMask {
  unsigned byte;
  __device__ __forceinline__ void fetch(const uint8_t* mask, const int b, const int Lk, const int step, const int lane) {
    const int key = step * 32 + (lane & 31);
    byte = key >= Lk ? 1u : (mask ? (unsigned)mask[(size_t)b * Lk + key] : 0u);
  }
  // wave-uniform: bit i <-> key 32 step + i; 0xffffffff = nothing to see in this step
  __device__ __forceinline__ unsigned bits() const { return (unsigned)__ballot(byte != 0); }
  // bit 16 t + r <-> lane group g's score register r of key tile t
  static __device__ __forceinline__ unsigned of_lane(const unsigned bits, const int g) { return bits >> (4 * g); }
};

// -------------------------------------------------------------- host --------------------------------------------------------------
// The dropout arguments of an entry point: a probability outside [0, 1) or one without a seed is EINVAL; more (batch, head, query,
// key) elements than the 32-bit dropout ids count is EUNSUPPORTED.  Called after the caller's own check of pointers and sizes and
// before its check of head size, head count and mask kind (EUNSUPPORTED as well).
inline int attn_check_drop(const float drop_p, const void* seed, const double elements) {
  if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && !seed)) return GD4D_EINVAL;
  if (drop_p > 0.f && elements >= 4294967296.0) return GD4D_EUNSUPPORTED;
  return GD4D_OK;
}

}  // namespace gd4d
