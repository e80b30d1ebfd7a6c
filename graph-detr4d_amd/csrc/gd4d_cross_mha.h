// What gd4d_cross_mha.hip (forward) and gd4d_cross_mha_train.hip (both packs, backward) share beyond the device pieces of
// gd4d_attn_pieces.h: the sizes, the key-split plan, the layout checks and the two fragment layouts of the split-bf16 planes.
//
// A plane holds rows (keys, or queries) x 32 channels of one (batch, head) in steps of 32 rows, two fragments of 64 lanes x 8 bf16
// per step, in one of two layouts - named after the planes the forward reads:
//   row fragments ("K layout"):    [b][h][step][t][lane = 16 g + i][8 channels 8 g ..]   <-> row 32 step + 16 t + i
//       the A or B operand of a 16x16x32 MFMA that reduces over CHANNELS (S^T = K Q^T, dP^T = V dout^T and their transposes)
//   column fragments ("V layout"): [b][h][step][half][lane = 16 g + i][j]                <-> channel 16 half + i,
//                                                                                            row 32 step + 16 (j >> 2) + 4 g + (j & 3)
//       the A operand of an MFMA that reduces over the step's 32 ROWS, against a B operand that is the other product's accumulator
//       registers as they stand (O^T += V^T P^T, dq^T += K^T dS^T, dk^T += Q^T dS, dv^T += dout^T P)
// Rows past the end of the last step are zeros.
// Who holds what, each as hi / mid / lo planes unless noted:
//   K rows      inference and training forward, both backward kernels        (gd4d_cross_mha_pack_kv / _pack_kv_train: k_planes)
//   V columns   the forwards; inference packs hi / lo only                    (v_planes)
//   V rows      both backward kernels: dP = dout V^T                          (vk_planes)
//   K columns   the query-side backward kernel: dq^T += K^T dS^T              (kv_planes)
//   q scale log2(e) and dout, each as rows and as columns: both backward kernels, packed per gd4d_cross_mha_bwd call into its workspace
//   (the rows are the queries; pad queries are zeros there too, with Dq = 0 and lse = +inf beside them).
#pragma once
#include "gd4d_attn_pieces.h"

namespace gd4d {

constexpr int XM_D = ATTN_D;      // head dimension
constexpr int XM_WAVES = 4;

__host__ __device__ inline int xm_split_first(int steps, int splits, int s) { return (int)((long long)steps * s / splits); }

// first element of fragment (b, h, step, t) of a plane, for this lane
__host__ __device__ inline size_t xm_frag(int H, int steps, int b, int h, int step, int t, int lane) {
  return ((((((size_t)b * H + h) * steps + step) * 2 + t) * 64) + lane) * 8;
}

// What the four entry points that take planes check after their own arguments and their plan, in this order: the
// smallest row stride of their fp32 operands and the plane stride (EINVAL), then `aligned` (EALIGN)
inline int xm_check_layout(int min_ld, long long plane_stride, int Lk, int B, int H, bool aligned) {
  if (min_ld < H * XM_D || plane_stride < (long long)gd4d_cross_mha_plane_elems(Lk, B, H) || (plane_stride & 7)) return GD4D_EINVAL;
  return aligned ? GD4D_OK : GD4D_EALIGN;
}

inline int xm_plan(int Lq, int Lk, int B, int H, int q_tile, int splits, int* qt_out, int* splits_out) {
  if (Lq <= 0 || Lk <= 0 || B <= 0 || H <= 0 || q_tile < 0 || splits < 0) return GD4D_EINVAL;
  if ((q_tile != 0 && q_tile != 32 && q_tile != 64) || splits > GD4D_CROSS_MHA_MAX_SPLITS || B > 65535 ||
      (long long)H * GD4D_CROSS_MHA_MAX_SPLITS > 65535)
    return GD4D_EUNSUPPORTED;
  const int steps = (Lk + 31) / 32;
  const int qt = q_tile ? q_tile : 64;
  int s = splits;
  if (s == 0) {
    // At two waves per SIMD (226 registers) two workgroups share a compute unit: as many splits as keep the grid within the 512
    // places of 256 compute units (one residency: 900 queries -> 4 splits, 480 workgroups; 6 splits need a second round and measure
    // slower), and at least one workgroup per compute unit.  A split is worth a workgroup from four steps per wave (below that the
    // merge's traffic is most of what it does).
    const long long groups = (long long)((Lq + qt - 1) / qt) * H * B;
    s = (int)((256 + groups - 1) / groups);
    if (512 / groups > s) s = (int)(512 / groups);
    const int most = steps / (4 * XM_WAVES) > 1 ? steps / (4 * XM_WAVES) : 1;
    if (s > most) s = most;
    if (s > GD4D_CROSS_MHA_MAX_SPLITS) s = GD4D_CROSS_MHA_MAX_SPLITS;
  }
  *qt_out = qt;
  *splits_out = s;
  return GD4D_OK;
}

}  // namespace gd4d
