// What the convolution families on the bf16 MFMA (gd4d_depth_net, gd4d_fpn, gd4d_vovnet, gd4d_dcn and their training halves) share
// that is not kernel-specific: the weight image's format and its one packer, and what the partitioned weight gradients have in
// common - the bound on the partition count (CONV_MAX_PARTITIONS, partitions_ok), a partition's share of the tile list
// (partition_range), the in-order sum of the partitions (sum_partitions) - and the workgroup's fixed-order sum (block_sum_256).
// gd4d_conv_wgrad.h holds the two weight-gradient GEMM bodies, gd4d_bf16x3.h the MFMA's C/D row (mfma32_row).
//
// The weight image.  Every one of these GEMMs reads its weight as the MFMA's A operand from a split-bf16 image made of 16-byte items:
// 8 consecutive K values of one output row, in the hi plane or the lo plane (gd4d_bf16x3.h: hi = bf16(x), lo = bf16(x - hi)), ordered
// the way the kernel walks K.  The weight is viewed as A[m][k][tap], M padded with zeros to m_pad, a multiple of the row block MB:
//
//     [..][plane hi, lo][k-group of 8 (KC / 8)][MB rows][8 x bf16]
//
// with the outer index [row block][chunk of KC][tap] (a kernel that walks K chunk by chunk and tap by tap inside a chunk), or
// [tap][row block][chunk] (tap_outer: tap by tap, chunk by chunk inside a tap).  The source is w[(oc * cin + ci) * taps + tap], read
// with M = oc and K = ci, or transposed (M = ci, K = oc: the data gradient's weight), then optionally with the taps flipped
// (taps - 1 - tap: the 180-degree rotation of a stride-1 convolution's adjoint).  The layouts in use:
//
//     image                          MB     KC     outer             transposed   other
//     gd4d_depth_net_image           256    32     block-chunk-tap   no           (also the FPN's 3x3 convolutions)
//     gd4d_depth_net_image_mode(1)   256    32     block-chunk-tap   yes          taps flipped
//     gd4d_fpn_lateral_image         256    32     block-chunk-tap   no           taps = 1
//     gd4d_fpn_lateral_image_mode(1) 256    32     block-chunk-tap   yes          taps = 1, m_pad = ceil(cin / 256) 256: zeros beyond cin
//     gd4d_conv3x3 / osa_concat      32     32     block-chunk-tap   no           taps 9 / 1; independent of the GEMM's M tiling
//     gd4d_dcn_weight_image          Mpad   kc     tap-outer         no           dcn_geometry's (Mpad, kc); one row block, zeros beyond cout
//     gd4d_dcn_weight_image_t        32     cout   tap-outer         yes          one chunk, no flip
//
// The split is split8 (v_cvt_pk_bf16_f32, to nearest even).  Weights are expected finite: a NaN's payload or an fp32 denormal may
// pack differently from a software rounding of the same value, and no test covers them (tests/test_weight_image_gpu.py checks every
// byte of every layout above on finite, normal values).
// hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage: conv_image_kernel 26 VGPRs, partition_sum_kernel 6; no scratch.
#pragma once
#include "gd4d_common.h"

namespace gd4d {

struct ConvImage {
  int cin, cout, taps;   // the source: w (cout, cin, taps) fp32, row-major
  int mb, kc;            // rows of a row block; K values of a chunk (a multiple of 8 that divides K)
  int m_pad;             // M padded to a multiple of mb; rows beyond M are zero
  int tap_outer;         // outer index [tap][row block][chunk] instead of [row block][chunk][tap]
  int transposed;        // M = cin, K = cout instead of M = cout, K = cin
  int flip;              // read tap taps - 1 - tap
};

// Pack w into image (16-byte aligned, 4 m_pad K taps bytes) on `stream`; check_launch()'s code, or GD4D_EUNSUPPORTED for an image of
// 2^31 items or more.
int pack_conv_image(const ConvImage& d, const float* w, void* image, hipStream_t stream);

// dw[i] (i < total) = sum over q of ws[q * total + i] and db[i] (i < nb) = sum over q of ws_b[q * nb + i], q = 0 .. partitions - 1 in
// order: the second launch of the partitioned weight gradients.  check_launch()'s code (of this launch and those before it).
int sum_partitions(const float* ws, const float* ws_b, int partitions, int total, int nb, float* dw, float* db, hipStream_t stream);

// The partition count every partitioned weight gradient accepts (its workspace has one slab per partition).
constexpr int CONV_MAX_PARTITIONS = 4096;
inline bool partitions_ok(int partitions) { return partitions >= 1 && partitions <= CONV_MAX_PARTITIONS; }

// The tiles [t_begin, t_end) of partition `part` of a list of `tiles` cut into `partitions` (empty when there are fewer tiles).
__device__ __forceinline__ void partition_range(int part, int tiles, int partitions, int& t_begin, int& t_end) {
  t_begin = (int)((long long)part * tiles / partitions);
  t_end = (int)((long long)(part + 1) * tiles / partitions);
}

// sum over the workgroup's 256 threads in a fixed order: a tree over LDS (red: 256 floats); the result in every thread
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

}  // namespace gd4d
