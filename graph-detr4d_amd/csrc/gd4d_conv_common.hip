// The weight-image packer and the partition sum of the convolution families: gd4d_conv_common.h has the format and the contracts.
#include "gd4d_conv_common.h"

#include "gd4d_bf16x3.h"

namespace gd4d {

// one 16-byte item per thread: item i = ((outer * 2 + plane) * (KC / 8) + k-group) * MB + row
__global__ __launch_bounds__(256) void conv_image_kernel(const ConvImage d, const float* __restrict__ w, char* __restrict__ image,
                                                         const unsigned items) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= items) return;
  const int m_rows = d.transposed ? d.cin : d.cout, k_len = d.transposed ? d.cout : d.cin;
  const unsigned kgs = d.kc / 8, chunks = k_len / d.kc, blocks = d.m_pad / d.mb;
  const int row = i % d.mb;
  unsigned r = i / d.mb;
  const int kgrp = r % kgs;
  r /= kgs;
  const int plane = r & 1;
  r >>= 1;
  int blk, chunk, tap;
  if (d.tap_outer) {
    chunk = r % chunks, r /= chunks;
    blk = r % blocks, tap = r / blocks;
  } else {
    tap = r % d.taps, r /= d.taps;
    chunk = r % chunks, blk = r / chunks;
  }
  const int m = blk * d.mb + row, k0 = chunk * d.kc + kgrp * 8;
  if (d.flip) tap = d.taps - 1 - tap;
  // w[(oc * cin + ci) * taps + tap]: consecutive k are consecutive ci (stride taps), transposed consecutive oc (stride cin taps)
  const float* const src = w + (d.transposed ? (size_t)k0 * d.cin + m : (size_t)m * d.cin + k0) * d.taps + tap;
  const size_t step = d.transposed ? (size_t)d.cin * d.taps : (size_t)d.taps;
  float v[8] = {};
  if (m < m_rows) {
    if (step == 1) {   // a 1x1 weight's K run is contiguous: two 16-byte loads
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[j * step];
    }
  }
  u32x4 hi, lo;
  split8(v, hi, lo);
  *reinterpret_cast<u32x4*>(image + (size_t)i * 16) = plane ? lo : hi;
}

int pack_conv_image(const ConvImage& d, const float* w, void* image, hipStream_t stream) {
  const long long items = (long long)d.m_pad * (d.transposed ? d.cout : d.cin) * d.taps / 4;   // 2 planes x groups of 8
  if (items <= 0 || items >= (1ll << 31)) return GD4D_EUNSUPPORTED;
  hipLaunchKernelGGL(conv_image_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, d, w, static_cast<char*>(image),
                     (unsigned)items);
  return check_launch();
}

__global__ __launch_bounds__(256) void partition_sum_kernel(const float* __restrict__ ws, const float* __restrict__ ws_b,
                                                            const int partitions, const int total, const int nb,
                                                            float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) {
    float s = 0.f;
    for (int q = 0; q < partitions; ++q) s += ws[(size_t)q * total + i];
    dw[i] = s;
  }
  if (i < nb) {
    float s = 0.f;
    for (int q = 0; q < partitions; ++q) s += ws_b[(size_t)q * nb + i];
    db[i] = s;
  }
}

int sum_partitions(const float* ws, const float* ws_b, int partitions, int total, int nb, float* dw, float* db, hipStream_t stream) {
  hipLaunchKernelGGL(partition_sum_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, ws, ws_b, partitions, total, nb, dw, db);
  return check_launch();
}

}  // namespace gd4d
