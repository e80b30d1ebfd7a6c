// The neck's nearest-upsampling index, defined once: the forward's fused top-down add (gd4d_fpn.hip) and its adjoint
// (gd4d_fpn_train.hip) both call it, so the adjoint's children are exactly the pixels the forward read a coarse pixel for.
#pragma once
#include <hip/hip_runtime.h>

namespace gd4d {

// ATen's nearest source index: min(floor(float(dst) * scale), n_in - 1) with scale = float(n_in) / float(n_out), every step in fp32
__host__ __device__ __forceinline__ int fpn_nearest_src(int dst, float scale, int n_in) {
  const int src = (int)floorf((float)dst * scale);
  return src < n_in - 1 ? src : n_in - 1;
}

}  // namespace gd4d
