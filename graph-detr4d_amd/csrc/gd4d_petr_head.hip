// gd4d_petr_keys_fwd: the key side of PETRHead / PETRv2Head in ONE kernel (dense_heads/petr_head.py:383-403, petrv2_head.py:444-469
// of the reference).  Per tile of 128 pixels of the R = bs n cameras:
//     pe      = position_encoder(frustum coordinates)            192 -> 1024 -> 256, the inputs generated in registers (Mlp2Fr)
//     gate    = conv_expand(relu(conv_reduce(x)))                256 ->  256 -> 256, x = input_proj(feat) read from its NCHW map
//     key_pos = pe * sigmoid(gate) + sine                        (no gate image - PETRHead, with_fpe=False: pe + sine)
//     memory  = x                                                the transpose of the tile
// both written as the KEY-MAJOR rows PETRTransformer's decoder takes, row (cam H W + pix) bs + b of (n H W, bs, 256): the two permute
// copies of (bs, n, 256, H, W) tensors PETRTransformer.forward makes are not made, and neither the (R, S, 192) frustum tensor, the
// (R, S, 1024) hidden activation nor the (R, S, 256) embedding between the two MLPs exists.
//
// The body is gd4d_mlp2_pe_se_fwd's: ml_frustum_split + ml_phase<12> for the embedding, which waits in 128 registers while
// ml_phase<16> runs the gate (gd4d_mlp2_body.h); what is new is the epilogue - no `feat +` term, two outputs - and the row map.
// Differences to the Detr3DHeadPE fuse: the gate reads input_proj's output, not the raw level, and the result is the transformer's
// key_pos, not a new feature map.
//
// Epilogue layout (C / D of v_mfma_f32_32x32x16): a lane holds, per tile of 32 channels, 4 groups of 4 consecutive pixels of ONE
// channel.  x's four pixels are one 16-byte read per lane from the NCHW map (the lines the gate's A operand was loaded from a
// moment ago; with no gate their first read), stored as `memory` - 32 consecutive channels of a key row per half-wave, 128 bytes -
// next to key_pos.  A bit copy: memory == x.permute exactly.
// The kernel, THE row map (petr_key_row) and the launch are in gd4d_petr_keys.h, shared with the training instantiation
// (gd4d_petr_head_train.hip).
#include "gd4d_petr_keys.h"

// The launch geometry, on the host (no GPU work): *grid = workgroups (one per tile of 128 rows), *rows_per_block = 128; key_rows, when
// not NULL, receives for every input row m = (b n + cam) H W + pix the key row the kernel writes it to, bs n H W entries.
extern "C" int gd4d_petr_keys_plan(int bs, int n, int H, int W, int32_t* grid, int32_t* rows_per_block, int64_t* key_rows) {
  using namespace gd4d;
  int M = 0;
  if (bs <= 0 || n <= 0 || H <= 0 || W <= 0) return GD4D_EINVAL;
  if (!petr_keys_shape(bs, n, H, W, &M)) return GD4D_EUNSUPPORTED;
  if (grid) *grid = (M + ML_BM - 1) / ML_BM;
  if (rows_per_block) *rows_per_block = ML_BM;
  if (key_rows)
    for (int m = 0; m < M; ++m) key_rows[m] = petr_key_row(m, H * W, bs, n);
  return GD4D_OK;
}

extern "C" int gd4d_petr_keys_fwd(const float* x, const float* img2lidar, int bs, int n, int C, int H, int W, float pad_h, float pad_w,
                                  int D, float depth_start, const double* position_range, const void* pe_image, const float* pe_b2,
                                  int pe_H, const void* se_image, const float* se_b2, int se_H, const float* sine, float* memory,
                                  float* key_pos, void* stream) {
  return gd4d::petr_keys_launch<false>(x, img2lidar, bs, n, C, H, W, pad_h, pad_w, D, depth_start, position_range, pe_image, pe_b2, pe_H,
                                       se_image, se_b2, se_H, sine, memory, key_pos, nullptr, nullptr, stream);
}
