// The training path's fp32 grid resize (GatedSelfAttentionDense2's residual, reference attention.py:288-291) and its adjoint. See
// train_fusers.hip; entry points in include/gligen_amd_train_fusers.h.
#pragma once
#include "common.h"

namespace gl {

constexpr int kGridResizeMaxSide = 1024;    // sg, sv <= this: the backward's tables (32 sv + 8 sg bytes of LDS) stay under 48 KiB

// dst [B][sv*sv][C] = bicubic resize (torch F.interpolate mode="bicubic", align_corners=False: src = (dst + 0.5) sg / sv - 0.5, A = -0.75,
// taps clamped to the grid) of src [B][sg*sg][C], fp32 rows, any sg, sv in [1, kGridResizeMaxSide]
int grid_resize_fwd_launch(const float* src, int B, int sg, int sv, int C, float* dst, hipStream_t s);
// dsrc [B][sg*sg][C] = the exact adjoint applied to g [B][sv*sv][C]: a gather in a fixed order, no atomics, the forward's weights bit for bit
int grid_resize_bwd_launch(const float* g, int B, int sg, int sv, int C, float* dsrc, hipStream_t s);

}  // namespace gl
