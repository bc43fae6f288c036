// Resize of an fp32 NCHW tensor fused with q_sample: the start point of a partial sampling (image-to-image, the second pass of a
// two-pass "hires" generation). See latent.hip; entry points in include/gligen_amd_latent.h.
#pragma once
#include "common.h"

namespace gl {

enum LatentResizeMode { LATENT_NEAREST_EXACT = 0, LATENT_BILINEAR = 1, LATENT_BICUBIC = 2 };

// dst [B][C][h2][w2] = sa * resize(src [B][C][h][w]) + s1 * noise [noise_B][C][h2][w2]   (noise null: dst = sa * resize(src)).
// torch's F.interpolate(mode, align_corners=False, antialias=False) for nearest-exact, bilinear and bicubic; noise_B is B or 1
// (one draw for every sample). Any h, w, h2, w2 >= 1 and any C; dst must not be src.
int latent_renoise_launch(const float* src, int B, int C, int h, int w, float* dst, int h2, int w2, int mode, float sa, float s1,
                          const float* noise, int noise_B, hipStream_t s);

// Host restatement of the kernel's taps of one axis resized n_in -> n_out: first_index[o] is the source index of tap 0 BEFORE clamping
// (tap p reads clamp(first_index[o] + p, 0, n_in - 1)), weights[4 o + p] its weight (taps beyond the mode's count: 0).
// Returns the tap count in *n_taps: 1, 2 or 4.
int latent_resize_taps(int n_in, int n_out, int mode, int* first_index, float* weights, int* n_taps);

}  // namespace gl
