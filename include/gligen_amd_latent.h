/* gligen_amd_latent.h -- the start point of a partial sampling in libgligen_amd.so: resize an fp32 latent (or image) and noise it to
 * a timestep in one launch. Image-to-image and the second pass of a two-pass ("hires") generation start a sampler's tail from it.
 * Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_LATENT_H
#define GLIGEN_AMD_LATENT_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the mode argument: torch's F.interpolate modes of the same names, align_corners = False, no antialias */
#define GL_LATENT_NEAREST_EXACT 0
#define GL_LATENT_BILINEAR 1
#define GL_LATENT_BICUBIC 2

/* dst [B][C][h2][w2] = sa * resize(src [B][C][h][w]) + s1 * noise [noise_B][C][h2][w2], fp32 device tensors, one launch, no
 * intermediate tensor. noise == NULL: dst = sa * resize(src) (noise_B is ignored). noise_B is B, or 1: one draw for every sample.
 *   nearest-exact: source index min(floor((2 o + 1) in / (2 out)), in - 1), in integers;
 *   bilinear:      source coordinate (o + 1/2) in / out - 1/2 clamped at 0, two taps per axis;
 *   bicubic:       the same coordinate unclamped, four taps per axis, A = -0.75, tap indices clamped to the edge.
 * The coordinate's floor and fraction are taken in integers; the horizontal taps are summed in ascending order, then the vertical
 * ones; the last step is two rounded products and one rounded sum. At equal sizes the result is therefore sa * src + s1 * noise as
 * fp32 rounds it, bit for bit, in every mode, and two calls give the same bits. Any h, w, h2, w2 >= 1 and any C.
 * Refused by name: dst == src, a noise_B that is neither 1 nor B, an unknown mode. */
int gl_op_latent_renoise(gl_ctx* ctx, const float* src, int B, int C, int h, int w, float* dst, int h2, int w2, int mode, float sa, float s1,
                         const float* noise, int noise_B, gl_stream stream);

/* The taps gl_op_latent_renoise uses along one axis resized in_size -> out_size, computed on the host (no device needed):
 * first_index[o] is the source index of output o's tap 0 before clamping (tap p reads clamp(first_index[o] + p, 0, in_size - 1)),
 * weights[4 o + p] its weight; slots beyond the tap count are 0. Returns the tap count (1, 2 or 4), or -1 with gl_last_error set. */
int gl_latent_resize_taps(int in_size, int out_size, int mode, int* first_index, float* weights);

#ifdef __cplusplus
}
#endif
#endif
