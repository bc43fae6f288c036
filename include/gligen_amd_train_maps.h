/* gligen_amd_train_maps.h -- training the semantic-map model from u8 class maps in libgligen_amd.so: the training iteration of
 * gl_unet_train_step_spatial with the tokenizer's map and grounding_extra_input as class indices (gligen_amd_maps.h) instead of their
 * one-hot fp32 planes, and the weight-gradient operator it is built on. Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_TRAIN_MAPS_H
#define GLIGEN_AMD_TRAIN_MAPS_H
#include "gligen_amd_maps.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gl_train_spatial_in with both maps as class indices: a value >= the class count (cfg->tok_in_dim for the tokenizer, ds_n_in for the
 * downsampler) is "no class", 255 is the null input. */
typedef struct gl_train_spatial_classes_in {
    const uint8_t* map;                 /* the tokenizer's class map [B][map_h][map_w] (sem) */
    int map_h, map_w;
    const float* mask;                  /* [B] */
    const uint8_t* extra;               /* grounding_extra_input as a class map [B][extra_h][extra_w] */
    int extra_h, extra_w;
    int ds_resize;                      /* the downsampler's resize_input */
    int ds_mode;                        /* 1 nearest: the only mode class maps have */
    int ds_n_in;                        /* classes the downsampler reads (sem: 152) */
    int ds_mid;                         /* channels of its first 4x4 stride-2 conv, a multiple of 4 (sem: 16) */
} gl_train_spatial_classes_in;
/* gl_unet_train_step_spatial for a semantic-map model (cfg->tok_in_dim > 0, extra_channels > 0, a nearest-mode downsampler with its
 * two convs) fed from class maps. The forward is bit for bit that of the one-hot planes, so the loss, eps_out and every gradient are
 * too, except the four tensors whose gradient is summed in another order: position_net.in_conv.{weight,bias} and
 * downsample_net.layers.0.{weight,bias} (gl_op_class_conv_wgrad). The resized planes and their im2col buffers are never allocated.
 * A tokenizer without in_dim, a downsampler that is not nearest mode or has no layers are refused by name. */
int gl_unet_train_step_spatial_classes(gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, const gl_train_spatial_classes_in* sp,
                                       int n_params, const char* const* names, const float* const* params, float* const* grads, float* eps_out,
                                       float* loss, gl_stream s);

/* Weight and bias gradient of a conv over the one-hot planes of a class map, from the map: with cls' = `cls` (device u8 [B][H][W])
 * through F.interpolate(size = R, mode = "nearest"),
 *   dW[o][c][ky][kx] = sum over (b, y, x) of [cls'(b, s y + ky - 1, s x + kx - 1) == c] dy[b][o][y][x],   db[o] = sum of dy[b][o][y][x]
 * kind 0: the tokenizer's in_conv (3x3, stride 1, pad 1; c_out = 3; dy fp32 [B][3][R][R]); kind 1: the downsampler's first conv (4x4,
 * stride 2, pad 1; c_out a multiple of 4; R even; dy fp32 [B][c_out][R/2][R/2]). dW: fp32 [c_out][n_classes][k][k], db: fp32 [c_out];
 * either may be NULL. A tap in the padding or a class >= n_classes (<= 256) adds nothing. No atomics: per-tile partial sums are added
 * in tile order, so two calls give the same bits. Anything outside the limits is refused with a message that names the limit. */
int gl_op_class_conv_wgrad(gl_ctx* ctx, int kind, const uint8_t* cls, int B, int H, int W, int n_classes, int R, const float* dy, int c_out,
                           float* dW, float* db, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
