/* gligen_amd_maps.h -- semantic maps as class indices in libgligen_amd.so: a u8 class map stands for its one-hot fp32 planes, and the
 * entry points below compute from the map, bit for bit, what gl_op_spatial_tokens and gl_op_grounding_downsample compute from the
 * planes. A class value >= the number of classes is "no class": all of its planes are zero (255 is the null input). Conventions as
 * in gligen_amd.h (error codes, gl_last_error(), raw device pointers unless a parameter says "host", work enqueued on the passed
 * stream). */
#ifndef GLIGEN_AMD_MAPS_H
#define GLIGEN_AMD_MAPS_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One map of a gl_op_class_map_resize batch: a single-channel u8 image and the box of it that is resized. Sides are limited to 16384. */
typedef struct gl_class_map_desc {
    const uint8_t* pixels;       /* device u8 [height][width], rows row_stride bytes apart */
    int width, height;
    int row_stride;              /* bytes, >= width */
    int box_x, box_y, box_w, box_h;   /* inside the image */
} gl_class_map_desc;

/* PIL.Image.crop(box).resize((out_w, out_h), Image.NEAREST) of S single-channel u8 images of different sizes in one launch, byte for
 * byte: `out` is the device tensor u8 [S][out_h][out_w]. `maps_host` is a host array. The index tables are built on the host
 * (gl_class_map_index_table) and copied with the descriptors in one block on `s`; the device is not synchronised. At most 1024 maps
 * per call; anything outside the limits is refused with a message that names it. */
int gl_op_class_map_resize(gl_ctx* ctx, const gl_class_map_desc* maps_host, int S, int out_w, int out_h, uint8_t* out, gl_stream s);
/* The source sample of each of out_size resized samples along one axis, as Pillow's nearest path accumulates it in double
 * (a = box_len / out_size; xo = a / 2; t[x] = (int)xo, xo += a), + box0. Host only; needs no context and no device. idx_host holds
 * `cap` ints; a buffer that is too small is refused and not written. */
int gl_class_map_index_table(int box0, int box_len, int out_size, int* idx_host, int cap);
/* gl_op_spatial_tokens for a semantic-map tokenizer, from the class map `cls` (device u8 [B][H][W]) instead of its in_dim one-hot
 * planes: the nearest resize to resize_input and in_conv are one gather launch, the rest is the same launches. tokens: fp32
 * [B][(resize_input/32)^2][out_dim], bit for bit those of the planes. */
int gl_op_spatial_tokens_classes(gl_ctx* ctx, const uint8_t* cls, int B, int H, int W, const float* mask, float* tokens, gl_stream s);
/* gl_op_grounding_downsample (mode nearest, with its two convs) from the class map `cls` (device u8 [B][H][W]) of n_classes classes
 * (<= 256): w1 fp32 [c_mid][n_classes][4][4] (c_mid a multiple of 4), w2 fp32 [c_out][c_mid][4][4], R a multiple of 4. out: fp32
 * [B][c_out][R/4][R/4], bit for bit that of the planes. */
int gl_op_grounding_downsample_classes(gl_ctx* ctx, const uint8_t* cls, int B, int H, int W, int n_classes, int R,
                                       const float* w1, const float* b1, int c_mid, const float* w2, const float* b2, int c_out,
                                       float* out, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
