/* gligen_amd_image.h -- the image front end of libgligen_amd.so: PIL.Image.resize + crop + normalisation of 8-bit RGB images on the
 * MI355X, bit for bit what Pillow and transformers' CLIPImageProcessor compute. Conventions as in gligen_amd.h (error codes,
 * gl_last_error(), raw device pointers unless a parameter says "host", work enqueued on the passed stream). */
#ifndef GLIGEN_AMD_IMAGE_H
#define GLIGEN_AMD_IMAGE_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One image of a gl_op_image_resample batch: the u8 source with 3 interleaved channels, the size it is resampled to and the box of the
 * resampled image that is kept. Sides (source and resized) are limited to 16384. */
typedef struct gl_image_desc {
    const uint8_t* pixels;       /* device u8 [height][width][3], rows row_stride bytes apart */
    int width, height;
    int row_stride;              /* bytes, >= 3 * width */
    int resized_w, resized_h;
    int crop_x, crop_y, crop_w, crop_h;   /* inside the resized image */
} gl_image_desc;

/* The image front end of the CLIP vision tower (transformers CLIPImageProcessor: resize, center_crop, rescale + normalize; reference
 * gligen_inference.py:104-128 calls it through CLIPProcessor) and, more generally, PIL.Image.resize + crop of 8-bit RGB images: S
 * images of different sizes in two launches, bit for bit what Pillow computes -- fixed-point coefficients, a u8 intermediate between
 * the horizontal and the vertical pass, an axis that keeps its size is copied. filter: 0 bicubic, 1 bilinear. `images` is a host array.
 *   out_kind 0: `out` is a host array of S device pointers, image i -> u8 [crop_h][crop_w][3] (crops may differ);
 *   out_kind 1: `out` is the device tensor fp32 [S][3][crop_h][crop_w] (all crops equal) = gl_clip_vision_encode's pixel_values; a
 *               sample v of channel c becomes lut_host[c * 256 + v] (host, 3 x 256 floats: (v / 255 - mean_c) / std_c as the caller
 *               rounds it) -- the device looks values up and never divides.
 * The source is read, and the intermediate kept (in the arena), only for the rows and columns the crop needs. Host work per call
 * (tables cached per (in, out, filter)), one host-to-device copy of descriptors and tables on `s`, no synchronisation of the device.
 * Anything outside the limits is refused with a message that names it. */
int gl_op_image_resample(gl_ctx* ctx, const gl_image_desc* images, int S, int filter, int out_kind, const float* lut_host, void* out, gl_stream s);
/* The resampler's table for one axis, computed on the host in double as Pillow's precompute_coeffs + normalize_coeffs_8bpc do; needs
 * no context and no device. *ksize = taps per output sample; bounds (host, 2 * out_size ints, or NULL): first source sample and tap
 * count of each output sample; coeffs (host, out_size * ksize ints, or NULL): the coefficients in units of 2^-22, 0 beyond the count.
 * bounds_cap / coeffs_cap: ints the buffers hold (call with NULL buffers first for ksize). */
int gl_image_resample_coeffs(int in_size, int out_size, int filter, int* ksize, int* bounds, int bounds_cap, int* coeffs, int coeffs_cap);

#ifdef __cplusplus
}
#endif
#endif
