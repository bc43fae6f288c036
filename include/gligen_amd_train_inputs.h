/* gligen_amd_train_inputs.h -- the input stage of a training iteration in libgligen_amd.so: what the reference's trainer computes
 * between the VAE and the model (trainer.py:329-364: q_sample, the inpainting mask from the boxes, z * mask, the concatenation), written
 * in one launch as the pixel rows gl_unet_train_step reads (gl_train_unet_in.x / .target). Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_TRAIN_INPUTS_H
#define GLIGEN_AMD_TRAIN_INPUTS_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every pointer is device memory. z, noise: fp32 NCHW [B][C][H][W] (C = the model's in_channels). timesteps: int64 [B], an index into
 * the schedule tables sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod (fp32 [n_t]); an index outside [0, n_t) is the caller's error
 * and is clamped into the range so that no read leaves the tables.
 *   x_noisy = fl(fl(a[t] z) + fl(s[t] noise))           two rounded products, one rounded sum: ldm.py:19-22 on the CPU, bit for bit
 * inpaint = 0: x_rows [B][H*W][C] = x_noisy. inpaint = 1: x_rows [B][H*W][2C + 1] = x_noisy, z * mask, mask (openaimodel.py:447,
 * trainer.py:343-344), with the mask from exactly one of
 *   boxes [B][n_boxes][4], (x0, y0, x1, y1) as fractions in [0, 1]: 1, and 0 inside [int(x0 W), int(x1 W)) x [int(y0 H), int(y1 H)) of
 *     any box (inpaint_mask_func.py:22-32 without its random branches; the products in fp32, truncated towards zero). An all-zero
 *     padding box and a box with x1 < x0 or y1 < y0 mask nothing; a coordinate of 1.0 reaches the border. The reference's mask is
 *     square: H == W is required. Coordinates outside [0, 1] are the caller's error (they mask what falls inside the image).
 *   mask [B][H*W]: an explicit mask, e.g. the reference's random stroke masks, which are drawn on the host.
 * target_rows [B][H*W][C] = noise; t_float [B] = the timesteps as gl_train_unet_in.timesteps takes them. */
typedef struct gl_train_step_inputs_args {
    unsigned struct_size;               /* sizeof(gl_train_step_inputs_args): a caller built against another layout is rejected */
    int B, C, H, W;
    int n_t;                            /* entries of the schedule tables (1000) */
    int n_boxes;                        /* boxes per sample; 0 when `mask` is given */
    int inpaint;
    const float* z;
    const float* noise;
    const int64_t* timesteps;
    const float* sqrt_alphas_cumprod;
    const float* sqrt_one_minus_alphas_cumprod;
    const float* boxes;                 /* inpaint: boxes or mask, the other NULL; else both NULL */
    const float* mask;
    float* x_rows;
    float* target_rows;
    float* t_float;
} gl_train_step_inputs_args;
int gl_train_step_inputs(gl_ctx* ctx, const gl_train_step_inputs_args* args, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
