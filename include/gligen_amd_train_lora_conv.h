/* gligen_amd_train_lora_conv.h -- training LoRA adapters on 3 x 3 convs in libgligen_amd.so (kohya's conv_dim / LoCon form): the
 * low-rank part of one adapted conv by itself. An adapted conv computes y = conv(x, W) + b + scale up(down(x)), scale = alpha / rank,
 * W frozen, down [rank][Ci][3][3] (OIHW, with the base conv's stride and padding: kohya's lora_down.weight as it is), up [Co][rank]
 * (1 x 1, kohya's lora_up.weight without its (1, 1) tail). Activations are fp32 pixel rows [B][H][W][C]. The products run on the
 * fp32-input MFMA of gfx950 over the neighbour rows themselves (no im2col copy); the weight gradients are sums of per-row-chunk
 * partials added in ascending order, so two runs give the same bits.
 * Conventions as in gligen_amd.h: fp32 device pointers, work queued on `s`, GL_OK or an error code with gl_last_error(). */
#ifndef GLIGEN_AMD_TRAIN_LORA_CONV_H
#define GLIGEN_AMD_TRAIN_LORA_CONV_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The low-rank part of one adapted 3 x 3 conv, forward and backward. x [B][H][W][Ci]. geom 0: stride 1, pad 1, output H x W (a
 * ResBlock's convs); 1: stride 2, pad 1, output H/2 x W/2 (Downsample; H and W even); 2: stride 1, pad 1 on the nearest-2x enlarged
 * grid, output 2H x 2W (Upsample). With Mo = B Ho Wo output pixels:
 * Forward: t [Mo][rank] = im2col(x) down^T; y [Mo][Co] += scale t up^T (y is read and written). With dy [Mo][Co]: u [Mo][rank] = dy up;
 * dx [B H W][Ci] += scale (the transposed conv of u with down; read and written); g_down [rank][Ci][3][3] = scale u^T im2col(x);
 * g_up [Co][rank] = scale dy^T t. x, down and up are required; an output that is NULL is not produced. Ci and Co are multiples of
 * 64, 1 <= rank <= 128; x and dy are 16-byte aligned. */
int gl_op_lora_conv3(gl_ctx* ctx, int B, int H, int W, int Ci, int Co, int rank, float scale, int geom, const float* x, const float* down,
                     const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
