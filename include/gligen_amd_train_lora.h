/* gligen_amd_train_lora.h -- training LoRA adapters in libgligen_amd.so: the training iteration of the discrete-tokenizer models with
 * an array of adapters on the frozen Linears of the SpatialTransformers, and the low-rank part of one adapted Linear by itself.
 * An adapted Linear computes y = x W^T + scale (x down^T) up^T, scale = alpha / rank, W [N][K] frozen, down [rank][K], up [N][rank]
 * (kohya's lora_down / lora_up). The low-rank products run on the fp32-input MFMA of gfx950 straight from the fp32 activations;
 * the weight gradients are sums of per-row-chunk partials added in ascending order, so two runs give the same bits.
 * Conventions as in gligen_amd.h: fp32 device pointers, work queued on `s`, GL_OK or an error code with gl_last_error(). */
#ifndef GLIGEN_AMD_TRAIN_LORA_H
#define GLIGEN_AMD_TRAIN_LORA_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One adapter. name: the state_dict key of the Linear's weight -- attn1 / attn2 .to_q / .to_k / .to_v / .to_out.0, ff.net.0.proj,
 * ff.net.2 of a SpatialTransformer's transformer_blocks.0, or the SpatialTransformer's proj_in / proj_out (1 x 1 convs, run as
 * Linears over pixel rows); a fuser's own Linears train in full and take none. g_down / g_up: where the gradients go, shaped like
 * down / up and overwritten (NULL: not formed). 1 <= rank <= 128. */
typedef struct gl_lora_adapter {
    const char* name;
    const float* down;
    const float* up;
    float* g_down;
    float* g_up;
    int rank;
    float scale;
} gl_lora_adapter;

/* The training iteration of gligen_amd.h (text, text+image and keypoint tokenizers, every fuser kind, with or without inpaint_mode)
 * with n_adapters adapters; every other argument as there. grads may be NULL for every parameter: adapters alone are trained then.
 * An adapter's gradients are final at the milestone of its SpatialTransformer (gl_train_wait_grads), like that block's fuser
 * gradients. The weight of an adapted Linear takes no gradient of its own. With n_adapters 0 this is the unadapted iteration, launch
 * for launch. */
int gl_unet_train_step_lora(gl_ctx* ctx, const gl_unet_config* cfg, const gl_train_unet_in* in, int n_params, const char* const* names,
                            const float* const* params, float* const* grads, const gl_lora_adapter* adapters, int n_adapters, float* eps_out,
                            float* loss, gl_stream s);

/* The low-rank part of one adapted Linear, forward and backward. x [M][K]; down is [rank][K] (down_kr 0) or [K][rank] (down_kr 1);
 * up is [N][rank] (up_rn 0) or [rank][N] (up_rn 1): both orientations of the small operand of every kernel can be reached.
 * Forward: t [M][rank] = x down^T; y [M][N] += scale t up^T (y is read and written). With dy [M][N]: u [M][rank] = dy up;
 * dx [M][K] += scale u down (read and written); g_down = scale u^T x in down's layout; g_up = scale dy^T t in up's layout.
 * x, down and up are required; an output that is NULL is not produced. K and N are multiples of 64, any M >= 1, 1 <= rank <= 128;
 * x and dy are 16-byte aligned. */
int gl_op_lora_linear(gl_ctx* ctx, int M, int K, int N, int rank, float scale, int down_kr, int up_rn, const float* x, const float* down,
                      const float* up, const float* dy, float* t, float* y, float* u, float* dx, float* g_down, float* g_up, gl_stream s);

/* Rows per partial sum of the weight-gradient kernel for M rows: a function of M alone. */
int gl_lora_wgrad_chunk_rows(int M);

#ifdef __cplusplus
}
#endif
#endif
