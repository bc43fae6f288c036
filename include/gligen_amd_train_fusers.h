/* gligen_amd_train_fusers.h -- training the gatedSA2 and gatedCA fuser models in libgligen_amd.so. The whole-UNet steps
 * (gl_unet_train_step, gl_unet_train_step_spatial, gl_unet_train_step_spatial_classes) take the fuser type from
 * gl_unet_config.fuser_kind (0 gatedSA, 1 gatedSA2, 2 gatedCA); this header holds the block slice with a kind and the fp32 grid resize
 * the gatedSA2 fuser is built on, forward and adjoint. Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_TRAIN_FUSERS_H
#define GLIGEN_AMD_TRAIN_FUSERS_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gl_op_block_train for a BasicTransformerBlock with fuser_type gatedSA (0), gatedSA2 (1) or gatedCA (2); kind 0 launches what
 * gl_op_block_train launches.
 * gatedSA2 (reference attention.py:272-297): the same 37 parameter slots; only the Ng grounding tokens are queries, their projected
 * outputs -- an sg x sg grid -- are resized to the sv x sv visual grid (gl_op_grid_resize) and gated. dims->Ng and dims->N must be
 * squares; anything else is refused by name.
 * gatedCA (attention.py:207-212): GatedCrossAttentionDense has no fuser.linear: the two slots "fuser.linear.weight" / ".bias" of
 * gl_train_block_param_names are NULL in params and grads (a pointer there is an error that names the key), and
 * fuser.attn.to_k / to_v are [C][ctx_dim] and read objs. */
int gl_op_block_train_fuser(gl_ctx* ctx, int fuser_kind, const gl_train_block_dims* dims, const float* const* params, const float* x,
                            const float* objs, const float* context, const float* target, float* y, float* loss, float* dx, float* dobjs,
                            float* const* grads, gl_stream s);

/* dst [B][sv*sv][C] = src [B][sg*sg][C] resized as torch's F.interpolate(mode = "bicubic", align_corners = False) resizes a square
 * grid: source coordinate (dst + 0.5) sg / sv - 0.5, cubic convolution with A = -0.75, taps clamped to the grid. fp32 device rows,
 * channels innermost; any sg, sv in [1, 1024] (upscale, identity, downscale, non-integer ratios). */
int gl_op_grid_resize(gl_ctx* ctx, const float* src, int B, int sg, int sv, int C, float* dst, gl_stream s);

/* dsrc [B][sg*sg][C] = the transpose of that operator applied to g [B][sv*sv][C]: <resize(t), g> = <t, dsrc> with the forward's
 * weights bit for bit. A gather in a fixed order without atomics: two calls give the same bits. */
int gl_op_grid_resize_backward(gl_ctx* ctx, const float* g, int B, int sg, int sv, int C, float* dsrc, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
