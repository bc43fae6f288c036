/* gligen_amd_train_run.h -- the gradient unit of a training run in libgligen_amd.so: what a trainer does to the gradients between the
 * backward and the update -- the sum over micro-batches (gradient accumulation), the global L2 norm and the coefficient of
 * torch.nn.utils.clip_grad_norm_(..., norm_type=2, error_if_nonfinite=False), AdamW (+ EMA) on the clipped gradient -- and per-sample
 * loss weights (min-SNR) for the training step. Conventions as in gligen_amd.h.
 *
 * Every range is flat fp32 device memory. 16-byte accesses when every pointer of a call is 16-byte aligned, 4-byte ones otherwise,
 * with the same bits from both; n = 0 launches nothing; one launch per call on `s`. No kernel uses atomics: every sum has one fixed
 * order, so two calls on the same data give the same bits. GL_ERR_ARG: a null pointer, n < 0, and what each entry names. */
#ifndef GLIGEN_AMD_TRAIN_RUN_H
#define GLIGEN_AMD_TRAIN_RUN_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GL_GRAD_ACCUM_FIRST 0  /* acc = g                                  (replaces zeroing acc)            */
#define GL_GRAD_ACCUM_MIDDLE 1 /* acc = acc + g                                                              */
#define GL_GRAD_ACCUM_LAST 2   /* g = (acc + g) * (float)(1.0 / k)         acc is left alone                 */

/* The sum of k micro-batch gradients and its mean, one pass per micro-batch; every sum and the product are rounded on their own.
 * The mean lands in the GRADIENT range, so whatever follows (exchange, update) reads what it reads without accumulation.
 * acc and g [n] do not overlap. GL_ERR_ARG also for k < 1 and an unknown mode. */
int gl_op_grad_accumulate(gl_ctx* ctx, float* acc, float* g, int64_t n, int mode, int k, gl_stream s);

/* The squared L2 norm of g [n] as gl_grad_sqnorm_partials(n) fp32 partial sums, one per GL_GRAD_NORM_CHUNK elements:
 * partials[c] = sum of g[i]^2 over chunk c, each square rounded, summed in a fixed order -- every thread of a 256-thread workgroup a
 * chain of GL_GRAD_NORM_CHAIN squares, the 64 chains of a wave in 6 pairwise levels, the 4 wave sums in index order.
 * The number of partials depends on n alone (0 for n <= 0); it is a host function and touches no device. */
#define GL_GRAD_NORM_CHUNK 16384
#define GL_GRAD_NORM_CHAIN 64
int64_t gl_grad_sqnorm_partials(int64_t n);
int gl_op_grad_sqnorm(gl_ctx* ctx, const float* g, int64_t n, float* partials, gl_stream s);

/* From `count` partials -- of one range, or of several laid side by side --, summed in double in a fixed order: the partials are cut
 * into 256 contiguous segments of ceil(count / 256), each summed in index order (one thread per segment), and the 256 segment sums
 * are then added in index order -- the index order of the partials with that one fixed grouping, a function of count alone:
 *   out2[0] = (float)sqrt(sum)                              the norm
 *   out2[1] = min(1, max_norm / (out2[0] + 1e-6f))          the coefficient, in fp32
 * which is what clip_grad_norm_ computes and clamps. A NaN or inf norm gives the coefficient torch's gives (NaN, 0); nothing is
 * skipped. One workgroup. count = 0: norm 0, coefficient 1. GL_ERR_ARG also for count < 0 and a max_norm that is not > 0. */
int gl_op_clip_coef(gl_ctx* ctx, const float* partials, int64_t count, float max_norm, float* out2, gl_stream s);

/* The updates of gl_op_adamw_step and of the AdamW + EMA entry point of gligen_amd_trainer.h with their arguments, on the gradient
 * fl(g * coef[0]): given the same coefficient, p, m, v (and ema) get bit for bit what those give on a gradient scaled by one fp32
 * product per element. coef is device memory (out2 + 1 above), read by the kernel: the step needs no host sync. g is NOT scaled in
 * place, as torch would: nothing behind the update reads it, and the store would be a fourth stream of an HBM-bound pass.
 * GL_ERR_ARG also for step < 1 and an ema_rate outside [0, 1]. */
int gl_op_adamw_clip_step(gl_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                          double weight_decay, int step, const float* coef, gl_stream s);
int gl_op_adamw_ema_clip_step(gl_ctx* ctx, float* p, const float* g, float* m, float* v, float* ema, int64_t n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, double ema_rate, int step, const float* coef, gl_stream s);

/* Per-sample loss weights w [B] (fp32, device) for the NEXT training step on this context -- any of the gl_unet_train_step* entry
 * points, the LoRA, spatial-map, class-map and inpainting ones included --: that step computes
 *   loss = (1/n) sum_b w[b] sum_i (y - target)^2,   d loss / dy = 2 w[b] (y - target) / n        n = all elements of y
 * instead of mse_loss (w = 1 everywhere is mse_loss up to the summation order). The step clears the weights whether it succeeds or
 * fails; a B other than the step's is GL_ERR_ARG from the step, before anything is launched. w must stay valid until the step has
 * run on its stream. w = NULL with B = 0 clears. Min-SNR-gamma weighting is w[b] = min(snr(t_b), gamma) / snr(t_b). */
int gl_train_set_loss_weights(gl_ctx* ctx, const float* w, int B);

#ifdef __cplusplus
}
#endif
#endif
