/* gligen_amd_trainer.h -- the optimizer unit of a training run in libgligen_amd.so: what the reference's trainer does to the
 * parameters after the backward (trainer.py:388-391: opt.step() of torch.optim.AdamW, then update_ema, trainer.py:121-123), in one
 * pass over a flat fp32 range. Conventions as in gligen_amd.h. */
#ifndef GLIGEN_AMD_TRAINER_H
#define GLIGEN_AMD_TRAINER_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every pointer is device memory, fp32 [n], no two ranges overlapping. p, m, v: gl_op_adamw_step's update with the same arguments, bit
 * for bit (step counts from 1). Then
 *   ema = fl(ema_rate) * ema + fl(1 - ema_rate) * p_new        p_new: the parameter AFTER this update; 1 - ema_rate formed in double
 * in fp32, two rounded products and a rounded sum. ema_rate 0 copies the parameters, 1 leaves ema alone.
 * 16-byte accesses when all five pointers are 16-byte aligned, 4-byte ones otherwise; n = 0 launches nothing. One launch on `s`.
 * GL_ERR_ARG: a null pointer, n < 0, step < 1, ema_rate outside [0, 1] (a NaN included). */
int gl_op_adamw_ema_step(gl_ctx* ctx, float* p, const float* g, float* m, float* v, float* ema, int64_t n, double lr, double beta1, double beta2,
                         double eps, double weight_decay, double ema_rate, int step, gl_stream s);

#ifdef __cplusplus
}
#endif
#endif
