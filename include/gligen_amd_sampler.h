/* gligen_amd_sampler.h -- how the sampler of libgligen_amd.so schedules the classifier-free-guidance pair. Conventions as in
 * gligen_amd.h. */
#ifndef GLIGEN_AMD_SAMPLER_H
#define GLIGEN_AMD_SAMPLER_H
#include "gligen_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two halves of a classifier-free-guidance evaluation inside the sampling loop (reference plms.py:116-127: the model runs on the
 * cond and the uncond input) get the same latent, the same extra first-conv input and the same timestep; they differ in their
 * conditioning only. on = 1 (default): the layers in front of the first one that reads conditioning -- the first ResBlock and the
 * first transformer's GroupNorm, proj_in, norm1 and attn1 in the shipped models -- run once per evaluation, at the latent batch, and
 * both halves read the result. The inputs of the two runs are bit-identical and the shared launches keep the full batch's kernel,
 * tile and K split, so this removes work and changes no bit of the result. on = 0: every layer at the full batch. The single-evaluation entry points take
 * per-sample timesteps and never share. Process-wide; contexts drop their captured graphs when it changes. The tail of
 * the row-policy report (";cfg_shared_prefix=1 evals=.. rows_at_prefix=.. rows_periodic=..") counts what the host issued in shared
 * form. A measurement aid (same-process A/B); the reference has no counterpart. */
int gl_set_cfg_shared_prefix(int on);

#ifdef __cplusplus
}
#endif
#endif
