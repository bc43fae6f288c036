// Host interface of train_run.hip (include/gligen_amd_train_run.h): what a training run does to the flat gradient ranges between the
// backward and the update -- accumulation over micro-batches, the global gradient norm and its clipping coefficient, the clipped
// AdamW (+ EMA) update -- and the per-sample weighted loss of the training step. Every kernel of these is defined in train_run.hip
// and launched from there (the build has no relocatable device code); the other units call these functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace gl {

// grad_sqnorm_kernel's geometry: one fp32 partial per kGradNormChunk elements; inside a chunk every thread of a 256-thread workgroup
// sums kGradNormChain squares in a fixed fp32 chain, a wave sums its 64 chains in kGradNormWaveDepth butterfly levels and thread 0
// adds the kGradNormWaves wave sums in index order
constexpr int kGradNormBlock = 256;
constexpr int kGradNormChain = 64;
constexpr int kGradNormChunk = kGradNormBlock * kGradNormChain;
constexpr int kGradNormWaves = kGradNormBlock / 64;
constexpr int kGradNormWaveDepth = 6;

enum GradAccumMode { GRAD_ACCUM_FIRST = 0, GRAD_ACCUM_MIDDLE = 1, GRAD_ACCUM_LAST = 2 };

// first: acc = g; middle: acc = acc + g; last: g = (acc + g) * (float)(1.0 / k), acc left alone. One launch; n = 0 launches nothing.
int grad_accumulate(float* acc, float* g, size_t n, int mode, int k, hipStream_t s);
size_t grad_sqnorm_partials(size_t n);      // ceil(n / kGradNormChunk)
// partials[c] = the sum of g[i]^2 over chunk c, in the fixed order above: the same bits from the 16-byte and the 4-byte path
int grad_sqnorm(const float* g, size_t n, float* partials, hipStream_t s);
// out2[0] = (float)sqrt(sum of the partials in double), out2[1] = min(1, max_norm / (out2[0] + 1e-6f)); a NaN stays a NaN
int clip_coef(const float* partials, size_t count, float max_norm, float* out2, hipStream_t s);
// adamw_step / adamw_ema_step (train.h) on g * coef[0] (one rounded fp32 product per element; g itself is not written). ema null: no EMA
int adamw_clip_step(float* p, const float* g, float* m, float* v, float* ema, const float* coef, size_t n, double lr, double b1, double b2, double eps,
                    double wd, double ema_rate, int step, hipStream_t s);
// loss[0] = (1/n) sum_b w[b] sum_i (y - t)^2 over rows [B][row], n = B row; dy = 2 w[b] (y - t) / n. part: B floats of workspace.
int weighted_mse(const float* y, const float* t, const float* w, int B, size_t row, float* part, float* dy, float* loss, hipStream_t s);

}  // namespace gl
