// The per-element AdamW update, shared by adamw_kernel (train_ops.hip) and adamw_ema_kernel (train_optim.hip) so that the two
// cannot drift: the same expression, inlined into both, gives the same bits for p, m and v.
#pragma once
#include <hip/hip_runtime.h>

namespace gl {

// torch.optim.AdamW (_single_tensor_adamw): every scalar is formed in double on the host, as torch forms them from Python floats, and
// rounded to fp32 once: decay = 1 - lr wd, omb = 1 - beta, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
struct AdamwScalars {
    float b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt;
};

inline AdamwScalars adamw_scalars(double lr, double b1, double b2, double eps, double wd, int step) {
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    return AdamwScalars{(float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, (float)(1.0 - lr * wd), (float)(lr / bc1), (float)sqrt(bc2)};
}

// decoupled weight decay, bias-corrected moments; p, m, v updated in place. Every product and sum is rounded on its own, as torch's
// separate kernels round them: contraction into fused multiply-adds is switched off for this function, so that what the compiler
// makes of the expression does not depend on the kernel it is inlined into (scalar, or four elements per lane).
__device__ __forceinline__ void adamw_update(float& p, const float gi, float& m, float& v, const float b1, const float omb1, const float b2,
                                             const float omb2, const float eps, const float decay, const float step_size, const float bc2_sqrt) {
#pragma clang fp contract(off)
    const float mi = b1 * m + omb1 * gi;
    const float vi = b2 * v + omb2 * gi * gi;
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p = p * decay - step_size * (mi / denom);
}

// update_ema (trainer.py:121-123): targ.mul_(rate).add_(src, alpha = 1 - rate) -- two rounded products and a rounded sum, on both
// paths of adamw_ema_kernel
__device__ __forceinline__ float ema_update(const float ema, const float p_new, const float rate, const float omr) {
#pragma clang fp contract(off)
    return rate * ema + omr * p_new;
}

}  // namespace gl
