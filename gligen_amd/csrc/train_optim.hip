// The optimizer unit of a training run (include/gligen_amd_trainer.h; reference trainer.py:121-123, 388-391: opt.step(), then
// update_ema): AdamW and the exponential moving average of the parameters in one pass over a flat fp32 range. HBM-bound: five loads
// and four stores per element, 36 B against AdamW's 28 B, and no second pass that reads the parameters back. 16-byte accesses per
// lane, a capped grid with a grid-stride loop, a scalar tail for n % 4 and a scalar path when a pointer is not 16-byte aligned. No
// LDS, no atomics. p, m and v get the bits of adamw_kernel (train_ops.hip): both inline adamw_update (adamw_update.h).
#include "adamw_update.h"
#include "train.h"

namespace gl {

namespace {

constexpr int kOptimBlock = 256;
// 64 blocks per CU; what lies beyond (above 16.8 M elements) is covered by the grid-stride loop. Measured on the 32.7 M-element bucket
// of the shipped model, one MI355X, medians of 20: 2048 blocks 218 us, 6144 211 us, 16384 206 us, one block per 1024 elements 204 us
//  -- the customary 8 blocks per CU cost this kernel 7 %.
constexpr unsigned kOptimGridCap = 16384;

// n4: float4 groups of the vector path (0 when a pointer is misaligned); the scalar loop covers [4 n4, n)
__global__ void __launch_bounds__(kOptimBlock) adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                                float* __restrict__ ema, size_t n, size_t n4, float b1, float omb1, float b2, float omb2,
                                                                float eps, float decay, float step_size, float bc2_sqrt, float rate, float omr) {
    const size_t stride = (size_t)gridDim.x * kOptimBlock;
    const size_t first = (size_t)blockIdx.x * kOptimBlock + threadIdx.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    for (size_t i = first; i < n4; i += stride) {
        float4 pv = p4[i], mv = m4[i], vv = v4[i], ev = e4[i];
        const float4 gv = g4[i];
        adamw_update(pv.x, gv.x, mv.x, vv.x, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        adamw_update(pv.y, gv.y, mv.y, vv.y, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        adamw_update(pv.z, gv.z, mv.z, vv.z, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        adamw_update(pv.w, gv.w, mv.w, vv.w, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        // the average of the parameter AFTER the update (opt.step(), then update_ema: targ.mul_(rate).add_(src, alpha = 1 - rate))
        ev.x = ema_update(ev.x, pv.x, rate, omr);
        ev.y = ema_update(ev.y, pv.y, rate, omr);
        ev.z = ema_update(ev.z, pv.z, rate, omr);
        ev.w = ema_update(ev.w, pv.w, rate, omr);
        m4[i] = mv;
        v4[i] = vv;
        p4[i] = pv;
        e4[i] = ev;
    }
    for (size_t i = 4 * n4 + first; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_update(pi, g[i], mi, vi, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        ema[i] = ema_update(ema[i], pi, rate, omr);
    }
}

}  // namespace

int adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr, double b1, double b2, double eps, double wd, double ema_rate,
                   int step, hipStream_t s) {
    if (step < 1) return set_error(GL_ERR_ARG, "adamw_ema_step: step counts from 1");
    if (!(ema_rate >= 0.0 && ema_rate <= 1.0)) return set_error(GL_ERR_ARG, "adamw_ema_step: ema_rate %g is outside [0, 1]", ema_rate);
    if (n == 0) return GL_OK;
    const AdamwScalars k = adamw_scalars(lr, b1, b2, eps, wd, step);
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema;
    const size_t n4 = (bits & 15) ? 0 : n / 4;
    const size_t lanes = n4 ? n4 + (n - 4 * n4 ? 1 : 0) : n;     // the vector groups (and one block's worth of tail), or every element
    const size_t blocks = (lanes + kOptimBlock - 1) / kOptimBlock;
    const unsigned grid = (unsigned)(blocks < kOptimGridCap ? blocks : kOptimGridCap);
    hipLaunchKernelGGL(adamw_ema_kernel, dim3(grid), dim3(kOptimBlock), 0, s, p, g, m, v, ema, n, n4, k.b1, k.omb1, k.b2, k.omb2, k.eps, k.decay, k.step_size,
                       k.bc2_sqrt, (float)ema_rate, (float)(1.0 - ema_rate));
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
