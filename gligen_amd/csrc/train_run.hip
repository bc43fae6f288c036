// The gradient unit of a training run (include/gligen_amd_train_run.h): what every SD-1.x trainer does between the backward and the
// update, over the flat fp32 gradient ranges of gligen_amd.dist.GradBuckets (209 M elements, 836 MB, for the shipped model) -- the sum
// over micro-batches, the global L2 norm and the clipping coefficient of torch.nn.utils.clip_grad_norm_, AdamW (+ EMA) on the clipped
// gradient -- and the per-sample weighted loss (min-SNR weights) of the training step. HBM-bound ground like train_optim.hip and
// shaped like it: 16-byte accesses per lane when every pointer is 16-byte aligned and a 4-byte path otherwise, a scalar tail for
// n % 4, a capped grid with a grid-stride loop, LDS in the reductions only, no atomics anywhere: every sum has one fixed order, so
// two runs, both schedules of TrainStep and both access paths give the same bits.
#include "adamw_update.h"
#include "train.h"
#include "train_run.h"

namespace gl {

namespace {

constexpr int kRunBlock = 256;
constexpr unsigned kRunGridCap = 16384;     // train_optim.hip's cap, measured there on the same kind of pass

// (the promised bits: every product and every sum below is rounded on its own, in the vector and in the scalar loop alike)
__device__ __forceinline__ float add_rounded(const float a, const float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float mul_rounded(const float a, const float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float mean_rounded(const float a, const float b, const float inv_k) {
#pragma clang fp contract(off)
    const float t = a + b;
    return t * inv_k;
}
__device__ __forceinline__ float square_add(const float s, const float x) {
#pragma clang fp contract(off)
    const float q = x * x;
    return s + q;
}

// MODE: GradAccumMode. n4: float4 groups of the vector path (0 when a pointer is misaligned); the scalar loop covers [4 n4, n)
template <int MODE>
__global__ void __launch_bounds__(kRunBlock) grad_accum_kernel(float* __restrict__ acc, float* __restrict__ g, size_t n, size_t n4, float inv_k) {
    const size_t stride = (size_t)gridDim.x * kRunBlock;
    const size_t first = (size_t)blockIdx.x * kRunBlock + threadIdx.x;
    float4* a4 = reinterpret_cast<float4*>(acc);
    float4* g4 = reinterpret_cast<float4*>(g);
    for (size_t i = first; i < n4; i += stride) {
        const float4 gv = g4[i];
        if (MODE == GRAD_ACCUM_FIRST) {
            a4[i] = gv;
        } else {
            const float4 av = a4[i];
            float4 r;
            if (MODE == GRAD_ACCUM_MIDDLE) {
                r.x = add_rounded(av.x, gv.x); r.y = add_rounded(av.y, gv.y); r.z = add_rounded(av.z, gv.z); r.w = add_rounded(av.w, gv.w);
                a4[i] = r;
            } else {
                r.x = mean_rounded(av.x, gv.x, inv_k); r.y = mean_rounded(av.y, gv.y, inv_k);
                r.z = mean_rounded(av.z, gv.z, inv_k); r.w = mean_rounded(av.w, gv.w, inv_k);
                g4[i] = r;
            }
        }
    }
    for (size_t i = 4 * n4 + first; i < n; i += stride) {
        if (MODE == GRAD_ACCUM_FIRST) acc[i] = g[i];
        else if (MODE == GRAD_ACCUM_MIDDLE) acc[i] = add_rounded(acc[i], g[i]);
        else g[i] = mean_rounded(acc[i], g[i], inv_k);
    }
}

// One partial per chunk of kGradNormChunk elements. Thread t of the workgroup owns the float4 groups t, t + 256, ... of the chunk and
// sums their squares in that order, x y z w inside a group: a chain of kGradNormChain terms. The 4-byte path reads the same elements
// in the same order and an element beyond n adds nothing (s + 0 = s), so both paths and a ragged last chunk give the same bits.
__global__ void __launch_bounds__(kGradNormBlock) grad_sqnorm_kernel(const float* __restrict__ g, size_t n, size_t n_chunks, int vec,
                                                                      float* __restrict__ partials) {
    __shared__ float red[kGradNormWaves];
    const int t = threadIdx.x;
    for (size_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const size_t base = c * (size_t)kGradNormChunk;
        float s = 0.f;
        if (vec && base + kGradNormChunk <= n) {
            const float4* g4 = reinterpret_cast<const float4*>(g + base);
            float4 x[kGradNormChain / 4];
#pragma unroll
            for (int j = 0; j < kGradNormChain / 4; ++j) x[j] = g4[j * kGradNormBlock + t];
#pragma unroll
            for (int j = 0; j < kGradNormChain / 4; ++j) {
                s = square_add(s, x[j].x);
                s = square_add(s, x[j].y);
                s = square_add(s, x[j].z);
                s = square_add(s, x[j].w);
            }
        } else {
            for (int j = 0; j < kGradNormChain / 4; ++j) {
                const size_t e = base + ((size_t)j * kGradNormBlock + t) * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (e + q < n) s = square_add(s, g[e + q]);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s = add_rounded(s, __shfl_xor(s, off, 64));     // a butterfly: every lane ends with the same sum
        if ((t & 63) == 0) red[t >> 6] = s;
        __syncthreads();
        if (t == 0) {
            float r = red[0];
#pragma unroll
            for (int w = 1; w < kGradNormWaves; ++w) r = add_rounded(r, red[w]);
            partials[c] = r;
        }
        __syncthreads();        // (red is written again by the next chunk of this workgroup)
    }
}

// One workgroup. Thread t sums the t-th contiguous segment of the partials in index order in double; thread 0 adds the 256 segment
// sums in index order. torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1 (a NaN stays:
// torch.clamp hands a NaN through, fminf would not).
__global__ void __launch_bounds__(kRunBlock) clip_coef_kernel(const float* __restrict__ partials, size_t count, float max_norm, float* __restrict__ out2) {
    __shared__ double seg_sum[kRunBlock];
    const size_t seg = (count + kRunBlock - 1) / kRunBlock;
    const size_t lo = (size_t)threadIdx.x * seg;
    const size_t hi = lo + seg < count ? lo + seg : count;
    double a = 0.0;
    for (size_t i = lo; i < hi; ++i) a += (double)partials[i];
    seg_sum[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int i = 0; i < kRunBlock; ++i) total += seg_sum[i];
    const float norm = (float)sqrt(total);
    const float c = max_norm / (norm + 1e-6f);
    out2[0] = norm;
    out2[1] = c > 1.f ? 1.f : c;
}

// adamw_ema_kernel (train_optim.hip) on g' = fl(g * coef): the same adamw_update / ema_update, so given the same coef the same bits as
// gl_op_adamw_step / gl_op_adamw_ema_step on a gradient scaled by one fp32 product per element. coef is read from device memory, one
// load per thread: the step needs no host sync. The gradient is NOT written back (torch scales it in place): that would be a fourth
// store stream for a value nothing behind the update reads.
template <bool EMA>
__global__ void __launch_bounds__(kRunBlock) adamw_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                               float* __restrict__ ema, const float* __restrict__ coef_p, size_t n, size_t n4, float b1,
                                                               float omb1, float b2, float omb2, float eps, float decay, float step_size, float bc2_sqrt,
                                                               float rate, float omr) {
    const size_t stride = (size_t)gridDim.x * kRunBlock;
    const size_t first = (size_t)blockIdx.x * kRunBlock + threadIdx.x;
    const float coef = coef_p[0];
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(ema);
    for (size_t i = first; i < n4; i += stride) {
        float4 pv = p4[i], mv = m4[i], vv = v4[i];
        float4 ev;
        if (EMA) ev = e4[i];
        const float4 gv = g4[i];
        adamw_update(pv.x, mul_rounded(gv.x, coef), mv.x, vv.x, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        adamw_update(pv.y, mul_rounded(gv.y, coef), mv.y, vv.y, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        adamw_update(pv.z, mul_rounded(gv.z, coef), mv.z, vv.z, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        adamw_update(pv.w, mul_rounded(gv.w, coef), mv.w, vv.w, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        m4[i] = mv;
        v4[i] = vv;
        p4[i] = pv;
        if (EMA) {
            ev.x = ema_update(ev.x, pv.x, rate, omr);
            ev.y = ema_update(ev.y, pv.y, rate, omr);
            ev.z = ema_update(ev.z, pv.z, rate, omr);
            ev.w = ema_update(ev.w, pv.w, rate, omr);
            e4[i] = ev;
        }
    }
    for (size_t i = 4 * n4 + first; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_update(pi, mul_rounded(g[i], coef), mi, vi, b1, omb1, b2, omb2, eps, decay, step_size, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        if (EMA) ema[i] = ema_update(ema[i], pi, rate, omr);
    }
}

// One workgroup per sample over its row of `row` elements: dy = 2 w_b (y - t) / n, part[b] = sum_i (y - t)^2 with thread t summing the
// elements t, t + 256, ... in order, then the wave butterfly and the wave sums in index order. A few times 10^4 elements: correct
// and the same bits every time, not fast.
__global__ void __launch_bounds__(kRunBlock) weighted_mse_kernel(const float* __restrict__ y, const float* __restrict__ t, const float* __restrict__ w,
                                                                 size_t row, size_t n, float* __restrict__ part, float* __restrict__ dy) {
    __shared__ float red[kRunBlock / 64];
    const size_t base = (size_t)blockIdx.x * row;
    const float wb = w[blockIdx.x];
    float s = 0.f;
    for (size_t i = threadIdx.x; i < row; i += kRunBlock) {
        const float d = y[base + i] - t[base + i];
        s = square_add(s, d);
        dy[base + i] = 2.f * wb * d / (float)n;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = add_rounded(s, __shfl_xor(s, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = red[0];
        for (int k = 1; k < kRunBlock / 64; ++k) r = add_rounded(r, red[k]);
        part[blockIdx.x] = r;
    }
}
// loss = (1/n) sum_b w_b part[b], the samples in index order
__global__ void weighted_mse_final_kernel(const float* __restrict__ part, const float* __restrict__ w, int B, size_t n, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float r = 0.f;
    for (int b = 0; b < B; ++b) r = add_rounded(r, mul_rounded(w[b], part[b]));
    loss[0] = r / (float)n;
}

// the vector groups (and one block's worth of tail), or every element: train_optim.hip's grid
unsigned run_grid(size_t n, size_t n4) {
    const size_t lanes = n4 ? n4 + (n - 4 * n4 ? 1 : 0) : n;
    const size_t blocks = (lanes + kRunBlock - 1) / kRunBlock;
    return (unsigned)(blocks < kRunGridCap ? blocks : kRunGridCap);
}

}  // namespace

int grad_accumulate(float* acc, float* g, size_t n, int mode, int k, hipStream_t s) {
    if (k < 1) return set_error(GL_ERR_ARG, "grad_accumulate: k = %d micro-batches, at least 1", k);
    if (mode != GRAD_ACCUM_FIRST && mode != GRAD_ACCUM_MIDDLE && mode != GRAD_ACCUM_LAST)
        return set_error(GL_ERR_ARG, "grad_accumulate: mode %d (0 first, 1 middle, 2 last)", mode);
    if (n == 0) return GL_OK;
    const size_t n4 = (((uintptr_t)acc | (uintptr_t)g) & 15) ? 0 : n / 4;
    const float inv_k = (float)(1.0 / (double)k);
    const dim3 grid(run_grid(n, n4)), block(kRunBlock);
    if (mode == GRAD_ACCUM_FIRST) hipLaunchKernelGGL(grad_accum_kernel<GRAD_ACCUM_FIRST>, grid, block, 0, s, acc, g, n, n4, inv_k);
    else if (mode == GRAD_ACCUM_MIDDLE) hipLaunchKernelGGL(grad_accum_kernel<GRAD_ACCUM_MIDDLE>, grid, block, 0, s, acc, g, n, n4, inv_k);
    else hipLaunchKernelGGL(grad_accum_kernel<GRAD_ACCUM_LAST>, grid, block, 0, s, acc, g, n, n4, inv_k);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

size_t grad_sqnorm_partials(size_t n) { return (n + kGradNormChunk - 1) / kGradNormChunk; }

int grad_sqnorm(const float* g, size_t n, float* partials, hipStream_t s) {
    if (n == 0) return GL_OK;
    const size_t chunks = grad_sqnorm_partials(n);
    const int vec = ((uintptr_t)g & 15) ? 0 : 1;        // (a chunk starts a multiple of 64 KB behind g: aligned when g is)
    const unsigned grid = (unsigned)(chunks < kRunGridCap ? chunks : kRunGridCap);
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(kGradNormBlock), 0, s, g, n, chunks, vec, partials);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int clip_coef(const float* partials, size_t count, float max_norm, float* out2, hipStream_t s) {
    if (!(max_norm > 0.f)) return set_error(GL_ERR_ARG, "clip_coef: max_norm %g is not > 0", (double)max_norm);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(kRunBlock), 0, s, partials, count, max_norm, out2);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int adamw_clip_step(float* p, const float* g, float* m, float* v, float* ema, const float* coef, size_t n, double lr, double b1, double b2, double eps,
                    double wd, double ema_rate, int step, hipStream_t s) {
    if (step < 1) return set_error(GL_ERR_ARG, "adamw_clip_step: step counts from 1");
    if (ema && !(ema_rate >= 0.0 && ema_rate <= 1.0)) return set_error(GL_ERR_ARG, "adamw_clip_step: ema_rate %g is outside [0, 1]", ema_rate);
    if (n == 0) return GL_OK;
    const AdamwScalars k = adamw_scalars(lr, b1, b2, eps, wd, step);
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema;
    const size_t n4 = (bits & 15) ? 0 : n / 4;
    const dim3 grid(run_grid(n, n4)), block(kRunBlock);
    if (ema)
        hipLaunchKernelGGL(adamw_clip_kernel<true>, grid, block, 0, s, p, g, m, v, ema, coef, n, n4, k.b1, k.omb1, k.b2, k.omb2, k.eps, k.decay, k.step_size,
                           k.bc2_sqrt, (float)ema_rate, (float)(1.0 - ema_rate));
    else
        hipLaunchKernelGGL(adamw_clip_kernel<false>, grid, block, 0, s, p, g, m, v, ema, coef, n, n4, k.b1, k.omb1, k.b2, k.omb2, k.eps, k.decay, k.step_size,
                           k.bc2_sqrt, 0.f, 0.f);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int weighted_mse(const float* y, const float* t, const float* w, int B, size_t row, float* part, float* dy, float* loss, hipStream_t s) {
    if (B < 1 || row == 0) return set_error(GL_ERR_ARG, "weighted_mse: empty batch");
    const size_t n = (size_t)B * row;
    hipLaunchKernelGGL(weighted_mse_kernel, dim3((unsigned)B), dim3(kRunBlock), 0, s, y, t, w, row, n, part, dy);
    hipLaunchKernelGGL(weighted_mse_final_kernel, dim3(1), dim3(64), 0, s, part, w, B, n, loss);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
