// Training the gatedSA2 fuser (reference attention.py:272-297): its residual is the attention output at the sg x sg grid of grounding
// tokens, resized to the sv x sv visual grid by torch's bicubic. Inference has that fused with the gate on bf16 rows
// (misc.hip:fuser_resize_kernel); the training step keeps fp32 rows [B][pixels][C] and needs the operator and its transpose.
// Lanes run along C, so a wave's 16 tap reads (forward) or its walk over the destinations (backward) are 256-byte row segments.
// Both kernels take a destination index's (4 clamped source indices, 4 weights) from axis_taps below, so the backward's weights are
// the forward's bit for bit. The grids are square on both sides, so one tap table serves the y and the x axis.
#include "train_fusers.h"
#include "misc.h"

namespace gl {

namespace {

// destination index o of an axis resized n_src -> n_dst: the clamped source indices and weights. torch's source coordinate
// (o + 0.5) n_src / n_dst - 0.5 is the integer ratio ((2 o + 1) n_src - n_dst) / (2 n_dst): its floor and remainder are taken in
// integers, so t and u = 1 - t are each one correctly rounded division (the fp32 product with the rounded scale, 1.6f for 8 -> 5, is
// off by an ulp of the coordinate, 30 ulp of a small weight), and the weights are cubic_taps_factored's (misc.h).
__device__ __forceinline__ void axis_taps(int o, int n_src, int n_dst, int idx[4], float w[4]) {
    const int num = (2 * o + 1) * n_src - n_dst, den = 2 * n_dst;
    const int i0 = num >= 0 ? num / den : -((den - 1 - num) / den);       // floor
    const int r = num - i0 * den;                                         // in [0, den)
    cubic_taps_factored((float)r / (float)den, (float)(den - r) / (float)den, w);
#pragma unroll
    for (int p = 0; p < 4; ++p) idx[p] = min(max(i0 - 1 + p, 0), n_src - 1);
}

// one thread per (sample, output pixel, channel): 16 taps, summed p-major (rows), q-minor
__global__ void __launch_bounds__(256) grid_resize_fwd_kernel(const float* __restrict__ src, int sg, int sv, int C, size_t total, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % (size_t)C);
    const size_t r = i / (size_t)C;
    const size_t npix = (size_t)sv * sv;
    const int pix = (int)(r % npix);
    const size_t b = r / npix;
    const int oy = pix / sv, ox = pix - oy * sv;
    int iy[4], ix[4];
    float wy[4], wx[4];
    axis_taps(oy, sg, sv, iy, wy);
    axis_taps(ox, sg, sv, ix, wx);
    const float* base = src + b * (size_t)sg * sg * C + c;
    float acc = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += (wy[p] * wx[q]) * base[((size_t)iy[p] * sg + ix[q]) * C];
    dst[i] = acc;
}

// The adjoint as a gather: one thread per (sample, source token, channel). Every workgroup first builds in LDS the tap table of the
// sv destination indices (tap_i / tap_w: 4 each) and, per source index, the range [lo, hi) of destination indices with a tap on it
// (floor(src) is monotone in the destination index, so that set is contiguous; empty: lo = hi). The thread then walks oy, ox in
// ascending order, and within a destination its taps in the forward's (p, q) order -- clamping can put several taps of one
// destination on one source index --, adding (wy wx) g: a fixed order, so two runs give the same bits.
__global__ void __launch_bounds__(256) grid_resize_bwd_kernel(const float* __restrict__ g, int sg, int sv, int C, size_t total, float* __restrict__ dsrc) {
    extern __shared__ int lds[];
    int* tap_i = lds;                                              // [sv][4]
    float* tap_w = reinterpret_cast<float*>(lds + 4 * sv);         // [sv][4]
    int* lo = lds + 8 * sv;                                        // [sg]
    int* hi = lo + sg;                                             // [sg]
    for (int o = threadIdx.x; o < sv; o += 256) {
        int idx[4];
        float w[4];
        axis_taps(o, sg, sv, idx, w);
#pragma unroll
        for (int p = 0; p < 4; ++p) { tap_i[4 * o + p] = idx[p]; tap_w[4 * o + p] = w[p]; }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < sg; s += 256) {
        int first = sv, last = -1;
        for (int o = 0; o < sv; ++o) {
            const bool on = tap_i[4 * o] == s || tap_i[4 * o + 1] == s || tap_i[4 * o + 2] == s || tap_i[4 * o + 3] == s;
            if (on) { first = min(first, o); last = o; }
        }
        lo[s] = last < 0 ? 0 : first;
        hi[s] = last + 1;
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % (size_t)C);
    const size_t r = i / (size_t)C;
    const size_t ntok = (size_t)sg * sg;
    const int tok = (int)(r % ntok);
    const size_t b = r / ntok;
    const int sy = tok / sg, sx = tok - sy * sg;
    const float* base = g + b * (size_t)sv * sv * C + c;
    const int ox0 = lo[sx], ox1 = hi[sx];
    float acc = 0.f;
    for (int oy = lo[sy]; oy < hi[sy]; ++oy) {
        for (int ox = ox0; ox < ox1; ++ox) {
            const float gv = base[((size_t)oy * sv + ox) * C];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (tap_i[4 * oy + p] != sy) continue;
                const float wyp = tap_w[4 * oy + p];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (tap_i[4 * ox + q] == sx) acc += (wyp * tap_w[4 * ox + q]) * gv;
            }
        }
    }
    dsrc[i] = acc;
}

int check(const char* what, const void* a, const void* b, int B, int sg, int sv, int C, size_t n_out) {
    if (!a || !b) return set_error(GL_ERR_ARG, "%s: null pointer", what);
    if (B < 1 || C < 1 || sg < 1 || sv < 1 || sg > kGridResizeMaxSide || sv > kGridResizeMaxSide)
        return set_error(GL_ERR_ARG, "%s: B and C must be positive and the grid sides in [1, %d] (sg = %d, sv = %d)", what, kGridResizeMaxSide, sg, sv);
    if ((n_out + 255) / 256 >= ((size_t)1 << 31)) return set_error(GL_ERR_ARG, "%s: more than 2^31 workgroups of output", what);
    return GL_OK;
}

}  // namespace

int grid_resize_fwd_launch(const float* src, int B, int sg, int sv, int C, float* dst, hipStream_t s) {
    const size_t total = (size_t)B * sv * sv * C;
    GL_TRY(check("grid_resize", src, dst, B, sg, sv, C, total));
    hipLaunchKernelGGL(grid_resize_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, sg, sv, C, total, dst);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int grid_resize_bwd_launch(const float* g, int B, int sg, int sv, int C, float* dsrc, hipStream_t s) {
    const size_t total = (size_t)B * sg * sg * C;
    GL_TRY(check("grid_resize_backward", g, dsrc, B, sg, sv, C, total));
    const size_t lds_bytes = (size_t)(8 * sv + 2 * sg) * 4;       // <= 40 KiB at kGridResizeMaxSide
    hipLaunchKernelGGL(grid_resize_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), lds_bytes, s, g, sg, sv, C, total, dsrc);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
