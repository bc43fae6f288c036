// The start point of a partial sampling (include/gligen_amd_latent.h): resize an fp32 NCHW tensor and noise it to a timestep in one
// launch, dst = sa * resize(src) + s1 * noise. Image-to-image starts a sampler's tail from an encoded image this way, the second pass
// of a two-pass generation from the first pass's latent at another size; with noise == NULL it is a plain resize (decoded images,
// C = 3). torch's F.interpolate semantics (align_corners = False, no antialias) for nearest-exact, bilinear and bicubic.
// One lane per output element, lanes along x: a wave's stores and noise loads are one contiguous row segment, its tap loads a few
// contiguous runs of the source rows. A latency-class kernel on latents (262 k elements at 1024 x 1024 pixels, batch 4): nothing is
// staged or tuned beyond that; the index arithmetic per element (two 64-bit divisions for the position, one per axis for the
// coordinate) is what it costs.
#include "latent.h"
#include "misc.h"

namespace gl {

namespace {

template <int MODE> struct TapCount { static constexpr int value = MODE == LATENT_BICUBIC ? 4 : MODE == LATENT_BILINEAR ? 2 : 1; };

// Output index o of an axis resized n_in -> n_out: the source index of tap 0 before clamping, and the weights. torch's source
// coordinate (o + 0.5) n_in / n_out - 0.5 is the integer ratio ((2 o + 1) n_in - n_out) / (2 n_out); floor and remainder are taken in
// integers (as train_fusers.hip:axis_taps does), so t = rem / den and u = (den - rem) / den are one correctly rounded division each
// and an identity resize gets the taps (0, 1, 0, 0) / (1, 0) exactly. 64-bit: (2 o + 1) n_in passes 2^31 from sides of 32768 on.
template <int MODE>
__host__ __device__ __forceinline__ void axis_taps(int o, int n_in, int n_out, int* first, float w[4]) {
    const int64_t den = 2 * (int64_t)n_out;
    const int64_t num = (2 * (int64_t)o + 1) * n_in - n_out;
    if (MODE == LATENT_NEAREST_EXACT) {
        const int64_t i = (num + n_out) / den;                       // floor((2 o + 1) n_in / (2 n_out))
        *first = (int)(i < n_in - 1 ? i : n_in - 1);
        w[0] = 1.f;
        return;
    }
    int64_t i0, r;
    if (num < 0) {                                                   // only o = 0 ... of an upscale: the coordinate is in (-0.5, 0)
        i0 = MODE == LATENT_BILINEAR ? 0 : -1;                       // bilinear clamps the coordinate at 0; bicubic keeps it
        r = MODE == LATENT_BILINEAR ? 0 : num + den;
    } else {
        i0 = num / den;
        r = num - i0 * den;
    }
    const float fden = (float)den;
    const float t = (float)r / fden, u = (float)(den - r) / fden;
    if (MODE == LATENT_BILINEAR) {
        *first = (int)i0;
        w[0] = u;
        w[1] = t;
    } else {
        *first = (int)i0 - 1;
#if defined(__HIP_DEVICE_COMPILE__)
        cubic_taps_factored(t, u, w);
#else
        const float A = -0.75f;                                      // cubic_taps_factored (misc.h), restated for the host table
        w[0] = A * t * u * u;
        w[1] = u * (1.f + t - 1.25f * t * t);
        w[2] = t * (1.f + u - 1.25f * u * u);
        w[3] = A * u * t * t;
#endif
    }
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// q_sample's last step as torch computes a * x + s * noise: two rounded products and one rounded sum. __fmul_rn / __fadd_rn say so; they
// are plain operators in this toolchain, which -ffp-contract=fast would still fuse into one v_fmac (seen in this unit's ISA), so
// contraction is switched off for the statement as well.
__device__ __forceinline__ float scale_rn(float sa, float r) {
#pragma clang fp contract(off)
    return __fmul_rn(sa, r);
}
__device__ __forceinline__ float q_sample_rn(float sa, float r, float s1, float nz) {
#pragma clang fp contract(off)
    const float a = __fmul_rn(sa, r), b = __fmul_rn(s1, nz);
    return __fadd_rn(a, b);
}

// Grid-stride over the B C h2 w2 outputs. Per output: the horizontal taps of each source row in ascending order, then the rows in
// ascending order -- a fixed order, no atomics --, then q_sample's two rounded products and one rounded sum (train_inputs.hip), so at
// equal sizes the result is a * src + s * noise as torch rounds it, in every mode.
template <int MODE>
__global__ void __launch_bounds__(256) latent_renoise_kernel(const float* __restrict__ src, int C, int h, int w, float* __restrict__ dst, int h2,
                                                             int w2, float sa, float s1, const float* __restrict__ noise, int noise_bcast,
                                                             size_t total) {
    constexpr int NT = TapCount<MODE>::value;
    const size_t plane = (size_t)h * w, plane2 = (size_t)h2 * w2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / (size_t)w2;
        const int ox = (int)(i - row * (size_t)w2);
        const size_t pl = row / (size_t)h2;                          // b * C + c
        const int oy = (int)(row - pl * (size_t)h2);
        int fx, fy;
        float wx[4], wy[4];
        axis_taps<MODE>(ox, w, w2, &fx, wx);
        axis_taps<MODE>(oy, h, h2, &fy, wy);
        const float* base = src + pl * plane;
        float acc = 0.f;
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const float* line = base + (size_t)clampi(fy + p, h - 1) * w;
            float hs = 0.f;
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const float v = line[clampi(fx + q, w - 1)];
                if (MODE == LATENT_NEAREST_EXACT) hs = v;
                else hs = q == 0 ? wx[0] * v : hs + wx[q] * v;
            }
            if (MODE == LATENT_NEAREST_EXACT) acc = hs;
            else acc = p == 0 ? wy[0] * hs : acc + wy[p] * hs;
        }
        if (noise) {
            const size_t ni = noise_bcast ? (pl % (size_t)C) * plane2 + (i - pl * plane2) : i;
            dst[i] = q_sample_rn(sa, acc, s1, noise[ni]);
        } else {
            dst[i] = scale_rn(sa, acc);
        }
    }
}

template <int MODE>
void host_taps(int n_in, int n_out, int* first_index, float* weights) {
    for (int o = 0; o < n_out; ++o) {
        float w[4] = {0.f, 0.f, 0.f, 0.f};
        axis_taps<MODE>(o, n_in, n_out, first_index + o, w);
        for (int p = 0; p < 4; ++p) weights[4 * (size_t)o + p] = w[p];
    }
}

constexpr unsigned kMaxBlocks = 8192;      // 32 workgroups per CU; larger tensors (decoded images) take the grid-stride loop

}  // namespace

int latent_renoise_launch(const float* src, int B, int C, int h, int w, float* dst, int h2, int w2, int mode, float sa, float s1,
                          const float* noise, int noise_B, hipStream_t s) {
    if (!src || !dst) return set_error(GL_ERR_ARG, "latent_renoise: null src / dst");
    if (dst == src) return set_error(GL_ERR_ARG, "latent_renoise: dst == src (the resize reads neighbours of what it writes; give it another tensor)");
    if (B < 1 || C < 1 || h < 1 || w < 1 || h2 < 1 || w2 < 1)
        return set_error(GL_ERR_ARG, "latent_renoise: B, C and the four sides must be positive (B %d, C %d, %d x %d -> %d x %d)", B, C, h, w, h2, w2);
    if (noise && noise_B != 1 && noise_B != B)
        return set_error(GL_ERR_ARG, "latent_renoise: noise_B = %d, the noise has the batch of the output (%d) or 1", noise_B, B);
    const size_t total = (size_t)B * C * h2 * w2;
    const size_t blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks));
    const int bcast = noise && noise_B == 1 && B > 1;
    switch (mode) {
    case LATENT_NEAREST_EXACT:
        hipLaunchKernelGGL(latent_renoise_kernel<LATENT_NEAREST_EXACT>, grid, dim3(256), 0, s, src, C, h, w, dst, h2, w2, sa, s1, noise, bcast, total);
        break;
    case LATENT_BILINEAR:
        hipLaunchKernelGGL(latent_renoise_kernel<LATENT_BILINEAR>, grid, dim3(256), 0, s, src, C, h, w, dst, h2, w2, sa, s1, noise, bcast, total);
        break;
    case LATENT_BICUBIC:
        hipLaunchKernelGGL(latent_renoise_kernel<LATENT_BICUBIC>, grid, dim3(256), 0, s, src, C, h, w, dst, h2, w2, sa, s1, noise, bcast, total);
        break;
    default:
        return set_error(GL_ERR_ARG, "latent_renoise: mode %d (0 nearest-exact, 1 bilinear, 2 bicubic)", mode);
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int latent_resize_taps(int n_in, int n_out, int mode, int* first_index, float* weights, int* n_taps) {
    if (!first_index || !weights || !n_taps) return set_error(GL_ERR_ARG, "latent_resize_taps: null table");
    if (n_in < 1 || n_out < 1) return set_error(GL_ERR_ARG, "latent_resize_taps: sizes must be positive (%d -> %d)", n_in, n_out);
    switch (mode) {
    case LATENT_NEAREST_EXACT: host_taps<LATENT_NEAREST_EXACT>(n_in, n_out, first_index, weights); *n_taps = 1; break;
    case LATENT_BILINEAR: host_taps<LATENT_BILINEAR>(n_in, n_out, first_index, weights); *n_taps = 2; break;
    case LATENT_BICUBIC: host_taps<LATENT_BICUBIC>(n_in, n_out, first_index, weights); *n_taps = 4; break;
    default: return set_error(GL_ERR_ARG, "latent_resize_taps: mode %d (0 nearest-exact, 1 bilinear, 2 bicubic)", mode);
    }
    return GL_OK;
}

}  // namespace gl
