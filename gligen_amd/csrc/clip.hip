// CLIP text tower kernels for gfx950 (see clip.h). Work per call is small (S <= ~32 sequences of <= 77 tokens, 13 GFLOP each at
// ViT-L/14 size): the aim is few, exact, spill-free launches. The projections run on the bf16 MFMA GEMM (gemm.hip).
#include "clip.h"

#include <math.h>

namespace gl {

// ---------------------------------------------------------------------------------------------------------------- embedding
__global__ __launch_bounds__(256) void clip_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                         float* __restrict__ h, int rows, int T, int w4, int vocab, unsigned* bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * w4) return;
    const int row = (int)(i / w4), c = (int)(i - (int64_t)row * w4);
    int id = ids[row];
    if (id < 0 || id >= vocab) {
        if (bad && c == 0) atomicAdd(bad, 1u);
        id = id < 0 ? 0 : vocab - 1;
    }
    const float4 a = reinterpret_cast<const float4*>(tok)[(size_t)id * w4 + c];
    const float4 b = reinterpret_cast<const float4*>(pos)[(size_t)(row % T) * w4 + c];
    reinterpret_cast<float4*>(h)[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

int clip_embed_launch(const int32_t* ids, const float* tok, const float* pos, float* h, int rows, int T, int width, int vocab, unsigned* bad,
                      hipStream_t stream) {
    if (rows <= 0 || T <= 0 || width <= 0 || width % 4 || vocab <= 0) return set_error(GL_ERR_ARG, "clip_embed: rows=%d T=%d width=%d vocab=%d", rows, T, width, vocab);
    const int64_t n = (int64_t)rows * (width / 4);
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, ids, tok, pos, h, rows, T, width / 4, vocab, bad);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ------------------------------------------------------------------------------------------- residual add + LayerNorm (fp32 stream)
// One wave per row; the row stays in registers between the add, the two statistics passes (mean, then centred variance) and the
// affine output, so the fp32 residual stream is read once and written once per sub-layer.
__global__ __launch_bounds__(256) void clip_add_ln_kernel(float* __restrict__ h, const float* __restrict__ delta, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, bf16* __restrict__ ybf, float* __restrict__ yf32,
                                                          int rows, int width) {
    constexpr int MAXV = kClipMaxWidth / 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* hr = h + (size_t)row * width;
    float4 v[MAXV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < width) {
            v[i] = *reinterpret_cast<const float4*>(hr + c);
            if (delta) {
                const float4 d = *reinterpret_cast<const float4*>(delta + (size_t)row * width + c);
                v[i].x += d.x; v[i].y += d.y; v[i].z += d.z; v[i].w += d.w;
                *reinterpret_cast<float4*>(hr + c) = v[i];
            }
            sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    const float mean = wave_sum(sum) / (float)width;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < width) {
            const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            sq += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)width + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < width) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            const float4 b = *reinterpret_cast<const float4*>(beta + c);
            float y[4] = {(v[i].x - mean) * rstd * g.x + b.x, (v[i].y - mean) * rstd * g.y + b.y, (v[i].z - mean) * rstd * g.z + b.z,
                          (v[i].w - mean) * rstd * g.w + b.w};
            if (yf32) {
                *reinterpret_cast<float4*>(yf32 + (size_t)row * width + c) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
                U2BF4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o.e[e] = f2bf(y[e]);
                *reinterpret_cast<uint2*>(ybf + (size_t)row * width + c) = o.u;
            }
        }
    }
}

int clip_add_ln_launch(float* h, const float* delta, const float* gamma, const float* beta, float eps, bf16* ybf, float* yf32, int rows, int width,
                       hipStream_t stream) {
    if (rows <= 0 || width <= 0 || width % 4 || width > kClipMaxWidth || !gamma || !beta || (!ybf == !yf32))
        return set_error(GL_ERR_ARG, "clip_add_ln: rows=%d width=%d (width %% 4 == 0, <= %d; one output)", rows, width, kClipMaxWidth);
    hipLaunchKernelGGL(clip_add_ln_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, h, delta, gamma, beta, eps, ybf, yf32, rows, width);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ---------------------------------------------------------------------------------------------------------------- attention
// One workgroup per (sequence, head), one wave per 32-query tile (T <= 96: three waves). Q, K and V^T of the head are staged once in
// LDS (40 KB: two workgroups per CU); rows / keys beyond T are zeros. Both products run on v_mfma_f32_32x32x16_bf16 in the swapped
// form of attention.hip: S^T = K Q^T puts the query on the lane and the 32 keys of a tile in the 16 accumulator registers of the two
// lane halves, so the row maximum / sum are register reductions plus one exchange with lane ^ 32, and the bf16-packed accumulator
// IS the B operand of O^T += V^T P^T (k order inside a step: key 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3), which is how the V^T
// fragment is gathered). All (at most three) score tiles of a query tile are held at once: plain two-pass softmax in fp32, no
// rescaling. Keys above the diagonal and keys >= T are set to -inf BEFORE the row maximum (p = 0 exactly: rows at or before a
// position do not depend on what follows it); key tiles entirely above the diagonal are not computed.
constexpr int CA_LDQ = kClipHeadDim + 8;     // Q / K row stride in LDS (elements): 144 B, 16-byte fragment reads
constexpr int CA_LDV = kClipMaxTokens + 4;   // V^T row stride: 200 B, 8-byte fragment reads, rows 50 dwords apart

__global__ __launch_bounds__(192) void clip_attn_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o, int T, int H, int causal) {
    __shared__ __attribute__((aligned(16))) bf16 sQ[kClipMaxTokens * CA_LDQ];
    __shared__ __attribute__((aligned(16))) bf16 sK[kClipMaxTokens * CA_LDQ];
    __shared__ __attribute__((aligned(16))) bf16 sVt[kClipHeadDim * CA_LDV];
    const int s = blockIdx.x / H, h = blockIdx.x - s * H;
    const int W = H * kClipHeadDim, ld = 3 * W;
    const bf16* base = qkv + (size_t)s * T * ld + h * kClipHeadDim;
    for (int i = threadIdx.x; i < kClipMaxTokens * 8; i += 192) {
        const int t = i >> 3, c = i & 7;
        uint4 q = make_uint4(0, 0, 0, 0), k = q;
        U4BF8 v;
        v.u = q;
        if (t < T) {
            const bf16* p = base + (size_t)t * ld + c * 8;
            q = *reinterpret_cast<const uint4*>(p);
            k = *reinterpret_cast<const uint4*>(p + W);
            v.u = *reinterpret_cast<const uint4*>(p + 2 * W);
        }
        *reinterpret_cast<uint4*>(sQ + t * CA_LDQ + c * 8) = q;
        *reinterpret_cast<uint4*>(sK + t * CA_LDQ + c * 8) = k;
#pragma unroll
        for (int j = 0; j < 8; ++j) sVt[(c * 8 + j) * CA_LDV + t] = v.e[j];
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hh = lane >> 5;
    const int q0 = wave * 32;
    if (q0 >= T) return;
    const int qi = q0 + r;
    const int nkt = causal ? wave + 1 : (T + 31) >> 5;

    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(sQ + qi * CA_LDQ + ks * 16 + hh * 8);

    // ---- S^T tiles: [32 keys][32 queries], masked, scaled into the exp2 domain
    const float scale = 0.125f * 1.4426950408889634f;   // 64^-0.5 * log2(e)
    f32x16 sc[3];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
        if (kt < nkt) {
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (kt * 32 + r) * CA_LDQ + ks * 16 + hh * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                const bool ok = key < T && (!causal || key <= qi);
                acc[e] = ok ? acc[e] * scale : -INFINITY;
                m = fmaxf(m, acc[e]);
            }
            sc[kt] = acc;
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));   // key 0 is valid for every query: m is finite

    // ---- p = exp2(s - m), row sum in fp32; O^T[d][query] += V^T[d][key] P^T[key][query]
    f32x16 ot[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) ot[dt][e] = 0.f;
    float lsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
        if (kt < nkt) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                bf16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = __builtin_amdgcn_exp2f(sc[kt][8 * st + j] - m);
                    lsum += p;
                    pf[j] = f2bf(p);
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const bf16* vp = sVt + (dt * 32 + r) * CA_LDV + kt * 32 + 16 * st + 4 * hh;
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vp);
                    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vp + 8);
                    const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                    ot[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, ot[dt], 0, 0, 0);
                }
            }
        }
    }
    lsum += __shfl_xor(lsum, 32, 64);
    if (qi >= T) return;
    const float inv = 1.f / lsum;
    bf16* orow = o + ((size_t)s * T + qi) * W + h * kClipHeadDim;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            U2BF4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov.e[e] = f2bf(ot[dt][4 * g + e] * inv);
            *reinterpret_cast<uint2*>(orow + dt * 32 + 8 * g + 4 * hh) = ov.u;
        }
}

int clip_attn_launch(const bf16* qkv, bf16* o, int S, int T, int heads, int causal, hipStream_t stream) {
    if (S <= 0 || heads <= 0 || T <= 0 || T > kClipMaxTokens)
        return set_error(GL_ERR_UNSUPPORTED, "clip_attn: S=%d heads=%d T=%d (1 <= T <= %d)", S, heads, T, kClipMaxTokens);
    hipLaunchKernelGGL(clip_attn_kernel, dim3(S * heads), dim3(192), 0, stream, qkv, o, T, heads, causal);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// ---------------------------------------------------------------------------------------------------------------- pooling
__global__ __launch_bounds__(256) void clip_pool_kernel(const float* __restrict__ x, const int32_t* __restrict__ eos, float* __restrict__ pooled, int T, int w4) {
    const int s = blockIdx.x;
    int t = eos[s];
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    const float4* src = reinterpret_cast<const float4*>(x) + ((size_t)s * T + t) * w4;
    float4* dst = reinterpret_cast<float4*>(pooled) + (size_t)s * w4;
    for (int c = threadIdx.x; c < w4; c += 256) dst[c] = src[c];
}

int clip_pool_launch(const float* x, const int32_t* eos, float* pooled, int S, int T, int width, hipStream_t stream) {
    if (S <= 0 || T <= 0 || width <= 0 || width % 4) return set_error(GL_ERR_ARG, "clip_pool: S=%d T=%d width=%d", S, T, width);
    hipLaunchKernelGGL(clip_pool_kernel, dim3(S), dim3(256), 0, stream, x, eos, pooled, T, width / 4);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
